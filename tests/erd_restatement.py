"""Elastic Response Distillation as this library defines it, restated in float64 (numpy for the selection, torch for the term,
whose gradient is float64 autograd's) -- the definition the kernels of csrc/erd.hip and cl_methods.erd.erd_term are held to.

Selection, per clip, over the valid positions V (position t of level l is valid when t < valid[l]), levels end to end:
    c_i = max_{y < n_old} z_iy;  mu = mean_V c;  sigma = sqrt(mean_V (c - mu)^2)   (population, the mean first)
    S_cls = {i in V: c_i > mu + alpha_cls sigma};  S_reg = {i in V: c_i > mu + alpha_reg sigma and o^_i0 + o^_i1 > 0}
Term, over the batch rows with a record:
    A = sum_b sum_{i in S_cls(b)} sum_{y < n_b} (x_iy - z_iy)^2,  N_c = sum_b |S_cls(b)| n_b
    D = sum_b sum_{i in S_reg(b)} diou(o_i, o^_i),                N_r = sum_b |S_reg(b)|
    loss = lambda_cls A / N_c + lambda_reg D / N_r; a part whose count is 0 is 0
    diou(p, g) = 1 - I / max(U, eps) + (rho / max(len, eps))^2 with I = min(p1, g1) + min(p0, g0), U = (p0 + p1) + (g0 + g1) - I,
    len = max(p0, g0) + max(p1, g1), rho = (p1 - p0 - g1 + g0) / 2, eps = 1e-8  (modeling/losses.py: ctr_diou_loss_1d)
With `scale` the offsets are raw and o = relu(scale_l raw)."""
import numpy as np
import torch

EPS = 1e-8


def valid_positions(level_T, valid):
    out, first = [], 0
    for T, V in zip(level_T, valid):
        V = max(0, min(int(V), int(T)))
        out.extend(range(first, first + V))
        first += int(T)
    return np.asarray(out, dtype=np.int64)


def select(z, o_hat, level_T, valid, n_old, alpha_cls, alpha_reg):
    """z [P, C], o_hat [P, 2] of ONE clip -> dict: c, V, mu, sigma, thr_cls, thr_reg, S_cls, S_reg (ascending int lists)"""
    z, o_hat = np.asarray(z, dtype=np.float64), np.asarray(o_hat, dtype=np.float64)
    c = z[:, :int(n_old)].max(axis=1)
    V = valid_positions(level_T, valid)
    if V.size == 0:
        return dict(c=c, V=V, mu=0.0, sigma=0.0, thr_cls=np.inf, thr_reg=np.inf, S_cls=[], S_reg=[])
    cv = c[V]
    mu = cv.sum() / cv.size
    sigma = np.sqrt(((cv - mu) ** 2).sum() / cv.size)
    tc, tr = mu + float(alpha_cls) * sigma, mu + float(alpha_reg) * sigma
    return dict(c=c, V=V, mu=mu, sigma=sigma, thr_cls=tc, thr_reg=tr,
                S_cls=[int(i) for i in V if c[i] > tc],
                S_reg=[int(i) for i in V if c[i] > tr and o_hat[i, 0] + o_hat[i, 1] > 0])


def margin(sel):
    """the smallest relative distance of a valid position's response from either threshold (inf: no valid position)"""
    if sel['V'].size == 0:
        return np.inf
    cv = sel['c'][sel['V']]
    return min(float((np.abs(cv - t) / np.maximum(np.maximum(np.abs(cv), abs(t)), 1e-300)).min())
               for t in (sel['thr_cls'], sel['thr_reg']))


def make_record(z, o_hat, sel, n_old):
    """-> dict(map_cls, map_reg int32 [P]; val_cls [K_c, n_old], val_reg [K_r, 2] float32; n_old): what a record keeps"""
    z, o_hat = np.asarray(z, dtype=np.float32), np.asarray(o_hat, dtype=np.float32)
    P = z.shape[0]
    rec = {'n_old': int(n_old)}
    for name, S in (('cls', sel['S_cls']), ('reg', sel['S_reg'])):
        m = np.full(P, -1, dtype=np.int32)
        m[S] = np.arange(len(S), dtype=np.int32)
        rec['map_' + name] = m
    rec['val_cls'] = z[sel['S_cls'], :int(n_old)].reshape(len(sel['S_cls']), int(n_old))
    rec['val_reg'] = o_hat[sel['S_reg']].reshape(len(sel['S_reg']), 2)
    return rec


def diou(p, g):
    """[K, 2] x [K, 2] float64 torch -> [K]"""
    p0, p1, g0, g1 = p[:, 0], p[:, 1], g[:, 0], g[:, 1]
    inter = torch.min(p1, g1) + torch.min(p0, g0)
    union = (p0 + p1) + (g0 + g1) - inter
    iou = inter / union.clamp(min=EPS)
    length = torch.max(p0, g0) + torch.max(p1, g1)
    rho = 0.5 * (p1 - p0 - g1 + g0)
    return 1.0 - iou + torch.square(rho / length.clamp(min=EPS))


def term(logits, offsets, scale, level_row, level_T, valid, records, lambda_cls, lambda_reg, g_out=1.0):
    """logits [B, R, C], offsets [B, R, 2], scale [L] or None (any float tensors / arrays); valid [B][L]; records: per row None
    or make_record's dict -> dict: loss, cls, reg (floats), N_c, N_r (ints), d_logits, d_offsets, d_scale (float64 tensors, the
    gradient of g_out * loss; d_scale None without scale)"""
    x = torch.as_tensor(np.asarray(logits, dtype=np.float64)).clone().requires_grad_(True)
    o = torch.as_tensor(np.asarray(offsets, dtype=np.float64)).clone().requires_grad_(True)
    s = None if scale is None else torch.as_tensor(np.asarray(scale, dtype=np.float64)).clone().requires_grad_(True)
    rows, level_of = [], []
    for l, (r, T) in enumerate(zip(level_row, level_T)):
        rows.extend(range(int(r), int(r) + int(T)))
        level_of.extend([l] * int(T))
    rows, level_of = torch.tensor(rows), torch.tensor(level_of)
    A, D, Nc, Nr = x.new_zeros(()), x.new_zeros(()), 0, 0
    for b, rec in enumerate(records):
        if rec is None:
            continue
        V = set(valid_positions(level_T, valid[b]).tolist())
        n_b = rec['n_old']
        Sc = [i for i in range(len(rows)) if rec['map_cls'][i] >= 0 and i in V]
        Sr = [i for i in range(len(rows)) if rec['map_reg'][i] >= 0 and i in V]
        if Sc:
            zc = torch.as_tensor(rec['val_cls'].astype(np.float64))[rec['map_cls'][Sc].astype(np.int64)]
            A = A + ((x[b, rows[Sc], :n_b] - zc) ** 2).sum()
            Nc += len(Sc) * n_b
        if Sr:
            zr = torch.as_tensor(rec['val_reg'].astype(np.float64))[rec['map_reg'][Sr].astype(np.int64)]
            ob = o[b, rows[Sr]]
            if s is not None:
                ob = torch.relu(ob * s[level_of[Sr]][:, None])
            D = D + diou(ob, zr).sum()
            Nr += len(Sr)
    cls = float(lambda_cls) * A / Nc if Nc else x.new_zeros(())
    reg = float(lambda_reg) * D / Nr if Nr else x.new_zeros(())
    loss = cls + reg
    if loss.requires_grad:
        (float(g_out) * loss).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(loss=float(loss.detach()), cls=float(cls.detach()), reg=float(reg.detach()), N_c=Nc, N_r=Nr, d_logits=zero(x), d_offsets=zero(o),
                d_scale=None if s is None else zero(s))
