"""Float64 restatement of the narration-SSL branch (csrc/ssl.hip, include/vilco_hip.h): masked mean pooling over a list of
levels, the memory bank's masked ring update and InfoNCE against the bank, with the analytic gradients.  Written from the
formulas of the header, in numpy, for the tests to hold the device path (and the reference golden) against.

  pool      out[b] = (1/L) sum_l (1/max(len_bl, 1)) sum_{t < len_bl} f_l[b, t, :]
  ring      rows with mask != 0, compacted in batch order, to bank rows (ptr + rank) mod M; ptr <- (ptr + n) mod M
  loss      (1/(2n)) sum_masked ((lse_t - p) + (lse_v - p)),  p = tn . vn / tau,
            lse_x = log(exp(p) + sum_j exp(xn . bank_j / tau)) over the bank AFTER the ring update
"""
import numpy as np

EPS = 1e-12


def pool(feats, lens):
    """feats: list of L arrays [B, T_l, C]; lens: int [B, L] -> [B, C]"""
    L = len(feats)
    B, _, C = feats[0].shape
    out = np.zeros((B, C), dtype=np.float64)
    for l, f in enumerate(feats):
        for b in range(B):
            n = int(min(max(lens[b][l], 0), f.shape[1]))
            if n > 0:
                out[b] += np.asarray(f[b, :n], dtype=np.float64).sum(0) / n
    return out / L


def pool_grad(dout, Ts, lens):
    """gradients of `pool` for every level: dout / (L max(len, 1)) below the length, 0 at and above it"""
    L = len(Ts)
    B, C = dout.shape
    grads = []
    for l, T in enumerate(Ts):
        g = np.zeros((B, T, C), dtype=np.float64)
        for b in range(B):
            n = int(min(max(lens[b][l], 0), T))
            g[b, :n] = dout[b] / (L * max(n, 1))
        grads.append(g)
    return grads


def normalize(x):
    x = np.asarray(x, dtype=np.float64)
    nrm = np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), EPS)
    return x / nrm, nrm


def ring_update(bank, ptr, rows, mask):
    """-> (new bank, new ptr, n); untouched when no row is masked"""
    bank = np.array(bank, dtype=np.float64)
    M = bank.shape[0]
    sel = [b for b in range(len(mask)) if mask[b] != 0]
    assert len(sel) <= M
    if not sel:
        return bank, int(ptr), 0
    p = int(ptr) % M
    for r, b in enumerate(sel):
        bank[(p + r) % M] = rows[b]
    return bank, (p + len(sel)) % M, len(sel)


def _lse(z):
    m = z.max()
    return m + np.log(np.exp(z - m).sum())


def nce(text, video, mask, bank, ptr, tau=0.07):
    """raw pooled text / video [B, D], mask [B], bank [M, D], ptr -> dict(loss, dtext, dvideo, bank, ptr, n, tn, vn):
    normalise, ring update, loss, gradients with respect to the RAW rows."""
    tn, nt = normalize(text)
    vn, nv = normalize(video)
    bank, ptr, n = ring_update(bank, ptr, tn, mask)
    B, D = tn.shape
    dtn, dvn = np.zeros((B, D)), np.zeros((B, D))
    loss = 0.0
    if n:
        for b in range(B):
            if mask[b] == 0:
                continue
            p = float(tn[b] @ vn[b]) / tau
            zt = np.concatenate([[p], bank @ tn[b] / tau])
            zv = np.concatenate([[p], bank @ vn[b] / tau])
            lt, lv = _lse(zt), _lse(zv)
            loss += (lt - p) + (lv - p)
            pt, pv = np.exp(zt - lt), np.exp(zv - lv)
            cpos = (pt[0] + pv[0] - 2.0) / tau
            dtn[b] = (cpos * vn[b] + (pt[1:] @ bank) / tau) / (2 * n)
            dvn[b] = (cpos * tn[b] + (pv[1:] @ bank) / tau) / (2 * n)
        loss /= 2 * n

    def through_norm(x, xn, nrm, g):
        raw = np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(1, keepdims=True))
        proj = (g - xn * (g * xn).sum(1, keepdims=True)) / nrm
        return np.where(raw > EPS, proj, g / nrm)
    return dict(loss=loss, dtext=through_norm(text, tn, nt, dtn), dvideo=through_norm(video, vn, nv, dvn), bank=bank, ptr=ptr,
                n=n, tn=tn, vn=vn)


def step(enc_w, enc_b, tokens_cf, tok_lens, feats, feat_lens, mask, bank, ptr, tau=0.07):
    """one SSL step from the branch's inputs: tokens_cf [B, Cn, n] narration tokens (channel-first, as the clip dictionaries
    hold them), tok_lens [B], feats list of [B, T_l, C], feat_lens [B, L] -> nce's dict + d_tokens_cf, d_feats, d_enc_w,
    d_enc_b"""
    x = np.asarray(tokens_cf, dtype=np.float64).transpose(0, 2, 1)                  # [B, n, Cn]
    w, bias = np.asarray(enc_w, dtype=np.float64), np.asarray(enc_b, dtype=np.float64)
    tok = x @ w.T + bias
    tl = np.asarray(tok_lens).reshape(-1, 1)
    text = pool([tok], tl)
    video = pool(feats, feat_lens)
    out = nce(text, video, mask, bank, ptr, tau)
    d_tok = pool_grad(out['dtext'], [tok.shape[1]], tl)[0]
    out['d_tokens_cf'] = (d_tok @ w).transpose(0, 2, 1)
    out['d_enc_w'] = np.einsum('bnd,bnc->dc', d_tok, x)
    out['d_enc_b'] = d_tok.sum((0, 1))
    out['d_feats'] = pool_grad(out['dvideo'], [f.shape[1] for f in feats], feat_lens)
    return out
