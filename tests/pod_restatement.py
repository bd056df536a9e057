"""PODNet's pooled feature distillation over a one-dimensional pyramid and its gradient, restated in float64 from the
formulas (not from vilco_amd.cl_methods.pod.pod_term, and without autograd):

  p[c] = sum_{t<V} h[t][c]^2   q[t] = sum_c h[t][c]^2   v = [p ; q]   n = max(||v||, 1e-12)   u = v / n
  r = the first C + V entries of the record's slice of the level ([p (C) ; q (T_l)], levels end to end)
  dist = ||u - r||   loss = scale / (L N_rec) sum_b sum_l dist   (0 when N_rec == 0; a level with V = 0 adds 0)
  g_u = w (u - r) / max(dist, 1e-12)   w = g_out scale / (L N_rec)   g_v = (g_u - u (u . g_u)) / n
  d_h[t][c] = 2 h[t][c] (g_v[c] + g_v[C + t]) for t < V, 0 elsewhere."""
import torch


def record_offsets(level_T, C):
    off, e = [], 0
    for T in level_T:
        off.append(e)
        e += int(C) + int(T)
    return off, e


def pooled(h, V):
    """h [T, C] float64 -> v = [p ; q] over the first V rows"""
    s = h[:V] * h[:V]
    return torch.cat([s.sum(0), s.sum(1)])


def make_record(feats_b, valid_b):
    """the normalised record of one clip: feats_b = per-level [T_l, C]; entries at t >= V are 0 -> float64 [sum (C + T_l)]"""
    out = []
    for h, V in zip(feats_b, valid_b):
        h = h.double()
        T, C = h.shape
        V = max(0, min(int(V), T))
        v = pooled(h, V)
        u = v / max(float(v.norm()), 1e-12)
        out.append(torch.cat([u, torch.zeros(T - V, dtype=torch.float64)]))
    return torch.cat(out)


def pod_term(feats, valid, records, scale, g_out=1.0):
    """feats: list of L tensors [B, T_l, C]; valid [B][L]; records: per row None or the record [sum (C + T_l)].
    -> dict(loss, n_rec, grads [L x [B, T_l, C] float64], dist [B][L], norm [B][L] (||v|| clamped), gv {(b, l): g_v},
            compared [L x bool [B, T_l]])"""
    feats = [f.detach().double().cpu() for f in feats]
    B, L, C = feats[0].shape[0], len(feats), feats[0].shape[2]
    off, _ = record_offsets([f.shape[1] for f in feats], C)
    n_rec = sum(1 for r in records if r is not None)
    grads = [torch.zeros_like(f) for f in feats]
    compared = [torch.zeros(f.shape[:2], dtype=torch.bool) for f in feats]
    dist = [[0.0] * L for _ in range(B)]
    norm = [[None] * L for _ in range(B)]
    gv = {}
    w = float(g_out) * float(scale) / (L * n_rec) if n_rec else 0.0
    total = 0.0
    for b in range(B):
        if records[b] is None:
            continue
        rec = records[b].detach().double().cpu().reshape(-1)
        for l in range(L):
            h = feats[l][b]
            T = h.shape[0]
            V = max(0, min(int(valid[b][l]), T))
            if V == 0:
                continue
            v = pooled(h, V)
            n = max(float(v.norm()), 1e-12)
            u = v / n
            e = u - rec[off[l]:off[l] + C + V]
            d = float(e.norm())
            g_u = w * e / max(d, 1e-12)
            g_v = (g_u - u * float(u @ g_u)) / n
            grads[l][b, :V] = 2.0 * h[:V] * (g_v[:C][None, :] + g_v[C:][:, None])
            compared[l][b, :V] = True
            dist[b][l], norm[b][l], gv[(b, l)] = d, n, g_v
            total += d
    loss = float(scale) / (L * n_rec) * total if n_rec else 0.0
    return dict(loss=loss, n_rec=n_rec, grads=grads, dist=dist, norm=norm, gv=gv, compared=compared)
