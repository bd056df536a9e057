"""Dark Experience Replay's step term in float64, written from its definition (include/vilco_hip.h: vilco_der_desc):

  S = sum_{b: rec} sum_l sum_{t < V_bl} sum_{y < n_b} (x[b, row_l + t, y] - z_b[off_l + t, y])^2
  N = sum_{b: rec} n_b sum_l V_bl
  loss = alpha S / N   (0 when N == 0),      d loss / d x = 2 alpha g (x - z) / N on the compared elements, 0 elsewhere

Plain loops over rows, levels and positions; nothing is shared with the kernel or with cl_methods.der.der_term."""
import torch


def der_term(x, level_row, level_T, valid, records, alpha, g_out=1.0):
    """x [B, R, C]; valid [B][L] valid lengths; records[b] = None or [sum T_l, n_b] (1 <= n_b <= C, anything else: no record).
    -> (loss float, N int, gradient float64 [B, R, C], mask bool [B, R, C] of the compared elements, S float)"""
    x = x.detach().double().cpu()
    B, R, C = x.shape
    grad = torch.zeros(B, R, C, dtype=torch.float64)
    mask = torch.zeros(B, R, C, dtype=torch.bool)
    S, N = 0.0, 0
    for b in range(B):
        z = records[b]
        if z is None:
            continue
        z = z.detach().double().cpu()
        n_b = z.shape[1]
        if n_b < 1 or n_b > C:
            continue
        off = 0
        for l in range(len(level_T)):
            V = min(max(int(valid[b][l]), 0), int(level_T[l]))
            for t in range(V):
                row = int(level_row[l]) + t
                d = x[b, row, :n_b] - z[off + t]
                S += float((d * d).sum())
                grad[b, row, :n_b] = d
                mask[b, row, :n_b] = True
            N += n_b * V
            off += int(level_T[l])
    if N == 0:
        return 0.0, 0, grad * 0.0, mask, 0.0
    return float(alpha) * S / N, N, grad * (2.0 * float(alpha) * float(g_out) / N), mask, S
