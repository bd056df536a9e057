"""fp64 restatement of the distillation term of iCaRL / BiC and its gradient, in the layout ops.cl_distill takes
(include/vilco_hip.h: vilco_distill_desc; reference MQ/libs/modeling/meta_archs.py:1482-1519).

  mode 0 (iCaRL): 0.01 * sum_l (1/T_l) sum_t sum_{y < n_known} bce(x[clip, t, y], p_l[t, y]),
                  bce(x, p) = max(x, 0) - x p + log1p(exp(-|x|))
  mode 1 (BiC):   scale * sum_l -(1/T_l) sum_t sum_{y < n_known} p_l[t, y] log_softmax(x[clip, t, :n_known] / 2)[y]

logits [B, R, C] with level l in rows level_row[l] .. level_row[l] + level_T[l]; targets [sum T_l, ldt], levels end to end.
The gradients are written out by hand (no autograd), so that the formulas themselves are what the kernel is held to."""
import torch


def distill_loss(logits, level_row, level_T, targets, n_known, mode, scale, clip=0):
    x, p = logits.double(), targets.double()
    total, first = torch.zeros((), dtype=torch.float64), 0
    for r, T in zip(level_row, level_T):
        xl, pl = x[clip, r:r + T, :n_known], p[first:first + T, :n_known]
        if mode == 0:
            bce = xl.clamp(min=0) - xl * pl + torch.log1p(torch.exp(-xl.abs()))
            total = total + 0.01 * bce.sum() / T
        else:
            z = xl / 2
            logp = z - torch.logsumexp(z, dim=1, keepdim=True)
            total = total + scale * -(pl * logp).sum() / T
        first += T
    return total


def distill_grad(logits, level_row, level_T, targets, n_known, mode, scale, clip=0, g=1.0):
    """d (g * loss) / d logits: zero outside [clip, level rows, :n_known]"""
    x, p = logits.double(), targets.double()
    d, first = torch.zeros_like(x), 0
    for r, T in zip(level_row, level_T):
        xl, pl = x[clip, r:r + T, :n_known], p[first:first + T, :n_known]
        if mode == 0:
            d[clip, r:r + T, :n_known] = g * 0.01 / T * (torch.sigmoid(xl) - pl)
        else:
            sm = torch.softmax(xl / 2, dim=1)
            d[clip, r:r + T, :n_known] = g * scale / T * 0.5 * (sm * pl.sum(dim=1, keepdim=True) - pl)
        first += T
    return d
