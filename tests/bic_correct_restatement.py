"""float64 NumPy restatement of BiC's bias correction (MQ/libs/modeling/meta_archs.py:26-35, :821-836) and its gradients:
what ops.bic_correct (csrc/bic.hip) is held to.

    y[r, c]   = alpha[s(c)] * x[r, c] + beta[s(c)]          s(c) = i with splits[i-1] <= c < splits[i]
    dx[r, c]  = alpha[s(c)] * dy[r, c]
    dalpha_i  = sum over all rows r and the columns c of split i of dy[r, c] * x[r, c]
    dbeta_i   = the same sum of dy[r, c]

x is [..., C]; every leading index is a row, none is special (separator rows and rows past a clip's valid length get the
affine like the rest).  The `*_terms` functions return what the fp32 error bounds of the tests are made of."""
import numpy as np


def column_split(splits, C):
    """s(c) for c < C; raises on a table that is not strictly increasing cumulative ends finishing at C"""
    ends = [int(v) for v in splits]
    if not ends or ends[0] <= 0 or any(b <= a for a, b in zip(ends, ends[1:])) or ends[-1] != C:
        raise ValueError("splits %s are not cumulative ends of %d columns" % (ends, C))
    s = np.zeros(C, dtype=np.int64)
    lo = 0
    for i, hi in enumerate(ends):
        s[lo:hi] = i
        lo = hi
    return s


def forward(x, splits, alphas, betas):
    x = np.asarray(x, dtype=np.float64)
    s = column_split(splits, x.shape[-1])
    a, b = np.asarray(alphas, dtype=np.float64)[s], np.asarray(betas, dtype=np.float64)[s]
    return a * x + b


def forward_terms(x, splits, alphas, betas):
    """|alpha x| + |beta| per element"""
    x = np.asarray(x, dtype=np.float64)
    s = column_split(splits, x.shape[-1])
    return np.abs(np.asarray(alphas, dtype=np.float64)[s] * x) + np.abs(np.asarray(betas, dtype=np.float64)[s])


def dx(dy, splits, alphas):
    dy = np.asarray(dy, dtype=np.float64)
    return np.asarray(alphas, dtype=np.float64)[column_split(splits, dy.shape[-1])] * dy


def dparams(dy, x, splits):
    """-> (dalpha [S], dbeta [S], sum |dy x| [S], sum |dy| [S])"""
    dy, x = np.asarray(dy, dtype=np.float64), np.asarray(x, dtype=np.float64)
    C = x.shape[-1]
    s = column_split(splits, C)
    dy2, x2 = dy.reshape(-1, C), x.reshape(-1, C)
    S = len(splits)
    out = [np.zeros(S) for _ in range(4)]
    for i in range(S):
        cols = s == i
        out[0][i] = (dy2[:, cols] * x2[:, cols]).sum()
        out[1][i] = dy2[:, cols].sum()
        out[2][i] = np.abs(dy2[:, cols] * x2[:, cols]).sum()
        out[3][i] = np.abs(dy2[:, cols]).sum()
    return tuple(out)
