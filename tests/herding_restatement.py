"""NumPy fp64 restatement of the herding exemplar selection (the contract of `type_sampling = 'herding'`), in two forms:

  herd_literal   the greedy loop over explicit descriptors: at every step the clip whose addition brings the normalised sum
                 of the selected descriptors closest to the normalised class mean, summed over the pyramid levels
  herd_gram      the same selection from the per-level Gram matrices G[l] = Phi[l] Phi[l]^T alone, with the running sums
                 and the expression order of vilco_herd_select (include/vilco_hip.h), so that the device's fp64 arithmetic
                 can be held to it bit for bit

Descriptors: `phis` = list over levels of [N, D_l] arrays whose rows have unit norm.  Ties go to the smallest index.
"""
import numpy as np


def normalise_rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def _pick(cost, taken):
    cost = np.where(np.isnan(cost), np.inf, cost)
    idx = np.flatnonzero(~taken)
    return int(idx[np.argmin(cost[idx])])          # argmin returns the first of equal minima: the smallest index


def literal_costs(phis, sel):
    """cost(i) of adding clip i to the selected list `sel`, for every i, from the descriptors themselves"""
    N = phis[0].shape[0]
    cost = np.zeros(N)
    for phi in phis:
        mu = phi.mean(axis=0)
        mu = mu / np.sqrt((mu * mu).sum())
        S = phi[list(sel)].sum(axis=0) if len(sel) else np.zeros(phi.shape[1])
        v = phi + S[None, :]
        v = v / np.sqrt((v * v).sum(axis=1, keepdims=True))
        cost = cost + ((mu[None, :] - v) ** 2).sum(axis=1)
    return cost


def herd_literal(phis, m):
    phis = [np.asarray(p, dtype=np.float64) for p in phis]
    N = phis[0].shape[0]
    sel, taken = [], np.zeros(N, dtype=bool)
    for _ in range(min(m, N)):
        p = _pick(literal_costs(phis, sel), taken)
        sel.append(p)
        taken[p] = True
    return sel


def gram_matrices(phis, dtype=np.float64):
    """[L, N, N] in fp64; computed in `dtype` (np.float32: NumPy's own fp32 product of the rounded descriptors)"""
    return np.stack([(np.asarray(p, dtype=dtype) @ np.asarray(p, dtype=dtype).T).astype(np.float64) for p in phis], axis=0)


class GramState:
    """the running quantities of vilco_herd_select, updated in its order"""

    def __init__(self, G):
        self.G = G = np.asarray(G, dtype=np.float64)
        L, N, _ = G.shape
        r = np.zeros((L, N))
        for j in range(N):                         # rowsum_i = sum_j G[i][j], j in index order
            r = r + G[:, :, j]
        tot = np.zeros(L)
        for i in range(N):                         # sum(G) = the row sums, in index order
            tot = tot + r[:, i]
        self.a = r / np.sqrt(tot)[:, None]         # a_i = mu . phi_i
        self.d = np.stack([np.diag(g) for g in G], axis=0)
        self.r = np.zeros((L, N))                  # sum_{j in sel} G_ij
        self.s = np.zeros(L)                       # sum_{j, j' in sel} G_jj'
        self.t = np.zeros(L)                       # sum_{j in sel} a_j
        self.sel, self.taken = [], np.zeros(N, dtype=bool)

    def costs(self):
        cost = np.zeros(self.G.shape[1])
        for l in range(self.G.shape[0]):
            num = 2.0 * (self.a[l] + self.t[l])
            den = np.sqrt((self.d[l] + 2.0 * self.r[l]) + self.s[l])
            cost = cost + (2.0 - num / den)
        return cost

    def best(self):
        return _pick(self.costs(), self.taken)

    def add(self, p):
        self.s = (self.s + 2.0 * self.r[:, p]) + self.G[:, p, p]
        self.t = self.t + self.a[:, p]
        self.r = self.r + self.G[:, p, :]
        self.sel.append(int(p))
        self.taken[p] = True


def herd_gram(G, m):
    st = GramState(G)
    for _ in range(min(m, st.G.shape[1])):
        st.add(st.best())
    return st.sel


def synthetic_class(seed, N, dims, spread=0.6):
    """descriptors of one class: a shared direction per level plus clip noise, rows normalised"""
    rng = np.random.default_rng(seed)
    return [normalise_rows(rng.standard_normal(d)[None, :] + spread * rng.standard_normal((N, d))) for d in dims]


def tie_grams(phis, lo, hi):
    """fp64 Gram matrices of descriptors whose clips lo and hi are equal, with rows / columns lo and hi made bit-equal
    (a BLAS product need not return them so)"""
    G = gram_matrices(phis)
    G[:, hi, :] = G[:, lo, :]
    G[:, :, hi] = G[:, :, lo]
    G[:, hi, hi] = G[:, lo, lo]
    G[:, lo, hi] = G[:, hi, lo] = G[:, lo, lo]
    return G
