"""fp64 NumPy restatement of the L2P prompt pool (reference: MQ/libs/cl_methods/prompt.py:47-117) -- what ops.prompt_pool
(csrc/prompt.hip) is held to.  Tied to the imported reference by tests/golden/prompt_pool.npz (test_prompt_cpu.py).

Every selection is a COUNTING RANK, which is what a stable sort produces: an entry's rank is the number of entries that come
first.  Similarities: larger first, equal values by smaller prompt index.  Vote counts: larger first, equal counts by
smaller prompt id.  (torch.topk leaves the order among equal values undefined; this pins it.)  NaN is out of contract.

The reference pads torch.unique's ids / counts to pool_size entries with count 0 before its second topk.  Every row
contributes k distinct ids, so at least k ids have a count >= 1 and a padding entry can never be chosen: no counterpart here."""
import numpy as np

EPS = 1e-12
KEY_MODES = ('mean', 'max', 'mean_max', 'cls')


def rank_desc(v):
    """counting rank of every entry of the 1-D array v: larger value first, equal values by smaller index"""
    v = np.asarray(v)
    i = np.arange(v.shape[0])
    first = (v[None, :] > v[:, None]) | ((v[None, :] == v[:, None]) & (i[None, :] < i[:, None]))
    return first.sum(axis=1)


def top_by_rank(v, k):
    """the indices of the k entries of lowest counting rank, in rank order"""
    r = rank_desc(v)
    out = np.empty(k, dtype=np.int64)
    for i, ri in enumerate(r):
        if ri < k:
            out[ri] = i
    return out


def row_key(x, embedding_key, cls_features=None):
    """-> (xk [B, C], arg [B, C] or None: first position of the maximum)"""
    x = np.asarray(x, dtype=np.float64)
    if embedding_key not in KEY_MODES:
        raise NotImplementedError("Not supported way of calculating embedding keys!")
    if embedding_key == 'cls' and cls_features is not None:
        return np.asarray(cls_features, dtype=np.float64), None
    mean, mx, arg = x.mean(axis=1), x.max(axis=1), x.argmax(axis=1)      # argmax: the first maximum
    if embedding_key == 'mean':
        return mean, None
    if embedding_key == 'mean_max':
        return mx + 2.0 * mean, arg
    return mx, arg


def normalize(v):
    ssq = (v * v).sum(axis=1, keepdims=True)
    return v / np.sqrt(np.maximum(ssq, EPS)), ssq[:, 0]


def select(sim, k, batchwise):
    B, P = sim.shape
    idx = np.stack([top_by_rank(sim[b], k) for b in range(B)])
    if batchwise:
        counts = np.bincount(idx.reshape(-1), minlength=P)
        idx = np.broadcast_to(top_by_rank(counts, k), (B, k)).copy()
    return idx


def forward(x, prompt, key, idx=None, k=None, batchwise=False, embedding_key='mean', cls_features=None):
    x, prompt, key = (np.asarray(t, dtype=np.float64) for t in (x, prompt, key))
    B, L, C = x.shape
    P, length, _ = prompt.shape
    xk, arg = row_key(x, embedding_key, cls_features)
    xn, ssq_x = normalize(xk)
    pn, ssq_k = normalize(key)
    sim = xn @ pn.T
    if idx is None:
        idx = select(sim, k, batchwise)
    idx = np.asarray(idx, dtype=np.int64)
    k = idx.shape[1]
    prompted = np.concatenate([prompt[idx].reshape(B, k * length, C), x], axis=1)
    reduce_sim = 0.0
    for b in range(B):
        for j in range(k):
            reduce_sim += sim[b, idx[b, j]]
    reduce_sim /= B
    return dict(prompt_idx=idx, similarity=sim, prompt_norm=pn, x_embed_norm=xn, selected_key=pn[idx], reduce_sim=reduce_sim,
                prompted_embedding=prompted, total_prompt_len=k * length, _xk=xk, _arg=arg, _ssq_x=ssq_x, _ssq_k=ssq_k)


def _norm_bwd(n, ssq, dn):
    """gradient through v -> v rsqrt(max(sum v^2, eps)); n = the normalised rows"""
    rs = 1.0 / np.sqrt(np.maximum(ssq, EPS))[:, None]
    free = (ssq >= EPS)[:, None]
    return np.where(free, rs * (dn - n * (n * dn).sum(axis=1, keepdims=True)), rs * dn)


def backward(x, prompt, key, fwd, g_prompted, g_reduce_sim, embedding_key='mean', cls_given=False):
    """-> (d_prompt, d_key, d_x) of sum(g_prompted * prompted) + g_reduce_sim * reduce_sim"""
    x, prompt, key, g_prompted = (np.asarray(t, dtype=np.float64) for t in (x, prompt, key, g_prompted))
    B, L, C = x.shape
    P, length, _ = prompt.shape
    idx, xn, pn = fwd['prompt_idx'], fwd['x_embed_norm'], fwd['prompt_norm']
    k = idx.shape[1]
    d_prompt = np.zeros_like(prompt)
    d_pn = np.zeros_like(pn)
    d_xn = np.zeros_like(xn)
    g = float(g_reduce_sim) / B
    for b in range(B):
        for j in range(k):
            p = idx[b, j]
            d_prompt[p] += g_prompted[b, j * length:(j + 1) * length]
            d_pn[p] += g * xn[b]
            d_xn[b] += g * pn[p]
    d_key = _norm_bwd(pn, fwd['_ssq_k'], d_pn)
    d_x = g_prompted[:, k * length:].copy()
    if not (embedding_key == 'cls' and cls_given):
        d_xk = _norm_bwd(xn, fwd['_ssq_x'], d_xn)
        if embedding_key in ('mean', 'mean_max'):
            d_x += (2.0 if embedding_key == 'mean_max' else 1.0) * d_xk[:, None, :] / L
        if embedding_key in ('max', 'mean_max', 'cls'):
            arg = fwd['_arg']
            bb, cc = np.meshgrid(np.arange(B), np.arange(C), indexing='ij')
            np.add.at(d_x, (bb, arg, cc), d_xk)
    return d_prompt, d_key, d_x
