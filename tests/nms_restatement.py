"""TEST INFRASTRUCTURE ONLY -- oracle/nms_oracle.py's `nms` and `softnms` with the INNER loop vectorised.

oracle/nms_oracle.py walks every (pick, candidate) pair in Python, which caps it near 1500 candidates; the edges of
csrc/nms.hip (a 4096-candidate chunk, 16000 deaths in one pick, 30720 / 65536 candidates per class) lie far beyond that.
Here the outer loop stays (one iteration per kept candidate / per pick) and the inner one is a numpy expression over float32
arrays with the same operations in the same order:

    area  = x2 - x1 + 1e-6f
    inter = max(0, min(ix2, jx2) - max(ix1, jx1))
    ovr   = inter / ((ai + aj) - inter)
    w     = expf_libm(-(ovr * ovr) / sigma)            (method 2; nms_oracle.expf_libm == glibc expf)

so indices AND decayed scores are the oracle's bit for bit (tests/test_nms_restatement_cpu.py pins that, and pins both to the
reference build where it is present).

The reference removes a dead candidate by overwriting it with the last one and visiting the slot again (nms_cpu.cpp:146-154).
The moved element has not been decayed yet, so every element is decayed exactly once and the final array is: the k-th hole
(ascending) below the new length takes the k-th survivor counted from the end.  The kernels rely on that equivalence;
`softnms_v` is written that way too, so the CPU test against the sequential oracle pins the equivalence itself.
"""
import numpy as np

from oracle import nms_oracle

f32 = np.float32
EPS = f32(1e-6)


def _prep(segs, scores):
    segs = np.asarray(segs, dtype=f32).reshape(-1, 2)
    return segs[:, 0].copy(), segs[:, 1].copy(), np.asarray(scores, dtype=f32).copy()


def _iou(ix1, ix2, ia, jx1, jx2, ja):
    inter = np.maximum(f32(0), np.minimum(ix2, jx2) - np.maximum(ix1, jx1))
    return inter / ((ia + ja) - inter)


def iou_pair(a, b):
    """the oracle's IoU of two segments as one float32"""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    return f32(_iou(a[0], a[1], f32(a[1] - a[0] + EPS), b[0], b[1], f32(b[1] - b[0] + EPS)))


def nms_v(segs, scores, iou_threshold, return_ranks=False):
    """hard NMS: kept input indices in descending-score order (stable).  return_ranks: also the rank (position in that
    order) of every keep -- rank // 4096 is the chunk of nms_sweep_kernel that keeps it."""
    x1, x2, sc = _prep(segs, scores)
    n = x1.size
    order = np.argsort(-sc, kind="stable")
    x1, x2 = x1[order], x2[order]
    ar = x2 - x1 + EPS
    thr = f32(iou_threshold)
    alive = np.ones(n, dtype=bool)
    for i in range(n):
        if not alive[i]:
            continue
        ovr = _iou(x1[i], x2[i], ar[i], x1[i + 1:], x2[i + 1:], ar[i + 1:])
        alive[i + 1:] &= ~(ovr >= thr)
    ranks = np.nonzero(alive)[0]
    inds = order[ranks].astype(np.int64)
    return (inds, ranks) if return_ranks else inds


def softnms_v(segs, scores, iou_threshold, sigma, min_score, method, max_num=0):
    """soft NMS -> (inds[K], dets[K, 3], deaths_per_pick[K]); deaths_per_pick[i] = candidates removed after pick i."""
    x1, x2, sc = _prep(segs, scores)
    n = x1.size
    ar = x2 - x1 + EPS
    inds = np.arange(n, dtype=np.int64)
    arrays = (x1, x2, sc, ar, inds)
    dets = np.zeros((n, 3), dtype=f32)
    deaths = []
    thr, sigma, min_score = f32(iou_threshold), f32(sigma), f32(min_score)
    nsegs, i = n, 0
    while i < nsegs:
        if max_num > 0 and i >= max_num:
            break
        mp = i + int(np.argmax(sc[i:nsegs]))                 # the first maximum
        for a in arrays:
            a[i], a[mp] = a[mp], a[i]
        dets[i] = (x1[i], x2[i], sc[i])
        first = i + 1
        span = nsegs - first
        nd = 0
        if span > 0:
            s = slice(first, nsegs)
            ovr = _iou(x1[i], x2[i], ar[i], x1[s], x2[s], ar[s])
            if method == 0:
                w = np.where(ovr >= thr, f32(0), f32(1))
            elif method == 1:
                w = np.where(ovr >= thr, f32(1) - ovr, f32(1))
            elif method == 2:
                w = nms_oracle.expf_libm(-(ovr * ovr) / sigma)
            else:
                w = np.ones(span, dtype=f32)
            sc[s] = sc[s] * w.astype(f32)
            dead = sc[s] < min_score
            nd = int(dead.sum())
            if nd:
                n_alive = span - nd
                holes = first + np.nonzero(dead[:n_alive])[0]                       # ascending, below the new length
                surv = first + n_alive + np.nonzero(~dead[n_alive:])[0]             # survivors at or beyond it
                assert holes.size == surv.size
                for a in arrays:
                    a[holes] = a[surv[::-1]]
                nsegs = first + n_alive
        deaths.append(nd)
        i += 1
    return inds[:i].copy(), dets[:i].copy(), np.asarray(deaths, dtype=np.int64)
