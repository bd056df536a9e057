"""Seeded edge cases of the MQ device evaluators (csrc/evaluate.hip) and their expected results from the fp64 restatement
(metrics_restatement.py), computed once per process and shared by the CPU guards (test_metrics_edges_cpu.py: each case really
contains what it is meant to exercise) and the device tests (test_metrics_edges_gpu.py).  Test infrastructure only.

Detection cases are in the device's index space: video ids are zero-padded decimal strings, so the evaluator's index (ids in
sorted string order) is the number itself, and out-of-range indices reach the kernel as they are written here."""
import functools

import numpy as np

import metrics_restatement as R

NAN, INF = float('nan'), float('inf')


class DetCase:
    def __init__(self, pred, gt, n_cls, n_vid, thr):
        self.vidx, self.cls, self.ts, self.te, self.score = pred
        self.gvid, self.gcls, self.gs, self.ge = gt
        self.vidx = np.asarray(self.vidx, np.int64)
        self.cls = np.asarray(self.cls, np.int64)
        self.n_cls, self.n_vid, self.thr = n_cls, n_vid, np.asarray(thr, np.float64)
        assert len(np.unique(self.gvid)) == n_vid and self.gvid.min() == 0 and self.gvid.max() == n_vid - 1
        self._expected = None

    @property
    def n_pred(self):
        return len(self.cls)

    def expected(self):
        """(ap[n_thr, n_cls], tp[n_thr, n_pred]) of the restatement; computed once, never modified"""
        if self._expected is None:
            ap, tp = R.det_ap(self.vidx, self.cls, self.ts, self.te, self.score, self.gvid, self.gcls, self.gs, self.ge,
                              self.n_cls, self.thr)
            ap.setflags(write=False)
            tp.setflags(write=False)
            self._expected = (ap, tp)
        return self._expected

    def device_gt(self):
        from vilco_amd.utils import metrics as M
        gt = M._DetGT({'video-id': ["%08d" % v for v in self.gvid], 't-start': self.gs, 't-end': self.ge, 'label': self.gcls},
                      {i: i for i in range(self.n_cls)})
        assert gt.n_vid == self.n_vid and gt.n_cls == self.n_cls
        return gt

    def run_device(self):
        from vilco_amd.utils import metrics as M
        return M.det_ap_device(self.device_gt(), self.vidx.astype(np.int32), self.cls.astype(np.int32), self.ts, self.te,
                               self.score, self.thr, want_flags=True)


def _from_random(seed, n_pred, n_cls, n_vid, thr):
    """metrics_restatement.random_case (integer boundaries, one-decimal scores) as a DetCase"""
    pred, gt = R.random_case(np.random.default_rng(seed), n_pred, n_cls, n_vid, True)
    return DetCase(pred, gt, n_cls, n_vid, thr)


# ---------------------------------------------------------------------------------------------------------- detection
MANY_GT = (1, 63, 64, 65, 128, 130)
MANY_GT_PRED = 400


@functools.lru_cache(maxsize=None)
def det_many_gt(n_gt):
    """one class, one video: the match kernel's loop over chunks of 64 GT.  Integer boundaries on a short axis, so tIoU
    values tie inside a chunk and across chunks (most are 0); GT and predictions at least one unit long, so every tIoU is
    in [0, 1] and at threshold 0.0 every GT is eligible for every prediction."""
    rng = np.random.default_rng(100 + n_gt)
    gs = rng.integers(0, 40, n_gt).astype(np.float64)
    ge = gs + rng.integers(1, 7, n_gt)
    n = MANY_GT_PRED
    ts = rng.integers(0, 40, n).astype(np.float64)
    te = ts + rng.integers(1, 7, n)
    score = np.round(rng.uniform(size=n), 2)
    z = np.zeros
    return DetCase((z(n, np.int64), z(n, np.int64), ts, te, score), (z(n_gt, np.int64), z(n_gt, np.int64), gs, ge), 1, 1,
                   [0.0, 0.1, 0.5, 1.0])


N_PRED = (0, 1, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def det_n_pred(n_pred):
    """prediction counts around the radix tile of 256; 3 classes, 4 videos"""
    return _from_random(200 + n_pred, n_pred, 3, 4, np.linspace(0.1, 0.5, 5))


N_CLS = (1, 255, 256, 257, 300)


@functools.lru_cache(maxsize=None)
def det_key_cls(n_cls):
    """class keys of one and two radix digits; labels -1, n_cls and n_cls + 1 are ignored by the kernel"""
    rng = np.random.default_rng(300 + n_cls)
    n_vid, n = 8, 3000
    gcls = np.r_[np.arange(n_cls), rng.integers(0, n_cls, 64)]
    n_gt = len(gcls)
    gvid = np.r_[np.arange(n_vid), rng.integers(0, n_vid, n_gt - n_vid)]
    gs = rng.integers(0, 100, n_gt).astype(np.float64)
    ge = gs + rng.integers(1, 20, n_gt)
    src = rng.integers(0, n_gt, n)
    cls = np.where(rng.uniform(size=n) < 0.9, gcls[src], rng.integers(-1, n_cls + 2, n))
    cls[:9] = [-1, n_cls, n_cls + 1] * 3
    ts = np.round(gs[src] + rng.normal(0, 3, n), 0)
    te = np.maximum(ts, np.round(ge[src] + rng.normal(0, 3, n), 0))
    return DetCase((gvid[src], cls, ts, te, np.round(rng.uniform(size=n), 2)), (gvid, gcls, gs, ge), n_cls, n_vid,
                   np.linspace(0.1, 0.5, 5))


N_VID = (1, 255, 256, 65535, 65536, 70000)


@functools.lru_cache(maxsize=None)
def det_key_vid(n_vid):
    """video keys of one, two and three radix digits, one GT per video; predictions in video n_vid - 1 and in videos outside
    [0, n_vid), which are FPs at every threshold"""
    rng = np.random.default_rng(400 + n_vid)
    n, n_cls = 2000, 2
    gvid = rng.permutation(n_vid)
    gcls = rng.integers(0, n_cls, n_vid)
    gs = rng.integers(0, 100, n_vid).astype(np.float64)
    ge = gs + rng.integers(1, 20, n_vid)
    src = rng.integers(0, n_vid, n)
    src[:40] = np.flatnonzero(gvid == n_vid - 1)[0]
    vidx = gvid[src].astype(np.int64)
    cls = np.where(rng.uniform(size=n) < 0.9, gcls[src], rng.integers(0, n_cls, n))
    outside = [-1, n_vid, n_vid + 1, n_vid + 255, n_vid + 256, (1 << 24) - 1, (1 << 24), (1 << 31) - 1, -(1 << 31)]
    vidx[40:40 + 4 * len(outside)] = outside * 4
    ts = np.round(gs[src] + rng.normal(0, 3, n), 0)
    te = np.maximum(ts, np.round(ge[src] + rng.normal(0, 3, n), 0))
    return DetCase((vidx, cls, ts, te, np.round(rng.uniform(size=n), 2)), (gvid, gcls, gs, ge), n_cls, n_vid,
                   np.linspace(0.1, 0.5, 5))


THR_SETS = {"one": [0.3], "sixteen": np.linspace(0.05, 0.95, 16), "above_one": [0.5, 1.0, 1.5]}


@functools.lru_cache(maxsize=None)
def det_thresholds(name):
    """1 and 16 thresholds (the argument block holds 16), and a threshold above 1, which only a NaN tIoU can still match:
    every 20th prediction has a NaN start"""
    c = _from_random(500, 600, 3, 4, THR_SETS[name])
    c.ts = c.ts.copy()
    c.ts[::20] = NAN
    return c


@functools.lru_cache(maxsize=None)
def det_special():
    """scores from {NaN, +inf, -inf, 0.0, -0.0, 0.5}; prediction boundaries with NaN, +-inf, end < start and zero length; GT
    rows of zero length.  2 classes, 3 videos, 6 GT per (class, video) group; threshold 0.0 separates the negative tIoU of a
    reversed prediction from -0.0 and 0.0"""
    rng = np.random.default_rng(600)
    n_cls, n_vid, per, n = 2, 3, 6, 720
    gcls = np.repeat(np.arange(n_cls), n_vid * per)
    gvid = np.tile(np.repeat(np.arange(n_vid), per), n_cls)
    n_gt = len(gcls)
    gs = rng.integers(0, 30, n_gt).astype(np.float64)
    ge = gs + rng.integers(0, 6, n_gt)                          # length 0 included
    ge[::per] = gs[::per]                                        # at least one zero-length GT per group
    src = rng.integers(0, n_gt, n)
    ts = np.round(gs[src] + rng.normal(0, 2, n), 0)
    te = np.round(ge[src] + rng.normal(0, 2, n), 0)              # end < start happens
    kind = rng.integers(0, 12, n)
    ts[kind == 0] = NAN
    te[kind == 1] = NAN
    ts[kind == 2] = -INF
    te[kind == 3] = INF
    ts[kind == 4] = INF
    te[kind == 5] = -INF
    te[kind == 6] = ts[kind == 6]                                # zero length
    z = kind == 7
    ts[z], te[z] = gs[src][z], gs[src][z]                        # zero length at a GT's start (0/0 on a zero-length GT)
    r = kind == 8
    ts[r], te[r] = ge[src][r] + 1, gs[src][r]                    # reversed
    score = np.array([NAN, INF, -INF, 0.0, -0.0, 0.5])[rng.integers(0, 6, n)]
    return DetCase((gvid[src], gcls[src], ts, te, score), (gvid, gcls, gs, ge), n_cls, n_vid, [0.0, 0.1, 0.3, 0.5, 1.0])


@functools.lru_cache(maxsize=None)
def det_class_without_gt():
    """the class index has one class more than the GT uses and predictions carry that label.  The reference builds its class
    index from the GT labels (metrics.py: load_gt_seg_from_json; wrapper_compute_average_precision's get_group(cidx) would
    raise otherwise) and cannot reach this state; the documented value is AP 0"""
    pred, gt = R.random_case(np.random.default_rng(700), 500, 2, 4, True)
    cls = np.asarray(pred[1]).copy()
    cls[::3] = 2
    return DetCase((pred[0], cls, pred[2], pred[3], pred[4]), gt, 3, 4, np.linspace(0.1, 0.5, 5))


# ---------------------------------------------------------------------------------------------------------- retrieval
def pack_groups(groups):
    """[(pred [n, 2], gt [m, 2])] -> the flat columns of vilco_retrieval_hits"""
    groups = [(np.asarray(p, np.float64).reshape(-1, 2), np.asarray(g, np.float64).reshape(-1, 2)) for p, g in groups]
    ps = np.concatenate([p[:, 0] for p, _ in groups])
    pe = np.concatenate([p[:, 1] for p, _ in groups])
    pcnt = np.array([len(p) for p, _ in groups], np.int32)
    poff = np.r_[0, np.cumsum(pcnt)[:-1]].astype(np.int32)
    gs = np.concatenate([g[:, 0] for _, g in groups])
    ge = np.concatenate([g[:, 1] for _, g in groups])
    goff = np.r_[0, np.cumsum([len(g) for _, g in groups])].astype(np.int32)
    return ps, pe, poff, pcnt, gs, ge, goff


def run_device_hits(groups, tious, ranks):
    from vilco_amd.utils import metrics as M
    return M.retrieval_hits_device(*pack_groups(groups), tious, ranks)


CUT_GT = (1, 64, 65, 129)
CUT_RANKS = (1, 5)
CUT_TIOUS = (0.1, 0.2, 0.3, 0.4, 0.5)


def cutoff_group(n_gt, count):
    """GT k = [100 k, 100 k + 10].  `count` predictions: far-away fillers, at position 0 an anchor that overlaps GT 0 by 0.15
    (a hit at threshold 0.1 only), and LAST the target, an exact copy of GT n_gt - 1 -- the only prediction that overlaps it
    (for n_gt == 1, by more than 0.15)."""
    gt = np.stack([100.0 * np.arange(n_gt), 100.0 * np.arange(n_gt) + 10.0], 1)
    pred = np.stack([1e6 + 2.0 * np.arange(count), 1e6 + 2.0 * np.arange(count) + 1.0], 1)
    if count:
        pred[0] = [0.0, 1.5]
        pred[-1] = gt[-1]
    return pred, gt


@functools.lru_cache(maxsize=None)
def ret_cutoffs(n_gt):
    """{(rank, count): group} with count in {0, 1, r n - 1, r n, r n + 1}: the target sits inside the first r * n_gt rows, at
    the last admitted position, and at the first excluded one"""
    out = {}
    for r in CUT_RANKS:
        for count in sorted({0, 1, r * n_gt - 1, r * n_gt, r * n_gt + 1}):
            out[(r, count)] = cutoff_group(n_gt, count)
    return out


LIMIT_RANKS = (0, 1, 2, 3, 5, 8, 13, 100)
LIMIT_TIOUS = tuple(np.linspace(0.05, 0.95, 16))


@functools.lru_cache(maxsize=None)
def ret_limits():
    """8 ranks (0 and 100 among them) and 16 thresholds; groups of 1..5 GT with 0..30 predictions and one group of 70 GT"""
    rng = np.random.default_rng(800)
    groups = []
    for k in range(200):
        m = 70 if k == 17 else int(rng.integers(1, 6))
        gs = np.round(rng.uniform(0, 50, m), 0)
        g = np.stack([gs, gs + np.round(rng.uniform(1, 10, m), 0)], 1)
        n = int(rng.integers(0, 31))
        ps = np.round(rng.uniform(0, 50, n), 0)
        groups.append((np.stack([ps, ps + np.round(rng.uniform(0, 10, n), 0)], 1), g))
    return tuple(groups)


# name -> (predictions, GT); one GT (0, 10) unless the GT itself is the edge
RET_DEGENERATE = {
    "pred_nan_start": ([(NAN, 10)], [(0, 10)]),                  # the ternary max / min took the GT side: overlap 1.0
    "pred_nan_end": ([(0, NAN)], [(0, 10)]),
    "pred_nan_both": ([(NAN, NAN)], [(0, 10)]),
    "gt_nan_start": ([(0, 10)], [(NAN, 10)]),
    "gt_nan_end": ([(0, 10)], [(0, NAN)]),
    "pred_neg_inf_start": ([(-INF, 10)], [(0, 10)]),             # 10 / inf = 0
    "pred_inf_end": ([(0, INF)], [(0, 10)]),
    "pred_all_axis": ([(-INF, INF)], [(0, 10)]),
    "pred_at_inf": ([(INF, INF)], [(0, 10)]),
    "pred_at_neg_inf": ([(-INF, -INF)], [(0, 10)]),
    "pred_inf_reversed": ([(INF, -INF)], [(0, 10)]),
    "gt_inf_end": ([(0, 10)], [(0, INF)]),                       # inf / inf
    "zero_width_hull": ([(5, 5)], [(5, 5)]),                     # 0 / 0
    "nan_then_exact": ([(NAN, 10), (0, 10)], [(0, 10)]),         # rank 1 sees the NaN row only, rank 5 the hit
    "exact_then_nan": ([(0, 10), (NAN, 10)], [(0, 10)]),         # a NaN row does not undo a hit
    "nan_among_gt": ([(0, 10), (20, NAN)], [(0, 10), (NAN, 30), (20, 30)]),
}
