"""Float64 numpy restatement of the candidate decode (vilco_decode, include/vilco_hip.h; the reference's
PtTransformer.inference_single_video, MQ meta_archs.py:1594-1692), the inputs of its edge tests and the comparison they
share.  No torch device code and no call into vilco_amd.

Per level l (rows row0[l] .. row0[l] + lens[l] - 1 of the shared row layout, flat index e = position * C + class):
  prob = sigmoid(logit);  admitted when prob > thresh, strictly;  of those the `topk` first in the order
  (float32(prob) descending, e ascending);  segment = (t - off_l * stride, t + off_r * stride);  kept when
  right - left > dur.  The duration filter comes AFTER the cut: a slot it frees stays empty.  Output in index order.

A float64 reference decides a discrete selection only on inputs where no decision hangs on the last bits of an fp32
sigmoid.  `assert_rankable` is that precondition and every builder below calls it: inside a level two float32-rounded
probabilities are bit-equal from equal logits or from saturation to 1.0f (a tie on any implementation) or >= 16 fp32 ulps apart, no
probability is within 16 ulps of the threshold unless it equals it by construction (logit 0 -> 0.5; logit >= 18 -> 1.0f), and
right - left is exactly `dur` in fp32 arithmetic or >= 1e-3 relative away from it.

tests/test_decode_restatement_cpu.py holds `decode` to the tensor-expression branch of inference_single_video and BAR_P to
its measurement; tests/test_decode_edges_gpu.py holds the HIP kernel to `decode`."""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of fp32
ULPS = 16                       # the separation assert_rankable demands
THRESH, DUR = 0.001, 0.05       # the recipes' pre_nms_thresh and duration_thresh

# Scores: 4 x the worst relative error of the fp32 formula 1 / (1 + expf(-x)), evaluated by numpy in float32, against its
# float64 evaluation over every grid and cluster value (measure_bar_p; the factor and the convention are BARS' of
# glue_restatement.py: the kernel's expf is another implementation).  test_decode_restatement_cpu.py recomputes the
# measurement and holds the constant between 1 x and 8 x of it.
BAR_P = 4 * 2.04e-07            # measured 2.04e-07, x 4


def f32(x):
    return np.asarray(x, dtype=np.float32)


def sigmoid64(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def prob32(x):
    """the ranking key: the float64 sigmoid rounded to fp32"""
    with np.errstate(under="ignore"):
        return sigmoid64(x).astype(np.float32)


def bits(p):
    """fp32 bit patterns as int64: for non-negative values their differences are distances in ulps"""
    return np.ascontiguousarray(p, dtype=np.float32).view(np.int32).astype(np.int64)


def segments64(offsets, points, rows):
    o, p = np.asarray(offsets, np.float64)[rows], np.asarray(points, np.float64)[rows]
    with np.errstate(invalid="ignore"):
        return p[:, 0] - o[:, 0] * p[:, 3], p[:, 0] + o[:, 1] * p[:, 3]


def decode(logits, offsets, points, row0, lens, C, topk, thresh, dur):
    """-> per level (index int64, prob float64, left float64, right float64, label int64), in index order"""
    logits = np.asarray(logits, np.float32).reshape(-1, C)
    th, du = np.float32(thresh), np.float64(np.float32(dur))
    out = []
    for r0, ln in zip(row0, lens):
        r0, ln = int(r0), int(ln)
        x = logits[r0:r0 + ln].reshape(-1)
        p64, key = sigmoid64(x), prob32(x)
        with np.errstate(invalid="ignore"):
            idx = np.nonzero(key > th)[0]
        order = np.lexsort((idx, -key[idx].astype(np.float64)))          # last key first: prob descending, then index
        idx = np.sort(idx[order[:topk]])
        left, right = segments64(offsets, points, r0 + idx // C)
        with np.errstate(invalid="ignore"):
            ok = (right - left) > du
        idx = idx[ok]
        out.append((idx.astype(np.int64), p64[idx], left[ok], right[ok], (idx % C).astype(np.int64)))
    return out


def assert_rankable(logits, thresh, row0, lens, offsets=None, points=None, dur=None):
    """AssertionError unless a float64 reference and any fp32 sigmoid within a few ulps of it take the same decisions"""
    C = logits.shape[1]
    tb = int(bits([thresh])[0])
    for l, (r0, ln) in enumerate(zip(row0, lens)):
        r0, ln = int(r0), int(ln)
        x = np.asarray(logits, np.float32)[r0:r0 + ln].reshape(-1)
        p = prob32(x)
        fin = ~np.isnan(p)
        b = bits(p[fin])
        u = np.unique(b)
        gap = np.diff(u)
        assert gap.size == 0 or int(gap.min()) >= ULPS, "level %d: two probabilities %d ulps apart" % (l, int(gap.min()))
        # bit-equal probabilities are a tie on every implementation only when the logits are equal too (or saturate to 1.0f)
        pairs = np.unique(np.stack([b, bits(x[fin])], 1), axis=0)
        below_one = pairs[:, 0] != int(bits([1.0])[0])
        assert np.unique(pairs[below_one, 0]).size == int(below_one.sum()), "level %d: two probabilities 0 ulps apart from different logits" % l
        near = np.abs(b - tb) < ULPS
        by_construction = (b == tb) & ((x[fin] == 0) | (x[fin] >= 18))
        assert not bool((near & ~by_construction).any()), "level %d: a probability within %d ulps of the threshold" % (l, ULPS)
        if offsets is not None and ln > 0:
            rows = np.arange(r0, r0 + ln)
            left, right = segments64(offsets, points, rows)
            d, du = right - left, np.float64(np.float32(dur))
            o, q = f32(offsets)[rows], f32(points)[rows]
            with np.errstate(invalid="ignore"):
                d32 = (q[:, 0] + o[:, 1] * q[:, 3]) - (q[:, 0] - o[:, 0] * q[:, 3])
                fine = np.isnan(d) | ((d == du) & (d32 == np.float32(dur))) | (np.abs(d - du) >= 1e-3 * abs(du))
            assert bool(fine.all()), "level %d: a segment length within 1e-3 of the duration threshold" % l


# ------------------------------------------------------------------------------------------------ values
GRID_N, CLUSTER_N = 120000, 2000
SATURATED = [18.0, 20.0, 25.0, 30.0, np.inf]          # all exactly 1.0f
EXCLUDED = [-100.0, -np.inf, np.nan]


def grid(i):
    """-8 + i 1e-4, i < 120 000: neighbours' probabilities are >= 29 fp32 ulps apart"""
    return (-8.0 + np.asarray(i, np.float64) * 1e-4).astype(np.float32)


def cluster(i):
    """1 + i 64 2^-23, i < 2000: neighbours 25-26 ulps apart, about ten values per top-24-bit prefix of the probability"""
    return (1.0 + np.asarray(i, np.float64) * 64 * 2.0 ** -23).astype(np.float32)


def grid_pool(thresh, lo=0, hi=GRID_N):
    """the grid indices in [lo, hi) whose probability keeps ULPS from the threshold"""
    i = np.arange(lo, hi)
    return i[np.abs(bits(prob32(grid(i))) - int(bits([thresh])[0])) >= ULPS]


def measure_bar_p():
    """worst relative error of numpy's float32 1 / (1 + exp(-x)) against float64 over the grid and the cluster"""
    x = np.concatenate([grid(np.arange(GRID_N)), cluster(np.arange(CLUSTER_N))])
    p = np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))
    assert p.dtype == np.float32
    w = sigmoid64(x)
    return float((np.abs(p.astype(np.float64) - w) / w).max())


# ------------------------------------------------------------------------------------------------ cases
def rng(seed):
    return np.random.RandomState(seed)


def level_rows(n_rows, stride, g, integer_t=False):
    """offsets uniform in [0.25, 3) (every length >= 0.5 stride: far from DUR), t = (r + 0.37) stride"""
    off = g.uniform(0.25, 3.0, (n_rows, 2)).astype(np.float32)
    t = (np.arange(n_rows) + (0.0 if integer_t else 0.37)) * stride
    pts = np.stack([t, np.zeros(n_rows), np.full(n_rows, 1e4), np.full(n_rows, float(stride))], 1).astype(np.float32)
    return off, pts


def make_case(logits, C, g, thresh=THRESH, dur=DUR, offsets=None, points=None, row0=None, lens=None, alloc=None):
    """a case dict; one level over all rows unless row0 / lens / alloc (rows allotted to a level) say otherwise"""
    logits = f32(logits).reshape(-1, C)
    R = logits.shape[0]
    if offsets is None:
        offsets, points = level_rows(R, 1.0, g)
    case = dict(logits=logits, offsets=f32(offsets), points=f32(points), C=C, thresh=thresh, dur=dur,
                row0=np.asarray([0] if row0 is None else row0, np.int32), lens=np.asarray([R] if lens is None else lens, np.int32))
    case["alloc"] = np.asarray(case["lens"] if alloc is None else alloc, np.int32)
    assert_rankable(case["logits"], thresh, case["row0"], case["lens"], case["offsets"], case["points"], dur)
    return case


def expected(case, topk):
    return decode(case["logits"], case["offsets"], case["points"], case["row0"], case["lens"], case["C"], topk,
                  case["thresh"], case["dur"])


def totals(case):
    """per level: how many probabilities pass the threshold"""
    th = np.float32(case["thresh"])
    with np.errstate(invalid="ignore"):
        return [int((prob32(case["logits"][int(r):int(r) + int(n)]) > th).sum()) for r, n in zip(case["row0"], case["lens"])]


def draw_grid(g, n, thresh=THRESH, repeat=False, lo=0, hi=GRID_N):
    pool = grid_pool(thresh, lo, hi)
    return grid(g.choice(pool, n, replace=repeat))


# n = len C on both sides of every multiple of 1024 that matters to per = ceil(n / 1024) and to the grid-stride loops
CHUNK_N = {1: [1, 1023, 1024, 1025, 2047, 4400, 5 * 1024 + 1],
           7: [7, 1022, 1029, 2044, 2051, 4396, 4403, 5117, 5124],
           110: [110, 990, 1100, 1980, 2090, 4400, 5060, 5170]}
CHUNK_CASES = [(C, n) for C in (1, 7, 110) for n in CHUNK_N[C]]


def chunk_case(C, n):
    assert n % C == 0
    g = rng(100 + n + C)
    return make_case(draw_grid(g, n), C, g)


def chunk_topks(n):
    """no cut, and the cut at n // 3 (n < 3: 1, the smallest topk the ABI takes)"""
    return [n + 3, max(1, n // 3)]


CUT_N, CUT_C = 4400, 110


def cut_case():
    """n = 4400, about a tenth of it below the threshold: total < n"""
    g = rng(7)
    case = make_case(draw_grid(g, CUT_N), CUT_C, g)
    total = totals(case)[0]
    assert 1 < total < CUT_N
    return case, [1, total - 1, total, total + 1, CUT_N + 5]


TIE_M, TIE_ABOVE = 40, 1500
TIE_NEED = [1, 20, TIE_M - 1, TIE_M]


def tie_case():
    """n = 4400 (per = 5, threads 0 .. 879 non-empty): the value of rank 1500 stands at 40 places: the whole range of thread
    0, the whole range of thread 879, two neighbours inside one thread, and 28 more over the waves in between"""
    g = rng(11)
    vals = np.sort(draw_grid(g, CUT_N - TIE_M + 1, lo=20000))[::-1]            # all above the threshold, distinct
    v, rest = vals[TIE_ABOVE], np.delete(vals, TIE_ABOVE)
    places = np.concatenate([np.arange(0, 5), np.arange(4395, 4400), [2001, 2002],
                             g.choice(np.setdiff1d(np.arange(64 * 5, 4390), [2001, 2002]), TIE_M - 12, replace=False)])
    assert np.unique(places).size == TIE_M and np.unique(places // (5 * 64)).size >= 8
    x = np.empty(CUT_N, np.float32)
    x[places] = v
    x[np.setdiff1d(np.arange(CUT_N), places)] = g.permutation(rest)
    case = make_case(x, CUT_C, g)
    return case, np.sort(places), [TIE_ABOVE + k for k in TIE_NEED]


def zeros_case(thresh):
    g = rng(13)
    return make_case(np.zeros(CUT_N, np.float32), CUT_C, g, thresh=thresh)


LOWBYTE_TOPK = [1000, 1001, 1009]


def lowbyte_case():
    """the 2000 cluster values (the top of the level) shuffled among 2400 grid values below them; a cut at rank ~1000 falls
    between values that share their top 24 bits with about nine others: the last radix pass decides"""
    g = rng(17)
    x = g.permutation(np.concatenate([cluster(np.arange(CLUSTER_N)), draw_grid(g, CUT_N - CLUSTER_N, hi=89000)]))
    return make_case(x, CUT_C, g)


SAT_TOPK = [25, 60, 200]
SAT_N_ONE, SAT_N_EXCL = 60, 30


def saturated_case():
    """60 logits that all give 1.0f (ties by index whatever the logit), 30 excluded ones, NaN offsets on rows that hold
    members of every top-k: they drop their candidates and keep their slots"""
    g = rng(19)
    x = draw_grid(g, CUT_N)
    where = g.choice(CUT_N, SAT_N_ONE + SAT_N_EXCL, replace=False)
    x[where[:SAT_N_ONE]] = f32(SATURATED)[np.arange(SAT_N_ONE) % len(SATURATED)]
    x[where[SAT_N_ONE:]] = f32(EXCLUDED)[np.arange(SAT_N_EXCL) % len(EXCLUDED)]
    off, pts = level_rows(CUT_N // CUT_C, 1.0, g)
    ones = np.sort(where[:SAT_N_ONE]) // CUT_C               # rows of the 1.0f ties, lowest index first
    off[ones[0], 0] = np.nan
    off[ones[3], 1] = np.nan
    off[ones[7]] = np.nan
    return make_case(x, CUT_C, g, offsets=off, points=pts)


DURCUT_N, DURCUT_TOPK = 4400, 1000


def duration_case():
    """C = 1 (a row is a candidate): every other member of the top-1000 has zero offsets; all others are long enough"""
    g = rng(23)
    x = draw_grid(g, DURCUT_N)
    off, pts = level_rows(DURCUT_N, 1.0, g)
    ranked = np.lexsort((np.arange(DURCUT_N), -prob32(x).astype(np.float64)))
    off[ranked[0:DURCUT_TOPK:2]] = 0.0
    return make_case(x, 1, g, offsets=off, points=pts), ranked


def exact_duration_case():
    """t integer, stride 1, dur 0.5: offsets (0.25, 0.25) give a length of exactly 0.5, which is not longer than 0.5;
    (0.25, 0.5) on the other rows"""
    g = rng(29)
    n = 2051
    x = draw_grid(g, n)
    off, pts = level_rows(n, 1.0, g, integer_t=True)
    off[:, 0], off[:, 1] = 0.25, 0.5
    off[::3, 1] = 0.25
    return make_case(x, 1, g, dur=0.5, offsets=off, points=pts)


LAYOUT_TOPK = [50, 5000]


def layout_case():
    """L = 6, C = 7; every level is allotted more rows than are valid and two gap rows follow it.  Every row outside a valid
    range holds logit +30 (1.0f: it would win every cut) and finite offsets.  Levels 1 and 5 are empty."""
    g = rng(31)
    alloc, lens, C = [400, 200, 100, 50, 25, 13], [390, 0, 100, 7, 25, 0], 7
    row0 = np.cumsum([0] + [a + 2 for a in alloc[:-1]])
    R = int(row0[-1]) + alloc[-1] + 2
    x = np.full((R, C), 30.0, np.float32)
    off = g.uniform(0.25, 3.0, (R, 2)).astype(np.float32)
    pts = np.zeros((R, 4), np.float32)
    pts[:, 2] = 1e4
    for l, (r0, a, n) in enumerate(zip(row0, alloc, lens)):
        x[r0:r0 + n] = draw_grid(g, n * C).reshape(n, C)
        pts[r0:r0 + a, 0] = (np.arange(a) + 0.37) * 2.0 ** l
        pts[r0:r0 + a, 3] = 2.0 ** l
    pts[pts[:, 3] == 0, 3] = 1.0
    return make_case(x, C, g, offsets=off, points=pts, row0=row0, lens=lens, alloc=alloc)


def many_levels_case():
    """L = 64 (the limit), C = 7, lengths cycling 0 .. 3, one gap row after each level"""
    g = rng(37)
    L, C = 64, 7
    lens = [l % 4 for l in range(L)]
    row0 = np.arange(L) * 4
    x = np.full((4 * L, C), 30.0, np.float32)
    for r0, n in zip(row0, lens):
        x[r0:r0 + n] = draw_grid(g, n * C).reshape(n, C)
    off, pts = level_rows(4 * L, 1.0, g)
    return make_case(x, C, g, offsets=off, points=pts, row0=row0, lens=lens, alloc=[3] * L)


RECIPE_T, RECIPE_C, RECIPE_L, RECIPE_TOPK = 2304, 110, 6, 5000
RECIPE_CLIPS = [2304, 1500]


def recipe_case(clip_len):
    """the recipe's pyramid: T = 2304, C = 110, six levels; valid lengths ceil(clip_len / 2^l); grid with repetition"""
    g = rng(41 + clip_len)
    alloc = [RECIPE_T >> l for l in range(RECIPE_L)]
    lens = [-(-clip_len // 2 ** l) for l in range(RECIPE_L)]
    row0 = np.cumsum([0] + alloc[:-1])
    R = sum(alloc)
    x = np.full((R, RECIPE_C), 30.0, np.float32)
    offs, ptss = [], []
    for l, (r0, a, n) in enumerate(zip(row0, alloc, lens)):
        x[r0:r0 + n] = draw_grid(g, n * RECIPE_C, repeat=True).reshape(n, RECIPE_C)
        o, p = level_rows(a, 2.0 ** l, g)
        offs.append(o)
        ptss.append(p)
    return make_case(x, RECIPE_C, g, offsets=np.concatenate(offs), points=np.concatenate(ptss), row0=row0, lens=lens, alloc=alloc)


# ------------------------------------------------------------------------------------------------ comparison
def compare(case, topk, segs, scores, labels):
    """the kernel's concatenated output (numpy: segs [n, 2], scores [n], labels [n]) against the restatement, level by level
    in index order; every element of every level is compared.  -> dict(count, score: worst relative score error, seg: worst
    ratio of a segment end's error to its bound 2 2^-24 (|t| + |off stride|)).  Counts, labels and order are asserted here;
    the two figures are the caller's to print and hold to BAR_P and 1."""
    want = expected(case, topk)
    n = sum(w[0].size for w in want)
    assert scores.shape[0] == n, "count %d, expected %d (per level %s)" % (scores.shape[0], n, [w[0].size for w in want])
    fig, lo = dict(count=n, score=0.0, seg=0.0), 0
    for l, (idx, p, left, right, lab) in enumerate(want):
        k = idx.size
        gs, gp, gl = segs[lo:lo + k].astype(np.float64), scores[lo:lo + k].astype(np.float64), labels[lo:lo + k]
        lo += k
        if k == 0:
            continue
        assert np.array_equal(gl, lab), "level %d: labels differ from the expected candidates in index order" % l
        assert not np.isnan(gp).any() and not np.isnan(gs).any(), "level %d: NaN in the output" % l
        fig["score"] = max(fig["score"], float((np.abs(gp - p) / p).max()))
        rows = int(case["row0"][l]) + idx // case["C"]
        o, q = case["offsets"][rows].astype(np.float64), case["points"][rows].astype(np.float64)
        for j, w in ((0, left), (1, right)):
            bound = 2 * U * (np.abs(q[:, 0]) + np.abs(o[:, j] * q[:, 3]))
            fig["seg"] = max(fig["seg"], float((np.abs(gs[:, j] - w) / bound).max()))
    return fig
