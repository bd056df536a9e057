"""TEST INFRASTRUCTURE ONLY -- input builders for tests/test_nms_edges_gpu.py, one per edge of csrc/nms.hip.

Every builder returns a dict of numpy inputs plus the parameters of the call.  `check_*` functions state, through
tests/nms_restatement.py alone, the precondition that makes the case reach its edge (">= 1025 keeps in chunk 0", "pick 1
kills exactly 16001", ...).  tests/test_nms_restatement_cpu.py runs every one of them without a GPU, so that no GPU test rests
on an edge its input does not reach; the GPU file imports the same builders.
"""
import functools

import numpy as np

import nms_restatement as R

f32 = np.float32
CH = 4096                      # nms_sweep_kernel: candidates per chunk
APPLY_TILE = 1024              # nms_apply_kernel: keeps staged per tile
REG_MAXN = 30720               # softnms_reg_kernel: 60 slots x 512 threads
ROWS_MAXN = 65536              # softnms_rows_kernel: 64 rows x 1024 threads
FILL_CAP = 16000               # softnms_reg_kernel: tail survivors of one pick kept in LDS


def random_case(n, seed, ties=False, span=200.0):
    """the generator of tests/test_nms_gpu.py"""
    g = np.random.RandomState(seed)
    c = g.uniform(0, span, n).astype(f32)
    w = g.uniform(0.5, 30, n).astype(f32)
    segs = np.stack([c - w / 2, c + w / 2], 1).astype(f32)
    scores = g.uniform(0.001, 1, n).astype(f32)
    if ties and n > 4:
        scores[n // 2:] = scores[: n - n // 2]
        segs[-1] = segs[0]
    return segs, scores


def untie(scores):
    """break the accidental float32 collisions of a random draw (the reference's tie order is implementation-defined)"""
    sc = np.asarray(scores, dtype=f32).copy()
    while True:
        _, first = np.unique(sc, return_index=True)
        dup = np.setdiff1d(np.arange(sc.size), first)
        if dup.size == 0:
            return sc
        sc[dup] = np.nextafter(sc[dup], f32(2))


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ================================================================================================ hard NMS
HARD_CHUNK_SIZES = [4095, 4096, 4097, 8192, 8193]
HARD_THR = 0.5


@functools.lru_cache(maxsize=None)
def hard_chunk_case(n, ties):
    """random candidates at a chunk-edge size.  ties=False: tie-free scores, a wide span so that keeps fall into every chunk.
    ties=True: ALL scores equal (rank == input index) and a few candidates of chunk 0 repeated exactly one chunk later and at the
    very end: only the stable rank decides which copy survives."""
    segs, scores = random_case(n, 3 * n + 1, span=200.0 * (n // 1000))
    if not ties:
        scores = untie(scores)
        segs[int(np.argmin(scores))] = (-500.0, -490.0)         # the last rank stands alone: the last chunk keeps, even a chunk of one
        return dict(segs=segs, scores=scores, thr=HARD_THR, dup=())
    scores = np.full(n, 0.5, dtype=f32)
    keeps = R.nms_v(segs, scores, HARD_THR)
    src = [int(k) for k in keeps[:6] if k < n - CH]            # kept candidates with a slot one chunk later
    dup = []
    for k in src:
        segs[k + CH] = segs[k]
        dup.append((k, k + CH))
    k = int(keeps[0])                                            # == 0: rank 0 is always kept
    segs[n - 1] = segs[k]
    dup.append((k, n - 1))
    return dict(segs=segs, scores=scores, thr=HARD_THR, dup=tuple(dup))


def check_hard_chunk_case(case, n, ties):
    inds, ranks = R.nms_v(case["segs"], case["scores"], case["thr"], return_ranks=True)
    nchunks = (n + CH - 1) // CH
    if not ties:
        assert np.unique(case["scores"]).size == n
        assert set(ranks // CH) == set(range(nchunks)), "a keep in every chunk"
        order = np.argsort(-case["scores"], kind="stable")
        dead_late = np.setdiff1d(order[CH:], inds)
        assert n <= CH + 1 or dead_late.size > 0                 # kills beyond chunk 0 (n = 4097: its one late candidate is the keep)
    else:
        assert np.array_equal(inds, np.sort(inds)) and np.array_equal(inds, ranks)       # rank == input index
        assert len(case["dup"]) >= 1 + (n > CH + 6)
        kept = set(inds.tolist())
        for a, b in case["dup"]:
            assert a in kept and b not in kept and a < b
        if n > CH:
            assert any(b // CH > a // CH for a, b in case["dup"]), "a copy removed across a chunk boundary"
    return inds


@functools.lru_cache(maxsize=None)
def hard_many_keeps_case(kc):
    """n = 8193, tie-free.  Rank layout (rank r has score 1 - r * 1e-4):
      ranks [0, kc)       kc disjoint unit segments on an even-integer grid: chunk 0's keeps
      ranks [kc, 4096)    exact copies of some of them: removed inside chunk 0 by the sweep
      ranks [4096, 8193)  further disjoint unit segments (kept) and 200 exact copies of chunk-0 keeps -- among them a copy of the
                          LAST keep of chunk 0 (alone in its staging tile when kc = 1025) and of the first and last keep of every
                          staging tile; the copy of the last keep has the lowest score of all (rank 8192: chunk 2, rest == 1)
    and a random input order."""
    n, ncopy = 2 * CH + 1, 200
    g = np.random.RandomState(kc)
    seg_of_rank = np.zeros((n, 2), dtype=f32)
    grid = iter(range(0, 4 * n, 2))

    def unit():
        a = next(grid)
        return (a, a + 1)
    for r in range(kc):
        seg_of_rank[r] = unit()
    for r in range(kc, CH):
        seg_of_rank[r] = seg_of_rank[g.randint(0, kc)]
    edges = {0} | set(range(APPLY_TILE - 1, kc - 1, APPLY_TILE)) | set(range(APPLY_TILE, kc - 1, APPLY_TILE))
    originals = [kc - 1] + sorted(edges)                         # the last keep first: it pairs with rank 8192
    originals += [int(k) for k in g.randint(0, kc, ncopy - len(originals))]
    copy_ranks = [n - 1] + [int(r) for r in CH + np.sort(g.choice(n - CH - 1, ncopy - 1, replace=False))]
    is_copy = np.zeros(n, dtype=bool)
    copy_of = {}
    for r, o in zip(copy_ranks, originals):
        seg_of_rank[r] = seg_of_rank[o]
        is_copy[r] = True
        copy_of[r] = o
    for r in range(CH, n):
        if not is_copy[r]:
            seg_of_rank[r] = unit()
    score_of_rank = (f32(1) - np.arange(n, dtype=f32) * f32(1e-4)).astype(f32)
    perm = g.permutation(n)                                      # input index -> rank
    return dict(segs=seg_of_rank[perm].copy(), scores=score_of_rank[perm].copy(), thr=HARD_THR, kc=kc,
                late_copies=tuple(sorted(copy_of.items())), rank_of_input=perm)


def check_hard_many_keeps_case(case):
    n, kc = case["scores"].size, case["kc"]
    assert n == 2 * CH + 1 and np.unique(case["scores"]).size == n
    order = np.argsort(-case["scores"], kind="stable")
    assert np.array_equal(case["rank_of_input"][order], np.arange(n))
    inds, ranks = R.nms_v(case["segs"], case["scores"], case["thr"], return_ranks=True)
    chunk0 = ranks[ranks < CH]
    assert chunk0.size == kc and kc > APPLY_TILE and np.array_equal(chunk0, np.arange(kc))
    kept = set(ranks.tolist())
    late = dict(case["late_copies"])
    assert len(late) == 200 and max(late) == n - 1 and late[n - 1] == kc - 1
    for r, o in late.items():
        assert r >= CH and o < kc and r not in kept              # a chunk-0 keep removes it: nms_apply_kernel's work
        assert np.array_equal(case["segs"][order[r]], case["segs"][order[o]])
    tiles = {o // APPLY_TILE for o in late.values()}
    assert tiles == set(range((kc + APPLY_TILE - 1) // APPLY_TILE)), "a copy of a keep in every staging tile"
    assert ranks.size == n - 200 - (CH - kc)                     # everything else is kept
    return inds


@functools.lru_cache(maxsize=None)
def threshold_pair_case(far):
    """two overlapping segments A (top score) and B (lowest score); thr = their IoU as the oracle computes it.  far=False: a
    handful of disjoint fillers (same chunk: the sweep decides).  far=True: 4200 disjoint fillers scored between them, so B ranks
    beyond chunk 0 (nms_apply_kernel decides)."""
    nfill = 4200 if far else 5
    g = np.random.RandomState(17 + far)
    a, b = np.array([1.3, 11.7], dtype=f32), np.array([4.9, 15.1], dtype=f32)
    fill = np.stack([100 + 3 * np.arange(nfill), 101 + 3 * np.arange(nfill)], 1).astype(f32)
    segs = np.concatenate([a[None], fill, b[None]]).astype(f32)
    scores = np.concatenate([[0.95], untie(g.uniform(0.2, 0.9, nfill)), [0.1]]).astype(f32)
    perm = g.permutation(nfill + 2)
    ia, ib = int(np.nonzero(perm == 0)[0][0]), int(np.nonzero(perm == nfill + 1)[0][0])
    thr = R.iou_pair(a, b)
    return dict(segs=segs[perm].copy(), scores=scores[perm].copy(), thr=thr, thr_up=np.nextafter(thr, f32(np.inf)), ia=ia, ib=ib)


def check_threshold_pair_case(case, far):
    segs, scores = case["segs"], case["scores"]
    n = scores.size
    assert np.unique(scores).size == n
    thr = R.iou_pair(segs[case["ia"]], segs[case["ib"]])
    assert thr.dtype == f32 and thr.tobytes() == f32(case["thr"]).tobytes() and 0.1 < thr < 0.9
    assert case["thr_up"] > case["thr"]
    at, ranks = R.nms_v(segs, scores, case["thr"], return_ranks=True)
    up = R.nms_v(segs, scores, case["thr_up"])
    assert case["ib"] not in at and case["ib"] in up and at.size == n - 1 and up.size == n
    order = np.argsort(-scores, kind="stable")
    assert order[0] == case["ia"] and order[-1] == case["ib"]
    assert (n - 1 >= CH) == far
    return at, up


HARD_LAYOUT_SIZES = [3, 0, 1, 0, 0, 4097, 2, 1, 1, 1, 300, 0]


@functools.lru_cache(maxsize=None)
def hard_layout_case():
    parts = [random_case(n, 31 + 7 * k, span=200.0 * max(1, n // 1000)) for k, n in enumerate(HARD_LAYOUT_SIZES)]
    parts = [(s, untie(sc)) for s, sc in parts]
    for s, sc in parts:
        if sc.size > CH:
            s[int(np.argmin(sc))] = (-500.0, -490.0)             # the one candidate of the long class's second chunk is kept
    return dict(sizes=tuple(HARD_LAYOUT_SIZES), off=offsets(HARD_LAYOUT_SIZES), thr=HARD_THR,
                segs=np.concatenate([p[0] for p in parts]), scores=np.concatenate([p[1] for p in parts]))


def check_hard_layout_case(case):
    off, sizes = case["off"], case["sizes"]
    assert sizes.count(0) >= 4 and sizes[-1] == 0 and sizes[1] == 0
    nch = [(n + CH - 1) // CH for n in sizes]
    assert max(nch) == 2 and sorted(set(nch)) == [0, 1, 2]
    last = off[-3] // 256                                         # the rank block where the long class ends
    assert sum(1 for k in range(len(sizes)) if sizes[k] and off[k] // 256 <= last <= (off[k + 1] - 1) // 256) >= 5
    want = []
    for k, n in enumerate(sizes):
        lo = int(off[k])
        inds, ranks = R.nms_v(case["segs"][lo:lo + n], case["scores"][lo:lo + n], case["thr"], return_ranks=True)
        if n > CH:
            assert (ranks >= CH).any()
        want.append(inds)
    return want


def hard_degenerate_case():
    """three copies of a zero-width segment (IoU 0: all kept), [0,1] / [1,2] touching (inter == 0: both kept), [0.25,0.875]
    inside [0,1] with a lower score (IoU 0.625: removed), a zero-width segment inside a kept one (kept)"""
    segs = np.array([[5, 5], [0, 1], [5, 5], [1, 2], [0.25, 0.875], [5, 5], [0.5, 0.5], [2, 2]], dtype=f32)
    scores = np.array([0.9, 0.8, 0.7, 0.75, 0.6, 0.5, 0.4, 0.3], dtype=f32)
    return dict(segs=segs, scores=scores, thr=HARD_THR)


def check_hard_degenerate_case(case):
    inds = R.nms_v(case["segs"], case["scores"], case["thr"])
    assert inds.tolist() == [0, 1, 3, 2, 5, 6, 7]
    assert R.iou_pair(case["segs"][0], case["segs"][2]) == 0 and R.iou_pair(case["segs"][1], case["segs"][3]) == 0
    return inds


# ================================================================================================ soft NMS
SOFT_POW2_SIZES = [63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 8191, 8192, 8193, 0, 1]
SOFT_POW2 = dict(thr=0.3, sigma=0.5, min_score=0.05)


@functools.lru_cache(maxsize=None)
def soft_pow2_case():
    parts = [random_case(n, 41 + 3 * k, span=200.0 * max(1, n // 2000)) for k, n in enumerate(SOFT_POW2_SIZES)]
    return dict(sizes=tuple(SOFT_POW2_SIZES), off=offsets(SOFT_POW2_SIZES), segs=np.concatenate([p[0] for p in parts]),
                scores=np.concatenate([p[1] for p in parts]), **SOFT_POW2)


@functools.lru_cache(maxsize=None)
def soft_pow2_expected(method):
    """restatement per class, computed once per method and shared"""
    c = soft_pow2_case()
    out = []
    for k, n in enumerate(c["sizes"]):
        lo = int(c["off"][k])
        out.append(R.softnms_v(c["segs"][lo:lo + n], c["scores"][lo:lo + n], c["thr"], c["sigma"], c["min_score"], method))
    return out


def check_soft_pow2_case(method):
    c = soft_pow2_case()
    assert sum(c["sizes"]) <= REG_MAXN                          # `reg` alone takes the whole call
    for n, (inds, dets, deaths) in zip(c["sizes"], soft_pow2_expected(method)):
        assert inds.size == n if n <= 1 else 1 <= inds.size <= n
        if n >= 63:
            assert 1 < inds.size and deaths.sum() > 0 and inds.size + deaths.sum() == n


SOFT_CAP = dict(thr=0.1, sigma=0.5, min_score=0.01, method=2)


@functools.lru_cache(maxsize=None)
def soft_capacity_case(n):
    """n candidates of which all but ~4000 start below min_score (they die on pick 0, wherever they are), scattered over all
    positions; the survivors are spread widely, so that most of them are picked"""
    nsurv = 4000
    g = np.random.RandomState(n)
    segs, _ = random_case(n, n + 5, span=40.0 * nsurv)
    scores = g.uniform(0.0005, 0.009, n).astype(f32)
    hi = g.choice(n, nsurv, replace=False)
    scores[hi] = g.uniform(0.05, 1.0, nsurv).astype(f32)
    # the last row of the rows kernel / the last slot of the register kernel holds both kinds
    scores[n - 3], scores[n - 2], scores[n - 1] = 0.5, 0.002, 0.25
    return dict(segs=segs, scores=scores, **SOFT_CAP)


@functools.lru_cache(maxsize=None)
def soft_capacity_expected(n):
    c = soft_capacity_case(n)
    return R.softnms_v(c["segs"], c["scores"], c["thr"], c["sigma"], c["min_score"], c["method"])


def check_soft_capacity_case(n):
    c = soft_capacity_case(n)
    inds, dets, deaths = soft_capacity_expected(n)
    low = int((c["scores"] < f32(c["min_score"])).sum())
    assert deaths[0] >= low and abs(low - (n - 4000)) <= 3
    assert 3000 <= inds.size <= 4003, inds.size
    assert inds.size + deaths.sum() == n
    assert c["scores"][n - 1] >= c["min_score"] > c["scores"][n - 2]
    return inds.size, int(deaths[0])


SOFT_FILL = dict(thr=0.1, sigma=0.1, min_score=0.01, method=2)


@functools.lru_cache(maxsize=None)
def soft_fill_case(pick, ndead):
    """n = 30720 (the register kernel's capacity); exactly `ndead` candidates die on pick `pick` and none on the other of the two.
    Pick 0 is an isolated segment with the top score.  pick 0: `ndead` initial scores below min_score, scattered.  pick 1: pick 1
    has the second score and `ndead` near-copies (jitter 0.01 on a width of 10, scores 0.3-0.6, random positions) which its decay
    exp(-IoU^2 / 0.1) < 1e-4 removes; every other score lies in [0.02, 0.9] and nothing else overlaps pick 0 or pick 1."""
    n = REG_MAXN
    g = np.random.RandomState(100 * pick + ndead % 7)
    nother = n - ndead - (2 if pick else 1)
    c = g.uniform(100.0, 100.0 + 0.3 * nother, nother).astype(f32)
    w = g.uniform(0.5, 30, nother).astype(f32)
    osegs = np.stack([c - w / 2, c + w / 2], 1).astype(f32)
    oscores = np.clip(g.uniform(0.001, 1, nother), 0.02, 0.9).astype(f32)
    if pick == 0:
        dc = g.uniform(100.0, 100.0 + 0.3 * nother, ndead).astype(f32)
        dsegs = np.stack([dc - 2, dc + 2], 1).astype(f32)
        dscores = g.uniform(0.0005, 0.009, ndead).astype(f32)
        segs = np.concatenate([np.array([[-1000.0, -990.0]], dtype=f32), osegs, dsegs])
        scores = np.concatenate([np.array([0.99], dtype=f32), oscores, dscores])
    else:
        j = g.uniform(-0.01, 0.01, (ndead, 2)).astype(f32)
        dsegs = (np.array([[0.0, 10.0]], dtype=f32) + j).astype(f32)
        dscores = g.uniform(0.3, 0.6, ndead).astype(f32)
        top = np.array([[-1000.0, -990.0], [0.0, 10.0]], dtype=f32)
        segs = np.concatenate([top, osegs, dsegs])
        scores = np.concatenate([np.array([0.99, 0.95], dtype=f32), oscores, dscores])
    perm = g.permutation(n)
    return dict(segs=segs[perm].astype(f32), scores=scores[perm].astype(f32), pick=pick, ndead=ndead, **SOFT_FILL)


@functools.lru_cache(maxsize=None)
def soft_fill_expected(pick, ndead):
    c = soft_fill_case(pick, ndead)
    return R.softnms_v(c["segs"], c["scores"], c["thr"], c["sigma"], c["min_score"], c["method"])


def check_soft_fill_case(pick, ndead):
    """the deaths of the pick, and that the compaction has work on both sides: holes below the new length, survivors beyond it"""
    c = soft_fill_case(pick, ndead)
    n = c["scores"].size
    inds, dets, deaths = soft_fill_expected(pick, ndead)
    assert n == REG_MAXN and ndead in (FILL_CAP, FILL_CAP + 1)
    assert deaths[pick] == ndead and deaths[:pick].sum() == 0
    # replay the picks up to `pick` on the score array to see where the dead sit at that pick
    one = R.softnms_v(c["segs"], c["scores"], c["thr"], c["sigma"], c["min_score"], c["method"], max_num=pick + 1)
    assert np.array_equal(one[0], inds[:pick + 1]) and one[2][pick] == ndead
    if pick == 0:
        dead = c["scores"] < f32(c["min_score"])
        top = int(inds[0])
        dead[top], dead[0] = dead[0], dead[top]                 # the pick's swap
    else:
        sc = c["scores"]
        dead = (sc >= f32(0.3)) & (sc <= f32(0.6)) & (c["segs"][:, 0] < 1) & (c["segs"][:, 1] > 9)
        assert int(dead.sum()) == ndead
        order = np.arange(n)
        for i in range(2):                                       # the two picks' swaps
            p = int(np.nonzero(order == inds[i])[0][0])
            order[i], order[p] = order[p], order[i]
        dead = dead[order]
    first = pick + 1
    new_n = n - ndead
    assert not dead[:first].any()
    holes, tail_surv = int(dead[first:new_n].sum()), int((~dead[new_n:]).sum())
    assert holes == tail_surv and holes > 1000
    return deaths[:3].tolist(), inds.size, holes


SOFT_DIE_SIZES = [2, 513, 4097]
SOFT_DIE = dict(thr=0.1, sigma=0.1, min_score=0.01, method=2)


def soft_all_die_case(n, from_start):
    """from_start=False: pick 0 is [0, 10] with the top score and every other candidate a near-copy that its decay removes.
    from_start=True: every score is below min_score already: the reference still emits the maximum, then removes the rest."""
    g = np.random.RandomState(n + from_start)
    if from_start:
        segs, _ = random_case(n, n, span=50.0 * n)
        scores = g.uniform(0.0005, 0.009, n).astype(f32)
    else:
        segs = (np.array([[0.0, 10.0]], dtype=f32) + g.uniform(-0.01, 0.01, (n, 2))).astype(f32)
        scores = g.uniform(0.3, 0.6, n).astype(f32)
        scores[g.randint(0, n)] = 0.9
    return dict(segs=segs, scores=scores, **SOFT_DIE)


def check_soft_all_die_case(case):
    inds, dets, deaths = R.softnms_v(case["segs"], case["scores"], case["thr"], case["sigma"], case["min_score"], 2)
    n = case["scores"].size
    assert inds.size == 1 and deaths.tolist() == [n - 1] and inds[0] == int(np.argmax(case["scores"]))
    return inds, dets


SOFT_SKIP = dict(thr=0.1, sigma=0.5, min_score=0.01)
SKIP_P, SKIP_T, SKIP_Z, SKIP_Q, SKIP_E = 0, 1, 2, 3, 4


@functools.lru_cache(maxsize=None)
def soft_skip_case():
    """P = [10, 20] is pick 0.  T = [20, 25] touches it; Z = [15, 15] has no width and lies inside it; Q = [100, 110] overlaps
    nothing and starts below min_score; E = [200, 210] overlaps nothing and scores min_score exactly.  700 random candidates far
    away fill a second slot of the register kernel."""
    fs, fsc = random_case(700, 5, span=400.0)
    fs = (fs + f32(1000)).astype(f32)
    segs = np.concatenate([np.array([[10, 20], [20, 25], [15, 15], [100, 110], [200, 210]], dtype=f32), fs])
    scores = np.concatenate([np.array([1.5, 0.5, 0.4, 0.005, SOFT_SKIP["min_score"]], dtype=f32), fsc])
    return dict(segs=segs, scores=scores, **SOFT_SKIP)


@functools.lru_cache(maxsize=None)
def soft_skip_expected():
    c = soft_skip_case()
    return R.softnms_v(c["segs"], c["scores"], c["thr"], c["sigma"], c["min_score"], 2)


def check_soft_skip_case():
    c = soft_skip_case()
    inds, dets, deaths = soft_skip_expected()
    low = int((c["scores"] < f32(c["min_score"])).sum())
    assert inds[0] == SKIP_P and deaths[0] == low and SKIP_Q not in inds
    for k in (SKIP_T, SKIP_Z, SKIP_E):                           # untouched by any decay: the initial score, bit for bit
        at = int(np.nonzero(inds == k)[0][0])
        assert dets[at, 2].tobytes() == c["scores"][k].tobytes()
    assert c["scores"][SKIP_E].tobytes() == f32(c["min_score"]).tobytes()
    assert inds.size > 100 and deaths[1:].sum() > 0
    return inds, dets


@functools.lru_cache(maxsize=None)
def soft_threshold_pair_case():
    """methods 0 and 1: A (top score) and B overlap with IoU == thr; a few disjoint fillers"""
    a, b = np.array([1.3, 11.7], dtype=f32), np.array([4.9, 15.1], dtype=f32)
    fill = np.stack([100 + 3 * np.arange(70), 101 + 3 * np.arange(70)], 1).astype(f32)
    segs = np.concatenate([fill[:30], a[None], fill[30:], b[None]]).astype(f32)
    g = np.random.RandomState(3)
    scores = np.concatenate([g.uniform(0.2, 0.8, 30), [0.95], g.uniform(0.2, 0.8, 40), [0.9]]).astype(f32)
    thr = R.iou_pair(a, b)
    return dict(segs=segs, scores=scores, thr=thr, thr_up=np.nextafter(thr, f32(np.inf)), ia=30, ib=71, sigma=0.5, min_score=0.05)


def check_soft_threshold_pair_case(method):
    c = soft_threshold_pair_case()
    assert R.iou_pair(c["segs"][c["ia"]], c["segs"][c["ib"]]).tobytes() == f32(c["thr"]).tobytes()
    at = R.softnms_v(c["segs"], c["scores"], c["thr"], c["sigma"], c["min_score"], method)
    up = R.softnms_v(c["segs"], c["scores"], c["thr_up"], c["sigma"], c["min_score"], method)
    n = c["scores"].size
    assert up[0].size == n and up[0][1] == c["ib"] and up[1][1, 2] == c["scores"][c["ib"]]     # just above: untouched
    if method == 0:
        assert at[0].size == n - 1 and c["ib"] not in at[0] and at[2][0] == 1
    else:
        assert at[0].size == n and at[0][1] != c["ib"]
        row = int(np.nonzero(at[0] == c["ib"])[0][0])
        assert at[1][row, 2] == f32(c["scores"][c["ib"]] * (f32(1) - f32(c["thr"])))
    return at, up


SOFT_MAXNUM = dict(thr=0.1, sigma=0.5, min_score=0.05, method=2)


@functools.lru_cache(maxsize=None)
def soft_maxnum_case():
    segs, scores = random_case(700, 77, span=150.0)
    return dict(segs=segs, scores=scores, **SOFT_MAXNUM)


@functools.lru_cache(maxsize=None)
def soft_maxnum_expected():
    c = soft_maxnum_case()
    return R.softnms_v(c["segs"], c["scores"], c["thr"], c["sigma"], c["min_score"], c["method"])


def check_soft_maxnum_case():
    c = soft_maxnum_case()
    inds, dets, deaths = soft_maxnum_expected()
    K = inds.size
    assert 8 < K < c["scores"].size - 8 and deaths.sum() == c["scores"].size - K
    for m in (1, K, K + 7):
        i2, d2, _ = R.softnms_v(c["segs"], c["scores"], c["thr"], c["sigma"], c["min_score"], c["method"], max_num=m)
        k = min(K, m)
        assert np.array_equal(i2, inds[:k]) and np.array_equal(d2, dets[:k])
    return K


# ================================================================================================ batched_nms
BATCHED_IDS = (0, 5, 21)


@functools.lru_cache(maxsize=None)
def batched_case():
    """three classes with ids {0, 5, 21}, interleaved: class 5 is large and spread out (more picks than max_seg_num), class 21
    scores in (0.9, 0.95) throughout, class 0 is small"""
    g = np.random.RandomState(8)
    sizes = {0: 40, 5: 260, 21: 60}
    segs, scores, cls = [], [], []
    for k, n in sizes.items():
        s, sc = random_case(n, 50 + k, span=2000.0 if k == 5 else 200.0)
        if k == 21:
            sc = (f32(0.9) + sc * f32(0.049)).astype(f32)
        else:
            sc[:3] = (0.99, 0.98, 0.97)                          # both other classes keep something above 0.95
        segs.append(s), scores.append(sc), cls.append(np.full(n, k, dtype=np.int64))
    perm = g.permutation(sum(sizes.values()))
    return dict(segs=np.concatenate(segs)[perm], scores=np.concatenate(scores)[perm], cls=np.concatenate(cls)[perm],
                max_seg_num=50, thr=0.1, sigma=0.75)


def check_batched_case():
    c = batched_case()
    assert tuple(np.unique(c["cls"])) == BATCHED_IDS
    m5 = c["cls"] == 5
    assert R.softnms_v(c["segs"][m5], c["scores"][m5], c["thr"], c["sigma"], 0.01, 2)[0].size > c["max_seg_num"]
    k5 = c["scores"][m5] > f32(0.01)
    assert R.nms_v(c["segs"][m5][k5], c["scores"][m5][k5], c["thr"]).size > c["max_seg_num"]
    assert c["scores"][c["cls"] == 21].max() < 0.95 < c["scores"][c["cls"] == 0].max()
    assert c["scores"].max() < 1.0
    from oracle import nms_oracle
    for soft, min_score in ((True, 0.01), (False, 0.01), (False, 0.95)):
        _, _, wc = nms_oracle.batched_nms(c["segs"], c["scores"], c["cls"], c["thr"], min_score, c["max_seg_num"], soft, True,
                                          c["sigma"], 0.0)
        assert (wc.size == c["max_seg_num"]) == (min_score < 0.95) and wc.size > 3      # the overall cut, where classes remain
        assert {0, 5} <= set(wc.tolist()) and (21 in wc) == (min_score < 0.95)
