"""CPU: (1) pins the vectorised restatement tests/nms_restatement.py to the elementwise oracle/nms_oracle.py -- and to the
reference build (oracle/_ref, compiled from the reference's nms_cpu.cpp) where it is present -- bit for bit; (2) runs every
input builder of tests/nms_cases.py and asserts, through the restatement alone, that the input reaches the edge of
csrc/nms.hip its GPU test is named after."""
import numpy as np
import pytest
import torch

import nms_cases as C
import nms_restatement as R
from oracle import build_ref, nms_oracle

SIZES = [0, 1, 2, 8, 257, 600]
SOFT_PARAMS = [(0.5, 0.001), (0.75, 0.01), (0.99, 0.2)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ties", [False, True])
def test_nms_v_is_the_oracle(n, ties):
    segs, scores = C.random_case(n, 11 + n, ties)
    for thr in (0.1, 0.5):
        want = nms_oracle.nms(segs, scores, thr)
        got, ranks = R.nms_v(segs, scores, thr, return_ranks=True)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert np.array_equal(np.argsort(-scores, kind="stable")[ranks], got)
    ref = build_ref.load_ref()
    if ref is not None and not ties and n:                       # (tie order of the reference's sort: implementation-defined)
        want = ref.nms(torch.from_numpy(segs), torch.from_numpy(scores), 0.5).numpy()
        assert np.array_equal(R.nms_v(segs, scores, 0.5), want)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("method", [0, 1, 2])
def test_softnms_v_is_the_oracle(n, ties, method):
    segs, scores = C.random_case(n, 7 * n + 3, ties)
    ref = build_ref.load_ref()
    for k, (sigma, min_score) in enumerate(SOFT_PARAMS):
        thr = 0.1 if method == 2 else 0.3
        for max_num in ((1, 5, 0) if k == 0 else (0,)):          # (0 last: `got` is the unrestricted run below)
            want, wdets = nms_oracle.softnms(segs, scores, thr, sigma, min_score, method, max_num)
            got, dets, deaths = R.softnms_v(segs, scores, thr, sigma, min_score, method, max_num)
            assert got.dtype == np.int64 and np.array_equal(got, want)
            assert dets.dtype == np.float32 and np.array_equal(dets, wdets)
            assert deaths.size == got.size and (max_num or got.size + deaths.sum() == n)
        if ref is not None and n:
            rdets = torch.zeros(n, 3)
            want = ref.softnms(torch.from_numpy(segs), torch.from_numpy(scores), rdets, thr, sigma, min_score, method).numpy()
            assert np.array_equal(got, want)
            assert np.array_equal(dets, rdets.numpy()[:len(want)])


def test_swap_with_last_is_holes_from_survivors_at_the_end():
    """a hand-made pick: deaths at positions 1, 2, 5 of [1, 7) -> the sequential loop leaves [p, 6, 4, 3] (nms_cpu.cpp:146-154)"""
    segs = np.array([[0, 10]] + [[0, 10], [0, 10], [50, 51], [60, 61], [0, 10], [70, 71]], dtype=np.float32)
    scores = np.array([0.9, 0.5, 0.5, 0.3, 0.4, 0.5, 0.2], dtype=np.float32)
    inds, dets, deaths = R.softnms_v(segs, scores, 0.1, 0.1, 0.01, 2)
    want, wdets = nms_oracle.softnms(segs, scores, 0.1, 0.1, 0.01, 2)
    assert np.array_equal(inds, want) and inds.tolist() == [0, 4, 3, 6] and deaths.tolist() == [3, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ preconditions of the GPU cases
@pytest.mark.parametrize("n", C.HARD_CHUNK_SIZES)
@pytest.mark.parametrize("ties", [False, True])
def test_case_hard_chunk(n, ties):
    C.check_hard_chunk_case(C.hard_chunk_case(n, ties), n, ties)


@pytest.mark.parametrize("kc", [1025, 3000])
def test_case_hard_many_keeps(kc):
    C.check_hard_many_keeps_case(C.hard_many_keeps_case(kc))


@pytest.mark.parametrize("far", [False, True])
def test_case_threshold_pair(far):
    C.check_threshold_pair_case(C.threshold_pair_case(far), far)


def test_case_hard_layout_and_degenerate():
    C.check_hard_layout_case(C.hard_layout_case())
    C.check_hard_degenerate_case(C.hard_degenerate_case())


@pytest.mark.parametrize("method", [0, 1, 2])
def test_case_soft_pow2(method):
    C.check_soft_pow2_case(method)


@pytest.mark.parametrize("n", [C.REG_MAXN, C.ROWS_MAXN, C.ROWS_MAXN + 1])
def test_case_soft_capacity(n):
    picks, d0 = C.check_soft_capacity_case(n)
    print("capacity n=%d: %d picks, %d deaths on pick 0" % (n, picks, d0))


@pytest.mark.parametrize("pick", [0, 1])
@pytest.mark.parametrize("ndead", [C.FILL_CAP, C.FILL_CAP + 1])
def test_case_soft_fill_cap(pick, ndead):
    deaths, picks, holes = C.check_soft_fill_case(pick, ndead)
    print("FILL_CAP pick=%d ndead=%d: deaths by pick %s, %d picks, %d holes refilled" % (pick, ndead, deaths, picks, holes))


@pytest.mark.parametrize("n", C.SOFT_DIE_SIZES)
@pytest.mark.parametrize("from_start", [False, True])
def test_case_soft_all_die(n, from_start):
    C.check_soft_all_die_case(C.soft_all_die_case(n, from_start))


def test_case_soft_skip_pair_maxnum_batched():
    C.check_soft_skip_case()
    C.check_soft_threshold_pair_case(0)
    C.check_soft_threshold_pair_case(1)
    C.check_soft_maxnum_case()
    C.check_batched_case()
