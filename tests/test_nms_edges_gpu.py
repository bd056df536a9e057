"""The six kernels of csrc/nms.hip at their chunk, tile and capacity edges.  Every case comes from tests/nms_cases.py, whose
preconditions ("chunk 0 yields 1025 keeps", "pick 1 kills exactly 16001", ...) tests/test_nms_restatement_cpu.py asserts on the
CPU.  The HIP result is compared with the vectorised restatement tests/nms_restatement.py AND with the reference build
(oracle/_ref/nms_1d_cpu.so): indices bit for bit, decayed scores at rtol 1e-5 / atol 1e-7 (device expf against glibc, the bar
of tests/test_nms_gpu.py).  Hard-NMS inputs with exact score ties are compared with the restatement only: the reference's tie
order is implementation-defined."""
import numpy as np
import pytest
import torch

import nms_cases as C
import nms_restatement as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
SOFT_KINDS = ["reg", "rows", "legacy"]


def ref_module():
    from oracle import build_ref
    ref = build_ref.load_ref()
    assert ref is not None, "oracle/_ref/nms_1d_cpu.so did not load on the GPU box"
    return ref


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dets_close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)


# ================================================================================================ hard NMS
def hard(segs, scores, thr):
    from vilco_amd.utils.nms import nms_1d_cpu
    return nms_1d_cpu.nms(t(segs), t(scores), float(thr)).numpy()


def hard_ref(segs, scores, thr):
    return ref_module().nms(t(segs), t(scores), float(thr)).numpy()


@pytest.mark.parametrize("n", C.HARD_CHUNK_SIZES)
@pytest.mark.parametrize("ties", [False, True])
def test_hard_chunk_sizes(dev, n, ties):
    """CH = 4096: an exactly full chunk, a chunk of one candidate, rest == 1; keeps and kills across chunk boundaries; with all
    scores equal, copies one chunk apart that only the stable rank tells apart"""
    c = C.hard_chunk_case(n, ties)
    want = C.check_hard_chunk_case(c, n, ties)
    got = hard(c["segs"], c["scores"], c["thr"])
    assert np.array_equal(got, want)
    if not ties:
        assert np.array_equal(got, hard_ref(c["segs"], c["scores"], c["thr"]))


@pytest.mark.parametrize("kc", [1025, 3000])
def test_hard_many_keeps_per_chunk(dev, kc):
    """nms_apply_kernel's staging loop: chunk 0 yields kc > 1024 keeps (kc = 1025: a second tile of one entry), and 200 later
    candidates are exact copies of chunk-0 keeps of every tile -- only nms_apply_kernel can remove them"""
    c = C.hard_many_keeps_case(kc)
    want = C.check_hard_many_keeps_case(c)
    got = hard(c["segs"], c["scores"], c["thr"])
    assert np.array_equal(got, want)
    assert np.array_equal(got, hard_ref(c["segs"], c["scores"], c["thr"]))


@pytest.mark.parametrize("far", [False, True])
def test_hard_threshold_equality(dev, far):
    """IoU == thr bit for bit suppresses (>=); one ulp above it does not.  far=False: nms_sweep_kernel decides; far=True: the
    lower-scored one ranks beyond chunk 0 and nms_apply_kernel decides"""
    c = C.threshold_pair_case(far)
    at, up = C.check_threshold_pair_case(c, far)
    for thr, want in ((c["thr"], at), (c["thr_up"], up)):
        got = hard(c["segs"], c["scores"], thr)
        assert np.array_equal(got, want), float(thr)
        assert np.array_equal(got, hard_ref(c["segs"], c["scores"], thr))


def test_hard_class_layout(dev):
    """one vilco_nms_1d call: empty classes in the middle and at the end, one-candidate classes, six classes inside one
    256-candidate rank block, one class of two chunks among classes of one"""
    from vilco_amd.utils.nms import _run_hard
    c = C.hard_layout_case()
    want = C.check_hard_layout_case(c)
    ref = ref_module()
    idx, cnt = _run_hard(t(c["segs"]).to(dev), t(c["scores"]).to(dev), t(c["off"]).to(dev), len(c["sizes"]), c["thr"])
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    assert cnt.shape == (len(c["sizes"]),)
    for k, n in enumerate(c["sizes"]):
        lo = int(c["off"][k])
        assert cnt[k] == want[k].size, k
        if n == 0:
            assert cnt[k] == 0
            continue
        assert np.array_equal(idx[lo:lo + cnt[k]], want[k]), k
        assert np.array_equal(want[k], ref.nms(t(c["segs"][lo:lo + n]), t(c["scores"][lo:lo + n]), c["thr"]).numpy()), k


def test_hard_zero_width_and_touching(dev):
    c = C.hard_degenerate_case()
    want = C.check_hard_degenerate_case(c)
    got = hard(c["segs"], c["scores"], c["thr"])
    assert np.array_equal(got, want)
    assert np.array_equal(got, hard_ref(c["segs"], c["scores"], c["thr"]))


# ================================================================================================ soft NMS
def soft_raw(dev, segs, scores, off, p, method, max_num=0):
    """vilco_softnms_1d as _run_soft calls it, but into a `dets` the test has pre-filled -> (dets, idx, cnt) on the host"""
    from vilco_amd import _lib
    lib = _lib.load()
    segs, scores, off = t(segs).to(dev), t(scores).to(dev), t(off).to(dev)
    n, nseg = segs.shape[0], off.numel() - 1
    dets = torch.full((max(n, 1), 3), SENTINEL, dtype=torch.float32, device=dev)
    idx = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(max(nseg, 1), dtype=torch.int64, device=dev)
    wsz = lib.vilco_nms_workspace(n, nseg)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    _lib.check(lib.vilco_softnms_1d(segs.data_ptr(), scores.data_ptr(), off.data_ptr(), nseg, n, float(p["thr"]), float(p["sigma"]),
                                    float(p["min_score"]), int(method), int(max_num), dets.data_ptr(), idx.data_ptr(),
                                    cnt.data_ptr(), ws.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream))
    return dets.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()


def soft_one(kernel, c, method, expect_kernels=None, thr=None):
    """one class through nms_1d_cpu.softnms under `kernel`, into a pre-filled dets -> (inds, dets[:K]); rows beyond K must keep
    the caller's values"""
    from vilco_amd.utils.nms import last_soft_kernels, nms_1d_cpu, soft_kernel
    n = c["scores"].size
    dets = torch.full((n, 3), SENTINEL)
    with soft_kernel(kernel):
        got = nms_1d_cpu.softnms(t(c["segs"]), t(c["scores"]), dets, float(c["thr"] if thr is None else thr), c["sigma"],
                                 c["min_score"], method).numpy()
        assert last_soft_kernels() == (expect_kernels or {kernel})
    dets = dets.numpy()
    assert (dets[got.size:] == SENTINEL).all()
    return got, dets[:got.size]


def soft_ref(c, method, thr=None):
    n = c["scores"].size
    rdets = torch.zeros(n, 3)
    want = ref_module().softnms(t(c["segs"]), t(c["scores"]), rdets, float(c["thr"] if thr is None else thr), c["sigma"],
                                c["min_score"], method).numpy()
    return want, rdets.numpy()[:want.size]


def check_soft_one(kernel, c, method, want, expect_kernels=None, thr=None):
    got, dets = soft_one(kernel, c, method, expect_kernels, thr)
    assert np.array_equal(got, want[0])
    dets_close(dets, want[1])
    rinds, rdets = soft_ref(c, method, thr)
    assert np.array_equal(got, rinds)
    dets_close(dets, rdets)
    return got, dets


@pytest.mark.parametrize("kernel,method", [("reg", 2), ("rows", 2), ("legacy", 2), ("rows", 0), ("legacy", 0), ("rows", 1), ("legacy", 1)])
def test_soft_power_of_two_sizes(dev, kernel, method):
    """sizes around a wave (64), the register kernel's workgroup (512), the other kernels' (1024) and the row kernel's load batch
    (8192), with an empty and a one-candidate class, in ONE launch per kernel"""
    from vilco_amd.utils.nms import last_soft_kernels, soft_kernel
    c = C.soft_pow2_case()
    want = C.soft_pow2_expected(method)
    ref = ref_module()
    with soft_kernel(kernel):
        dets, idx, cnt = soft_raw(dev, c["segs"], c["scores"], c["off"], c, method)
        assert last_soft_kernels() == {kernel}
    for k, n in enumerate(c["sizes"]):
        lo = int(c["off"][k])
        winds, wdets, _ = want[k]
        K = int(cnt[k])
        assert K == winds.size, (k, n)
        assert np.array_equal(idx[lo:lo + K], winds), (k, n)
        dets_close(dets[lo:lo + K], wdets)
        assert (dets[lo + K:lo + n] == SENTINEL).all()
        if n:
            rdets = torch.zeros(n, 3)
            rinds = ref.softnms(t(c["segs"][lo:lo + n]), t(c["scores"][lo:lo + n]), rdets, c["thr"], c["sigma"], c["min_score"],
                                method).numpy()
            assert np.array_equal(winds, rinds), (k, n)
            dets_close(dets[lo:lo + K], rdets.numpy()[:K])


@pytest.mark.parametrize("n,kernel,expect", [
    (C.REG_MAXN, "reg", {"reg"}),                                # the full register file: rmax == 60, every home in use
    (C.ROWS_MAXN, "rows", {"rows"}),                             # rows == 64: bit 63 of the masks, s_cnt[SROWS * NW] the total
    (C.ROWS_MAXN, "auto", {"reg", "rows"}),                      # the rows kernel's last size
    (C.ROWS_MAXN + 1, "auto", {"reg", "rows", "legacy"}),        # the first size that falls through to softnms_kernel
])
def test_soft_capacity(dev, n, kernel, expect):
    c = C.soft_capacity_case(n)
    check_soft_one(kernel, c, c["method"], C.soft_capacity_expected(n), expect)


@pytest.mark.parametrize("pick", [0, 1])
@pytest.mark.parametrize("ndead", [C.FILL_CAP, C.FILL_CAP + 1])
def test_soft_fill_cap(dev, pick, ndead):
    """softnms_reg_kernel with 16000 deaths in one pick (the survivor list still fits LDS) and 16001 (it spills to the global
    scratch array: full barrier, 32-bit entries), on pick 0 and on pick 1"""
    c = C.soft_fill_case(pick, ndead)
    want = C.soft_fill_expected(pick, ndead)
    assert want[2][pick] == ndead
    check_soft_one("reg", c, c["method"], want)


@pytest.mark.parametrize("n", C.SOFT_DIE_SIZES)
@pytest.mark.parametrize("from_start", [False, True])
@pytest.mark.parametrize("kernel", SOFT_KINDS)
def test_soft_everything_dies(dev, n, from_start, kernel):
    c = C.soft_all_die_case(n, from_start)
    winds, wdets = C.check_soft_all_die_case(c)
    got, dets = check_soft_one(kernel, c, 2, (winds, wdets))
    assert got.size == 1 and np.array_equal(dets, wdets)        # the pick's own row is never decayed: exact


@pytest.mark.parametrize("kernel", SOFT_KINDS)
def test_soft_stretch_skip_and_min_score_equality(dev, kernel):
    """a candidate touching the pick, a zero-width one inside it, one that overlaps nothing and starts below min_score (dies on
    pick 0), one that scores min_score exactly (survives: the test is <)"""
    c = C.soft_skip_case()
    winds, wdets = C.check_soft_skip_case()
    got, dets = check_soft_one(kernel, c, 2, (winds, wdets))
    assert C.SKIP_Q not in got
    for k in (C.SKIP_T, C.SKIP_Z, C.SKIP_E):
        assert dets[int(np.nonzero(got == k)[0][0]), 2] == c["scores"][k]


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("kernel", ["rows", "legacy"])
def test_soft_threshold_equality(dev, method, kernel):
    c = C.soft_threshold_pair_case()
    at, up = C.check_soft_threshold_pair_case(method)
    check_soft_one(kernel, c, method, at)
    check_soft_one(kernel, c, method, up, thr=c["thr_up"])


@pytest.mark.parametrize("kernel", SOFT_KINDS)
def test_soft_max_num(dev, kernel):
    """max_num at 1, at the unrestricted pick count K and beyond it: min(K, max_num) picks, the first rows those of the
    unrestricted run, dets rows beyond the count untouched"""
    from vilco_amd.utils.nms import last_soft_kernels, soft_kernel
    c = C.soft_maxnum_case()
    winds, wdets, _ = C.soft_maxnum_expected()
    K, n = C.check_soft_maxnum_case(), c["scores"].size
    off = C.offsets([n])
    with soft_kernel(kernel):
        full = soft_raw(dev, c["segs"], c["scores"], off, c, c["method"], 0)
        assert last_soft_kernels() == {kernel}
        runs = {m: soft_raw(dev, c["segs"], c["scores"], off, c, c["method"], m) for m in (1, K, K + 7)}
    assert int(full[2][0]) == K and np.array_equal(full[1][:K], winds)
    dets_close(full[0][:K], wdets)
    for m, (dets, idx, cnt) in runs.items():
        k = min(K, m)
        assert int(cnt[0]) == k, m
        assert np.array_equal(idx[:k], winds[:k]) and np.array_equal(dets[:k], full[0][:k]), m
        assert (dets[k:] == SENTINEL).all() and (idx[k:] == -1).all(), m


# ================================================================================================ batched_nms
@pytest.mark.parametrize("soft,min_score", [(True, 0.01), (False, 0.01), (False, 0.95)])
def test_batched_nms_class_ids_and_cuts(dev, soft, min_score):
    """class ids {0, 5, 21}; class 5 yields more than max_seg_num picks; on the hard path min_score = 0.95 lies above every score of
    class 21, which vanishes"""
    from oracle import nms_oracle
    from vilco_amd.utils.nms import batched_nms
    c = C.batched_case()
    C.check_batched_case()
    args = dict(iou_threshold=c["thr"], min_score=min_score, max_seg_num=c["max_seg_num"], use_soft_nms=soft, multiclass=True,
                sigma=c["sigma"], voting_thresh=0.0)
    gs, gsc, gc = batched_nms(t(c["segs"]), t(c["scores"]), t(c["cls"]), **args)
    ws, wsc, wc = nms_oracle.batched_nms(c["segs"], c["scores"], c["cls"], **args)
    assert 3 < wc.size <= c["max_seg_num"] and set(wc.tolist()) <= set(C.BATCHED_IDS)
    assert np.array_equal(gc.numpy(), wc)
    np.testing.assert_allclose(gs.numpy(), ws, rtol=1e-6)
    np.testing.assert_allclose(gsc.numpy(), wsc, rtol=1e-5, atol=1e-7)
    assert (21 in gc.numpy()) == (min_score < 0.95)


def test_batched_nms_everything_filtered(dev):
    """hard path, min_score above every score: the n == 0 return after the filter"""
    from oracle import nms_oracle
    from vilco_amd.utils.nms import batched_nms
    c = C.batched_case()
    args = dict(iou_threshold=c["thr"], min_score=1.0, max_seg_num=c["max_seg_num"], use_soft_nms=False, multiclass=True,
                sigma=c["sigma"], voting_thresh=0.0)
    ws, wsc, wc = nms_oracle.batched_nms(c["segs"], c["scores"], c["cls"], **args)
    assert ws.shape == (0, 2) and wsc.shape == (0,) and wc.shape == (0,)
    for where in ("cpu", dev):
        gs, gsc, gc = batched_nms(t(c["segs"]).to(where), t(c["scores"]).to(where), t(c["cls"]).to(where), **args)
        assert gs.shape == (0, 2) and gsc.shape == (0,) and gc.shape == (0,)
        assert gs.dtype == torch.float32 and gsc.dtype == torch.float32 and gc.dtype == torch.int64
        assert gs.device.type == gsc.device.type == gc.device.type == torch.device(where).type
