"""Grouped single-part products (vilco_gemm_group, precision 4: gemm_pp_group_kernel) and the collector that runs a backward's
equal weight gradients through it (ops._dw_gemm / ops._dw_group_flush).

Reference, as in test_ops_gpu.py::test_single_part_products_two_k_steps_per_interval: the fp16 leading parts of both operands
multiplied in float64 on the host -- here read back from vilco_pack's own planes -- and that test's bound for a single-part
product, 2e-6 of max|want| (fp32 accumulation of exact fp16 x fp16 products).  The reference has no counterpart of the grouping
(autograd computes each nn.Linear's weight gradient alone, MQ/libs/modeling/blocks.py)."""
import ctypes

import pytest
import torch

from parity_util import build_hip_model, golden_inputs, load_golden

pytestmark = pytest.mark.gpu

BOUND = 2e-6            # test_single_part_products_two_k_steps_per_interval's bound
HDR = 4096 + 512        # vilco_pack buffers: amax partials, {1/s, s}, then the planes


def rel(got, want):
    want, got = want.double().cpu(), got.double().cpu()
    return ((got - want).abs().max() / (want.abs().max() + 1e-12)).item()


def lead_of_planes(planes, rows, cols):
    """the leading fp16 part of a packed [rows][cols] tensor, unscaled, float64"""
    hdr = planes[:HDR].view(torch.float32)
    inv_s = float(hdr[1024])
    r32, c32 = (rows + 31) // 32 * 32, (cols + 31) // 32 * 32
    body = planes[HDR:].view(torch.float16)[:r32 * c32].view(r32, c32)
    return body[:rows, :cols].double().cpu() * inv_s


def operands(form, M, N, K, dev, gen):
    def rn(*s):
        return torch.randn(*s, generator=gen).to(dev)
    if form == "nt":
        A, B = rn(M, K), rn(N, K)
        return A, B, (1, 1, K, K), lambda a, b: a @ b.t()
    if form == "nn":
        A, B = rn(M, K), rn(K, N)
        return A, B, (1, 0, K, N), lambda a, b: a @ b
    A, B = rn(K, M), rn(K, N)
    return A, B, (0, 0, M, N), lambda a, b: a.t() @ b


def make_group(form, M, N, K, n, dev):
    from vilco_amd import ops
    gen = torch.Generator().manual_seed(1000 * n + M + N + K)
    calls, wants, outs, keep = [], [], [], []
    for i in range(n):
        A, B, (a_kc, b_kc, lda, ldb), mm = operands(form, M, N, K, dev, gen)
        pa, pb = ops.pack(A, A.shape[0], A.shape[1]), ops.pack(B, B.shape[0], B.shape[1])
        wants.append(mm(lead_of_planes(pa, *A.shape), lead_of_planes(pb, *B.shape)))
        C = torch.full((M, N), float("nan"), device=dev)
        outs.append(C)
        keep.append((A, B, pa, pb))
        calls.append(((None, None, C, M, N, K, a_kc, b_kc, lda, ldb, N), dict(precision=4, a_planes=pa, b_planes=pb)))
    return calls, wants, outs, keep


def profiled(fn):
    """run fn between vilco_gemm_profile_begin / end; returns the launch records (M, N, K, batch | group size, BM, ksplit, ...)"""
    from vilco_amd import _lib
    lib = _lib.load()
    _lib.check(lib.vilco_gemm_profile_begin())
    fn()
    torch.cuda.synchronize()
    ms, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
    _lib.check(lib.vilco_gemm_profile_end(ctypes.byref(ms), ctypes.byref(cnt)))
    desc = (ctypes.c_int64 * (10 * max(cnt.value, 1)))()
    n = lib.vilco_gemm_profile_records(desc, None, cnt.value)
    return [tuple(desc[i * 10:(i + 1) * 10]) for i in range(n)]


SHAPES = [(128, 128, 64),        # one tile, one interval
          (192, 128, 96),        # a ragged last K2 interval (K not a multiple of 64)
          (256, 384, 200),       # K not a multiple of 32
          (130, 136, 128)]       # partial edge tiles in both directions


@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_grouped_products_match_float64_and_the_single_launches(dev, M, N, K, form):
    """n = 1, 2, 5, 16 products as one vilco_gemm_group call: each against the float64 product of its planes' leading parts;
    bit-equal to one launch per product with vilco_gemm_force(0, 1) (one split: the same arithmetic in the same order); and
    the default plan of the lone launch under the same bound."""
    from vilco_amd import _lib, ops
    lib = _lib.load()
    for n in (1, 2, 5, 16):
        calls, wants, outs, keep = make_group(form, M, N, K, n, dev)
        recs = profiled(lambda: ops.gemm_group(calls))
        if n > 1:
            assert len(recs) == 1 and recs[0][3] == n and recs[0][6] == 4 and recs[0][5] == 1, recs      # one launch, no split
        for C, want in zip(outs, wants):
            assert rel(C, want) < BOUND, (n, rel(C, want))
        plain = [torch.empty_like(C) for C in outs]
        for (a, k), P in zip(calls, plain):                    # today's plan of the lone product
            ops.gemm(*a[:2], P, *a[3:], **k)
        for P, want in zip(plain, wants):
            assert rel(P, want) < BOUND
        _lib.check(lib.vilco_gemm_force(0, 1))
        try:
            for (a, k), C in zip(calls, outs):
                P = torch.empty_like(C)
                ops.gemm(*a[:2], P, *a[3:], **k)
                assert torch.equal(P, C), (n, rel(P, C))
        finally:
            _lib.check(lib.vilco_gemm_force(0, 0))


@pytest.mark.parametrize("tall", [False, True])
def test_a_group_short_of_a_round_takes_a_split(dev, tall):
    """n x tiles < 256 with a long contraction: the plan splits K (slabs + the ordinary slab sum) and still matches"""
    from vilco_amd import ops
    M, N, K, n = (256, 128, 4096, 3) if tall else (128, 128, 2048, 2)
    calls, wants, outs, keep = make_group("tn", M, N, K, n, dev)
    recs = profiled(lambda: ops.gemm_group(calls))
    assert len(recs) == 1 and recs[0][3] == n and recs[0][5] > 1, recs
    for C, want in zip(outs, wants):
        assert rel(C, want) < BOUND, rel(C, want)


def test_a_group_of_many_tiles_runs_on_256_row_tiles(dev):
    """16 x 24 tiles of 128 rows are 1.5 rounds, 16 x 12 of 256 rows fit one: the plan takes the 256-row tile (K not a multiple
    of 32: the last interval reads the planes' zero padding), bit-equal to the lone launches with one split"""
    from vilco_amd import _lib, ops
    lib = _lib.load()
    calls, wants, outs, keep = make_group("tn", 1024, 384, 200, 16, dev)
    recs = profiled(lambda: ops.gemm_group(calls))
    assert len(recs) == 1 and recs[0][3] == 16 and recs[0][4] == 256 and recs[0][5] == 1, recs
    for C, want in zip(outs, wants):
        assert rel(C, want) < BOUND, rel(C, want)
    _lib.check(lib.vilco_gemm_force(0, 1))
    try:
        for (a, k), C in list(zip(calls, outs))[::5]:
            P = torch.empty_like(C)
            ops.gemm(*a[:2], P, *a[3:], **k)
            assert torch.equal(P, C)
    finally:
        _lib.check(lib.vilco_gemm_force(0, 0))


def test_more_products_than_one_launch_holds(dev):
    """19 products: two launches (10 + 9), every product right"""
    from vilco_amd import ops
    calls, wants, outs, keep = make_group("tn", 130, 136, 128, 19, dev)
    recs = profiled(lambda: ops.gemm_group(calls))
    assert sorted(r[3] for r in recs) == [9, 10], recs
    for C, want in zip(outs, wants):
        assert rel(C, want) < BOUND


def test_the_switch_and_a_forced_plan_leave_the_group_ungrouped(dev):
    from vilco_amd import _lib, ops
    lib = _lib.load()
    calls, wants, outs, keep = make_group("tn", 128, 128, 64, 3, dev)
    gen0 = lib.vilco_gemm_config_gen()
    _lib.check(lib.vilco_gemm_set_group_dw(0))
    try:
        assert lib.vilco_gemm_config_gen() > gen0 and lib.vilco_gemm_group_dw() == 0
        recs = profiled(lambda: ops.gemm_group(calls))
        assert len(recs) == 3 and all(r[3] == 1 for r in recs), recs
    finally:
        _lib.check(lib.vilco_gemm_set_group_dw(1))
    _lib.check(lib.vilco_gemm_force(128, 0))
    try:
        recs = profiled(lambda: ops.gemm_group(calls))
        assert len(recs) == 3, recs
    finally:
        _lib.check(lib.vilco_gemm_force(0, 0))
    for C, want in zip(outs, wants):
        assert rel(C, want) < BOUND


# ---- model level: the two-block golden transformer (T = 128, D = 128, H = 2), weight gradients taken single-part from K = 64 on
def other_batch(gold):
    """the golden clips with their features reversed in time: the shapes the graph was captured with, other values"""
    return [dict(d, feats=d['feats'].flip(-1).contiguous()) for d in golden_inputs(gold)]


@pytest.fixture
def short_single_part():
    from vilco_amd import _lib, ops
    keep = ops.DW_FAST_MIN_K
    ops.DW_FAST_MIN_K = 64
    yield
    ops.DW_FAST_MIN_K = keep
    _lib.check(_lib.load().vilco_gemm_set_group_dw(1))
    _lib.check(_lib.load().vilco_seed_word_set(0, None))
    torch.cuda.synchronize()


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_model_gradients_grouped_replayed_and_ungrouped(dev, short_single_part):
    """switch on: eager and replayed parameter gradients are torch.equal (on a batch the graph was not captured with), and
    the collector really groups; switch off: gradients within the single-part bound of the grouped ones (every compared tensor
    is kept away from zero norm by tests/test_gemm_group_dw_cpu.py)."""
    from vilco_amd import _lib, ops
    from vilco_amd.graph import GraphedStep
    lib = _lib.load()
    gold = load_golden("noxl")
    first, second = golden_inputs(gold), other_batch(gold)
    first = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for d in first]
    second = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for d in second]

    def make():
        m = build_hip_model(gold, dev).train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
            if hasattr(mod, "drop_prob"):
                mod.drop_prob = 0.0
        m.loss_normalizer = 100.0
        return m

    def eager(m, batch):
        for p in m.parameters():
            p.grad = None
        m(batch, task_id=gold['task_id'], is_training=True)['final_loss'].backward()
        torch.cuda.synchronize()
        return _grads(m)

    def atomics(n):      # (loss.hip adds the gaussian-weight / regression-scale gradients with float atomics: equal up to their order)
        return any(t in n for t in ("mu", "sigma", "scale"))

    def same(a, b, n):
        return torch.equal(a, b) or (atomics(n) and torch.allclose(a, b, rtol=1e-5, atol=1e-9))

    # every run takes the same three steps (the loss normaliser moves with each): first, first, second
    me = make()
    eager(me, first)
    eager(me, first)
    recs = profiled(lambda: eager(me, second))
    groups = [r for r in recs if r[6] == 4 and r[3] > 1]
    assert groups, "no grouped single-part launch in the backward: %s" % [r for r in recs if r[6] == 4]
    want = _grads(me)
    mg = make()
    gs = GraphedStep(mg, None, eager_steps=1)
    gs(first, task_id=gold['task_id'])           # eager
    gs(first, task_id=gold['task_id'])           # capture + replay
    gs(second, task_id=gold['task_id'])          # replay on other values
    torch.cuda.synchronize()
    assert gs.stats['replayed'] >= 2, gs.stats
    got = _grads(mg)
    assert set(got) == set(want)
    for n in want:
        assert same(got[n], want[n], n), n
    _lib.check(lib.vilco_gemm_set_group_dw(0))
    mo = make()
    eager(mo, first)
    eager(mo, first)
    recs = profiled(lambda: eager(mo, second))
    assert [r for r in recs if r[6] == 4] and not [r for r in recs if r[6] == 4 and r[3] > 1]
    off = _grads(mo)
    for n in want:
        g = want[n]
        if n.endswith("weight") and g.dim() >= 2 and g.shape[0] > 1 and g.shape[1] > 1:
            # a matrix product's weight: one pass over K against the sum of the split plan's slabs
            assert rel(off[n], want[n]) < BOUND, (n, rel(off[n], want[n]))
        else:                           # nothing else depends on how a weight gradient was summed
            assert same(off[n], want[n], n), n
