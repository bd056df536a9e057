"""XLNet's relative attention (ops.rel_attention, vilco_xl_scores; mask mode 3 of vilco_attn_fwd / vilco_attn_bwd) against the
float64 restatement of tests/xl_attention_restatement.py where its kernels can go wrong: the position-score kernel at the ends
of every row's band, odd T, T on, one before and one past the 64-key tile / 128-row workgroup edges, lengths on and next to a
tile edge, at 1 and at 0, every head-width template, kr shared and per clip, B = 1 and B = 2 (the two ways dkr is reduced),
every switch that sends the op down another path (band-limited GEMM scores, fp32 dS + relshift pack, no pack reuse, the
materialised path), the operand precisions, and probability dropout.

Forward and the five gradients (dqw, dqr, dk, dv, dkr) are compared.  The measure is test_ops_gpu.rel taken per batch element
(a slice whose reference is identically zero must be identically zero; a shared kr's gradient is one tensor); the bars are that
module's: TOL_GEMM = 2e-5 at the default precision (f16x2) and in split3, 5e-4 in split.  Each test prints its worst figure per
tensor before it asserts.

What the tests found, and what was changed for it (csrc/attn.hip):

1. xl_scores64_kernel stored a lane's four columns p .. p+3 only when p + 3 < 2T.  For odd T, 2T = 2 (mod 4), so the last
   group p = 2T - 2 was never stored: bd[b,h,0,2T-2], bd[b,h,0,2T-1] and bd[b,h,1,2T-2] -- the position scores of (i=0, j=T-2),
   (i=0, j=T-1) and (i=1, j=T-1) -- kept whatever the buffer held, and at T = 1 nothing was stored at all.  Shown by
   test_position_scores_fill_every_band at every odd T (1, 3, 63, 65, 127, 129, 191, 193, 257): before the fix exactly those
   three entries per (b, h) -- the one band entry per (b, h) at T = 1 -- were still the NaN the buffer was filled with, every
   other band entry was within the bar, and every even T passed.  test_T_sweep at T = 1, 63, 65, 127, 129, 193 (and the
   T = 65, hd = 64 cases of the other groups on that kernel) then read the poisoned entries and returned NaN in o and in every
   gradient.  Now the last group stores its in-range columns one by one; every other group keeps the 16-byte store.
2. Rows with ONE visible key under the XLNet mask -- an empty clip (kv_len = 0: each query sees only its own position), row 0
   of a clip of length 1, T = 1 -- have the constant softmax 1, so dqw, dqr, dk (and a per-clip dkr) of such a row are exactly
   zero in the float64 reference and the measure asks for exact zeros.  The kernels' dS = P (dP - delta) left rounding there:
   test_empty_clip, all eight cases, max |dqw|, |dqr|, |dk| of the empty clip 0.9e-6 .. 2.2e-6 and max |dkr| of it up to
   4.4e-6 before the change, general kernels (hd 32) and hd = 64 XL kernels alike.  one_key_row() now knows the XLNet mask, and
   the hd = 64 XL backward kernels drop dS of such a row as the general ones do; o and dv of the row are untouched.

Worst figure per tensor over each case group, MI355X, after the fixes:
    group (cases)                      o         dqw       dqr       dk        dv        dkr       bar
    a  position scores (48)            3.72e-07 over the band entries, none left unwritten          2e-5
    b  T sweep (10)                    5.82e-07  3.79e-06  3.04e-06  3.90e-06  2.31e-06  1.54e-06  2e-5
    c  lengths (6)                     5.12e-07  1.77e-06  1.79e-06  1.57e-06  1.47e-06  9.96e-07  2e-5
    c0 empty clip (8)                  6.17e-07  1.98e-06  1.92e-06  1.22e-06  1.82e-06  1.53e-06  2e-5
    d  head widths, kr layouts (48)    9.35e-07  1.98e-06  1.92e-06  1.47e-06  1.97e-06  1.64e-06  2e-5
    e  xl_scores_kernel off (6)        6.74e-07  2.34e-06  2.22e-06  1.48e-06  1.97e-06  2.58e-06  2e-5
    e  xl_ds_planes off (6)            6.17e-07  1.98e-06  2.29e-06  1.50e-06  1.97e-06  2.75e-06  2e-5
    e  _reuse_packs off (6)            6.17e-07  1.98e-06  2.29e-06  1.50e-06  1.97e-06  2.75e-06  2e-5
    e  use_flash off (3)               7.63e-07  5.86e-07  7.29e-07  4.51e-07  6.10e-07  4.18e-07  2e-5
    e  split3 (6)                      6.86e-07  7.28e-07  7.58e-07  7.04e-07  7.04e-07  5.58e-07  2e-5
    e  split (6)                       1.32e-05  1.54e-05  1.67e-05  1.73e-05  1.38e-05  1.30e-05  5e-4
    f  probability dropout (8)         4.95e-07  1.88e-06  1.84e-06  1.67e-06  2.01e-06  1.90e-06  2e-5"""
import functools
import math

import pytest
import torch

import glue_restatement as G
import xl_attention_restatement as XL
from test_ops_gpu import TOL_GEMM

pytestmark = pytest.mark.gpu

BARS = {None: TOL_GEMM, "split3": TOL_GEMM, "split": 5e-4}
NAMES = XL.NAMES


@functools.lru_cache(maxsize=None)
def inputs(B, T, H, hd, per_clip):
    """qw, qr, k, v, dout [B, T, H*hd] and kr [2T, H*hd] or [B, 2T, H*hd] on the CPU (float32); shared, never modified"""
    g = torch.Generator().manual_seed(100000 * B + 100 * T + hd + 50000 * int(per_clip))
    qw, qr, k, v, dout = [torch.randn(B, T, H * hd, generator=g) for _ in range(5)]
    kr = torch.randn(*((B,) if per_clip else ()), 2 * T, H * hd, generator=g)
    return qw, qr, k, v, dout, kr


@functools.lru_cache(maxsize=None)
def wanted(B, T, H, hd, per_clip, lens):
    """the float64 reference without dropout, computed once per problem"""
    qw, qr, k, v, dout, kr = inputs(B, T, H, hd, per_clip)
    return XL.reference(qw, qr, k, v, kr, torch.tensor(lens, dtype=torch.int32), H, 1.0 / math.sqrt(hd), dout)


def run_hip(dev, B, T, H, hd, per_clip, lens, drop_p=0.0, poison=True):
    from vilco_amd import ops
    qw, qr, k, v, dout, kr = inputs(B, T, H, hd, per_clip)
    leaves = [t.to(dev).requires_grad_(True) for t in (qw, qr, k, v, kr)]
    kv_len, g = torch.tensor(lens, dtype=torch.int32, device=dev), dout.to(dev)
    if poison:       # the caching allocator most likely hands this block to the op's torch.empty for bd
        junk = torch.full((B * H * T * 2 * T,), float("nan"), dtype=torch.float32, device=dev)
        del junk
    o = ops.rel_attention(*leaves, kv_len, H, 1.0 / math.sqrt(hd), drop_p=drop_p)
    o.backward(g)
    torch.cuda.synchronize()
    return dict(zip(NAMES, [o.detach()] + [t.grad for t in leaves]))


def compare(tag, got, want, bar):
    """prints the figure of every tensor, then asserts them all"""
    errs, broken = {}, []
    for n in NAMES:
        assert got[n].shape == want[n].shape, (tag, n, tuple(got[n].shape), tuple(want[n].shape))
        try:
            errs[n] = XL.rel_of(n, got[n], want[n])
        except AssertionError as e:                   # a zero reference slice that is not zero in `got`
            errs[n] = math.inf
            broken.append("%s: %s" % (n, e))
    print("%-52s %s  (bar %.1e)" % (tag, "  ".join("%s %.3e" % (n, errs[n]) for n in NAMES), bar))
    assert not broken, (tag, broken)
    for n in NAMES:
        assert errs[n] < bar, (tag, n, errs[n], bar)
    return errs


def check(dev, group, B, T, H, hd, per_clip, lens, bar=TOL_GEMM, tag=""):
    got = run_hip(dev, B, T, H, hd, per_clip, lens)
    want = wanted(B, T, H, hd, per_clip, tuple(lens))
    compare("xl[%s] %sB %d T %d hd %d %s lens %s" % (group, tag, B, T, hd, "clip" if per_clip else "shared", list(lens)), got, want, bar)
    return got, want


# ------------------------------------------------------------------------------------------------ a. position scores alone
WS_PAD = 512


@pytest.mark.parametrize("per_clip", [0, 1])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 193, 257])
def test_position_scores_fill_every_band(dev, T, B, per_clip):
    """vilco_xl_scores into a NaN-filled bd between canaries, its workspace between guard bytes: every element of every row's
    band p in [T - i, 2T - i) is written and is qr_i . kr_p; nothing outside bd or the workspace is touched.  Outside the band
    the kernel may write or not (its 16-byte stores spill up to three columns past a band edge, inside the row)."""
    from vilco_amd import _lib, ops
    lib = _lib.load()
    H, hd, prec = 2, 64, 3
    _, qr, _, _, _, kr = inputs(B, T, H, hd, bool(per_clip))
    want = XL.position_scores(qr.double(), kr.double(), H)                     # [B, H, T, 2T]
    band = XL.band_mask(T)
    qg, kg = qr.to(dev).contiguous(), kr.to(dev).contiguous()
    bd, canaries = G.guarded(B * H * T * 2 * T, dev)
    nws = int(lib.vilco_xl_scores_workspace(B, H, T, per_clip))
    ws = torch.full((nws + 2 * WS_PAD,), 0xA5, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256 + 256
    rc = lib.vilco_xl_scores(qg.data_ptr(), kg.data_ptr(), bd.data_ptr(), B, H, T, hd, per_clip, prec, ws.data_ptr() + off, nws,
                             ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = bd.view(B, H, T, 2 * T).cpu().double()
    inside, ref = got[..., band], want[..., band]
    holes = (~torch.isfinite(got)) & band
    where = [tuple(x) for x in holes.nonzero().tolist()[:8]]
    finite = torch.isfinite(inside)
    err = float((inside - ref)[finite].abs().max() / ref.abs().max()) if bool(finite.any()) else math.inf
    print("xl[a] B %d T %d %s: %d of %d band entries not finite %s; the others: %.3e  (bar %.1e)" % (
        B, T, "clip" if per_clip else "shared", int(holes.sum()), inside.numel(), where, err, TOL_GEMM))
    assert int(holes.sum()) == 0, (T, where)
    assert err < TOL_GEMM, (T, err)
    canaries()
    w = ws.cpu()
    assert bool((w[:off] == 0xA5).all()), "write in front of the workspace"
    assert bool((w[off + nws:] == 0xA5).all()), "write past the end of the workspace"


# ------------------------------------------------------------------------------------------------ b. T sweep
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 127, 128, 129, 192, 193])
def test_T_sweep(dev, T):
    """hd = 64, default switches: the position-score kernel, the hd = 64 XL forward and backward kernels, dS as operand planes
    from the dQ kernel when T % 64 == 0 and as fp32 dS + relshift pack otherwise.  bd most likely lands in NaN-filled memory."""
    check(dev, "b", 2, T, 2, 64, False, (T, max(1, T - 9)))


# ------------------------------------------------------------------------------------------------ c. lengths
def _triples(T):
    return [(T, 64, 1), (65, 63, 2), (T - 1, 128 if T > 128 else 127, 1)]


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("T", [130, 128])
def test_lengths(dev, T, which):
    """lengths on a 64-key tile edge and next to one, at 1 (row 0 of that clip has one key) and at T"""
    check(dev, "c", 3, T, 2, 64, False, _triples(T)[which])


@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("T", [130, 128])
def test_empty_clip(dev, T, hd, per_clip):
    """lens = [T, 0]: every row of the empty clip sees only its own key -- o = v, dv = dout, and dqw, dqr, dk (per clip: dkr)
    of that clip exactly zero (see the module docstring).  hd 64: the XL kernels; hd 32: the general ones."""
    got, _ = check(dev, "c0", 2, T, 2, hd, per_clip, (T, 0))
    for n in ("dqw", "dqr", "dk") + (("dkr",) if per_clip else ()):
        assert int(torch.count_nonzero(got[n][1])) == 0, n
    for n in NAMES:
        assert bool(torch.isfinite(got[n]).all()), n


# ------------------------------------------------------------------------------------------------ d. head widths, kr layout
@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [65, 130])
@pytest.mark.parametrize("hd", [8, 32, 64, 96, 128, 160])
def test_head_widths_and_kr_layouts(dev, hd, T, B, per_clip):
    """the four tile widths of the general kernels and the hd = 64 XL kernels; B = 1: dkr is the batch's only slice, B = 2 and a
    shared kr: the sum over the batch.  Position 0 is picked by no (i, j): its row of dkr is exactly zero."""
    lens = (T, T - 9)[2 - B:]
    got, _ = check(dev, "d", B, T, 2, hd, per_clip, lens)
    assert int(torch.count_nonzero(got["dkr"][..., 0, :])) == 0


# ------------------------------------------------------------------------------------------------ e. switches and precisions
SWITCHES = [("xl_scores_kernel", False), ("xl_scores_kernel", True), ("xl_ds_planes", False), ("xl_ds_planes", True),
            ("_reuse_packs", False), ("_reuse_packs", True), ("use_flash", False)]


@pytest.mark.parametrize("T", [64, 65, 130])
@pytest.mark.parametrize("switch,per_clip", SWITCHES)
def test_switches(dev, switch, per_clip, T):
    """xl_scores_kernel off: the band-1 GEMM writes bd; xl_ds_planes off: fp32 dS + relshift pack at T % 64 == 0 too;
    _reuse_packs off: relshift_bwd and the per-batch dkr loop; use_flash off: the materialised path (shared kr only)"""
    from vilco_amd import ops
    before = getattr(ops, switch)
    assert before is True
    setattr(ops, switch, False)
    try:
        check(dev, "e", 2, T, 2, 64, per_clip, (T, max(1, T - 9)), tag="%s=0 " % switch)
    finally:
        setattr(ops, switch, before)


@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("T", [64, 65, 130])
@pytest.mark.parametrize("mode", ["split3", "split"])
def test_precisions(dev, mode, T, hd):
    from vilco_amd import ops
    ops.set_precision(mode)
    try:
        check(dev, "e-" + mode, 2, T, 2, hd, False, (T, max(1, T - 9)), bar=BARS[mode], tag=mode + " ")
    finally:
        ops.set_precision(None)


# ------------------------------------------------------------------------------------------------ f. probability dropout
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("T", [65, 128])
@pytest.mark.parametrize("drop_p", [0.2, 0.5])
def test_probability_dropout(dev, drop_p, T, hd):
    """per-clip kr; the mask the kernels drew is recovered from the dropout log and handed to the restatement"""
    from vilco_amd import ops
    B, H, lens = 2, 2, (T, T - 9)
    ops.dropout_log = []
    try:
        got = run_hip(dev, B, T, H, hd, True, lens, drop_p=drop_p)
        (site, p, seed, shape), = ops.dropout_log
    finally:
        ops.dropout_log = None
    assert tuple(shape) == (B, H, T, T) and site == "attn_prob" and p == drop_p
    keep = ops.dropout_mask(p, seed, shape, dev, site).double().cpu()
    assert abs(float((keep == 0).double().mean()) - drop_p) < 0.05
    qw, qr, k, v, dout, kr = inputs(B, T, H, hd, True)
    want = XL.reference(qw, qr, k, v, kr, torch.tensor(lens, dtype=torch.int32), H, 1.0 / math.sqrt(hd), dout, keep)
    compare("xl[f] drop %.1f T %d hd %d clip lens %s" % (drop_p, T, hd, list(lens)), got, want, TOL_GEMM)
