"""Sliding-window attention (mask mode 4 of vilco_attn_fwd / vilco_attn_bwd, ops.MASK_LOCAL) against the float64
restatement of tests/local_attention_restatement.py where its three tile-skipping kernels can go wrong: windows that end on,
one before and one past a 64-key / 32-query tile edge, lengths on and next to a tile edge, query rows with no key left, T off
the tile sizes, every head-width template, every operand precision, probability dropout, empty clips, and a window too
large for the kernels' int tile bounds.

Forward, dq, dk and dv are compared.  The measure is test_ops_gpu.rel taken per batch element (a slice whose reference is
identically zero must be identically zero); the bars are that module's: 2e-5 at the default precision and in split3, 5e-4
in split, 2e-2 in bf16.  Each test prints its worst figure per tensor before it asserts.

Rows with exactly ONE key -- window 0, a clip of length 1, T = 1 -- have the constant softmax 1, so dq and dk of such a clip
are exactly zero in the float64 reference (autograd: 1 * (dP - 1 * dP)) and the measure asks for exact zeros.  The kernels'
dS = P (dP - delta) takes dP from an MFMA over the operand planes and delta = dO . O from the stored fp32 output, which agree
to rounding only (that left max |dq|, |dk| of 1.3e-7 .. 1.35e-6 in 8 cases of the sweep, the ragged lengths and the
degenerate clips); the backward kernels therefore drop dS of such a row (one_key_row() in csrc/attn.hip)."""
import ctypes as C
import functools
import math

import pytest
import torch

import glue_restatement as G
import local_attention_restatement as LA
from test_ops_gpu import TOL_GEMM

pytestmark = pytest.mark.gpu

BARS = {None: TOL_GEMM, "split3": TOL_GEMM, "split": 5e-4, "bf16": 2e-2}
NAMES = ("o", "dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def inputs(B, T, H, hd, seed=0):
    """q, k, v, dout [B, T, H*hd] on the CPU (float32); shared, never modified"""
    g = torch.Generator().manual_seed(1000 * T + 10 * hd + seed)
    return tuple(torch.randn(B, T, H * hd, generator=g) for _ in range(4))


def run_hip(dev, q, k, v, dout, lens, H, scale, window, mode=None, drop_p=0.0):
    from vilco_amd import ops
    qg, kg, vg = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
    o = ops.attention(qg, kg, vg, lens.to(dev), H, scale, mode=ops.MASK_LOCAL if mode is None else mode, drop_p=drop_p, window=window)
    o.backward(dout.to(dev))
    torch.cuda.synchronize()
    return dict(o=o.detach(), dq=qg.grad, dk=kg.grad, dv=vg.grad)


def compare(tag, got, want, bar):
    """prints the figure of every tensor, then asserts them all"""
    errs, broken = {}, []
    for n in NAMES:
        try:
            errs[n] = LA.rel(got[n], want[n])
        except AssertionError as e:                   # a zero reference slice that is not zero in `got`
            errs[n] = math.inf
            broken.append("%s: %s" % (n, e))
    print("%-34s %s  (bar %.1e)" % (tag, "  ".join("%s %.3e" % (n, errs[n]) for n in NAMES), bar))
    assert not broken, (tag, broken)
    for n in NAMES:
        assert errs[n] < bar, (tag, n, errs[n], bar)
    return errs


def check(dev, B, T, H, hd, lens, window, bar=TOL_GEMM, tag=""):
    q, k, v, dout = inputs(B, T, H, hd)
    lens = torch.tensor(lens, dtype=torch.int32)
    scale = 1.0 / math.sqrt(hd)
    got = run_hip(dev, q, k, v, dout, lens, H, scale, window)
    want = LA.reference(q, k, v, lens, H, scale, window, dout)
    compare("%sT %d hd %d w %d lens %s" % (tag, T, hd, window, lens.tolist()), got, want, bar)
    return got, want


# ------------------------------------------------------------------------------------------------ a. tile-boundary sweep
SWEEP_T, SWEEP_LENS = 320, [320, 257, 64]


@pytest.mark.parametrize("window", [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 319, 320, 1000])
def test_window_sweep_across_tile_boundaries(dev, window):
    """T = 320: five 64-key tiles, ten 32-query tiles; len one key into a tile (257), on a tile edge (320, 64), and rows at or
    beyond 64 + w with no key.  w >= T - 1 covers everything: the result must also be what plain key masking gives.
    w = 0 leaves one key per row: dq and dk are exactly zero (see the module docstring)."""
    from vilco_amd import ops
    B, T, H, hd = 3, SWEEP_T, 2, 32
    got, _ = check(dev, B, T, H, hd, SWEEP_LENS, window)
    has = LA.row_has_key(torch.tensor(SWEEP_LENS), T, window)
    assert bool(has[2, :min(T, 64 + window)].all()) and not bool(has[2, 64 + window:].any())
    if window >= T - 1:
        q, k, v, dout = inputs(B, T, H, hd)
        lens = torch.tensor(SWEEP_LENS, dtype=torch.int32)
        keys = run_hip(dev, q, k, v, dout, lens, H, 1.0 / math.sqrt(hd), 0, mode=ops.MASK_KEYS)
        below = (torch.arange(T)[None, :] < lens[:, None])[:, :, None].to(dev)
        compare("  against MASK_KEYS below len", {n: got[n] * below for n in NAMES}, {n: keys[n] * below for n in NAMES}, TOL_GEMM)


# ------------------------------------------------------------------------------------------------ b. ragged lengths
@pytest.mark.parametrize("window", [1, 9, 64])
@pytest.mark.parametrize("T", [1, 2, 63, 65, 130, 193])
def test_ragged_lengths(dev, T, window):
    """T = 1 and the clip of length 1 at T = 2 have one key: dq = dk = 0 exactly (see the module docstring)"""
    check(dev, 2, T, 2, 64, [T, max(1, T - 9)], window)


# ------------------------------------------------------------------------------------------------ c. head widths
@pytest.mark.parametrize("window", [9, 70])
@pytest.mark.parametrize("hd", [4, 8, 24, 64, 96, 128, 132, 160])
def test_head_widths(dev, hd, window):
    """the four tile widths (32, 64, 128, 160), full and partly filled"""
    check(dev, 2, 193, 2, hd, [193, 120], window)


# ------------------------------------------------------------------------------------------------ d. precisions
@pytest.mark.parametrize("mode,hd", [("split3", 32), ("split3", 64), ("split", 32), ("bf16", 32)])
def test_precisions(dev, mode, hd):
    from vilco_amd import ops
    ops.set_precision(mode)
    try:
        check(dev, 2, 193, 2, hd, [193, 120], 33, bar=BARS[mode], tag=mode + " ")
    finally:
        ops.set_precision(None)


# ------------------------------------------------------------------------------------------------ e. probability dropout
@pytest.mark.parametrize("hd", [32, 96])
def test_probability_dropout(dev, hd):
    """the mask the kernels drew is recovered from the dropout log and handed to the restatement"""
    from vilco_amd import ops
    B, T, H, window = 2, 193, 2, 33
    q, k, v, dout = inputs(B, T, H, hd)
    lens = torch.tensor([193, 120], dtype=torch.int32)
    scale = 1.0 / math.sqrt(hd)
    ops.dropout_log = []
    try:
        got = run_hip(dev, q, k, v, dout, lens, H, scale, window, drop_p=0.2)
        (site, p, seed, shape), = ops.dropout_log
    finally:
        ops.dropout_log = None
    assert tuple(shape) == (B, H, T, T) and site == "attn_prob"
    keep = ops.dropout_mask(p, seed, shape, dev, site).double().cpu()
    assert 0.15 < float((keep == 0).double().mean()) < 0.25
    want = LA.reference(q, k, v, lens, H, scale, window, dout, keep)
    compare("dropout 0.2 T %d hd %d w %d" % (T, hd, window), got, want, TOL_GEMM)


# ------------------------------------------------------------------------------------------------ f. degenerate clips
@pytest.mark.parametrize("short", [1, 0])
def test_degenerate_clips(dev, short):
    """a clip of one key (dq = dk = 0 exactly, see the module docstring), and an empty one: exact zeros in everything of the
    empty clip, no NaN anywhere"""
    T = 130
    got, _ = check(dev, 2, T, 2, 64, [short, T], 9)
    for n in NAMES:
        assert bool(torch.isfinite(got[n]).all()), n
        if short == 0:
            assert int(torch.count_nonzero(got[n][0])) == 0, n


# ------------------------------------------------------------------------------------------------ g. exact structure
def test_exact_structure(dev):
    """Exact zeros where nothing is attended, and bitwise independence of everything outside the window.  The perturbed
    blocks are 150..191: keys (and queries) 128..149 of the same 64-wide tile stay as they were, and the rows that must not
    move (below 117 = 150 - 33, above 224 = 191 + 33) share the tiles 64..127 and 192..255 with rows that do.

    The default precision scales each operand by a power of two taken from the max|x| of the WHOLE tensor, so a perturbation
    that moves max|x| into another binade rescales every row's fp16 planes, and the smallest dS values of unrelated rows then
    round differently (measured without the pin below: o bitwise equal, dq not).  That is the format, not a leak between rows.
    One element of 12.0 in the last row of each tensor therefore holds max|x| in [8, 16) before and after (|randn| + 5 < 16)."""
    B, T, H, hd, w = 2, 320, 2, 32, 33
    L = [320, 200]
    q, k, v, dout = [t.clone() for t in inputs(B, T, H, hd)]
    for t in (q, k, v, dout):
        t[0, T - 1, 0] = 12.0
    lens = torch.tensor(L, dtype=torch.int32)
    scale = 1.0 / math.sqrt(hd)
    got = run_hip(dev, q, k, v, dout, lens, H, scale, w)
    compare("T %d hd %d w %d lens %s" % (T, hd, w, L), got, LA.reference(q, k, v, lens, H, scale, w, dout), TOL_GEMM)
    for n in NAMES:
        assert bool(torch.isfinite(got[n]).all()), n
    assert int(torch.count_nonzero(got["dk"][1, L[1]:])) == 0 and int(torch.count_nonzero(got["dv"][1, L[1]:])) == 0
    has = LA.row_has_key(lens, T, w).to(dev)
    assert int((~has).sum()) == T - (L[1] + w)
    assert int(torch.count_nonzero(got["o"][~has])) == 0 and int(torch.count_nonzero(got["dq"][~has])) == 0
    lo, hi = 150, 192
    still = torch.ones(T, dtype=torch.bool)
    still[lo - w:hi + w] = False                                   # rows no window connects with the block
    assert bool(still[lo - w - 1]) and not bool(still[lo - w]) and bool(still[hi + w]) and not bool(still[hi + w - 1])
    k2, v2 = k.clone(), v.clone()
    k2[:, lo:hi] += 5.0
    v2[:, lo:hi] += 5.0
    moved = run_hip(dev, q, k2, v2, dout, lens, H, scale, w)
    for n in ("o", "dq"):
        print("keys %d..%d moved: %-2s of the unreached queries changes by at most %.3e" % (
            lo, hi - 1, n, float((moved[n][:, still] - got[n][:, still]).abs().max())))
    for n in ("o", "dq"):
        assert torch.equal(moved[n][:, still], got[n][:, still]), n
        assert not torch.equal(moved[n][0, lo - w:hi + w], got[n][0, lo - w:hi + w]), n
    q2, d2 = q.clone(), dout.clone()
    q2[:, lo:hi] += 5.0
    d2[:, lo:hi] -= 3.0
    moved = run_hip(dev, q2, k, v, d2, lens, H, scale, w)
    for n in ("dk", "dv"):
        print("queries %d..%d moved: %-2s of the unreached keys changes by at most %.3e" % (
            lo, hi - 1, n, float((moved[n][:, still] - got[n][:, still]).abs().max())))
    for n in ("dk", "dv"):
        assert torch.equal(moved[n][:, still], got[n][:, still]), n
        assert not torch.equal(moved[n][0, lo - w:hi + w], got[n][0, lo - w:hi + w]), n


# ------------------------------------------------------------------------------------------------ h. every element written, none outside
@pytest.mark.parametrize("T,hd,lens,window", [(320, 32, [320, 257, 64], 33), (193, 132, [193, 120], 9)])
def test_c_abi_writes_every_element_and_nothing_else(dev, T, hd, lens, window):
    """vilco_attn_fwd / vilco_attn_bwd through the descriptor, as ops._flash_fwd / _flash_bwd fill it: o, lse, dq, dk, dv go
    into NaN-filled buffers between canaries"""
    from vilco_amd import _lib as L, ops
    lib = L.load()
    B, H = len(lens), 2
    Cn = H * hd
    q, k, v, dout = [t.to(dev).contiguous() for t in inputs(B, T, H, hd)]
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(hd)
    prec = ops.get_precision()
    bufs = {n: G.guarded(B * T * Cn, dev) for n in NAMES}
    lse, lse_check = G.guarded(B * H * T, dev)
    nf = lib.vilco_attn_fwd_workspace(B, H, T, T, hd, prec)
    nb = lib.vilco_attn_bwd_workspace(B, H, T, T, hd, prec)
    ws = torch.empty(max(nf, nb), dtype=torch.uint8, device=dev)
    common = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), kv_len=kv_len.data_ptr(), o=bufs["o"][0].data_ptr(),
                  lse=lse.data_ptr(), B=B, H=H, Tq=T, Tk=T, hd=hd, scale=scale, mode=ops.MASK_LOCAL, window=window,
                  precision=prec, drop_p=0.0, drop_seed=0, workspace=ws.data_ptr())
    d = L.AttnDesc(workspace_bytes=nf, **common)
    rc = lib.vilco_attn_fwd(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    d = L.AttnDesc(workspace_bytes=nb, dout=dout.data_ptr(), dq=bufs["dq"][0].data_ptr(), dk=bufs["dk"][0].data_ptr(),
                   dv=bufs["dv"][0].data_ptr(), **common)
    rc = lib.vilco_attn_bwd(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for n in NAMES:
        pay, canaries = bufs[n]
        left = int(torch.isnan(pay).sum())
        print("%-3s %d of %d elements left unwritten" % (n, left, pay.numel()))
        assert left == 0, n
        canaries()
    assert int(torch.isnan(lse).sum()) == 0
    lse_check()
    has = LA.row_has_key(kv_len.cpu(), T, window)
    dead = torch.isinf(lse.view(B, H, T)).cpu()
    assert torch.equal(dead, ~has[:, None, :].expand(B, H, T))           # lse = -inf exactly on the rows with no key
    cpu = inputs(B, T, H, hd)
    want = LA.reference(cpu[0], cpu[1], cpu[2], kv_len.cpu(), H, scale, window, cpu[3])
    compare("C ABI T %d hd %d w %d" % (T, hd, window), {n: bufs[n][0].view(B, T, Cn) for n in NAMES}, want, TOL_GEMM)


# ------------------------------------------------------------------------------------------------ i. huge window
@pytest.mark.parametrize("T", [65, 193])
@pytest.mark.parametrize("window", [2 ** 31 - 1, 2 ** 30])
def test_huge_window_is_window_T(dev, T, window):
    """a caller that spells "unbounded" as the largest int: the same bits as window = T (the launcher clamps to Tk)"""
    B, H, hd = 2, 2, 64
    q, k, v, dout = inputs(B, T, H, hd)
    lens = torch.tensor([T, max(1, T - 9)], dtype=torch.int32)
    scale = 1.0 / math.sqrt(hd)
    want = run_hip(dev, q, k, v, dout, lens, H, scale, T)
    got = run_hip(dev, q, k, v, dout, lens, H, scale, window)
    for n in NAMES:
        assert int(torch.count_nonzero(want[n])) > 0, n
        same = torch.equal(got[n], want[n])
        print("window %d T %d %-3s %s" % (window, T, n, "bitwise equal" if same else
                                         "differs: max |got| %.3e, max |want| %.3e" % (float(got[n].abs().max()), float(want[n].abs().max()))))
    for n in NAMES:
        assert torch.equal(got[n], want[n]), n
