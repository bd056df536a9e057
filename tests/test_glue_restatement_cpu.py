"""The float64 restatements of tests/glue_restatement.py against torch.nn.functional and autograd (so that the GPU test's
reference is itself checked), and the committed tolerances BARS against the fp32 CPU error they are derived from."""
import math

import pytest
import torch
import torch.nn.functional as F

import glue_restatement as R

TIGHT = 1e-12


def _grad(out, dout, *ins):
    """gradients of <out, dout> for the inputs that are tensors (None for the others)"""
    got = iter(torch.autograd.grad(out, [t for t in ins if t is not None], dout, allow_unused=True))
    return tuple(None if t is None else next(got) for t in ins)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C,rows,variant", R.LN_CASES)
def test_layernorm_matches_functional_and_autograd(C, rows, variant, relu):
    inp = {k: R.dbl(v) for k, v in R.ln_inputs(C, rows, variant).items()}
    x = inp["x"].clone().requires_grad_(True)
    gamma = None if inp["gamma"] is None else inp["gamma"].clone().requires_grad_(True)
    beta = None if inp["beta"] is None else inp["beta"].clone().requires_grad_(True)
    y = F.layer_norm(x, (C,), gamma, beta, R.LN_EPS)
    if relu:
        y = torch.relu(y)
    if inp["row_mask"] is not None:
        y = y * inp["row_mask"].repeat(rows // 7)[:, None]
    got = R.layernorm(inp["x"], inp["gamma"], inp["beta"], R.LN_EPS, relu, inp["row_mask"], inp["dy"], inp["dres"])
    # x = 1000 + 0.01 randn: xhat is conditioned like mean / spread = 1e5, which float64 rounding is multiplied by
    assert R.rowwise_err(got[0], y) <= (1e-10 if variant == "cancel" else TIGHT)
    assert R.rowwise_err(got[1][:, None], inp["x"].mean(1)[:, None]) <= TIGHT
    assert R.rowwise_err(got[2][:, None], (inp["x"].var(1, unbiased=False) + R.LN_EPS).rsqrt()[:, None]) <= (1e-10 if variant == "cancel" else TIGHT)
    if variant == "const":
        # var = 0: aten's own backward differs from the formula by rounding of order rstd^2 = 1e5 here; the analytic values
        # instead: xhat = 0, so dx = rstd (g gamma - mean(g gamma)) + dres, dgamma = 0, dbeta = sum_r g
        g = inp["dy"] * (y.detach() > 0).double() if relu else inp["dy"]
        gg = g * inp["gamma"]
        want = (gg - gg.mean(1, keepdim=True)) / math.sqrt(R.LN_EPS)
        assert R.rowwise_err(got[3], want) <= TIGHT
        assert bool((got[4] == 0).all()) and R.rowwise_err(got[5][None], g.sum(0)[None]) <= TIGHT
        return
    dx, dg, db = _grad(y, inp["dy"], x, gamma, beta)
    if inp["dres"] is not None:
        dx = dx + inp["dres"]
    # 1e-12 of the row (column) maximum, except where the cancellation case amplifies float64 rounding (see above; rstd = 100)
    tol = 1e-7 if variant == "cancel" else TIGHT
    assert R.rowwise_err(got[3], dx) <= tol
    if gamma is not None:
        if variant == "zerochan" and relu:
            assert float(got[4][R.LN_ZERO_CHANNEL]) == 0 and float(got[5][R.LN_ZERO_CHANNEL]) == 0
        assert R.rowwise_err(got[4][None], dg[None]) <= (1e-7 if variant == "cancel" else TIGHT)
        assert R.rowwise_err(got[5][None], db[None]) <= TIGHT


def test_layernorm_constant_rows_and_masked_rows_are_exact():
    inp = {k: R.dbl(v) for k, v in R.ln_inputs(100, 5, "const").items()}
    y, mean, rstd = R.layernorm_fwd(inp["x"], inp["gamma"], inp["beta"], R.LN_EPS)
    assert torch.equal(y, inp["beta"].expand_as(y)) and torch.equal(mean, torch.full((5,), 3.0, dtype=torch.float64))
    assert torch.allclose(rstd, torch.full((5,), 1 / math.sqrt(R.LN_EPS), dtype=torch.float64), rtol=1e-15)
    inp = {k: R.dbl(v) for k, v in R.ln_inputs(100, 21, "mask").items()}
    y, _, _, dx, _, _ = R.layernorm(inp["x"], inp["gamma"], inp["beta"], R.LN_EPS, True, inp["row_mask"], inp["dy"], inp["dres"])
    off = inp["row_mask"].repeat(3) == 0
    assert int(off.sum()) == 6 and bool((y[off] == 0).all()) and torch.equal(dx[off], inp["dres"][off])


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,lens", R.CONV_SHAPES)
def test_dwconv3_matches_conv1d(shape, lens, stride):
    B, T, C = shape
    lens = torch.tensor(lens, dtype=torch.int32)
    i = {k: v.double() for k, v in R.conv_inputs(shape, stride).items()}
    x, w = i["x"].clone().requires_grad_(True), i["w"].clone().requires_grad_(True)
    y = F.conv1d(x.transpose(1, 2), w[:, None, :], stride=stride, padding=1, groups=C).transpose(1, 2)
    y = y * R.valid_rows(lens, T, stride)[..., None]
    assert y.shape == (B, T // stride, C)
    assert R.rowwise_err(R.dwconv3_fwd(i["x"], i["w"], lens, stride), y) <= TIGHT
    dx, dw = _grad(y, i["dy"], x, w)
    gdx, gdw, gabs, n = R.dwconv3_bwd(i["dy"], i["x"], i["w"], lens, stride)
    assert R.rowwise_err(gdx, dx) <= TIGHT
    assert n == B * (T // stride) and bool((gabs >= gdw.abs() - 1e-9).all())
    assert R.rowwise_err(gdw.reshape(1, -1), dw.reshape(1, -1), scale=gabs.max()[None]) <= TIGHT
    for b in range(B):
        if int(lens[b]) == 0:
            assert bool((R.dwconv3_fwd(i["x"], i["w"], lens, stride)[b] == 0).all()) and bool((gdx[b] == 0).all())


@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("shape,lens", R.CONV_SHAPES)
def test_maxpool_matches_max_pool1d_first_maximum_wins(shape, lens, kind):
    B, T, C = shape
    lens = torch.tensor(lens, dtype=torch.int32)
    i = {k: v.double() for k, v in R.pool_inputs(shape, kind).items()}
    x = i["x"].clone().requires_grad_(True)
    y = F.max_pool1d(x.transpose(1, 2), 3, 2, 1).transpose(1, 2) * R.valid_rows(lens, T, 2)[..., None]
    assert torch.equal(R.maxpool3s2_fwd(i["x"], lens), y.detach())
    (dx,) = _grad(y, i["dy"], x)
    assert torch.equal(R.maxpool3s2_bwd(i["dy"], i["x"], lens), dx)       # ties included: the first maximum takes the gradient
    if kind == "b" and T >= 6:
        win = i["x"].unfold(1, 2, 2)
        assert float((win[..., 0] == win[..., 1]).double().mean()) > 0.2  # the input does tie


@pytest.mark.parametrize("Tk", R.SOFTMAX_TK)
@pytest.mark.parametrize("so", R.SOFTMAX_SCORES)
def test_softmax_matches_torch(Tk, so):
    for mode, Tq, kv in R.softmax_configs(Tk):
        i = R.softmax_inputs(Tk, Tq, so, mode)
        s = i["s"].double().requires_grad_(True)
        kvt = None if kv is None else torch.tensor(kv, dtype=torch.int32)
        got = R.softmax_fwd(i["s"].double(), kvt, mode)
        if mode == 2:
            want = torch.softmax(s, dim=-1)
        else:
            pad = torch.arange(Tk)[None, None, None, :] >= kvt.long()[:, None, None, None]
            if mode == 0:
                want = torch.softmax(s.masked_fill(pad, -math.inf), dim=-1)
            else:
                off = pad & ~torch.eye(Tq, Tk, dtype=torch.bool)[None, None]
                want = torch.softmax(s - 1e30 * off.double(), dim=-1)      # as the model writes it
        assert R.rowwise_err(got, want) <= TIGHT
        assert bool(torch.isfinite(got).all()) and float((got.sum(-1) - 1).abs().max()) <= 1e-12
        if mode == 0:
            assert bool((got.masked_select(pad.expand_as(got)) == 0).all())
        if mode == 1 and kv[1] == 0 and Tq > Tk:
            assert torch.equal(got[1, :, Tk:], torch.full_like(got[1, :, Tk:], 1.0 / Tk))      # everything masked: uniform
            assert torch.equal(got[1, 0, :Tk], torch.eye(Tk, dtype=torch.float64))             # the diagonal survives
        (ds,) = _grad(want, i["dp"].double(), s)
        p = want.detach()
        assert R.softmax_bwd_err(R.softmax_bwd(i["dp"].double(), p), ds, i["dp"], p) <= TIGHT


@pytest.mark.parametrize("T", [1, 2, 63, 65])
def test_relshift_is_rel_shift_bnij_and_its_adjoint(T):
    g = R.gen(T)
    bd, ds = torch.randn(3, T, 2 * T, generator=g, dtype=torch.float64), torch.randn(3, T, T, generator=g, dtype=torch.float64)
    x = bd[None]                                                      # rel_shift_bnij as test_rel_attention writes it out
    xs = x.shape
    want = x.reshape(xs[0], xs[1], xs[3], xs[2])[:, :, 1:, :].reshape(xs[0], xs[1], xs[2], xs[3] - 1)[:, :, :, :T][0]
    assert torch.equal(R.relshift(bd), want)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    assert torch.equal(R.relshift(bd), torch.gather(bd, 2, (T - i + j)[None].expand(3, T, T)))
    dbd = R.relshift_bwd(ds, 0.37)
    lhs, rhs = (0.37 * R.relshift(bd) * ds).sum(), (bd * dbd).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * max(1.0, abs(float(lhs)))
    assert int((dbd != 0).sum()) <= 3 * T * T


@pytest.mark.parametrize("shape,lens", R.SCALE_ADD_SHAPES[:5])
def test_scale_add_and_act_bwd_match_autograd(shape, lens):
    B, T, C = shape
    lens = torch.tensor(lens, dtype=torch.int32)
    i = {k: v.double() for k, v in R.scale_add_inputs(shape).items()}
    for cs, rs, ln, ma in R.SCALE_ADD_COMBOS:
        a, b, c = (i[k].clone().requires_grad_(True) for k in ("a", "b", "colscale"))
        m = R.prefix_mask(lens, T, torch.float64) if (ln and ma) else 1.0
        out = a * m + (c if cs else 1.0) * (i["rowscale"][:, None, None] if rs else 1.0) * b
        opt = (i["colscale"] if cs else None, i["rowscale"] if rs else None, lens if ln else None, ma)
        assert R.rowwise_err(R.scale_add_fwd(i["a"], i["b"], *opt), out) <= TIGHT
        da, db, dc = _grad(out, i["dout"], a, b, c)
        gda, gdb, gdc, gabs = R.scale_add_bwd(i["dout"], i["b"], *opt)
        assert R.rowwise_err(gda, da) <= TIGHT and R.rowwise_err(gdb, db) <= TIGHT
        if cs:      # dcolscale is defined at colscale = 1 too; autograd only sees it when colscale is an input
            assert R.rowwise_err((gdc * 1.0)[None], dc[None], scale=gabs.max()[None] + 1e-300) <= TIGHT


@pytest.mark.parametrize("shape,T,lens", R.ACT_SHAPES)
def test_act_bwd_matches_autograd(shape, T, lens):
    rows, C = shape
    lens = torch.tensor(lens, dtype=torch.int32)
    i = {k: v.double() for k, v in R.act_inputs(shape).items()}
    dm = (torch.rand(shape, generator=R.gen(1)) >= 0.3).double() / 0.7
    for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_GELU):
        z = i["aux"].clone().requires_grad_(True)
        h = [z, torch.relu(z), F.gelu(z)][act]
        out = h * dm * R.prefix_mask(lens, T, torch.float64).reshape(rows, 1) * i["row_mask"][:, None]
        (dz,) = _grad(out, i["dy"], z)
        got = R.act_bwd(i["dy"], i["aux"], act, lens, T, i["row_mask"], dm)
        assert bool(torch.isfinite(got).all())
        assert R.rowwise_err(got, dz) <= TIGHT
        if act == R.ACT_RELU:
            assert bool((got[i["aux"] == 0] == 0).all())
    if i["aux"].numel() >= 15:
        assert sorted(i["aux"].reshape(-1)[1:15:3].tolist()) == sorted(R.ACT_SPECIALS)


def test_small_glue_references():
    lens = torch.tensor(R.GLUE_LENS, dtype=torch.int32)
    for C in R.GLUE_C:
        i = {k: v.double() for k, v in R.glue_inputs(C).items()}
        m, a = R.mask_rows(i["x"], lens), R.add_pe(i["x"], i["pe"], lens)
        for b, n in enumerate(R.GLUE_LENS):
            assert bool((m[b, n:] == 0).all()) and torch.equal(m[b, :n], i["x"][b, :n])
            assert torch.equal(a[b, n:], i["x"][b, n:]) and torch.equal(a[b, :n], i["x"][b, :n] + i["pe"][:n])
    x = torch.randn(3, 31, 33, generator=R.gen(2), dtype=torch.float64)
    assert torch.equal(R.transpose2d(x), x.permute(0, 2, 1).contiguous())
    w = torch.randn(4 + 5 * 7 * 3, generator=R.gen(3), dtype=torch.float64)
    assert torch.equal(R.permute3(w, (5, 3, 7), 4, (21, 1, 3)), w[4:].reshape(5, 7, 3).permute(0, 2, 1).contiguous())
    s, sa = R.colsum(x[0])
    assert torch.allclose(s, x[0].sum(0)) and torch.equal(sa, x[0].abs().sum(0))
    assert torch.equal(R.axpby(x, None, 2.0, 3.0), 2.0 * x)


def test_comparison_helpers():
    want = torch.tensor([[1.0, 2.0], [0.0, 0.0], [1e-6, 0.0]], dtype=torch.float64)
    got = want.clone()
    got[2, 0] = 2e-6                      # a wrong SMALL row: invisible to a global metric, an error of 1 here
    assert R.rowwise_err(got, want) == pytest.approx(1.0)
    assert R.rowwise_err(got, want, cols=True) == pytest.approx(1e-6)
    got[1, 1] = 1e-30
    with pytest.raises(AssertionError):
        R.rowwise_err(got, want)
    got[1, 1] = float("nan")
    with pytest.raises(AssertionError):
        R.rowwise_err(got, want)
    got[1, 1] = -0.0
    got[0, 0] = float("nan")
    assert R.rowwise_err(got, want) == math.inf
    ok, ratio = R.sum_bound_ok(torch.tensor([3.0 + 3 * R.U]), torch.tensor([3.0], dtype=torch.float64), torch.tensor([3.0]), 3)
    assert ok and ratio < 1
    assert not R.sum_bound_ok(torch.tensor([2.0]), torch.tensor([3.0], dtype=torch.float64), torch.tensor([3.0]), 3)[0]   # a dropped row
    pay, check = R.guarded(5, torch.device("cpu"))
    assert pay.numel() == 5 and bool(torch.isnan(pay).all())
    pay.fill_(1.0)
    check()
    pay.data.as_strided((1,), (1,), pay.storage_offset() + 5).fill_(0.0)      # one float past the end
    with pytest.raises(AssertionError):
        check()


def test_bars_are_four_times_the_fp32_cpu_error():
    """every measured family: committed bar >= the recomputed fp32 CPU error and <= 8x it (the floor 2^-22 aside), so a bar
    cannot be loosened quietly -- and none is missing or left over"""
    measured = R.measure_fp32_errors()
    assert set(measured) == set(R.BARS)
    for k, e in measured.items():
        assert R.BARS[k] >= e, (k, R.BARS[k], e)
        assert R.BARS[k] <= max(8 * e, R.FLOOR), (k, R.BARS[k], e)
        assert R.BARS[k] >= R.FLOOR
