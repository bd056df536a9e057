"""The memory-bound glue kernels (csrc/norm.hip, conv.hip, eltwise.hip) against the float64 restatements of
tests/glue_restatement.py at the shapes where such kernels go wrong: widths that take the guarded LayerNorm templates, widths
below one wave and off the vector width, second trips of every grid-stride loop, lengths 0 / 1 / odd, ties, constant rows.

Every output goes into a NaN-filled buffer between two canaries (glue_restatement.guarded): an element left unwritten or a
write outside the buffer fails.  Errors are taken per row against that row's own maximum (rowwise_err); the tolerances are
glue_restatement.BARS (4 x the fp32 CPU error of the same formula on the same inputs, tests/test_glue_restatement_cpu.py), the
worst-case fp32 summation bound n 2^-24 sum|term| for the column reductions, and bit equality wherever the result is a
copy, a maximum, a single product or an exact zero.  Each test prints its figures before it asserts.

The calls go through the C ABI with raw pointers (the ops wrappers allocate their outputs themselves), except where a
wrapper works in place or takes `out=` (ops.mask_rows_, ops._softmax_, ops.permute3)."""
import ctypes as ct

import pytest
import torch

import glue_restatement as R

pytestmark = pytest.mark.gpu

OK, BADARG, UNSUPPORTED = 0, -1, -2
NAN = float("nan")


def _L():
    import vilco_amd._lib as L
    return L, L.load()


def _s():
    from vilco_amd import ops
    return ops._stream()


def P(t):
    return None if t is None else t.data_ptr()


def to(dev, t):
    return None if t is None else t.to(dev).contiguous()


def out(dev, *shape, fill=NAN):
    n = 1
    for d in shape:
        n *= d
    pay, check = R.guarded(n, dev, fill)
    return pay.view(*shape), check


def words(nbytes, dev):
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=dev)


def within(name, value, bar):
    print("%-28s %.3e  (bar %.3e)" % (name, value, bar))
    assert value <= bar, (name, value, bar)


def summed(name, got, want, abs_terms, n):
    ok, ratio = R.sum_bound_ok(got, want, abs_terms, n)
    print("%-28s %.3f of n 2^-24 sum|term|, n = %d" % (name, ratio, n))
    assert ok, (name, ratio, n)


def same(got, want):
    """bit for bit (either zero sign), no NaN"""
    return got.shape == want.shape and torch.equal(got.cpu(), want.cpu().to(got.dtype))


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C,rows,variant", R.LN_CASES)
def test_layernorm(dev, C, rows, variant, relu):
    """vilco_layernorm_fwd / _bwd.  The backward is handed the REFERENCE's y, mean and rstd rounded to fp32, so it is judged on
    its own.

    dbeta: the summation bound n 2^-24 sum|term| with n = rows against the float64 reference (a term is a copy of dy).
    dgamma, twice.  (1) The same bound, n = rows, on the SUMMATION: the terms are g xhat with xhat = fl(fl(x - mean) rstd) as
    fp32 forms it from the same inputs (two correctly rounded operations, the same on any IEEE machine), summed in float64.
    That is what "fp32 summation of n terms in any order" bounds, one product rounding per term included.  (2) Against the
    float64 reference's terms, (n + 2) 2^-24 sum|term|: a term g (x - mean) rstd takes three fp32 roundings where the bound
    allows one, whatever the kernel does.  With n 2^-24 against the float64 terms the kernel -- which is not wrong -- measured
    1.887 x the bound at rows = 1 (C = 12, nothing to sum, one rounding allowed) and <= 0.56 from rows = 5 on (MI355X);
    against (1) it is at 0.84 at rows = 1.  A dropped or doubled row misses either bound by orders of magnitude.  The
    formation of xhat itself is held to the float64 reference by dx and its measured bar."""
    L, lib = _L()
    inp = R.ln_inputs(C, rows, variant)
    ref = R.ln_reference(inp, bool(relu), torch.float64)
    d = {k: to(dev, v) for k, v in inp.items()}
    fam = "ln_cancel_" if variant == "cancel" else "ln_"
    y, cy = out(dev, rows, C)
    mean, cm = out(dev, rows)
    rstd, cr = out(dev, rows)
    parts, cp = out(dev, 2048)
    n = ct.c_int32(0)
    fd = L.LnFwdDesc(x=P(d["x"]), gamma=P(d["gamma"]), beta=P(d["beta"]), y=P(y), mean=P(mean), rstd=P(rstd), rows=rows, C=C,
                     eps=R.LN_EPS, relu=relu, amax_parts=P(parts), n_parts=ct.addressof(n), row_mask=P(d["row_mask"]),
                     mask_rows=7 if d["row_mask"] is not None else 0)
    assert lib.vilco_layernorm_fwd(ct.byref(fd), _s()) == OK
    torch.cuda.synchronize()
    for c in (cy, cm, cr, cp):
        c()
    assert n.value == min((rows + 3) // 4, 2048) and same(parts[:n.value].max(), y.abs().max())

    sv = {k: to(dev, v) for k, v in ref["saved"].items()}
    dx, cdx = out(dev, rows, C)
    dg, cdg = out(dev, C)
    db, cdb = out(dev, C)
    parts2, cp2 = out(dev, 2048)
    ws = words(lib.vilco_layernorm_bwd_workspace(rows, C), dev)
    bd = L.LnBwdDesc(dy=P(d["dy"]), x=P(d["x"]), y=P(sv["y"]), gamma=P(d["gamma"]), mean=P(sv["mean"]), rstd=P(sv["rstd"]),
                     dres=P(d["dres"]), dx=P(dx), dgamma=P(dg), dbeta=P(db), rows=rows, C=C, relu=relu, workspace=P(ws),
                     workspace_bytes=ws.numel() * 4, dx_amax_parts=P(parts2), n_parts=ct.addressof(n))
    assert lib.vilco_layernorm_bwd(ct.byref(bd), _s()) == OK
    torch.cuda.synchronize()
    for c in (cdx, cdg, cdb, cp2):
        c()
    assert n.value == min((rows + 3) // 4, 256) and same(parts2[:n.value].max(), dx.abs().max())

    e = R.ln_errs(dict(y=y, mean=mean, rstd=rstd, dx=dx), ref, inp["x"])
    for k in ("y", "mean", "rstd", "dx"):
        within(fam + k, e[k], R.BARS[fam + k])
    summed("ln dbeta", db, ref["dbeta"], ref["dbeta_abs"], rows)
    if variant == "mask":
        off = (inp["row_mask"].repeat(rows // 7) == 0).to(dev)
        assert int(off.sum()) == 6 and bool((y[off] == 0).all())
        if relu:                                     # the saved y is 0 there: nothing but the residual's gradient passes
            assert same(dx[off], d["dres"][off])
    if variant == "const":
        want = torch.relu(d["beta"]) if relu else d["beta"]
        assert same(y, want.expand(rows, C)) and same(mean, torch.full((rows,), 3.0))
    if variant == "zerochan" and relu:
        ch = R.LN_ZERO_CHANNEL
        assert bool((y[:, ch] == 0).all()) and float(dg[ch]) == 0 and float(db[ch]) == 0
    xh = ((inp["x"] - ref["saved"]["mean"][:, None]) * ref["saved"]["rstd"][:, None]).double()      # fp32 xhat, then exact
    g = inp["dy"].double() * ((ref["saved"]["y"] > 0).double() if relu else 1.0)
    summed("ln dgamma (summation)", dg, (g * xh).sum(0), (g * xh).abs().sum(0), rows)
    ok, ratio = R.sum_bound_ok(dg, ref["dgamma"], ref["dgamma_abs"], rows + 2)
    print("ln dgamma (float64 terms)    %.3f of (n + 2) 2^-24 sum|term|, n = %d" % (ratio, rows))
    assert ok, ("ln dgamma (float64 terms)", ratio, rows)


def test_layernorm_status_without_launch(dev):
    L, lib = _L()
    buf = torch.zeros(2 * 4100 + 8, device=dev)
    st = torch.zeros(8, device=dev)
    ws = words(lib.vilco_layernorm_bwd_workspace(2, 4100), dev)

    def fwd(C, x=buf, **kw):
        d = L.LnFwdDesc(x=P(x), y=P(buf), mean=P(st), rstd=P(st), rows=2, C=C, eps=R.LN_EPS, **kw)
        return lib.vilco_layernorm_fwd(ct.byref(d), _s())

    def bwd(C, x=buf, dy=buf, dx=buf):
        d = L.LnBwdDesc(dy=P(dy), x=P(x), mean=P(st), rstd=P(st), dx=P(dx), rows=2, C=C, workspace=P(ws), workspace_bytes=ws.numel() * 4)
        return lib.vilco_layernorm_bwd(ct.byref(d), _s())
    assert fwd(6) == UNSUPPORTED and fwd(4100) == UNSUPPORTED and bwd(6) == UNSUPPORTED and bwd(4100) == UNSUPPORTED
    assert fwd(8, x=buf[1:]) == BADARG
    assert bwd(8, x=buf[1:]) == BADARG and bwd(8, dy=buf[1:]) == BADARG and bwd(8, dx=buf[1:]) == BADARG
    assert fwd(8, row_mask=P(st), mask_rows=0) == BADARG
    assert fwd(8) == OK and bwd(8) == OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ dwconv3 / maxpool3s2
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,lens", R.CONV_SHAPES)
def test_dwconv3(dev, shape, lens, stride):
    """rows with stride t' >= len are exactly 0 in y and feed nothing into dx / dw (a clip of length 0: y = dx = 0); dx alone
    and dw alone give the same bits as both together"""
    L, lib = _L()
    B, T, C = shape
    To = T // stride
    i = R.conv_inputs(shape, stride)
    lens = torch.tensor(lens, dtype=torch.int32)
    i64 = {k: v.double() for k, v in i.items()}
    ry = R.dwconv3_fwd(i64["x"], i64["w"], lens, stride)
    rdx, rdw, rabs, n = R.dwconv3_bwd(i64["dy"], i64["x"], i64["w"], lens, stride)
    d = {k: to(dev, v) for k, v in i.items()}
    ld = lens.to(dev)
    y, cy = out(dev, B, To, C)
    assert lib.vilco_dwconv3_fwd(P(d["x"]), P(d["w"]), P(ld), P(y), B, T, C, stride, _s()) == OK
    ws = words(lib.vilco_dwconv3_bwd_workspace(B, T, C, stride), dev)
    res = []
    for want_dx, want_dw in ((1, 1), (1, 0), (0, 1)):
        dx, cdx = out(dev, B, T, C)
        dw, cdw = out(dev, C, 3)
        assert lib.vilco_dwconv3_bwd(P(d["dy"]), P(d["x"]), P(d["w"]), P(ld), P(dx) if want_dx else None, P(dw) if want_dw else None,
                                     B, T, C, stride, P(ws), ws.numel() * 4, _s()) == OK
        torch.cuda.synchronize()
        cdx(), cdw(), cy()
        res.append((dx, dw))
    (dx, dw), (dx1, dw1), (dx2, dw2) = res
    assert same(dx1, dx) and same(dw2, dw) and bool(torch.isnan(dw1).all()) and bool(torch.isnan(dx2).all())
    within("dwconv3_y", R.rowwise_err(y, ry), R.BARS["dwconv3_y"])
    within("dwconv3_dx", R.rowwise_err(dx, rdx), R.BARS["dwconv3_dx"])
    summed("dwconv3 dw", dw, rdw, rabs, n)
    assert bool((y.cpu()[~R.valid_rows(lens, T, stride)] == 0).all())


def test_dwconv3_status_without_launch(dev):
    L, lib = _L()
    b = torch.zeros(256, device=dev)
    ln = torch.ones(2, dtype=torch.int32, device=dev)
    assert lib.vilco_dwconv3_fwd(P(b), P(b), P(ln), P(b), 1, 5, 4, 2, _s()) == UNSUPPORTED
    assert lib.vilco_dwconv3_fwd(P(b), P(b), P(ln), P(b), 1, 4, 6, 1, _s()) == UNSUPPORTED
    assert lib.vilco_dwconv3_bwd(P(b), P(b), P(b), P(ln), P(b), P(b), 1, 5, 4, 2, P(b), 1024, _s()) == UNSUPPORTED
    assert lib.vilco_dwconv3_bwd(P(b), P(b), P(b), P(ln), P(b), P(b), 1, 4, 6, 1, P(b), 1024, _s()) == UNSUPPORTED
    assert lib.vilco_maxpool3s2_fwd(P(b), P(ln), P(b), 1, 5, 4, _s()) == UNSUPPORTED


@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("shape,lens", R.CONV_SHAPES)
def test_maxpool3s2(dev, shape, lens, kind):
    """forward: a maximum, exact.  backward: every dx element is 0, one dy value or the sum of two, so the fp32 evaluation of the
    reference is its exact value too: bit for bit under ties (b: the FIRST maximum of a window takes the gradient, as aten's)
    and under all-negative input (c: the pad is -inf, not 0).  By design the kernel's fmaxf drops a NaN where aten propagates
    it; the workload's activations are finite (masked rows are zeros), and no NaN is fed here."""
    L, lib = _L()
    B, T, C = shape
    i = R.pool_inputs(shape, kind)
    lens = torch.tensor(lens, dtype=torch.int32)
    d = {k: to(dev, v) for k, v in i.items()}
    ld = lens.to(dev)
    y, cy = out(dev, B, T // 2, C)
    dx, cdx = out(dev, B, T, C)
    assert lib.vilco_maxpool3s2_fwd(P(d["x"]), P(ld), P(y), B, T, C, _s()) == OK
    assert lib.vilco_maxpool3s2_bwd(P(d["dy"]), P(d["x"]), P(ld), P(dx), B, T, C, _s()) == OK
    torch.cuda.synchronize()
    cy(), cdx()
    assert same(y, R.maxpool3s2_fwd(i["x"], lens))
    want = R.maxpool3s2_bwd(i["dy"], i["x"], lens)
    assert same(want.double(), R.maxpool3s2_bwd(i["dy"].double(), i["x"].double(), lens).float().double())
    assert same(dx, want)
    assert bool((y.cpu()[~R.valid_rows(lens, T, 2)] == 0).all())


# ------------------------------------------------------------------------------------------------ softmax / relshift
@pytest.mark.parametrize("Tk", R.SOFTMAX_TK)
@pytest.mark.parametrize("so", R.SOFTMAX_SCORES)
def test_softmax(dev, Tk, so):
    """vilco_softmax_fwd in modes 0 / 1 / 2 and vilco_softmax_bwd (on the reference's P rounded to fp32).  The backward's error is
    taken against sum_j |dP_j P_j| of the row (glue_restatement.softmax_bwd_err); rows whose P is one-hot give dS = 0 exactly."""
    from vilco_amd import ops
    L, lib = _L()
    fam = "softmax_off_" if so[1] else "softmax_"
    B, H = 2, 2
    for mode, Tq, kv in R.softmax_configs(Tk):
        i = R.softmax_inputs(Tk, Tq, so, mode)
        kvt = None if kv is None else torch.tensor(kv, dtype=torch.int32)
        ref = R.softmax_fwd(i["s"].double(), kvt, mode)
        s, cs = out(dev, B, H, Tq, Tk, fill=i["s"])
        ops._softmax_(s, to(dev, kvt), B, H, Tq, Tk, mode)
        torch.cuda.synchronize()
        cs()
        got = s.cpu()
        assert bool(torch.isfinite(got).all())
        within(fam + "fwd mode %d kv %s" % (mode, kv), R.rowwise_err(got, ref), R.BARS[fam + "fwd"])
        within(fam + "fwd row sums", float((got.double().sum(-1) - 1).abs().max()), R.BARS[fam + "fwd"])
        if mode == 0:
            pad = torch.arange(Tk)[None, None, None, :] >= kvt.long()[:, None, None, None]
            assert bool((got.masked_select(pad.expand_as(got)) == 0).all())
            for b in range(B):
                if kv[b] == 1:
                    assert bool((got[b, :, :, 0] == 1).all())
        if mode == 1:
            for b in range(B):
                if kv[b] == 0:              # nothing but the diagonal survives; a row without one (i >= Tk) comes out uniform
                    n = min(Tq, Tk)
                    assert same(got[b, :, :n], torch.eye(n, Tk).expand(H, n, Tk))
                    if Tq > Tk:
                        within("uniform rows", R.rowwise_err(got[b, :, Tk:], torch.full((H, Tq - Tk, Tk), 1.0 / Tk, dtype=torch.float64)),
                               R.BARS[fam + "fwd"])
        p = ref.float()
        dp, cdp = out(dev, B, H, Tq, Tk, fill=i["dp"])
        assert lib.vilco_softmax_bwd(P(dp), P(to(dev, p)), B, H, Tq, Tk, _s()) == OK
        torch.cuda.synchronize()
        cdp()
        ds = dp.cpu()
        within(fam + "bwd mode %d kv %s" % (mode, kv), R.softmax_bwd_err(ds, R.softmax_bwd(i["dp"].double(), p.double()), i["dp"], p),
               R.BARS[fam + "bwd"])
        onehot = (p != 0).sum(dim=-1) == 1
        assert bool((ds[onehot] == 0).all())


@pytest.mark.parametrize("T", [1, 2, 63, 65])
def test_relshift(dev, T):
    """one multiply per element: onto s = 0 the forward is the fp32 product scale * bd[i][T - i + j] bit for bit, the backward is
    scale * ds inside the band and exactly 0 (written, not left over) outside it.  Onto a random s the add is one more
    rounding, fused or not: |got - (s + scale bd)| <= 2 * 2^-24 (|s| + |scale bd|).  <relshift(bd), ds> = <bd, relshift_bwd(ds)>."""
    L, lib = _L()
    B, H, scale = 1, 3, 0.37
    g = R.gen(100 + T)
    bd, ds, s0 = torch.randn(H, T, 2 * T, generator=g), torch.randn(H, T, T, generator=g), torch.randn(H, T, T, generator=g)
    bd_d = to(dev, bd)
    z, cz = out(dev, H, T, T, fill=0.0)
    s, cs = out(dev, H, T, T, fill=s0)
    dbd, cd = out(dev, H, T, 2 * T)
    assert lib.vilco_relshift_add(P(z), P(bd_d), scale, B, H, T, _s()) == OK
    assert lib.vilco_relshift_add(P(s), P(bd_d), scale, B, H, T, _s()) == OK
    assert lib.vilco_relshift_bwd(P(to(dev, ds)), P(dbd), scale, B, H, T, _s()) == OK
    torch.cuda.synchronize()
    cz(), cs(), cd()
    assert same(z, scale * R.relshift(bd))
    prod = scale * R.relshift(bd.double())
    assert bool(((s.cpu().double() - (s0.double() + prod)).abs() <= 2 * R.U * (s0.double().abs() + prod.abs())).all())
    assert same(dbd, R.relshift_bwd(ds, scale))
    lhs, rhs = float((z.cpu().double() * ds.double()).sum()), float((bd.double() * dbd.cpu().double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), 1e-30)


# ------------------------------------------------------------------------------------------------ residual glue
@pytest.mark.parametrize("shape,lens", R.SCALE_ADD_SHAPES)
def test_scale_add(dev, shape, lens):
    """every presence combination of colscale / rowscale / len (mask_a 0 and 1 with len); da, db, dcolscale each alone NULL.
    A masked row of `a` adds exactly nothing: out there is the fp32 product (colscale rowscale) bval bit for bit, da is 0."""
    L, lib = _L()
    B, T, C = shape
    i = R.scale_add_inputs(shape)
    lens = torch.tensor(lens, dtype=torch.int32)
    i64 = {k: v.double() for k, v in i.items()}
    d = {k: to(dev, v) for k, v in i.items()}
    ld = lens.to(dev)
    ws = words(lib.vilco_colsum_workspace(B * T, C), dev)
    bar = R.BARS["scale_add"]
    for cs, rs, ln, ma in R.SCALE_ADD_COMBOS:
        pick = lambda s_: (s_["colscale"] if cs else None, s_["rowscale"] if rs else None)
        o, co = out(dev, B, T, C)
        assert lib.vilco_scale_add_fwd(P(o), P(d["a"]), P(d["b"]), P(pick(d)[0]), P(pick(d)[1]), P(ld) if ln else None, ma, B, T, C, _s()) == OK
        tag = "cs%d rs%d len%d mask_a%d" % (cs, rs, ln, ma)
        ref = R.scale_add_fwd(i64["a"], i64["b"], *pick(i64), lens if ln else None, ma)
        rda, rdb, rdc, rabs = R.scale_add_bwd(i64["dout"], i64["b"], *pick(i64), lens if ln else None, ma)
        full = (cs, rs, ln, ma) == (1, 1, 1, 1)
        for skip in ((None, "da", "db", "dcolscale") if full else (None,)):
            da, cda = out(dev, B, T, C)
            db, cdb = out(dev, B, T, C)
            dc, cdc = out(dev, C)
            parts, cp = out(dev, 2048)
            n = ct.c_int32(0)
            desc = L.ScaleAddBwdDesc(dout=P(d["dout"]), bval=P(d["b"]), colscale=P(pick(d)[0]), rowscale=P(pick(d)[1]),
                                     len=P(ld) if ln else None, mask_a=ma, da=None if skip == "da" else P(da),
                                     db=None if skip == "db" else P(db), dcolscale=None if skip == "dcolscale" else P(dc), B=B, T=T, C=C,
                                     workspace=P(ws), workspace_bytes=ws.numel() * 4, db_amax_parts=P(parts), n_parts=ct.addressof(n))
            assert lib.vilco_scale_add_bwd(ct.byref(desc), _s()) == OK
            torch.cuda.synchronize()
            co(), cda(), cdb(), cdc(), cp()
            if skip != "da":
                within("scale_add da " + tag, R.rowwise_err(da, rda), bar)
            else:
                assert bool(torch.isnan(da).all())
            if skip != "db":
                within("scale_add db " + tag, R.rowwise_err(db, rdb), bar)
                assert n.value >= 1 and same(parts[:n.value].max(), db.abs().max())
            else:
                assert bool(torch.isnan(db).all()) and n.value == 0
            if skip != "dcolscale":
                summed("scale_add dcolscale " + tag, dc, rdc, rabs, B * T)
            else:
                assert bool(torch.isnan(dc).all())
        within("scale_add out " + tag, R.rowwise_err(o, ref), bar)
        if ln and ma:
            off = ~R.valid_rows(lens, T)
            assert same(o.cpu()[off], R.scale_add_fwd(None, i["b"], *pick(i), None, 0)[off])


@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_GELU])
@pytest.mark.parametrize("shape,T,lens", R.ACT_SHAPES)
def test_act_bwd(dev, shape, T, lens, act, drop_p):
    """dz = dropmask(dy) act'(aux) rowmask with dbias / row_mask / the prefix mask on and off; aux holds exact 0, +-10, +-40
    (GELU' stays finite, RELU' at 0 is 0).  The dropout mask is the one vilco_dropout(x = NULL) writes for (p, seed), handed to
    the reference.  dbias: the summation bound against the column sums of the kernel's OWN dz (whose elements are held to the
    reference above) -- its terms as the kernel has them; and, where a term is a copy or one product (NONE, RELU), against the
    reference's terms as well.  GELU' through erff / expf is not a one-rounding term."""
    L, lib = _L()
    rows, C = shape
    i = R.act_inputs(shape)
    lens = torch.tensor(lens, dtype=torch.int32)
    i64 = {k: v.double() for k, v in i.items()}
    d = {k: to(dev, v) for k, v in i.items()}
    ld = lens.to(dev)
    seed = 1234
    dm = None
    if drop_p:
        dmd = torch.empty(rows, C, device=dev)
        assert lib.vilco_dropout(None, P(dmd), rows * C, drop_p, seed, 0, _s()) == OK
        dm = dmd.cpu()
        assert bool(((dm == 0) | (dm == torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(drop_p)))).all())
    ws = words(lib.vilco_colsum_workspace(rows, C), dev)
    for want_bias in (0, 1):
        for rm in (0, 1):
            for ln in (0, 1):
                dz, cdz = out(dev, rows, C)
                dbias, cdb = out(dev, C)
                desc = L.ActBwdDesc(dy=P(d["dy"]), aux=P(d["aux"]), dz=P(dz), dbias=P(dbias) if want_bias else None, act=act,
                                    len=P(ld) if ln else None, T=T, rows=rows, C=C, drop_p=drop_p, drop_seed=seed, workspace=P(ws),
                                    workspace_bytes=ws.numel() * 4, row_mask=P(d["row_mask"]) if rm else None)
                assert lib.vilco_act_bwd(ct.byref(desc), _s()) == OK
                torch.cuda.synchronize()
                cdz(), cdb()
                ref = R.act_bwd(i64["dy"], i64["aux"], act, lens if ln else None, T, i64["row_mask"] if rm else None,
                                None if dm is None else dm.double())
                got = dz.cpu()
                assert bool(torch.isfinite(got).all())
                within("act_bwd dz act%d bias%d rm%d len%d" % (act, want_bias, rm, ln), R.rowwise_err(got, ref), R.BARS["act_bwd"])
                if act == R.ACT_RELU:
                    assert bool((got[i["aux"] == 0] == 0).all())
                if want_bias:
                    summed("act_bwd dbias (own dz)", dbias, *R.colsum(got.double()), rows)
                    if act != R.ACT_GELU:
                        summed("act_bwd dbias (reference)", dbias, ref.sum(0), ref.abs().sum(0), rows)
                else:
                    assert bool(torch.isnan(dbias).all())


@pytest.mark.parametrize("C", [1, 63, 65, 300])
@pytest.mark.parametrize("rows", [1, 31, 33, 1000, 70001])
def test_colsum(dev, rows, C):
    L, lib = _L()
    x = torch.randn(rows, C, device=dev, generator=torch.Generator(device=dev).manual_seed(rows + C))
    want, wabs = R.colsum(x.double())
    ws = words(lib.vilco_colsum_workspace(rows, C), dev)
    o1, c1 = out(dev, C)
    o2, c2 = out(dev, C)
    for o in (o1, o2):
        assert lib.vilco_colsum(P(x), P(o), rows, C, P(ws), ws.numel() * 4, _s()) == OK
    torch.cuda.synchronize()
    c1(), c2()
    summed("colsum %d x %d" % (rows, C), o1, want, wabs, rows)
    assert same(o1, o2)


@pytest.mark.parametrize("C", R.GLUE_C)
def test_mask_rows_and_add_pe(dev, C):
    from vilco_amd import ops
    L, lib = _L()
    B, T = R.GLUE_BT
    i = R.glue_inputs(C)
    lens = torch.tensor(R.GLUE_LENS, dtype=torch.int32)
    ld = lens.to(dev)
    x, cx = out(dev, B, T, C, fill=i["x"])
    ops.mask_rows_(x, ld)
    o, co = out(dev, B, T, C)
    assert lib.vilco_add_pe(P(o), P(to(dev, i["x"])), P(to(dev, i["pe"])), P(ld), B, T, C, _s()) == OK
    torch.cuda.synchronize()
    cx(), co()
    assert same(x, R.mask_rows(i["x"], lens))
    within("add_pe", R.rowwise_err(o, R.add_pe(i["x"].double(), i["pe"].double(), lens)), R.BARS["add_pe"])
    off = ~R.valid_rows(lens, T)
    assert bool((x.cpu()[off] == 0).all()) and same(o.cpu()[off], i["x"][off])


@pytest.mark.parametrize("n", R.AXPBY_N)
def test_axpby(dev, n):
    L, lib = _L()
    i = R.axpby_inputs(n)
    al, be = R.AXPBY_AB
    a, b = to(dev, i["a"]), to(dev, i["b"])
    for bb, bd in ((None, None), (i["b"], b)):
        o, co = out(dev, n)
        assert lib.vilco_axpby(P(o), P(a), P(bd), al, be, n, _s()) == OK
        torch.cuda.synchronize()
        co()
        within("axpby", R.axpby_err(o.cpu(), R.axpby(i["a"].double(), R.dbl(bb), al, be), i["a"], bb, al, be), R.BARS["axpby"])


@pytest.mark.parametrize("batch,Rr,S", [(1, 1, 1), (2, 1, 70), (2, 70, 1), (3, 31, 33), (1, 64, 64), (2, 65, 127)])
def test_transpose2d(dev, batch, Rr, S):
    L, lib = _L()
    x = torch.randn(batch, Rr, S, generator=R.gen(batch + Rr + S))
    o, co = out(dev, batch, S, Rr)
    assert lib.vilco_transpose2d(P(to(dev, x)), P(o), batch, Rr, S, _s()) == OK
    torch.cuda.synchronize()
    co()
    assert same(o, R.transpose2d(x))


@pytest.mark.parametrize("d0", [5, 1])
def test_permute3_as_conv3_uses_it(dev, d0):
    """[Cout, Cin, 3] -> [Cout, 3, Cin] out of a larger buffer: non-zero offset, strides (3 Cin, 1, 3)"""
    from vilco_amd import ops
    Cin, off = 7, 4
    src = torch.randn(off + d0 * Cin * 3 + 5, generator=R.gen(d0))
    dims, strides = (d0, 3, Cin), (3 * Cin, 1, 3)
    o, co = out(dev, *dims)
    ops.permute3(to(dev, src), dims, off, strides, out=o)
    torch.cuda.synchronize()
    co()
    assert same(o, R.permute3(src, dims, off, strides))
    assert same(o, src[off:off + d0 * Cin * 3].reshape(d0, Cin, 3).permute(0, 2, 1))
