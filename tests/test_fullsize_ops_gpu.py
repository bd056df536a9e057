"""The public ops at the signatures the full-size training steps really call, each against float64, forward + backward.

FULL_SIZE_SIGNATURES (tests/fullsize_op_table.py) lists every (op, shapes, actual lengths / row masks, path flags) that one
eager step of config P (as benchmarked), config W and cfg1 calls; `test_op_at_step_signature` runs each entry in isolation
against a float64 restatement on the GPU (the style of test_ops_gpu.run_pair; bars as there: 2e-5 for GEMM-backed and
elementwise ops, the qkv_pre gradients at test_qkvpre_gpu's 1e-4; dropout masks replayed from ops.dropout_log).  Upstream
gradients carry exact max|x| partials, as a producing kernel leaves them, so the backward passes take the paths the step
takes (act_bwd_planes*, the LayerNorm backward's amax partials).  `test_step_signatures_are_in_the_table` runs the three
steps under the recorder and fails on any signature the table does not hold.

Exempt (held elsewhere): see fullsize_op_sigs.EXEMPT."""
import math

import pytest
import torch
import torch.nn.functional as F

from fullsize_op_sigs import EXEMPT, RECORDED, Recorder, freeze
from fullsize_op_table import FULL_SIZE_SIGNATURES

pytestmark = pytest.mark.gpu

TOL_GEMM = 2e-5
TOL_EW = 2e-5
TOL_EXACT = 1e-7
TOL_QKV_GRAD = 1e-4            # tests/test_qkvpre_gpu.py


def _rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-12))


def _rowmask(rle, dev):
    return torch.cat([torch.full((n,), float(v), dtype=torch.float64, device=dev) for v, n in rle])


def _lensmask(lens, T, dev):
    return (torch.arange(T, device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None]).double()


def _taps(x):
    """[B, T, C] -> [B, T, 3C] = [x[t-1] | x[t] | x[t+1]] (zero outside the sequence)"""
    T = x.shape[1]
    p = F.pad(x, (0, 0, 1, 1))
    return torch.cat([p[:, 0:T], p[:, 1:T + 1], p[:, 2:T + 2]], -1)


def _ln(x, g, b, eps):
    r = x - x.mean(-1, keepdim=True)
    return r / torch.sqrt((r * r).mean(-1, keepdim=True) + eps) * g + b


def _drop_masks(dev):
    from vilco_amd import ops
    return [ops.dropout_mask(p, seed, shape, dev, site).double() for site, p, seed, shape in ops.dropout_log]


def _rel_ref(qw, qr, k, v, kr, lens, H, scale, pmask):
    """XLNet relative attention (modeling_xlnet_x.py:256-320, rel_shift_bnij), as tests/test_ops_gpu.py::test_rel_attention;
    kr [2T, C] shared or [B, 2T, C] per clip; pmask: dropout factors on the probabilities or None"""
    B, T, C = qw.shape
    hd = C // H
    f = lambda x: x.view(B, T, H, hd).permute(1, 0, 2, 3)          # ibnd
    ac = torch.einsum("ibnd,jbnd->bnij", f(qw), f(k))
    krr = (kr.view(2 * T, 1, H, hd).expand(2 * T, B, H, hd) if kr.dim() == 2 else kr.view(B, 2 * T, H, hd).permute(1, 0, 2, 3))
    bd = torch.einsum("ibnd,jbnd->bnij", f(qr), krr)
    xs = bd.shape
    bd = bd.reshape(xs[0], xs[1], xs[3], xs[2])[:, :, 1:, :].reshape(xs[0], xs[1], xs[2], xs[3] - 1)[:, :, :, :T]
    score = (ac + bd) * scale
    pad = 1.0 - _lensmask(lens, T, qw.device)
    mask = ((pad[:, None, None, :] - torch.eye(T, dtype=torch.float64, device=qw.device)[None, None]) > 0).double()
    score = score - 1e30 * mask
    p = torch.softmax(score, dim=3)
    if pmask is not None:
        p = p * pmask
    o = torch.einsum("bnij,jbnd->ibnd", p, f(v))
    return o.permute(1, 0, 2, 3).reshape(B, T, C)


# ------------------------------------------------------------------------------------------------ one case per op
# each returns (inputs: name -> float64 tensor, names that take a gradient, hip(**fp32 inputs) -> tensor(s),
# ref(**fp64 inputs, masks=dropout factors) -> tensor(s), forward bar, gradient bar)
def _case(op, d, dev):
    from vilco_amd import ops
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device=dev)
    rg = d.get("rg", ())
    if op == "linear":
        K, N = d["x"][-1], d["w"][0]
        inp = dict(x=rn(*d["x"]), w=rn(N, K) / math.sqrt(K), b=rn(N) * 0.1)
        grad = [n for n, r in zip(("x", "w", "b"), rg) if r]
        lens = None if d["lens"] is None else torch.tensor(d["lens"], dtype=torch.int32, device=dev)
        if not d["bias"]:
            del inp["b"]

        def hip(x, w, b=None):
            return ops.linear(x, w, b, d["act"], lens, d["T"], d["drop_p"], "dropout", d["bwd_precision"])

        def ref(x, w, b=None, masks=()):
            y = x @ w.t() + (0 if b is None else b)
            y = torch.relu(y) if d["act"] == ops.ACT_RELU else (F.gelu(y) if d["act"] == ops.ACT_GELU else y)
            if lens is not None:
                m = _lensmask(d["lens"], d["T"], dev).reshape(-1, 1)
                y = (y.reshape(-1, N) * m).reshape(y.shape)
            for mk in masks:
                y = y * mk.reshape(y.shape)
            return y
        return inp, grad, hip, ref, TOL_GEMM, TOL_GEMM
    if op == "linear_group":
        n, K, N = d["n"], d["x"][-1], d["w"][0]
        inp = {}
        for i in range(n):
            inp.update({"x%d" % i: rn(*d["x"]), "w%d" % i: rn(N, K) / math.sqrt(K), "b%d" % i: rn(N) * 0.1})
        grad = [k for k in inp if (k[0] == "x" and rg[0]) or (k[0] in "wb" and rg[1])]

        def hip(**t):
            return tuple(ops.linear_group([t["x%d" % i] for i in range(n)], [t["w%d" % i] for i in range(n)],
                                          [t["b%d" % i] for i in range(n)]))

        def ref(masks=(), **t):
            return tuple(t["x%d" % i] @ t["w%d" % i].t() + t["b%d" % i] for i in range(n))
        return inp, grad, hip, ref, TOL_GEMM, TOL_GEMM
    if op == "linear_kn":
        K = d["x"][-1]
        N = math.prod(d["w"]) // K
        inp = dict(x=rn(*d["x"]), w=rn(*d["w"]) / math.sqrt(K), b=rn(N) * 0.1)
        if not d["bias"]:
            del inp["b"]
        grad = [n for n, r in zip(("x", "w", "b"), rg) if r and n in inp]
        return (inp, grad, lambda x, w, b=None: ops.linear_kn(x, w, b),
                lambda x, w, b=None, masks=(): x @ w.reshape(K, N) + (0 if b is None else b), TOL_GEMM, TOL_GEMM)
    if op == "conv3":
        B, T, Cin = d["x"]
        Cout = d["w"][0]
        inp = dict(x=rn(B, T, Cin), w=rn(Cout, Cin, 3) / math.sqrt(3 * Cin), b=rn(Cout) * 0.1)
        if not d["bias"]:
            del inp["b"]
        grad = [n for n, r in zip(("x", "w", "b"), rg) if r and n in inp]
        lens = None if d["lens"] is None else torch.tensor(d["lens"], dtype=torch.int32, device=dev)
        rm = None if d["row_mask"] is None else _rowmask(d["row_mask"], dev)
        if lens is not None:
            m = _lensmask(d["lens"], T, dev)[..., None]
        elif rm is not None:
            m = rm.reshape(B, T, 1)
        else:
            m = None

        def hip(x, w, b=None):
            return ops.conv3(x, w, b, lens, None if rm is None else rm.float().reshape(B, T).contiguous())

        def ref(x, w, b=None, masks=()):
            y = _taps(x) @ w.permute(0, 2, 1).reshape(Cout, 3 * Cin).t() + (0 if b is None else b)
            return y if m is None else y * m
        return inp, grad, hip, ref, TOL_GEMM, TOL_GEMM
    if op == "layernorm":
        C = d["x"][-1]
        inp = dict(x=rn(*d["x"]) * 2 + 0.5, g=1 + 0.3 * rn(C), bt=0.3 * rn(C))
        grad = [n for n, r in zip(("x", "g", "bt"), rg) if r]
        rm = None if d["row_mask"] is None else _rowmask(d["row_mask"], dev)

        def hip(x, g, bt):
            out = ops.layernorm(x, g, bt, d["eps"], d["relu"], planes=d["planes"],
                                row_mask=None if rm is None else rm.float().contiguous(), skip=d["skip"])
            return tuple(out) if d["skip"] else out

        def ref(x, g, bt, masks=()):
            y = _ln(x, g, bt, d["eps"])
            if d["relu"]:
                y = torch.relu(y)
            if rm is not None:          # one mask entry per row, repeating every rm.numel() rows
                y = (y.reshape(-1, rm.numel(), C) * rm[None, :, None]).reshape(y.shape)
            return (y, x) if d["skip"] else y
        return inp, grad, hip, ref, TOL_EW, TOL_EW
    if op == "dwconv3":
        B, T, C = d["x"]
        s = d["stride"]
        inp = dict(x=rn(B, T, C), w=rn(C, 1, 3))
        grad = [n for n, r in zip(("x", "w"), rg) if r]
        lens = torch.tensor(d["lens"], dtype=torch.int32, device=dev)

        def ref(x, w, masks=()):
            y = (_taps(x).view(B, T, 3, C) * w[:, 0, :].t()).sum(2)[:, ::s]
            m = (s * torch.arange(T // s, device=dev)[None, :] < lens[:, None]).double()[..., None]
            return y[:, :T // s] * m
        return inp, grad, lambda x, w: ops.dwconv3(x, w, lens, s), ref, TOL_EW, TOL_EW
    if op == "maxpool3s2":
        B, T, C = d["x"]
        lens = torch.tensor(d["lens"], dtype=torch.int32, device=dev)

        def ref(x, masks=()):
            m = (2 * torch.arange(T // 2, device=dev)[None, :] < lens[:, None]).double()[..., None]
            return F.max_pool1d(x.transpose(1, 2), 3, 2, 1).transpose(1, 2) * m
        return dict(x=rn(B, T, C)), ["x"] if rg[0] else [], lambda x: ops.maxpool3s2(x, lens), ref, TOL_EW, TOL_EW
    if op == "scale_add":
        B, T, C = d["b"]
        inp = dict(b=rn(B, T, C))
        if d["a"] is not None:
            inp["a"] = rn(*d["a"])
        if d["colscale"] is not None:
            inp["cs"] = rn(*d["colscale"])
        if d["rowscale"] is not None:
            inp["rs"] = torch.rand(*d["rowscale"], dtype=torch.float64, device=dev) + 0.5
        grad = [n for n, r in zip(("a", "b", "cs", "rs"), rg) if r and n in inp]
        lens = None if d["lens"] is None else torch.tensor(d["lens"], dtype=torch.int32, device=dev)

        def hip(b, a=None, cs=None, rs=None):
            return ops.scale_add(a, b, cs, rs, lens, d["mask_a"])

        def ref(b, a=None, cs=None, rs=None, masks=()):
            y = b * (1 if cs is None else cs.reshape(C)) * (1 if rs is None else rs.reshape(B, 1, 1))
            if a is not None:
                y = y + (a * _lensmask(d["lens"], T, dev)[..., None] if d["mask_a"] else a)
            return y
        return inp, grad, hip, ref, TOL_EW, TOL_EW
    if op == "axpby":
        inp = dict(a=rn(*d["a"]), b=rn(*d["b"]))
        grad = [n for n, r in zip(("a", "b"), rg) if r]
        return (inp, grad, lambda a, b: ops.axpby(a, b, d["alpha"], d["beta"]),
                lambda a, b, masks=(): d["alpha"] * a + d["beta"] * b, TOL_EW, TOL_EW)
    if op == "add_pe":
        B, T, C = d["x"]
        lens = torch.tensor(d["lens"], dtype=torch.int32, device=dev)
        inp = dict(x=rn(B, T, C), pe=rn(*d["pe"]))
        grad = [n for n, r in zip(("x", "pe"), rg) if r]
        return (inp, grad, lambda x, pe: ops.add_pe(x, pe, lens),
                lambda x, pe, masks=(): x + pe * _lensmask(d["lens"], T, dev)[..., None], TOL_EW, TOL_EW)
    if op == "attention":
        assert d["mode"] == ops.MASK_KEYS and d["window"] == 0, "add the reference of this mask mode"
        B, Tq, C = d["q"]
        Tk, H = d["k"][1], d["H"]
        hd = C // H
        lens = torch.tensor(d["kv_len"], dtype=torch.int32, device=dev)
        inp = dict(q=rn(B, Tq, C), k=rn(B, Tk, C), v=rn(B, Tk, C))
        grad = [n for n, r in zip(("q", "k", "v"), rg) if r]

        def hip(q, k, v):
            keep = ops.use_flash
            ops.use_flash = d["flash"]
            try:
                return ops.attention(q, k, v, lens, H, d["scale"], drop_p=d["drop_p"])
            finally:
                ops.use_flash = keep

        def ref(q, k, v, masks=()):
            qh, kh, vh = [t.view(B, -1, H, hd).transpose(1, 2) for t in (q, k, v)]
            s = (qh * d["scale"]) @ kh.transpose(-1, -2)
            km = _lensmask(d["kv_len"], Tk, dev).bool()[:, None, None, :]
            p = torch.softmax(s.masked_fill(~km, float("-inf")), dim=-1)
            for mk in masks:
                p = p * mk
            return (p @ vh).transpose(1, 2).reshape(B, Tq, C)
        return inp, grad, hip, ref, TOL_GEMM, TOL_GEMM
    if op == "rel_attention":
        B, T, C = d["q"]
        H = d["H"]
        lens = torch.tensor(d["kv_len"], dtype=torch.int32, device=dev)
        inp = dict(qw=rn(B, T, C), qr=rn(B, T, C), k=rn(B, T, C), v=rn(B, T, C), kr=rn(*d["kr"]))
        grad = [n for n, r in zip(("qw", "qr", "k", "v", "kr"), rg) if r]

        def hip(qw, qr, k, v, kr):
            return ops.rel_attention(qw, qr, k, v, kr, lens, H, d["scale"], d["drop_p"])

        def ref(qw, qr, k, v, kr, masks=()):
            return _rel_ref(qw, qr, k, v, kr, d["kv_len"], H, d["scale"], masks[0] if masks else None)
        return inp, grad, hip, ref, TOL_GEMM, TOL_GEMM
    if op == "channel_attention":
        B, T, C3 = d["qkv"]
        H = d["H"]
        C = C3 // 3
        hd = C // H

        def ref(qkv, masks=()):
            x = qkv.reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
            q, k, v = x[0], x[1], x[2]
            att = ((k * d["scale"]).transpose(-1, -2) @ v).softmax(dim=-1)
            return (att @ q.transpose(-1, -2)).transpose(-1, -2).transpose(1, 2).reshape(B, T, C)
        return (dict(qkv=rn(B, T, C3)), ["qkv"] if rg[0] else [],
                lambda qkv: ops.channel_attention(qkv, H, d["scale"], d["bwd_precision"]), ref, TOL_GEMM, TOL_GEMM)
    if op == "qkv_pre":          # LN1 + three depthwise k = 3 convs + their LayerNorms (tests/test_qkvpre_gpu.py::_ref)
        B, T, C = d["x"]
        s = d["stride"]
        eps1, eps = d["eps"]
        x = rn(B, T, C) * _lensmask(d["lens"], T, dev)[..., None]           # inputs are masked upstream
        inp = dict(x=x, ln_g=1 + 0.1 * rn(C), ln_b=0.1 * rn(C))
        for j in range(3):
            inp.update({"w%d" % j: 0.5 * rn(C, 1, 3), "g%d" % j: 1 + 0.1 * rn(C), "bb%d" % j: 0.1 * rn(C)})
        grad = list(inp)
        lens = torch.tensor(d["lens"], dtype=torch.int32, device=dev)

        def hip(x, ln_g, ln_b, **t):
            outs = ops.qkv_pre(x, (ln_g, ln_b, eps1), tuple(t["w%d" % j] for j in range(3)),
                               tuple((t["g%d" % j], t["bb%d" % j]) for j in range(3)) + (eps,), lens, s, d["want_h"], skip=d["skip"])
            return tuple(outs)

        def ref(x, ln_g, ln_b, masks=(), **t):
            h = _ln(x, ln_g, ln_b, eps1)
            m = (s * torch.arange(T // s, device=dev)[None, :] < lens[:, None]).double()[..., None]
            outs = []
            for j in range(3):
                c = (_taps(h).view(B, T, 3, C) * t["w%d" % j][:, 0, :].t()).sum(2)[:, ::s][:, :T // s] * m
                outs.append(_ln(c, t["g%d" % j], t["bb%d" % j], eps))
            return tuple(outs) + ((h,) if d["want_h"] else ()) + ((x,) if d["skip"] else ())
        return inp, grad, hip, ref, TOL_EW, TOL_QKV_GRAD
    if op == "bias_add":
        inp = dict(x=rn(*d["x"]), b=rn(*d["b"]))
        grad = [n for n, r in zip(("x", "b"), rg) if r]
        return inp, grad, lambda x, b: ops.bias_add(x, b), lambda x, b, masks=(): x + b.reshape(-1), TOL_EW, TOL_EW
    if op == "colsum":
        return dict(x=rn(*d["x"])), [], lambda x: ops.colsum(x), lambda x, masks=(): x.sum(0), TOL_EW, TOL_EW
    if op == "transpose":
        return (dict(x=rn(*d["x"])), ["x"] if rg[0] else [], lambda x: ops.transpose(x),
                lambda x, masks=(): x.transpose(1, 2), TOL_EXACT, TOL_EXACT)
    if op == "permute3":
        def ref(src, masks=()):        # out[i][j][k] = src[off + i s0 + j s1 + k s2] (strides may be negative)
            idx = torch.tensor(d["off"], device=dev)
            for n, st in zip(d["dims"], d["strides"]):
                idx = idx[..., None] + torch.arange(n, device=dev) * st
            return src.reshape(-1)[idx]
        return dict(src=rn(*d["src"])), [], lambda src: ops.permute3(src, d["dims"], d["off"], d["strides"]), ref, TOL_EXACT, TOL_EXACT
    if op == "dropout":
        def ref(x, masks=()):
            for mk in masks:
                x = x * mk
            return x
        return (dict(x=rn(*d["x"])), ["x"] if rg[0] else [], lambda x: ops.dropout(x, d["p"], d["training"], d["site"]), ref,
                TOL_EW, TOL_EW)
    raise AssertionError("no float64 reference for op %r" % op)


def _tagged(t):
    """t with the exact max|t| partials a producing kernel would leave (the backward then takes the step's paths)"""
    from vilco_amd import ops
    return ops._tag_amax(t, t.abs().max().reshape(1).contiguous(), 1)


def _ids():
    return ["%s-%d" % (op, i) for i, (op, _, _) in enumerate(FULL_SIZE_SIGNATURES)]


@pytest.mark.parametrize("i", range(len(FULL_SIZE_SIGNATURES)), ids=_ids())
def test_op_at_step_signature(dev, i, monkeypatch):
    """one table entry: forward and every input gradient against float64.  The weight-gradient products run in three MFMAs here
    (ops.dw_precision = None): the single-part format of the long-contraction dW products (~3e-4 from exact by design, ops.py:
    dw_precision) is held to its own 2e-6 bar against lead-rounded operands by tests/test_step_gemm_census_gpu.py."""
    from vilco_amd import ops
    monkeypatch.setattr(ops, "dw_precision", None)
    op, d, _steps = FULL_SIZE_SIGNATURES[i]
    torch.manual_seed(1000 + i)
    inp, grad, hip, ref, tol_f, tol_g = _case(op, d, dev)
    h_in = {k: v.float().contiguous().requires_grad_(k in grad) for k, v in inp.items()}
    r_in = {k: v.detach().clone().requires_grad_(k in grad) for k, v in inp.items()}
    ops.dropout_log = []
    try:
        got = hip(**h_in)
        masks = _drop_masks(dev)
    finally:
        ops.dropout_log = None
    want = ref(masks=masks, **r_in)
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert tuple(g.shape) == tuple(w.shape), (j, g.shape, w.shape)
        e = _rel(g, w)
        assert e < tol_f, "%s output %d: forward rel err %.3e >= %.0e" % (op, j, e, tol_f)
    outs = [(g, w) for g, w in zip(got, want) if w.requires_grad and g.requires_grad]
    if grad and outs:
        douts = [torch.randn_like(w) for _, w in outs]
        torch.autograd.backward([g for g, _ in outs], [_tagged(dw.float().contiguous()) for dw in douts])
        torch.autograd.backward([w for _, w in outs], douts)
        for k in grad:
            assert h_in[k].grad is not None, "%s: no gradient for %s" % (op, k)
            e = _rel(h_in[k].grad, r_in[k].grad)
            assert e < tol_g, "%s grad %s: rel err %.3e >= %.0e" % (op, k, e, tol_g)
    del got, want, outs, h_in, r_in, inp
    torch.cuda.empty_cache()


def test_step_signatures_are_in_the_table(dev):
    """every signature the three steps call is in FULL_SIZE_SIGNATURES (and so has its float64 test)"""
    from fullsize_steps import STEPS, build_step, run_step
    table = {freeze(op, d) for op, d, _ in FULL_SIZE_SIGNATURES}
    missing = {}
    for name in STEPS:
        model, batch = build_step(name, dev)
        mp = pytest.MonkeyPatch()
        with Recorder(mp) as rec:
            run_step(model, batch)
        del model
        torch.cuda.empty_cache()
        for key in rec.seen:
            if key not in table:
                missing.setdefault(key, []).append(name)
        assert {k[0] for k in rec.seen} <= set(RECORDED)
    assert not missing, "signatures the steps call but FULL_SIZE_SIGNATURES does not cover (%d):\n%s" % (
        len(missing), "\n".join("(%r, %r, %r)," % (k[0], dict(k[1]), tuple(v)) for k, v in missing.items()))


def test_table_and_exemptions_are_well_formed():
    """(runs without a GPU) every table entry names a recorded op; the exemptions name where they are covered"""
    assert all(op in RECORDED for op, _, _ in FULL_SIZE_SIGNATURES)
    assert len({freeze(op, d) for op, d, _ in FULL_SIZE_SIGNATURES}) == len(FULL_SIZE_SIGNATURES)
    assert all(EXEMPT.values())
