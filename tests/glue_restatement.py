"""Plain PyTorch restatements of the memory-bound glue operators of include/vilco_hip.h (LayerNorm, depthwise conv,
max-pool, materialised softmax, XLNet shift, residual / activation-backward / column-sum / layout kernels), the inputs of
their edge-shape tests, and the comparison helpers those tests share.  No call into vilco_amd.

Every function computes in the dtype of its inputs: with float64 tensors it is the reference, with the same values in
float32 it is the "fp32 CPU evaluation" the measured tolerances (BARS) come from.  tests/test_glue_restatement_cpu.py holds
the functions to torch.nn.functional / autograd and BARS to the recomputed fp32 error; tests/test_glue_edges_gpu.py holds
the HIP kernels to the functions."""
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
U = 2.0 ** -24                 # unit roundoff of fp32
FLOOR = 2.0 ** -22


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dbl(t):
    return None if t is None else (t.double() if t.is_floating_point() else t)


# ------------------------------------------------------------------------------------------------ comparison helpers
def rowwise_err(got, want, cols=False, scale=None):
    """max over rows (cols=True: over output columns) of max|got - want| / max|want| of THAT row.  A row whose reference is
    identically zero has no scale: it must be zero in `got` too (either sign; NaN is not zero), else AssertionError.  `scale`
    ([rows]) replaces the row's own max|want| where the natural scale of a result is not its own size (a mean: max|x|)."""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert g.shape == w.shape, (tuple(g.shape), tuple(w.shape))
    if g.numel() == 0:
        return 0.0
    if g.dim() == 0:
        g, w = g[None], w[None]
    g, w = g.reshape(-1, g.shape[-1]), w.reshape(-1, w.shape[-1])
    if cols:
        g, w = g.t(), w.t()
    s = w.abs().amax(dim=1) if scale is None else scale.detach().double().cpu().reshape(-1)
    assert s.shape[0] == g.shape[0]
    zero = s == 0
    if bool(zero.any()):
        bad = (g[zero] != 0) | torch.isnan(g[zero])
        assert not bool(bad.any()), "%d non-zero entries in rows whose reference is identically zero" % int(bad.sum())
    if bool(torch.isnan(g[~zero]).any()) or bool(torch.isinf(g[~zero]).any()):
        return math.inf
    if bool((~zero).any()):
        return float(((g[~zero] - w[~zero]).abs().amax(dim=1) / s[~zero]).max())
    return 0.0


def sum_bound_ok(got, want, abs_terms, n):
    """the derived bar of the column reductions: |got - want| <= n 2^-24 sum_r |term_r| per output element (fp32 summation of
    n terms in any order); returns (ok, worst ratio of error to bound)."""
    g, w, a = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1), abs_terms.detach().double().cpu().reshape(-1)
    assert g.shape == w.shape == a.shape
    if bool(torch.isnan(g).any()):
        return False, math.inf
    err, bound = (g - w).abs(), n * U * a
    ok = bool((err <= bound).all())
    nz = bound > 0
    return ok, (float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0)


CANARY = 64


def guarded(n, device, fill=float("nan")):
    """[64 floats canary | n floats | 64 floats canary] as one tensor; returns (payload view, 16-byte aligned and pre-filled
    with `fill` -- NaN, so an element the kernel leaves unwritten fails the comparison -- or with a tensor's values, check) where
    check() asserts that both canaries still hold their bit pattern."""
    buf = torch.empty(n + 2 * CANARY, dtype=torch.float32, device=device)
    pat = (torch.arange(2 * CANARY, dtype=torch.int32) * 40503 + 0x5A5A0000).to(device)
    bits = buf.view(torch.int32)
    bits[:CANARY] = pat[:CANARY]
    bits[CANARY + n:] = pat[CANARY:]
    pay = buf[CANARY:CANARY + n]
    if torch.is_tensor(fill):
        pay.copy_(fill.reshape(-1).to(device))
    else:
        pay.fill_(fill)
    assert pay.data_ptr() % 16 == 0

    def check():
        b = buf.view(torch.int32)
        assert torch.equal(b[:CANARY], pat[:CANARY]), "write in front of the buffer"
        assert torch.equal(b[CANARY + n:], pat[CANARY:]), "write past the end of the buffer"
    return pay, check


def valid_rows(lens, T, stride=1):
    """[B, T/stride] bool: stride * t' < lens[b]"""
    return (stride * torch.arange(T // stride)[None, :]) < lens[:, None].long()


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, gamma, beta, eps, relu=False, row_mask=None):
    """y = ((x - mean) * rstd * gamma + beta), relu'd, times row_mask[row % mask_rows]; biased variance.  -> y, mean, rstd"""
    mean = x.mean(dim=1)
    xc = x - mean[:, None]
    var = (xc * xc).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = xc * rstd[:, None]
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    if relu:
        y = torch.relu(y)
    if row_mask is not None:
        y = y * row_mask[torch.arange(x.shape[0]) % row_mask.shape[0]][:, None]
    return y, mean, rstd


def layernorm_bwd(dy, x, y, gamma, mean, rstd, relu=False, dres=None):
    """g = dy (zero where the saved y is not > 0 when relu); dx = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat)) + dres;
    dgamma = sum_r g xhat, dbeta = sum_r g.  mean / rstd / y are INPUTS (what the forward saved).
    -> dx, dgamma, dbeta, sum_r |g xhat|, sum_r |g|"""
    g = dy * (y > 0).to(dy.dtype) if relu else dy
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = g * gamma if gamma is not None else g
    s1 = gg.mean(dim=1, keepdim=True)
    s2 = (gg * xh).mean(dim=1, keepdim=True)
    dx = rstd[:, None] * (gg - s1 - xh * s2)
    if dres is not None:
        dx = dx + dres
    return dx, (g * xh).sum(0), g.sum(0), (g * xh).abs().sum(0), g.abs().sum(0)


def layernorm(x, gamma, beta, eps, relu=False, row_mask=None, dy=None, dres=None):
    """forward and, for a given dy, backward of the whole operator (row_mask included: a masked row passes no gradient)"""
    y, mean, rstd = layernorm_fwd(x, gamma, beta, eps, relu, row_mask)
    if dy is None:
        return y, mean, rstd
    if row_mask is not None:
        dy = dy * row_mask[torch.arange(x.shape[0]) % row_mask.shape[0]][:, None]
    if relu and row_mask is not None:        # the saved y is 0 on a masked row whatever the pre-activation was
        y0, _, _ = layernorm_fwd(x, gamma, beta, eps, True, None)
    else:
        y0 = y
    dx, dg, db, _, _ = layernorm_bwd(dy, x, y0, gamma, mean, rstd, relu, dres)
    return y, mean, rstd, dx, dg, db


LN_EPS = 1e-5
LN_WIDTHS = [4, 12, 100, 252, 260, 1540, 1792, 2308, 2816, 3076, 4096]
LN_VARIANTS = ["nullgb", "dres", "mask", "const", "zerochan", "cancel"]
LN_CASES = ([(C, 5, "plain") for C in LN_WIDTHS] + [(12, r, "plain") for r in (1, 1029, 8195)]
            + [(C, 21 if v == "mask" else 5, v) for C in (100, 1792) for v in LN_VARIANTS])
LN_ZERO_CHANNEL = 5


def ln_inputs(C, rows, variant):
    """fp32 inputs of one LayerNorm case: dict x, gamma, beta, dy, dres, row_mask (None where the case has none)"""
    g = gen(1000 + 7 * C + rows + 131 * (["plain"] + LN_VARIANTS).index(variant))
    x = torch.randn(rows, C, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    dres = row_mask = None
    if variant == "nullgb":
        gamma = beta = None
    elif variant == "dres":
        dres = torch.randn(rows, C, generator=g)
    elif variant == "mask":
        dres = torch.randn(rows, C, generator=g)
        row_mask = torch.ones(7)
        row_mask[2] = row_mask[6] = 0.0
    elif variant == "const":
        x = torch.full((rows, C), 3.0)
    elif variant == "zerochan":
        gamma[LN_ZERO_CHANNEL] = beta[LN_ZERO_CHANNEL] = 0.0
    elif variant == "cancel":
        x = 1000 + 0.01 * torch.randn(rows, C, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, dres=dres, row_mask=row_mask)


def ln_reference(inp, relu, dtype):
    """the case in `dtype`: forward from x; backward from the forward's float64 results rounded to fp32 (the values the
    backward kernel is handed), so that both evaluations -- and the kernel -- take the SAME mean, rstd and y."""
    d64 = {k: dbl(v) for k, v in inp.items()}
    y64, mean64, rstd64 = layernorm_fwd(d64["x"], d64["gamma"], d64["beta"], float(torch.tensor(LN_EPS)), relu, d64["row_mask"])
    saved = dict(y=y64.float(), mean=mean64.float(), rstd=rstd64.float())
    c = lambda t: None if t is None else t.to(dtype)
    y, mean, rstd = layernorm_fwd(c(inp["x"]), c(inp["gamma"]), c(inp["beta"]), float(torch.tensor(LN_EPS)), relu, c(inp["row_mask"]))
    # without the ReLU the backward kernel sees no mask; the masked case's backward is checked under relu = 1 only
    dx, dg, db, dg_abs, db_abs = layernorm_bwd(c(inp["dy"]), c(inp["x"]), c(saved["y"]), c(inp["gamma"]), c(saved["mean"]),
                                               c(saved["rstd"]), relu, c(inp["dres"]))
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dg, dbeta=db, dgamma_abs=dg_abs, dbeta_abs=db_abs, saved=saved)


def ln_errs(got, want, x):
    """the four measured figures of one case: y and dx per row against the row's own maximum, rstd against itself, mean
    against max|x| of its row (a mean is a sum of C values of that size; its own size may be anything down to 0)."""
    return dict(y=rowwise_err(got["y"], want["y"]), dx=rowwise_err(got["dx"], want["dx"]),
                rstd=rowwise_err(got["rstd"][:, None], want["rstd"][:, None]),
                mean=rowwise_err(got["mean"][:, None], want["mean"][:, None], scale=x.abs().amax(dim=1)))


# ------------------------------------------------------------------------------------------------ dwconv3 / maxpool3s2
def dwconv3_fwd(x, w, lens, stride):
    """y[b][t'][c] = valid(t') sum_j w[c][j] x[b][stride t' + j - 1][c], zero pad 1; valid(t') = stride t' < lens[b]"""
    B, T, C = x.shape
    To = T // stride
    xp = F.pad(x, (0, 0, 1, 1))
    y = sum(w[:, j] * xp[:, j:j + stride * To:stride] for j in range(3))
    return y * valid_rows(lens, T, stride)[..., None].to(x.dtype)


def dwconv3_bwd(dy, x, w, lens, stride):
    """-> dx, dw, sum |terms of dw|, number of terms of a dw element"""
    B, T, C = x.shape
    To = T // stride
    dym = dy * valid_rows(lens, T, stride)[..., None].to(x.dtype)
    xp = F.pad(x, (0, 0, 1, 1))
    dxp = torch.zeros(B, T + 2, C, dtype=x.dtype)
    dw = torch.zeros(C, 3, dtype=x.dtype)
    dw_abs = torch.zeros(C, 3, dtype=x.dtype)
    for j in range(3):
        dxp[:, j:j + stride * To:stride] += w[:, j] * dym
        t = dym * xp[:, j:j + stride * To:stride]
        dw[:, j] = t.sum(dim=(0, 1))
        dw_abs[:, j] = t.abs().sum(dim=(0, 1))
    return dxp[:, 1:T + 1], dw, dw_abs, B * To


def maxpool3s2_fwd(x, lens):
    """y[b][t'][c] = valid(t') max(x[2t'-1], x[2t'], x[2t'+1]), -inf outside [0, T); valid(t') = 2 t' < lens[b]"""
    B, T, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1), value=-math.inf)
    y = torch.maximum(torch.maximum(xp[:, 0:T:2], xp[:, 1:T + 1:2]), xp[:, 2:T + 2:2])
    return torch.where(valid_rows(lens, T, 2)[..., None], y, torch.zeros((), dtype=x.dtype))


def maxpool3s2_bwd(dy, x, lens):
    """dx[b][t][c] = sum of valid(t') dy[b][t'][c] over the windows t' whose FIRST maximum is at t"""
    B, T, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1), value=-math.inf)
    win = torch.stack([xp[:, 0:T:2], xp[:, 1:T + 1:2], xp[:, 2:T + 2:2]], dim=0)          # [3, B, T/2, C]
    best = win.amax(dim=0)
    first = torch.where(win[0] == best, 0, torch.where(win[1] == best, 1, 2))             # first index of the maximum
    dym = dy * valid_rows(lens, T, 2)[..., None].to(dy.dtype)
    dxp = torch.zeros(B, T + 2, C, dtype=dy.dtype)
    for j in range(3):
        dxp[:, j:j + T:2] += dym * (first == j).to(dy.dtype)
    return dxp[:, 1:T + 1]


CONV_SHAPES = [((1, 2, 4), [1]), ((3, 6, 4), [0, 3, 6]), ((2, 10, 260), [0, 9]), ((2, 8, 1028), [1, 8]),
               ((1, 8200, 4), [8199]), ((1, 4100, 1024), [4100])]          # (B, T, C), lens: 0, 1, odd, T - 1, T


def conv_inputs(shape, stride):
    B, T, C = shape
    g = gen(2000 + T + C + stride)
    return dict(x=torch.randn(B, T, C, generator=g), w=torch.randn(C, 3, generator=g),
                dy=torch.randn(B, T // stride, C, generator=g))


def pool_inputs(shape, kind):
    """kind a: randn; b: {-1, 0, 1} (nearly every window ties); c: all negative (a zero pad would win at both ends)"""
    B, T, C = shape
    g = gen(3000 + T + C + ord(kind))
    if kind == "a":
        x = torch.randn(B, T, C, generator=g)
    elif kind == "b":
        x = torch.randint(-1, 2, (B, T, C), generator=g).float()
    else:
        x = -1.0 - torch.rand(B, T, C, generator=g)
    return dict(x=x, dy=torch.randn(B, T // 2, C, generator=g))


# ------------------------------------------------------------------------------------------------ softmax / relshift
def softmax_fwd(s, kv_len, mode):
    """rows of s[B][H][Tq][Tk].  mode 0: key j >= kv_len[b] excluded (-inf); mode 1: score - 1e30 where j >= kv_len[b] and
    j != i, applied IN FP32 as the model does (so any realistic score becomes -1e30 exactly) before the cast; mode 2: none."""
    B, H, Tq, Tk = s.shape
    if mode != 2:
        pad = torch.arange(Tk)[None, None, None, :] >= kv_len.long()[:, None, None, None]
        if mode == 0:
            s = s.masked_fill(pad, -math.inf)
        else:
            off = pad & (torch.arange(Tk)[None, :] != torch.arange(Tq)[:, None])[None, None]
            s = torch.where(off, s.float() - 1e30, s.float()).to(s.dtype)
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    return e / e.sum(dim=-1, keepdim=True)


def softmax_bwd(dp, p):
    return p * (dp - (dp * p).sum(dim=-1, keepdim=True))


def softmax_bwd_err(got, want, dp, p):
    """per row against sum_j |dP_j P_j|, the size of the terms of the row's dot product: on a nearly one-hot row dP - dot
    cancels at the dominant entry and the row's own max|dS| can be any number of orders below what fp32 resolves there"""
    return rowwise_err(got, want, scale=(dp.double() * p.double()).abs().sum(dim=-1).reshape(-1))


SOFTMAX_TK = [1, 63, 64, 65, 129]
SOFTMAX_SCORES = [(1.0, 0.0), (30.0, 0.0), (1.0, 1e4)]


def softmax_configs(Tk):
    """(mode, Tq, kv_len of the B = 2 clips)"""
    return [(0, 5, [1, max(Tk - 1, 1)]), (0, 5, [Tk, 1]), (1, 70, [0, min(3, Tk)]), (1, 70, [Tk, 0]), (2, 5, None)]


def softmax_inputs(Tk, Tq, so, mode):
    g = gen(4000 + Tk + 7 * Tq + int(so[0]) + int(so[1]) + mode)
    return dict(s=torch.randn(2, 2, Tq, Tk, generator=g) * so[0] + so[1], dp=torch.randn(2, 2, Tq, Tk, generator=g))


def relshift(bd):
    """rel_shift_bnij: bd[N][T][2T] -> [N][T][T], element (i, j) = bd[i][T - i + j]"""
    N, T, _ = bd.shape
    return bd.reshape(N, 2 * T, T)[:, 1:, :].reshape(N, T, 2 * T - 1)[:, :, :T]


def relshift_add(s, bd, scale):
    return s + scale * relshift(bd)


def relshift_bwd(ds, scale):
    """dbd[i][T - i + j] = scale ds[i][j], every other entry 0"""
    N, T, _ = ds.shape
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    dbd = torch.zeros(N, T, 2 * T, dtype=ds.dtype)
    dbd[:, i.expand(T, T), (T - i + j)] = scale * ds
    return dbd


# ------------------------------------------------------------------------------------------------ residual glue
def prefix_mask(lens, T, dtype):
    return (torch.arange(T)[None, :] < lens.long()[:, None]).to(dtype)[..., None]


def scale_add_fwd(a, b, colscale, rowscale, lens, mask_a):
    """out = a (mask_a ? m : 1) + (colscale[c] rowscale[b]) bval"""
    B, T, C = b.shape
    f = torch.ones((), dtype=b.dtype)
    if colscale is not None:
        f = f * colscale
    if rowscale is not None:
        f = f * rowscale[:, None, None]
    out = f * b
    if a is not None:
        out = (a * prefix_mask(lens, T, b.dtype) if (mask_a and lens is not None) else a) + out
    return out


def scale_add_bwd(dout, b, colscale, rowscale, lens, mask_a):
    """-> da, db, dcolscale, sum |terms of dcolscale|"""
    B, T, C = dout.shape
    da = dout * prefix_mask(lens, T, dout.dtype) if (mask_a and lens is not None) else dout.clone()
    f = torch.ones((), dtype=dout.dtype)
    if colscale is not None:
        f = f * colscale
    if rowscale is not None:
        f = f * rowscale[:, None, None]
    t = dout * b * (rowscale[:, None, None] if rowscale is not None else 1.0)
    return da, dout * f, t.sum(dim=(0, 1)), t.abs().sum(dim=(0, 1))


SCALE_ADD_SHAPES = [((1, 1, 1), [0]), ((3, 7, 3), [0, 7, 4]), ((2, 33, 22), [33, 5]), ((2, 9, 257), [0, 9]),
                    ((3, 5, 260), [5, 0, 3]), ((1, 4100, 1024), [4000])]
SCALE_ADD_COMBOS = [(cs, rs, ln, ma) for cs in (0, 1) for rs in (0, 1) for ln in (0, 1) for ma in ((0, 1) if ln else (0,))]


def scale_add_inputs(shape):
    B, T, C = shape
    g = gen(5000 + T + C)
    return dict(a=torch.randn(B, T, C, generator=g), b=torch.randn(B, T, C, generator=g), dout=torch.randn(B, T, C, generator=g),
                colscale=torch.randn(C, generator=g), rowscale=torch.rand(B, generator=g) + 0.5)


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440)) + x * 0.39894228040143267794 * torch.exp(-0.5 * x * x)


def act_bwd(dy, aux, act, lens=None, T=None, row_mask=None, drop_mask=None):
    """dz = dy dropmask rowmask act'(aux); aux = the pre-activation (GELU) or the output (RELU: derivative 0 at aux <= 0);
    row r is off when r % T >= lens[r / T] or row_mask[r] == 0.  drop_mask: the factors 0 | 1/(1-p), an input."""
    rows, C = dy.shape
    g = dy * drop_mask if drop_mask is not None else dy
    if lens is not None:
        g = g * prefix_mask(lens, T, dy.dtype).reshape(rows, 1)
    if row_mask is not None:
        g = g * (row_mask != 0).to(dy.dtype)[:, None]
    if act == ACT_RELU:
        g = g * (aux > 0).to(dy.dtype)
    elif act == ACT_GELU:
        g = g * gelu_grad(aux)
    return g


ACT_SHAPES = [((1, 1), 1, [1]), ((7, 3), 7, [4]), ((33, 22), 11, [11, 0, 6]), ((9, 260), 3, [0, 3, 2]), ((70, 96), 35, [35, 0])]
ACT_SPECIALS = [0.0, 10.0, -10.0, 40.0, -40.0]


def act_inputs(shape):
    rows, C = shape
    g = gen(6000 + rows + C)
    aux = torch.randn(rows, C, generator=g)
    if aux.numel() >= 15:                 # one special value per row at most: no row consists of the far tails alone
        aux.view(-1)[1:15:3] = torch.tensor(ACT_SPECIALS)
    rm = torch.ones(rows)
    rm[::3] = 0.0
    return dict(dy=torch.randn(rows, C, generator=g), aux=aux, row_mask=rm)


def colsum(x):
    """-> column sums, column sums of |x|"""
    return x.sum(dim=0), x.abs().sum(dim=0)


def mask_rows(x, lens):
    return x * prefix_mask(lens, x.shape[1], x.dtype)


def add_pe(x, pe, lens):
    return x + pe[None] * prefix_mask(lens, x.shape[1], x.dtype)


def axpby(a, b, alpha, beta):
    return alpha * a + (beta * b if b is not None else 0.0)


def axpby_err(got, want, a, b, alpha, beta):
    """every element is its own row; its scale is |alpha a| + |beta b| (the sum itself may cancel to anything)"""
    sc = (alpha * a.double()).abs() + ((beta * b.double()).abs() if b is not None else 0.0)
    return rowwise_err(got[:, None], want[:, None], scale=sc)


def transpose2d(x):
    return x.transpose(1, 2).contiguous()


def permute3(src, dims, off, strides):
    return torch.as_strided(src.reshape(-1), dims, strides, off).contiguous()


GLUE_C = [1, 22, 64, 260]
GLUE_BT, GLUE_LENS = (3, 5), [0, 1, 5]
AXPBY_N = [1, 3, 5, 4 * 2 ** 20 + 3]
AXPBY_AB = (0.75, -1.5)


def glue_inputs(C):
    B, T = GLUE_BT
    g = gen(7000 + C)
    return dict(x=torch.randn(B, T, C, generator=g), pe=torch.randn(T, C, generator=g))


def axpby_inputs(n):
    g = gen(8000 + n % 1000)
    return dict(a=torch.randn(n, generator=g), b=torch.randn(n, generator=g))


# ------------------------------------------------------------------------------------------------ the measured bars
def _f32_vs_f64(fn, *args):
    """rowwise_err of fn on the fp32 inputs against fn on the same values in float64"""
    c64 = [dbl(a) if torch.is_tensor(a) else a for a in args]
    return rowwise_err(fn(*args), fn(*c64))


def measure_fp32_errors():
    """family -> the largest rowwise_err, over the GPU test's own inputs, of the reference formula evaluated in fp32 on the
    CPU against its float64 evaluation.  Nothing here comes from a HIP kernel."""
    m = {}

    def up(k, v):
        m[k] = max(m.get(k, 0.0), v)
    for C, rows, variant in LN_CASES:
        inp = ln_inputs(C, rows, variant)
        for relu in (False, True):
            e = ln_errs(ln_reference(inp, relu, torch.float32), ln_reference(inp, relu, torch.float64), inp["x"])
            for k, v in e.items():
                up(("ln_cancel_" if variant == "cancel" else "ln_") + k, v)
    for shape, lens in CONV_SHAPES:
        lens = torch.tensor(lens, dtype=torch.int32)
        for stride in (1, 2):
            i = conv_inputs(shape, stride)
            up("dwconv3_y", _f32_vs_f64(lambda x, w: dwconv3_fwd(x, w, lens, stride), i["x"], i["w"]))
            up("dwconv3_dx", _f32_vs_f64(lambda dy, x, w: dwconv3_bwd(dy, x, w, lens, stride)[0], i["dy"], i["x"], i["w"]))
    for Tk in SOFTMAX_TK:
        for so in SOFTMAX_SCORES:
            fam = "softmax_off_" if so[1] else "softmax_"
            for mode, Tq, kv in softmax_configs(Tk):
                i = softmax_inputs(Tk, Tq, so, mode)
                kv = None if kv is None else torch.tensor(kv, dtype=torch.int32)
                up(fam + "fwd", _f32_vs_f64(lambda s: softmax_fwd(s, kv, mode), i["s"]))
                p = softmax_fwd(i["s"].double(), kv, mode).float()
                up(fam + "bwd", softmax_bwd_err(softmax_bwd(i["dp"], p), softmax_bwd(i["dp"].double(), p.double()), i["dp"], p))
    for shape, lens in SCALE_ADD_SHAPES:
        i, lens = scale_add_inputs(shape), torch.tensor(lens, dtype=torch.int32)
        for cs, rs, ln, ma in SCALE_ADD_COMBOS:
            opt = (i["colscale"] if cs else None, i["rowscale"] if rs else None)
            ln_ = lens if ln else None
            up("scale_add", _f32_vs_f64(lambda a, b, c, r: scale_add_fwd(a, b, c, r, ln_, ma), i["a"], i["b"], *opt))
            for k in (0, 1):
                up("scale_add", _f32_vs_f64(lambda d, b, c, r: scale_add_bwd(d, b, c, r, ln_, ma)[k], i["dout"], i["b"], *opt))
    for shape, T, lens in ACT_SHAPES:
        i, lens = act_inputs(shape), torch.tensor(lens, dtype=torch.int32)
        dm = (torch.rand(shape, generator=gen(9)) >= 0.3).float() * (1.0 / (1.0 - 0.3))     # a mask of the same kind, for the bar only
        for act in (ACT_NONE, ACT_RELU, ACT_GELU):
            for d in (None, dm):
                up("act_bwd", _f32_vs_f64(lambda dy, aux, rm, d_: act_bwd(dy, aux, act, lens, T, rm, d_), i["dy"], i["aux"], i["row_mask"], d))
    lens = torch.tensor(GLUE_LENS, dtype=torch.int32)
    for C in GLUE_C:
        i = glue_inputs(C)
        up("add_pe", _f32_vs_f64(lambda x, pe: add_pe(x, pe, lens), i["x"], i["pe"]))
    for n in AXPBY_N:
        i = axpby_inputs(n)
        for b in (None, i["b"]):
            up("axpby", axpby_err(axpby(i["a"], b, *AXPBY_AB), axpby(i["a"].double(), dbl(b), *AXPBY_AB), i["a"], b, *AXPBY_AB))
    return m


BAR_FACTOR = 4.0          # the kernels reduce in another order and use expf / rsqrt variants of their own


def bar_from(measured):
    return max(BAR_FACTOR * measured, FLOOR)


# family -> bar = max(4 x the fp32 CPU error that measure_fp32_errors() finds, 2^-22), the measured value next to each; the
# CPU test recomputes the measurement and holds every bar between 1x and 8x of it (or at the floor)
BARS = {
    "ln_y": 4 * 3.691e-07,                       # measured 3.691e-07, x 4
    "ln_dx": 4 * 5.427e-07,                      # measured 5.427e-07, x 4
    "ln_rstd": 4 * 1.906e-07,                    # measured 1.906e-07, x 4
    "ln_mean": 4 * 7.402e-08,                    # measured 7.402e-08, x 4
    "ln_cancel_y": 4 * 2.718e-03,                # measured 2.718e-03, x 4
    "ln_cancel_dx": 4 * 1.772e-07,               # measured 1.772e-07, x 4
    "ln_cancel_rstd": 4 * 2.662e-05,             # measured 2.662e-05, x 4
    "ln_cancel_mean": 4 * 8.117e-08,             # measured 8.117e-08, x 4
    "dwconv3_y": 4 * 5.684e-07,                  # measured 5.684e-07, x 4
    "dwconv3_dx": 4 * 4.233e-07,                 # measured 4.233e-07, x 4
    "softmax_fwd": 4 * 2.028e-07,                # measured 2.028e-07, x 4
    "softmax_bwd": 4 * 1.364e-07,                # measured 1.364e-07, x 4
    "softmax_off_fwd": 4 * 1.953e-07,            # measured 1.953e-07, x 4
    "softmax_off_bwd": 4 * 7.364e-08,            # measured 7.364e-08, x 4
    "scale_add": 4 * 1.495e-07,                  # measured 1.495e-07, x 4
    "act_bwd": 4 * 1.133e-07,                    # measured 1.133e-07, x 4
    "add_pe": FLOOR,                             # measured 5.960e-08, x 4 is below the floor
    "axpby": 4 * 1.181e-07,                      # measured 1.181e-07, x 4
}
