"""The multi-tensor step kernels of vilco_amd/csrc/optim.hip at their chunk edges -- vilco_grad_norm, vilco_optim_step (AdamW, SGD),
vilco_cl_penalty (plain and atomic), vilco_store_f32 -- against the float64 restatement (tests/optim_restatement.py), and
FusedOptimizer against torch.optim over a trajectory and through checkpoints.

Kernel tests call the C entry points with hand-built chunk tables, so every tensor is a view into its own buffer: it starts 1 to 4
elements in (bases are not 16-byte aligned, and differ between the streams of one tensor), everything around the view is guard
elements that must keep their bits, and the streams a kernel only reads must keep all of theirs.

Bounds are counted roundings, u = 2^-24 (gamma(n) = n u / (1 - n u)), never measurements; one call is checked at a time, from the
device's own fp32 state before the call.  sqrtf, expm1f count as 1 ulp = 2 u, + - * / as u."""
import copy
import ctypes as C
import warnings

import pytest
import torch

import optim_restatement as R

U = 2.0 ** -24
CHUNK = R.CHUNK
pytestmark = pytest.mark.gpu

SIZES_A = [1, 3, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
SIZES_B = [(7 * i) % 65 + 1 for i in range(300)]            # 300 chunks: more than the 256 threads that sum the partials
TABLES = {"edges": SIZES_A, "many": SIZES_B}
STEPS = [1, 2, 3, 5, 10, 100, 1000]
LRS = [1e-2 * (1 + 0.25 * k) for k in range(8)]
WDS = [0.05, 0.0, 0.01, 0.1, 0.04, 0.02, 0.0, 0.2]
BETA1, BETA2, EPS, MOM = 0.9, 0.999, 1e-8, 0.9


def gamma(n):
    return n * U / (1 - n * U)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class Slot:
    """one tensor of a table: a view of `n` elements into a buffer of its own, `start` = 1..4 elements in, one guard behind"""

    def __init__(self, values, rot, dev):
        self.n, self.start = values.numel(), 1 + rot % 4
        host = torch.full((self.start + self.n + 1,), 1234.5)
        host[self.start:self.start + self.n] = values.float()
        self.buf = host.to(dev)
        self.view = self.buf[self.start:self.start + self.n]
        assert self.view.data_ptr() % 16 == (4 * self.start) % 16
        self.before = self.buf.clone()

    def snap(self):
        self.before = self.buf.clone()

    def restore(self):
        self.buf.copy_(self.before)

    def old(self):
        return self.before[self.start:self.start + self.n]

    def guards_kept(self):
        s, e = self.start, self.start + self.n
        return _same_bits(self.buf[:s], self.before[:s]) and _same_bits(self.buf[e:], self.before[e:])

    def untouched(self):
        return _same_bits(self.buf, self.before)


def _slots(dev, sizes, seed, stream, scale=1.0, fn=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        x = torch.randn(n, generator=g) * scale
        out.append(Slot(fn(x) if fn else x, i + stream, dev))
    return out


def Table(dev, rows, numels):
    """R.Table over slot rows: the addresses are those of the misaligned views"""
    return R.Table(dev, [[s.view.data_ptr() for s in r] for r in rows], numels)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from vilco_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------------------------------------------------------- vilco_grad_norm
def _grad_norm(tb, max_norm):
    L, lib = _lib()
    out = torch.full((2,), float('nan'), device=tb.dev)
    L.check(lib.vilco_grad_norm(C.byref(tb.struct()), float(max_norm), tb.partial.data_ptr(), out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return out.cpu()


def _grad_table(dev, sizes, seed, scale=1.0):
    gs = _slots(dev, sizes, seed, 1, scale)
    with torch.no_grad():
        gs[0].view[0] = 3.0 * scale          # the first partial carries weight: dropping it cannot hide in the bound
    gs[0].snap()
    return Table(dev, [gs, gs, gs, gs], sizes), gs


NORM_ROUNDINGS = 38          # sum: 1 square + 64 adds per thread + 6 wave levels + 2 adds = 73 u; sqrt halves it; + the cast


@pytest.mark.parametrize("name", list(TABLES))
def test_grad_norm_and_coefficient(dev, name):
    """sum of squares: non-negative terms, each thread squares (1) and adds (64) at most CHUNK / 256 = 64 elements, six wave
    levels, two adds, the rest in double: 73 u on the sum, 36.5 u on its root, one more for the cast to fp32: 38 u on the norm.
    Coefficient: the norm's 38 u, the add of 1e-6 and the division: 40 u, and 1 u for 1e-6 as fp32: 41 u.  Where the norm is
    below max_norm, and where max_norm <= 0, the coefficient is 1.0f exactly."""
    sizes = TABLES[name]
    probe, gs = _grad_table(dev, sizes, 1)
    norm1, _ = R.clip([s.view for s in gs], -1.0)
    tb, gs = _grad_table(dev, sizes, 1, scale=0.3 / norm1)          # norm 0.3: between max_norm / 2 and max_norm = 0.5
    for max_norm, scale_g in ((-1.0, 1.0), (0.5, 1.0), (0.5, 10.0)):
        if scale_g != 1.0:
            tb, gs = _grad_table(dev, sizes, 1, scale=3.0 / norm1)
        want_norm, want_coef = R.clip([s.view for s in gs], max_norm)
        out = _grad_norm(tb, max_norm)
        again = _grad_norm(tb, max_norm)
        e_n, e_c = abs(float(out[0]) - want_norm) / want_norm, abs(float(out[1]) - want_coef) / want_coef
        print("%s max_norm %g norm %.4f: norm err / bound = %.3f, coef err / bound = %.3f"
              % (name, max_norm, want_norm, e_n / gamma(NORM_ROUNDINGS), e_c / gamma(NORM_ROUNDINGS + 3)))
        assert e_n <= gamma(NORM_ROUNDINGS) and e_c <= gamma(NORM_ROUNDINGS + 3)
        if scale_g == 1.0:
            assert want_norm < 0.5 and float(out[1]) == 1.0
        else:
            assert want_coef < 0.2
        assert _same_bits(out, again)
        assert all(s.untouched() for s in gs)


def test_grad_norm_of_nothing(dev):
    tb, gs = _grad_table(dev, SIZES_A, 2, scale=0.0)
    assert all(float(s.view.abs().max()) == 0.0 for s in gs)
    for max_norm in (0.5, -1.0):
        out = _grad_norm(tb, max_norm)
        assert out.tolist() == [0.0, 1.0]
    empty = Table(dev, [[], [], [], []], [])
    assert empty.nchunks == 0 and _grad_norm(empty, 0.5).tolist() == [0.0, 1.0]


# --------------------------------------------------------------------------------------------------------------- vilco_optim_step
class StepCase:
    """p, g, m, v slots of one table with per-tensor step counts, eight groups in scrambled order, and the regimes of table
    'edges': tensor 5 has g = m = v = 0, tensor 7 has |g| ~ 1e-10 and m = v = 0"""

    def __init__(self, dev, name, kind, seed):
        sizes = TABLES[name]
        self.dev, self.kind, self.sizes, n = dev, kind, sizes, len(sizes)
        self.p = _slots(dev, sizes, seed, 0, 1e-3)
        self.g = _slots(dev, sizes, seed + 1, 1)
        self.m = _slots(dev, sizes, seed + 2, 2, 0.1)
        self.v = _slots(dev, sizes, seed + 3, 3, 0.01, fn=torch.abs)
        self.steps = [float(STEPS[(3 * i + 1) % len(STEPS)]) for i in range(n)]
        self.group = [(5 * i + 3) % 8 for i in range(n)]
        self.zero_g = self.tiny_g = None
        if name == "edges":
            self.zero_g, self.tiny_g = 5, 7
            with torch.no_grad():
                self.g[5].view.zero_()
                self.g[7].view.mul_(1e-10)
                for i in (5, 7):
                    self.m[i].view.zero_()
                    self.v[i].view.zero_()
        if kind == "SGD":
            with torch.no_grad():
                for i, t in enumerate(self.steps):
                    if t <= 1:
                        self.m[i].view.fill_(float('nan'))
        for s in self.p + self.g + self.m + self.v:
            s.snap()
        self.table = Table(dev, [self.p, self.g, self.m, self.v], sizes)
        self.tstep = torch.tensor(self.steps, dtype=torch.float32).to(dev)
        self.tgroup = torch.tensor(self.group, dtype=torch.int32).to(dev)
        self.amax = torch.full((self.table.nchunks,), float('nan'), device=dev)

    def restore(self):
        for s in self.p + self.g + self.m + self.v:
            s.restore()
        self.amax.fill_(float('nan'))

    def run(self, coef=None, lr_dev=None, ngroups=8, kind=None, lrs=LRS):
        L, lib = _lib()
        tb = self.table
        lr, wd = (C.c_float * 9)(*(list(lrs) + [0.0])), (C.c_float * 9)(*(WDS + [0.0]))
        kind = (0 if self.kind == "AdamW" else 1) if kind is None else kind
        d = L.OptimDesc(table=tb.struct(), kind=kind, group=self.tgroup.data_ptr(), lr=C.addressof(lr), wd=C.addressof(wd),
                        ngroups=ngroups, beta1=BETA1, beta2=BETA2, eps=EPS, momentum=MOM,
                        tensor_step=self.tstep.data_ptr(), norm_coef=None if coef is None else coef.data_ptr(),
                        chunk_amax=self.amax.data_ptr(), lr_dev=None if lr_dev is None else lr_dev.data_ptr())
        try:
            L.check(lib.vilco_optim_step(C.byref(d), _stream()))
        finally:
            torch.cuda.synchronize()

    def check_placement(self, written):
        for s in self.g:
            assert s.untouched()
        for rows in written:
            for s in rows:
                assert s.guards_kept()

    def check_amax(self):
        """max over a tensor's chunk partials == max |p_new|, exactly"""
        for i, s in enumerate(self.p):
            parts = self.amax[self.table.first[i]:self.table.first[i + 1]]
            assert float(parts.max()) == float(s.view.abs().max()), (i, s.n)


def _ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


ADAM_A, ADAM_B = 4, 22


def _check_adamw(case, coef_value):
    """m: beta1 m and (1 - beta1)(c g) carry 1 and 2 roundings, their sum one more: gamma(3) (|t1| + |t2|)   (1 - beta is exact).
    v: beta2 v carries 1, ((1 - beta2)(c g))(c g) carries 4, the sum one more: gamma(5) (|t1| + |t2|), relative as v >= 0.
    p: a = 4: 1 - lr wd (2), the decay product (1), the final subtraction (1, also on |delta|).
       b = 22 on delta = step_size (|t1| + |t2|) / denom: bias corrections -expm1f(t log beta): fp32 log beta (1), t log beta (1),
       expm1f (2) = 4 each; step_size = lr / bc1: 5; sqrtf(bc2): 2 + 2 = 4; sqrtf(v): 2.5 + 2; / rs2: + 4 + 1; + eps: + 1 = 10.5 on
       denom; m / denom: 3 (m, on its absolute addends) + 10.5 + 1; times step_size: + 5 + 1; the subtraction: + 1 = 21.5."""
    worst = {}
    for i, n in enumerate(case.sizes):
        gi = case.group[i]
        p, m, v, mags = R.adamw_step(case.p[i].old(), case.g[i].old(), case.m[i].old(), case.v[i].old(), case.steps[i], LRS[gi],
                                     WDS[gi], BETA1, BETA2, EPS, coef_value)
        e_m = (case.m[i].view.double().cpu() - m).abs()
        e_v = (case.v[i].view.double().cpu() - v).abs()
        e_p = (case.p[i].view.double().cpu() - p).abs()
        b_m = gamma(3) * (mags['m_terms'][0] + mags['m_terms'][1])
        b_v = gamma(5) * (mags['v_terms'][0] + mags['v_terms'][1])
        b_p = gamma(ADAM_A) * mags['p_old'] + gamma(ADAM_B) * mags['delta']
        r = (_ratio(e_m, b_m), _ratio(e_v, b_v), _ratio(e_p, b_p))
        print("adamw numel %6d step %4d group %d: max err / bound  m %.3f  v %.3f  p %.3f   (delta part of p's bound: %.2f)"
              % (n, case.steps[i], gi, r[0], r[1], r[2], float((gamma(ADAM_B) * mags['delta'] / b_p.clamp_min(1e-300)).median())))
        worst[case.steps[i]] = max(worst.get(case.steps[i], 0.0), r[2])
        assert bool((e_m <= b_m).all()) and bool((e_v <= b_v).all()), (n, case.steps[i])
        assert bool((e_p <= b_p).all()), (n, case.steps[i], r[2])
        if i == case.zero_g:             # g == 0: m and v stay zero, p only decays
            assert float(case.m[i].view.abs().max()) == 0.0 and float(case.v[i].view.abs().max()) == 0.0
            assert float(mags['delta'].max()) == 0.0 and not _same_bits(case.p[i].view, case.p[i].old())
        if i == case.tiny_g:             # eps dominates the denominator
            assert float((case.v[i].view.double().cpu().sqrt() / (1 - R.f32(BETA2) ** case.steps[i]) ** 0.5).max()) < 0.1 * EPS
    print("adamw worst p ratio per step count:", {int(k): round(x, 3) for k, x in sorted(worst.items())})


@pytest.mark.parametrize("with_coef", [False, True], ids=["nocoef", "coef"])
@pytest.mark.parametrize("name", list(TABLES))
def test_adamw_one_call(dev, name, with_coef):
    """step counts 1, 2, 3, 5, 10, 100, 1000 and eight (lr, wd) groups mixed over the tensors of one call; bounds in _check_adamw"""
    case = StepCase(dev, name, "AdamW", 10)
    coef = torch.tensor([7.0, 0.37]).to(dev) if with_coef else None
    case.run(coef=coef)
    assert sorted(set(case.steps)) == STEPS and len(set(case.group)) == 8
    _check_adamw(case, R.f32(0.37) if with_coef else 1.0)
    case.check_placement([case.p, case.m, case.v])
    case.check_amax()
    # learning rates read from device memory: the same bits
    got = [[s.view.clone() for s in rows] for rows in (case.p, case.m, case.v)]
    case.restore()
    case.run(coef=coef, lr_dev=torch.tensor(LRS, dtype=torch.float32).to(dev), lrs=[123.0] * 8)
    for rows, kept in zip((case.p, case.m, case.v), got):
        assert all(_same_bits(s.view, k) for s, k in zip(rows, kept))


@pytest.mark.parametrize("with_coef", [False, True], ids=["nocoef", "coef"])
@pytest.mark.parametrize("name", list(TABLES))
def test_sgd_one_call(dev, name, with_coef):
    """buffer: c g (1), wd p (1), their sum (1), momentum buf (1), the sum (1): gamma(3) on the absolute addends.
    p = p - lr buf: a = 1 (the subtraction); b = 5 on delta = lr (sum of absolute addends): buffer 3, lr buf 1, subtraction 1.
    Tensors at step 1 start with a NaN buffer: it is not read, the new buffer is the decayed, clipped gradient.
    Groups 1 and 6 have wd = 0."""
    case = StepCase(dev, name, "SGD", 20)
    coef = torch.tensor([7.0, 0.37]).to(dev) if with_coef else None
    case.run(coef=coef)
    c = R.f32(0.37) if with_coef else 1.0
    assert {WDS[g] == 0 for g in case.group} == {True, False}
    for i, n in enumerate(case.sizes):
        gi = case.group[i]
        p, buf, mags = R.sgd_step(case.p[i].old(), case.g[i].old(), case.m[i].old(), case.steps[i], LRS[gi], WDS[gi], MOM, c)
        e_b = (case.m[i].view.double().cpu() - buf).abs()
        e_p = (case.p[i].view.double().cpu() - p).abs()
        tb, tg, tp = mags['buf_terms']
        b_b = gamma(3) * (tb + tg + tp)
        b_p = gamma(1) * mags['p_old'] + gamma(5) * mags['delta']
        print("sgd numel %6d step %4d group %d: max err / bound  buf %.3f  p %.3f" % (n, case.steps[i], gi, _ratio(e_b, b_b),
                                                                                      _ratio(e_p, b_p)))
        assert bool(torch.isfinite(case.m[i].view).all()) and bool(torch.isfinite(case.p[i].view).all()), n
        assert bool((e_b <= b_b).all()) and bool((e_p <= b_p).all()), (n, case.steps[i])
        if case.steps[i] <= 1:
            assert float(tb.max()) == 0.0 and bool(case.m[i].old().isnan().all())
    case.check_placement([case.p, case.m])
    assert all(s.untouched() for s in case.v)
    case.check_amax()
    got = [[s.view.clone() for s in rows] for rows in (case.p, case.m)]
    case.restore()
    case.run(coef=coef, lr_dev=torch.tensor(LRS, dtype=torch.float32).to(dev), lrs=[123.0] * 8)
    for rows, kept in zip((case.p, case.m), got):
        assert all(_same_bits(s.view, k) for s, k in zip(rows, kept))


def test_optim_step_argument_errors(dev):
    case = StepCase(dev, "edges", "AdamW", 30)
    for bad in (dict(ngroups=9), dict(kind=2), dict(ngroups=0)):
        with pytest.raises(RuntimeError):
            case.run(**bad)
        assert all(s.untouched() for s in case.p + case.g + case.m + case.v), bad


# --------------------------------------------------------------------------------------------------------------- vilco_cl_penalty
class PenaltyCase:
    """params / grads of one table and a list of (param index, prefix length) entries, each with its own importance (>= 0) and
    consolidated value"""

    def __init__(self, dev, sizes, entries, seed, zero_imp=()):
        self.dev, self.sizes, self.entries = dev, sizes, entries
        self.p = _slots(dev, sizes, seed, 0)
        self.g = _slots(dev, sizes, seed + 1, 1)
        pre = [n for _, n in entries]
        self.f = _slots(dev, pre, seed + 2, 2, fn=torch.abs)
        self.o = _slots(dev, pre, seed + 3, 3)
        with torch.no_grad():
            for e in zero_imp:
                self.f[e].view.zero_()
                self.f[e].snap()
        rows = [[self.p[i] for i, _ in entries], [self.g[i] for i, _ in entries], self.f, self.o]
        self.table = Table(dev, rows, pre)

    def run(self, lam, shared):
        L, lib = _lib()
        tb = self.table
        out = torch.full((1,), float('nan'), device=self.dev)
        L.check(lib.vilco_cl_penalty(C.byref(tb.struct()), float(lam), int(shared), tb.partial.data_ptr(), out.data_ptr(),
                                     _stream()))
        torch.cuda.synchronize()
        return float(out[0])

    def want(self, lam):
        ent = [(i, f.old(), o.old()) for (i, _), f, o in zip(self.entries, self.f, self.o)]
        return R.penalty([s.old() for s in self.p], [s.old() for s in self.g], ent, lam)

    def check(self, lam, value, tag):
        """value: F >= 0; every term is formed in double and rounded once (1), 64 adds per thread, 6 wave levels, 2 adds, the
        cast of the double total: 74 u relative.  Gradient: u * (entries touching the element + 1) * (|g| + sum |terms|): one
        rounding for each added term (formed in double) and one per add, each at most u times the sum of the absolute terms,
        whatever the order the terms arrive in."""
        want_v, want_g, mags = self.want(lam)
        e_v = abs(value - want_v) / want_v
        print("%s penalty value err / bound = %.3f" % (tag, e_v / gamma(74)))
        assert e_v <= gamma(74)
        for i, n in enumerate(self.sizes):
            err = (self.g[i].view.double().cpu() - want_g[i]).abs()
            k = mags['touched'][i]
            bound = U * (k + 1).double() * mags['abs_sum'][i]
            print("%s numel %6d entries %d: grad max err / bound = %.3f" % (tag, n, int(k.max()), _ratio(err, bound)))
            assert bool((err <= bound).all()), (tag, n)
            beyond = k == 0
            assert torch.equal(_bits(self.g[i].view).cpu()[beyond], _bits(self.g[i].old()).cpu()[beyond]), (tag, n)
            assert int(k.max()) == 0 or not _same_bits(self.g[i].view, self.g[i].old())
            assert self.g[i].guards_kept()
        assert all(s.untouched() for s in self.p + self.f + self.o)


def _prefix(n, j):
    """prefix length of a parameter's j-th entry: all of it, then two shorter ones (for 2 CHUNK + 5: one ends inside the second
    chunk, one inside the first)"""
    return (n, max(1, n - n // 3), max(1, n // 3 + 1))[j]


@pytest.mark.parametrize("name", list(TABLES))
def test_penalty_plain_path(dev, name):
    """every parameter once, whole ('many') or with a prefix on every second tensor ('edges'); both kernels agree within the
    bound when no parameter is shared"""
    sizes = TABLES[name]
    entries = [(i, _prefix(n, 1) if (name == "edges" and i % 2) else n) for i, n in enumerate(sizes)]
    lam = 0.37
    plain, atomic = PenaltyCase(dev, sizes, entries, 40), PenaltyCase(dev, sizes, entries, 40)
    v_plain, v_atomic = plain.run(lam, 0), atomic.run(lam, 1)
    plain.check(lam, v_plain, name + " plain")
    atomic.check(lam, v_atomic, name + " atomic")
    _, _, mags = plain.want(lam)
    for a, b, s in zip(plain.g, atomic.g, mags['abs_sum']):
        assert bool(((a.view.double() - b.view.double()).abs().cpu() <= 2 * 2 * U * s).all())


def test_penalty_atomic_path_shared_parameters(dev):
    """every parameter in 1, 2 or 3 entries of different prefix lengths; the entries of one parameter are far apart in the
    table, so their blocks are in flight together"""
    sizes = SIZES_A
    entries = [(i, _prefix(n, j)) for j in range(3) for i, n in enumerate(sizes) if j <= i % 3]
    assert sorted(sum(1 for e in entries if e[0] == i) for i in range(3)) == [1, 2, 3]
    case = PenaltyCase(dev, sizes, entries, 50)
    case.check(0.37, case.run(0.37, 1), "shared")
    assert any(0 < n % CHUNK < CHUNK - 1 for _, n in entries if n > CHUNK)


@pytest.mark.parametrize("shared", [0, 1])
def test_penalty_zero_importance_and_zero_lambda(dev, shared):
    """importance 0 over a whole tensor: its gradient keeps its bits; lambda = 0: value 0, every gradient keeps its bits"""
    sizes = SIZES_A
    entries = [(i, n) for i, n in enumerate(sizes)]
    zero = (4, 9, 11)
    case = PenaltyCase(dev, sizes, entries, 60, zero_imp=zero)
    case.table.partial.fill_(float('nan'))
    want_v, want_g, mags = case.want(0.37)
    value = case.run(0.37, shared)
    assert abs(value - want_v) <= gamma(74) * want_v
    for i in range(len(sizes)):
        assert case.g[i].untouched() == (i in zero), i
    for s in case.g:
        s.restore()
    assert case.run(0.0, shared) == 0.0
    assert all(s.untouched() for s in case.g + case.p + case.f + case.o)


# ---------------------------------------------------------------------------------------------------------------- vilco_store_f32
def test_store_f32(dev):
    L, lib = _lib()
    vals = (C.c_float * 17)(*[1.5 + i for i in range(17)])
    for n in (0, 1, 16):
        dst = Slot(torch.zeros(16), 1, dev)
        L.check(lib.vilco_store_f32(dst.view.data_ptr(), vals, n, _stream()))
        torch.cuda.synchronize()
        assert dst.view[:n].tolist() == [1.5 + i for i in range(n)]
        assert _same_bits(dst.view[n:], dst.old()[n:]) and dst.guards_kept()
    dst = Slot(torch.zeros(32), 1, dev)
    assert lib.vilco_store_f32(dst.view.data_ptr(), vals, 17, _stream()) == -1
    assert lib.vilco_store_f32(None, vals, 4, _stream()) == -1
    assert lib.vilco_store_f32(dst.view.data_ptr(), vals, -1, _stream()) == -1
    torch.cuda.synchronize()
    assert dst.untouched()


# ------------------------------------------------------------------------------------------------------------------ FusedOptimizer
# every tensor has at least 1000 elements: the yardstick below is the maximum over a tensor's elements of fp32 torch.optim's own
# rounding error, and over a few dozen elements that maximum is as often as not a fraction of one rounding (measured with a
# 96-element tensor: 0.6 u on exp_avg, the kernel's 2.7 u then stood 4.3 times above it while inside its counted bound of 3 u).
# The small sizes are the one-call tests' business, element by element.
T_SHAPES = [(300, 17), (1100,), (20000,), (64, 16, 1), (33, 31, 3), (1024,)]
T_LRS, T_WDS = (1e-2, 3e-3, 2e-2), (0.05, 0.0, 0.01)
STATE_KEYS = {"AdamW": ("exp_avg", "exp_avg_sq"), "SGD": ("momentum_buffer",)}


def _t_groups(ps):
    """three groups; ps[2] is listed twice, like the adapter aliases"""
    return [{"params": [ps[0], ps[1]], "lr": R.f32(T_LRS[0]), "weight_decay": R.f32(T_WDS[0])},
            {"params": [ps[2], ps[3], ps[2]], "lr": R.f32(T_LRS[1]), "weight_decay": R.f32(T_WDS[1])},
            {"params": [ps[4], ps[5]], "lr": R.f32(T_LRS[2]), "weight_decay": R.f32(T_WDS[2])}]


def _make(kind, impl, values, dev):
    """impl: 'f64' / 'f32' = torch.optim on the CPU in that precision, 'hip' = FusedOptimizer on the device"""
    from vilco_amd.utils.train_utils import FusedOptimizer
    dt, where = (torch.float64, 'cpu') if impl == 'f64' else (torch.float32, dev if impl == 'hip' else 'cpu')
    ps = [v.detach().to(dt).to(where).clone().requires_grad_(True) for v in values]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if impl == 'hip':
            opt = FusedOptimizer(_t_groups(ps), lr=1e-2, kind=kind, momentum=R.f32(MOM), betas=(R.f32(BETA1), R.f32(BETA2)),
                                 eps=R.f32(EPS))      # a checkpoint's groups carry these to the other implementation
        elif kind == "AdamW":
            opt = torch.optim.AdamW(_t_groups(ps), lr=1e-2, betas=(R.f32(BETA1), R.f32(BETA2)), eps=R.f32(EPS))
        else:
            opt = torch.optim.SGD(_t_groups(ps), lr=1e-2, momentum=R.f32(MOM))
    return ps, opt


def _set_grads(ps, it, skip):
    for i, p in enumerate(ps):
        g = torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * it + i))
        p.grad = None if (i == 1 and it in skip) else g.to(p.dtype).to(p.device)


def _snapshot(ps, opt, kind):
    """per parameter: (p, state tensors..., step) as float64 CPU; step from state_dict() as a checkpoint would hold it"""
    sd = opt.state_dict()
    ids = [i for g in sd['param_groups'] for i in g['params']]
    idx = dict(zip([id(p) for p in (ps[0], ps[1], ps[2], ps[3], ps[2], ps[4], ps[5])], ids))
    out = []
    for p in ps:
        st = sd['state'].get(idx[id(p)], {})
        out.append(dict(p=p.detach().double().cpu(), step=float(st['step']) if 'step' in st else None,
                        **{k: st[k].double().cpu() for k in STATE_KEYS[kind] if st.get(k) is not None}))
    return out


def _compare(tag, kind, it, hip, f32, f64, want_steps, rows):
    """HIP error <= 4 x the error of fp32 torch.optim, both against float64 torch.optim, per tensor in the max norm"""
    for i, (h, a, w) in enumerate(zip(hip, f32, f64)):
        if want_steps is not None:
            assert (h['step'] or 0.0) == want_steps[i], (tag, it, i, h['step'])
        for k in ('p',) + STATE_KEYS[kind]:
            assert (k in h) == (k in w), (tag, it, i, k)
            if k not in w:
                continue
            e_h, e_t = float((h[k] - w[k]).abs().max()), float((a[k] - w[k]).abs().max())
            rows.append((tag, kind, it, i, k, e_t, e_h))
            assert e_h <= 4 * e_t, (tag, kind, it, i, k, e_h, e_t)


def _print_rows(rows):
    worst = {}
    for tag, kind, it, i, k, e_t, e_h in rows:
        key = (tag, kind, i, k)
        if key not in worst or e_h / max(e_t, 1e-300) > worst[key][2]:
            worst[key] = (e_t, e_h, e_h / max(e_t, 1e-300), it)
    for (tag, kind, i, k), (e_t, e_h, r, it) in sorted(worst.items()):
        print("%-8s %-5s tensor %d %-15s step %d: fp32 torch.optim %.3e  HIP %.3e  ratio %.2f" % (tag, kind, i, k, it, e_t, e_h, r))


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_trajectory_against_torch_optim(dev, kind):
    """8 steps, three groups, tensor 2 listed twice (its count advances by 2), tensor 1 without a gradient on steps 2 and 5 (its
    count lags); after every step parameters, state tensors and the checkpoint's step counts.  This comparison drifts, so its
    bar is measured against the reference: the same trajectory through fp32 torch.optim on the CPU, error against the float64
    run per tensor, and the HIP error at most 4 times that -- both are fp32 implementations of the same few operations and
    differ in where they round; a wrong coefficient, group or step count is off by orders of magnitude."""
    gen = torch.Generator().manual_seed(5)
    values = [1e-2 * torch.randn(s, generator=gen) for s in T_SHAPES]
    runs = {impl: _make(kind, impl, values, dev) for impl in ('f64', 'f32', 'hip')}
    want_steps, rows = [0.0] * len(T_SHAPES), []
    for it in range(8):
        for impl, (ps, opt) in runs.items():
            _set_grads(ps, it, skip=(2, 5))
            opt.step()
        for i in range(len(T_SHAPES)):
            want_steps[i] += 0 if (i == 1 and it in (2, 5)) else (2 if i == 2 else 1)
        snaps = {impl: _snapshot(ps, opt, kind) for impl, (ps, opt) in runs.items()}
        _compare("traj", kind, it, snaps['hip'], snaps['f32'], snaps['f64'], want_steps, rows)
    _print_rows(rows)
    assert want_steps == [8, 6, 16, 8, 8, 8]


@pytest.mark.parametrize("direction", ["hip_to_torch", "torch_to_hip"])
@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_checkpoint_interchange(dev, kind, direction):
    """3 steps with one implementation, its state_dict() loaded into the other over copies of the parameters, 3 more steps on
    each; both continuations stay within the trajectory test's yardstick of the float64 run.  torch.optim.SGD's state holds a
    momentum_buffer and no step: a parameter loaded that way has been stepped, its buffer is used."""
    gen = torch.Generator().manual_seed(6)
    values = [1e-2 * torch.randn(s, generator=gen) for s in T_SHAPES]
    first, second = ('hip', 'f32') if direction == "hip_to_torch" else ('f32', 'hip')
    runs = {impl: _make(kind, impl, values, dev) for impl in ('f64', 'f32', 'hip')}
    want_steps, rows = [0.0] * len(T_SHAPES), []
    for it in range(6):
        if it == 3:
            ps, opt = runs[first]
            sd = copy.deepcopy(opt.state_dict())
            twin_p, twin = _make(kind, second, [p.detach() for p in ps], dev)
            twin.load_state_dict(sd)
            for a, b in zip(twin.param_groups, opt.param_groups):
                assert a['lr'] == b['lr'] and a['weight_decay'] == b['weight_decay']
            runs['twin'] = (twin_p, twin)
        for impl, (ps, opt) in runs.items():
            _set_grads(ps, it, skip=(1, 4))
            opt.step()
        for i in range(len(T_SHAPES)):
            want_steps[i] += 0 if (i == 1 and it in (1, 4)) else (2 if i == 2 else 1)
        snaps = {impl: _snapshot(ps, opt, kind) for impl, (ps, opt) in runs.items()}
        if it >= 3:
            # torch.optim.SGD keeps no step count: nothing to compare where the state went through it
            for tag, impl in [("resumed", 'twin')] + ([("straight", 'hip')] if first == 'hip' else []):
                counted = kind == "AdamW" or (impl == 'hip' and first == 'hip')
                _compare(direction[:3] + " " + tag, kind, it, snaps[impl], snaps['f32'], snaps['f64'],
                         want_steps if counted else None, rows)
    _print_rows(rows)
