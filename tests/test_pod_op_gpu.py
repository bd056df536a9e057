"""Pooled feature distillation on the device: vilco_pod_fwd / _bwd / _record (csrc/pod.hip) and ops.pod_distill / pod_record
against the float64 restatement tests/pod_restatement.py.

The C entry points are called directly with every gradient tensor pre-filled with a sentinel and the workspace with 0xA5, so
every case also checks the footprint: the backward assigns EVERY element -- the compared ones (t < V in a row with a record)
their value, all others an exact zero.

Bounds are counted roundings, u = 2^-24, gamma(n) = n u / (1 - n u) -- never measurements.  k = C + V.
  u-vector.  A square is fl(h h): relative u.  p and q are fp64 sums of non-negative terms, so every v_i is relative u off (the
    fp64 additions, 2^-53 each, are far inside the slack below), and so is n = ||v||.  v_i / n: gamma(2); rounded to fp32 once
    (the value a record holds): gamma(3).  With the fp64 operations: |u^_i - u_i| <= gamma(4) |u_i|, so ||u^ - u|| <= eta :=
    gamma(4), because ||u|| = 1 (or u = 0 exactly when all features of the level are 0).
  dist.  u - r and the norm are fp64: |dist^ - dist| <= eta, an ABSOLUTE term -- the cancellation in u - r.  The scalar:
    |out - loss| <= W n_pairs eta + u |loss|,  W = scale / (L N_rec), n_pairs = the (row, level) pairs compared; the last term
    is the one rounding of out to fp32.
  gradient.  a = (u - r) / dist is a unit vector; a^ - a = (eps dist - e ddist) / (dist dist^) with ||eps||, |ddist| <= eta, so
    ||a^ - a|| <= alpha := 2 eta / (dist - eta): the 1 / dist factor, dist from the restatement.  The projection
    a - u (u . a) with u^ for u, a^ for a: ||error|| <= beta := 2 alpha + 2 eta (1 + alpha) (1 + eta).  Division by n^ (relative
    u): ||g_v^ - g_v|| <= E := |w| / n (beta + 2 u) (1 + 4 u), n = max(||v||, 1e-12) from the restatement.  g_v is rounded to
    fp32 (u), d_h = fl(fl(2 h) fl(g_v[c] + g_v[C + t])): 2 h is exact, the sum and the product round once each, so
    |d_h^ - d_h| <= 2 |h| (2 E + gamma(3) (|g_v[c]| + |g_v[C + t]| + 2 E)) + 2^-149.
  N_rec: equal as an integer.  Two calls: equal bits.
The bounded cases use independent random records, so dist is O(1); `check` asserts dist > 0.1 for every compared pair, on the
CPU, with the restatement."""
import ctypes as C

import pytest
import torch

import pod_restatement as P

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SCALE = 1.5
LEVELS = (8, 4, 2, 1)
SENTINEL = -777.25
# V = T on every level; a level with V = 1 and one with V = 0; a clip so short that only the first level has valid positions
VALID = [[8, 4, 2, 1], [5, 3, 1, 0], [3, 0, 0, 0]]


def gamma(n):
    return n * U / (1 - n * U)


ETA = gamma(4)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


class Case:
    """feats: L tensors [B, T_l, C]; has[b]: row b has a record -- independent random, every level's slice a unit vector.
    misalign: the records are views one float into their buffers."""

    def __init__(self, dev, C_, has, levels=LEVELS, valid=None, seed=0, misalign=False):
        g = torch.Generator().manual_seed(seed)
        self.levels, self.B, self.C, self.dev = tuple(levels), len(has), C_, dev
        self.W = sum(C_ + T for T in levels)
        self.feats = [torch.randn(self.B, T, C_, generator=g).to(dev) for T in levels]
        self.valid = [list(v) for v in (valid if valid is not None else VALID[:self.B])]
        self.bufs, self.records = [], []
        for h in has:
            if not h:
                self.records.append(None)
                continue
            parts = [torch.randn(C_ + T, generator=g) for T in levels]
            vec = torch.cat([p / p.norm() for p in parts])
            buf = torch.cat([torch.zeros(1), vec, torch.zeros(1)]).to(dev)
            self.bufs.append(buf)
            self.records.append(buf[1:1 + self.W] if misalign else buf[1:1 + self.W].clone())
        self.set_table()
        self.level_len = torch.tensor(self.valid, dtype=torch.int32, device=dev)

    def set_table(self):
        self.tab = torch.tensor([0 if z is None else z.data_ptr() for z in self.records], dtype=torch.int64, device=self.dev)

    def desc(self):
        from vilco_amd import _lib
        L = len(self.levels)
        self._T = (_lib.i32 * L)(*self.levels)
        self._ptrs = (_lib.c_fp * L)(*[f.data_ptr() for f in self.feats])
        d = _lib.PodDesc()
        d.feats, d.level_T = C.addressof(self._ptrs), C.addressof(self._T)
        d.level_len, d.pod_tab = self.level_len.data_ptr(), self.tab.data_ptr()
        d.B, d.C, d.L, d.scale = self.B, self.C, L, SCALE
        return d

    def workspace(self):
        from vilco_amd import _lib
        d = self.desc()
        nws = _lib.load().vilco_pod_workspace(self._T, len(self.levels), self.B, self.C)
        assert nws > 0
        return d, nws, torch.full((nws,), 0xA5, dtype=torch.uint8, device=self.dev)

    def run(self, g_out=1.0):
        """-> (out float32 tensor [1], N_rec int, gradients pre-filled with the sentinel)"""
        from vilco_amd import _lib
        lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
        d, nws, ws = self.workspace()
        out = torch.full((1,), float('nan'), device=self.dev)
        g = torch.full((1,), float(g_out), device=self.dev)
        grads = [torch.full_like(f, SENTINEL) for f in self.feats]
        gptrs = (_lib.c_fp * len(grads))(*[t.data_ptr() for t in grads])
        try:
            _lib.check(lib.vilco_pod_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws, s))
            _lib.check(lib.vilco_pod_bwd(C.byref(d), g.data_ptr(), gptrs, ws.data_ptr(), nws, s))
        finally:
            torch.cuda.synchronize()
        off = (-ws.data_ptr()) % 256
        return out, int(ws[off:off + 8].view(torch.int64)[0]), grads

    def record(self):
        """vilco_pod_record over the case's features -> [B, W], pre-filled with the sentinel"""
        from vilco_amd import _lib
        lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
        d, nws, ws = self.workspace()
        d.pod_tab = None
        rec = torch.full((self.B, self.W), SENTINEL, device=self.dev)
        try:
            _lib.check(lib.vilco_pod_record(C.byref(d), rec.data_ptr(), ws.data_ptr(), nws, s))
        finally:
            torch.cuda.synchronize()
        return rec

    def want(self, g_out=1.0):
        return P.pod_term(self.feats, self.valid, self.records, SCALE, g_out)


def check(case, g_out=1.0, label="", bounded=True):
    """one forward + backward of the C entry points against the restatement, footprint included -> (out, N_rec, gradients)"""
    out, N, grads = case.run(g_out)
    w = case.want(g_out)
    assert N == w['n_rec'], (N, w['n_rec'])
    got = float(out[0].double())
    L = len(case.levels)
    for l, (gr, m) in enumerate(zip(grads, w['compared'])):
        outside = gr[~m.to(gr.device)]
        assert bool((outside == 0).all()), "level %d: an element that is not compared was not assigned zero" % l
    if N == 0:
        assert got == 0.0 and int(_bits(out)[0]) == 0, got
        return out, N, grads
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(gr).all()) for gr in grads)
    pairs = sorted(w['gv'])
    if bounded:
        assert pairs and min(w['dist'][b][l] for b, l in pairs) > 0.1, "a bounded case needs dist > 0.1 on every compared pair"
    Wt = SCALE / (L * N)
    b_loss = Wt * len(pairs) * ETA + U * abs(w['loss']) + 2.0 ** -149
    worst = 0.0
    for b, l in pairs:
        V = min(case.valid[b][l], case.levels[l])
        h = case.feats[l][b, :V].double().cpu()
        gv, d, n = w['gv'][(b, l)], w['dist'][b][l], w['norm'][b][l]
        alpha = 2 * ETA / (d - ETA)
        beta = 2 * alpha + 2 * ETA * (1 + alpha) * (1 + ETA)
        E = abs(g_out) * Wt / n * (beta + 2 * U) * (1 + 4 * U)
        mag = gv[:case.C].abs()[None, :] + gv[case.C:].abs()[:, None]
        bound = 2 * h.abs() * (2 * E + gamma(3) * (mag + 2 * E)) + 2.0 ** -149
        err = (grads[l][b, :V].double().cpu() - w['grads'][l][b, :V]).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (label, b, l, float((err / bound).max()))
    print("%s loss %.6g err / bound = %.3f, gradient max err / bound = %.3f (N_rec = %d, %d pairs)"
          % (label, got, abs(got - w['loss']) / b_loss, worst, N, len(pairs)))
    assert abs(got - w['loss']) <= b_loss, (got, w['loss'], b_loss)
    return out, N, grads


@pytest.mark.parametrize("C_", [1, 5, 64, 70])
def test_against_the_restatement(dev, C_):
    """C = 1 (one lane), 5 (scalar loads), 64 (one float4 per lane of 16 lanes), 70 (C % 4 != 0, two scalar column chunks); rows with
    V = T, V = 1, V = 0 and a clip with one valid level"""
    case = Case(dev, C_, [True, True, True], seed=100 + C_)
    assert (case.feats[0].data_ptr() % 16 == 0) and all(z.data_ptr() % 4 == 0 for z in case.records)
    _, N, _ = check(case, g_out=0.75, label="C=%d" % C_)
    assert N == 3


@pytest.mark.parametrize("C_", [5, 64])
def test_a_row_without_a_record_in_the_middle(dev, C_):
    case = Case(dev, C_, [True, False, True], seed=200 + C_)
    assert int(case.tab[1]) == 0
    _, N, grads = check(case, label="hole C=%d" % C_)
    assert N == 2 and all(bool((g[1] == 0).all()) for g in grads)


def test_no_row_has_a_record(dev):
    """the output is an exact 0, N_rec = 0 and every gradient element an exact 0 -- through autograd too"""
    from vilco_amd import ops
    case = Case(dev, 5, [False, False, False], seed=30)
    out, N, grads = check(case, bounded=False)
    assert N == 0 and int(_bits(out)[0]) == 0 and all(bool((g == 0).all()) for g in grads)
    xs = [f.clone().requires_grad_(True) for f in case.feats]
    loss, count = ops.pod_distill(xs, case.level_len, case.tab, SCALE, return_count=True)
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    assert float(loss.detach()) == 0.0 and int(count) == 0
    assert all(x.grad is not None and bool((x.grad == 0).all()) for x in xs)


@pytest.mark.parametrize("C_", [5, 64])
def test_misaligned_records(dev, C_):
    """records one float into their buffers"""
    case = Case(dev, C_, [True, True, True], seed=300 + C_, misalign=True)
    assert all(z.data_ptr() % 16 == 4 for z in case.records)
    check(case, label="misaligned C=%d" % C_)


@pytest.mark.parametrize("C_", [1, 5, 64, 70])
def test_records_of_the_same_features_give_zero_distance_and_gradient(dev, C_):
    """vilco_pod_record: u within gamma(4) of the restatement's, entries at t >= V zero; fed back as the records of the same
    features the distance is an exact 0 and so is every gradient element, none of them NaN"""
    case = Case(dev, C_, [True, True, True], seed=400 + C_)
    rec = case.record()
    for b in range(case.B):
        want = P.make_record([f[b].cpu() for f in case.feats], case.valid[b])
        got = rec[b].double().cpu()
        assert bool(((got - want).abs() <= ETA * want.abs() + 2.0 ** -149).all()), b
        assert bool((got[want == 0] == 0).all())
    case.records = [rec[b] for b in range(case.B)]
    case.set_table()
    out, N, grads = case.run(0.5)
    assert N == 3 and int(_bits(out)[0]) == 0, float(out[0])
    assert all(bool((g == 0).all()) and not bool(torch.isnan(g).any()) for g in grads)


def test_all_zero_features_in_one_level(dev):
    """||v|| = 0 is clamped at 1e-12: u = 0, dist = ||r||, the level's gradient 2 * 0 * g_v = 0, everything finite"""
    case = Case(dev, 5, [True, True, True], seed=50)
    case.feats[1].zero_()
    torch.cuda.synchronize()
    w = case.want()
    assert w['norm'][0][1] == 1e-12 and w['dist'][0][1] > 0.1
    _, N, grads = check(case, label="zero level")
    assert N == 3 and bool((grads[1] == 0).all()) and bool((grads[0] != 0).any())


@pytest.mark.parametrize("C_", [5, 64])
def test_first_level_one_row_longer_than_a_tile(dev, C_):
    """two blocks on level 0, the second with one row: its column partial is added behind the first's"""
    from vilco_amd import ops
    tile = ops.pod_tile_rows()
    assert tile >= 1
    levels = (tile + 1, 4, 2, 1)
    valid = [[tile + 1, 4, 2, 1], [tile, 3, 1, 0], [3, 0, 0, 0]]
    case = Case(dev, C_, [True, True, True], levels=levels, valid=valid, seed=600 + C_)
    check(case, g_out=-1.25, label="tile+1 C=%d" % C_)


def test_two_calls_give_the_same_bits(dev):
    from vilco_amd import ops
    tile = ops.pod_tile_rows()
    for case in (Case(dev, 70, [True, False, True], seed=70),
                 Case(dev, 64, [True, True, True], levels=(3 * tile + 5, 9), valid=[[3 * tile + 5, 9], [2 * tile, 1], [tile + 1, 0]], seed=71)):
        o1, n1, g1 = case.run(0.5)
        o2, n2, g2 = case.run(0.5)
        r1, r2 = case.record(), case.record()
        assert n1 == n2 > 0 and torch.equal(_bits(o1), _bits(o2)) and torch.equal(_bits(r1), _bits(r2))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(g1, g2))


def test_bad_arguments(dev):
    from vilco_amd import _lib
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    case = Case(dev, 5, [True, True, True], seed=80)
    d, nws, ws = case.workspace()
    out = torch.zeros(1, device=dev)
    grads = [torch.zeros_like(f) for f in case.feats]
    gptrs = (_lib.c_fp * 4)(*[t.data_ptr() for t in grads])

    def fwd(**kw):
        d = case.desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.vilco_pod_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws, s)
    assert fwd() == 0
    for bad in (dict(L=0), dict(L=17), dict(B=0), dict(C=0), dict(feats=None), dict(level_T=None), dict(level_len=None),
                dict(pod_tab=None)):
        assert fwd(**bad) == -1, bad
    d = case.desc()
    assert lib.vilco_pod_fwd(C.byref(d), None, ws.data_ptr(), nws, s) == -1
    assert lib.vilco_pod_fwd(C.byref(d), out.data_ptr(), None, nws, s) == -1
    assert lib.vilco_pod_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws - 1, s) == -4
    assert lib.vilco_pod_bwd(C.byref(d), out.data_ptr(), gptrs, ws.data_ptr(), nws - 1, s) == -4
    assert lib.vilco_pod_bwd(C.byref(d), out.data_ptr(), None, ws.data_ptr(), nws, s) == -1
    assert lib.vilco_pod_bwd(C.byref(d), None, gptrs, ws.data_ptr(), nws, s) == -1
    assert lib.vilco_pod_record(C.byref(d), None, ws.data_ptr(), nws, s) == -1
    torch.cuda.synchronize()


def test_op_and_autograd(dev):
    """ops.pod_distill / pod_record: the same bits as the entry points, a gradient per level scaled by the upstream gradient;
    argument checks"""
    from vilco_amd import ops
    case = Case(dev, 22, [True, False, True], seed=90)
    out, N, grads = case.run(2.0)
    xs = [f.clone().requires_grad_(True) for f in case.feats]
    loss, count = ops.pod_distill(xs, case.level_len, case.tab, SCALE, return_count=True)
    (2.0 * loss).backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and torch.equal(_bits(loss.reshape(1)), _bits(out)) and int(count) == N == 2
    assert all(torch.equal(_bits(x.grad), _bits(g)) for x, g in zip(xs, grads))
    assert torch.equal(_bits(ops.pod_record(case.feats, case.level_len)), _bits(case.record()))
    with pytest.raises(ValueError):
        ops.pod_distill(case.feats, case.level_len[:, :3].contiguous(), case.tab, SCALE)
    with pytest.raises(ValueError):
        ops.pod_distill(case.feats, case.level_len, case.tab.int(), SCALE)
    with pytest.raises(ValueError):
        ops.pod_distill(case.feats[:3] + [case.feats[3][:, :, :5]], case.level_len, case.tab, SCALE)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pod_distill([f.cpu() for f in case.feats], case.level_len, case.tab, SCALE)


def test_against_the_tensor_op_body(dev):
    """the A/B reference a CPU model runs (cl_methods.pod.pod_term), on the device in fp32: both within the op's loss bound of the
    restatement, the body's widened by its fp32 sums (gamma(k) per norm, k <= C + T_0 entries, twice: ||v|| and ||u - r||)"""
    from vilco_amd import ops
    from vilco_amd.cl_methods import pod
    case = Case(dev, 22, [True, True, False], seed=95)
    w = case.want()
    xs = [f.clone().requires_grad_(True) for f in case.feats]
    body, n = pod.pod_term(xs, case.valid, case.records, SCALE)
    loss, count = ops.pod_distill(case.feats, case.level_len, case.tab, SCALE, return_count=True)
    assert n == w['n_rec'] == int(count) == 2
    npairs, L = len(w['gv']), len(case.levels)
    b_op = SCALE / (L * 2) * npairs * ETA + U * w['loss']
    k = case.C + max(case.levels)
    b_body = SCALE / (L * 2) * npairs * (2 * gamma(k + 4) + ETA) + gamma(npairs + 2) * w['loss']
    assert abs(float(loss) - w['loss']) <= b_op
    assert abs(float(body) - w['loss']) <= b_body
