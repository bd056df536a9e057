"""Dark Experience Replay's term on the device: vilco_der_fwd / vilco_der_bwd (csrc/der.hip) and ops.der_replay against the
float64 restatement tests/der_restatement.py, over a pyramid with separator rows.

The C entry points are called directly with a gradient tensor pre-filled with a sentinel, so every case also checks the
footprint: the compared elements are assigned, everything else keeps the sentinel's bits.

Bounds are counted roundings, u = 2^-24, gamma(n) = n u / (1 - n u) -- never measurements.  No transcendentals, every term
of S is non-negative, so nothing cancels:
  loss:  a term is fl(fl(x - z)^2): the difference's rounding enters twice, the square's once -- (1 + d)^3, gamma(3) of the
    term; the sums run in fp64 (2^-53 per addition: far inside the step from gamma(3) to gamma(4)), as do alpha * S / N; the
    result is rounded to fp32 once:    |out - loss| <= gamma(4) loss + u loss.
  gradient:  fl(fl(x - z) * c): one rounding for the difference, one for the product, and c = fl(2 alpha g / N) itself, whose
    double value is exact to 2^-52:    |got - value| <= gamma(3) |value| + ulp(c) / |c| * |value|, ulp(c) / |c| <= 2 u.
  N: equal as an integer."""
import ctypes as C

import pytest
import torch

import der_restatement as D

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ALPHA = 0.1
LEVELS = (8, 4, 2, 1)
SENTINEL = -777.25
# V = T on every level; a level with V = 1 and one with V = 0; a clip so short that only the first level has valid positions
VALID = [[8, 4, 2, 1], [5, 3, 1, 0], [3, 0, 0, 0]]


def gamma(n):
    return n * U / (1 - n * U)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


class Case:
    """x [B, R, C] over `levels` with one separator row behind every level; nbs[b] = None (no record: address 0) or the record's
    class count.  misalign: the records are views one float into their buffers."""

    def __init__(self, dev, C_, nbs, levels=LEVELS, valid=None, seed=0, misalign=False, spread=1.0):
        from vilco_amd import ops
        g = torch.Generator().manual_seed(seed)
        self.levels, self.rows = tuple(levels), sum(levels)
        self.level_row, r = [], 0
        for T in levels:
            self.level_row.append(r)
            r += T + 1
        self.B, self.R, self.C = len(nbs), r, C_
        self.x = (spread * torch.randn(self.B, r, C_, generator=g)).to(dev)
        self.valid = [list(v) for v in (valid if valid is not None else VALID[:self.B])]
        self.bufs, self.records = [], []
        for nb in nbs:
            if nb is None:
                self.records.append(None)
                continue
            buf = torch.randn(self.rows * nb + 1, generator=g).to(dev)
            self.bufs.append(buf)
            self.records.append(buf[1:].view(self.rows, nb) if misalign else buf[:self.rows * nb].view(self.rows, nb))
        self.tab = torch.tensor([[0, 0] if z is None else [z.data_ptr(), z.shape[1]] for z in self.records],
                                dtype=torch.int64, device=dev)
        self.level_len = torch.tensor(self.valid, dtype=torch.int32, device=dev)
        self.ltab = ops._distill_levels(self.level_row, self.levels, dev)

    def desc(self, x=None):
        from vilco_amd import _lib
        d = _lib.DerDesc()
        d.logits, d.level_len, d.der_tab = (self.x if x is None else x).data_ptr(), self.level_len.data_ptr(), self.tab.data_ptr()
        d.level_row, d.level_T, d.level_dev = C.addressof(self.ltab[0]), C.addressof(self.ltab[1]), self.ltab[2].data_ptr()
        d.B, d.R, d.C, d.L, d.alpha = self.B, self.R, self.C, len(self.levels), ALPHA
        return d

    def run(self, g_out=1.0):
        """-> (out float32 tensor [1], N int, d_logits pre-filled with the sentinel)"""
        from vilco_amd import _lib
        lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
        dev = self.x.device
        nws = lib.vilco_der_workspace(self.B * self.rows)
        ws = torch.full((nws,), 0xA5, dtype=torch.uint8, device=dev)
        out = torch.full((1,), float('nan'), device=dev)
        g = torch.full((1,), float(g_out), device=dev)
        dl = torch.full_like(self.x, SENTINEL)
        d = self.desc()
        try:
            _lib.check(lib.vilco_der_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws, s))
            _lib.check(lib.vilco_der_bwd(C.byref(d), g.data_ptr(), dl.data_ptr(), ws.data_ptr(), nws, s))
        finally:
            torch.cuda.synchronize()
        off = (-ws.data_ptr()) % 256
        return out, int(ws[off:off + 8].view(torch.int64)[0]), dl

    def want(self, g_out=1.0, records=None):
        return D.der_term(self.x, self.level_row, self.levels, self.valid, self.records if records is None else records, ALPHA, g_out)


def check(case, g_out=1.0, records=None, label=""):
    """one forward + backward of the C entry points against the restatement, footprint included -> (out, N, d_logits)"""
    out, N, dl = case.run(g_out)
    w_loss, w_N, w_grad, mask, _ = case.want(g_out, records)
    mask = mask.to(dl.device)
    assert N == w_N, (N, w_N)
    got = float(out[0].double())
    b_loss = gamma(4) * w_loss + U * w_loss
    outside = dl[~mask]
    assert torch.equal(_bits(outside), _bits(torch.full_like(outside, SENTINEL))), "something outside the compared elements was written"
    if w_N == 0:
        assert got == 0.0 and int(_bits(out)[0]) == 0, got
        return out, N, dl
    c = 2.0 * ALPHA * g_out / w_N
    inside, w_in = dl[mask].double().cpu(), w_grad[mask.cpu()]
    bound = (gamma(3) + 2 * U) * w_in.abs() + 2.0 ** -149
    err = (inside - w_in).abs()
    print("%s loss err / bound = %.3f, gradient max err / bound = %.3f (N = %d, c = %.3g)"
          % (label, abs(got - w_loss) / b_loss, float((err / bound).max()), N, c))
    assert abs(got - w_loss) <= b_loss, (got, w_loss, b_loss)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(inside).all())
    return out, N, dl


@pytest.mark.parametrize("C_", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_against_the_restatement(dev, C_, rot):
    """n_b in {1, C - 1, C} mixed across the rows of a B = 3 batch (rotated, so every class count meets every pattern of
    valid lengths: V = T, V = 1 and V = 0, a clip with one valid level)"""
    nbs = [1, max(C_ - 1, 1), C_]
    nbs = nbs[rot:] + nbs[:rot]
    case = Case(dev, C_, nbs, seed=10 * C_ + rot)
    _, N, _ = check(case, g_out=0.75, label="C=%d nbs=%s" % (C_, nbs))
    assert N == sum(nb * sum(v) for nb, v in zip(nbs, VALID))


def test_vector_body_with_a_scalar_tail(dev):
    """C = 64: every row of x is 16-byte aligned; n_b = 62 leaves the even rows of the record aligned (15 float4 and two
    elements more), n_b = 64 all of them, n_b = 4 one float4 in lane 0"""
    case = Case(dev, 64, [62, 64, 4], seed=5)
    assert case.x.data_ptr() % 16 == 0 and all(z.data_ptr() % 16 == 0 for z in case.records)
    check(case, label="vector+tail")


def test_one_row_without_a_record(dev):
    for hole in range(3):
        nbs = [3, 5, 4]
        nbs[hole] = None
        case = Case(dev, 5, nbs, seed=20 + hole)
        assert int(case.tab[hole, 0]) == 0
        _, N, dl = check(case, label="hole=%d" % hole)
        assert N > 0 and bool((dl[hole] == SENTINEL).all())


def test_no_row_has_a_record(dev):
    """loss exactly 0, N = 0, backward writes nothing; through autograd the gradient is all zero and nothing is non-finite"""
    from vilco_amd import ops
    case = Case(dev, 5, [None, None, None], seed=30)
    out, N, dl = check(case)
    assert N == 0 and float(out[0]) == 0.0 and bool((dl == SENTINEL).all())
    x = case.x.clone().requires_grad_(True)
    loss, count = ops.der_replay(x, case.level_row, case.levels, case.level_len, case.tab, ALPHA, return_count=True)
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    assert float(loss.detach()) == 0.0 and int(count) == 0 and bool(torch.isfinite(loss.detach()))
    assert x.grad is not None and bool((x.grad == 0).all())


def test_class_count_out_of_range_is_skipped(dev):
    """n_b = 0, -1, C + 1 in the table: the row is skipped -- its record, all NaN, would poison the loss if it were read"""
    for bad in (0, -1, 6, 1 << 40):
        case = Case(dev, 5, [3, 5, 4], seed=40)
        poison = torch.full((case.rows * 6 + 1,), float('nan'), device=dev)
        case.tab[1, 0] = poison.data_ptr()
        case.tab[1, 1] = bad
        torch.cuda.synchronize()
        _, N, dl = check(case, records=[case.records[0], None, case.records[2]], label="n_b=%d" % bad)
        assert N == 3 * sum(VALID[0]) + 4 * sum(VALID[2]) and bool((dl[1] == SENTINEL).all())


def test_misaligned_records_take_the_scalar_path(dev):
    case = Case(dev, 64, [64, 64, 4], seed=50, misalign=True)
    assert all(z.data_ptr() % 16 == 4 for z in case.records)
    check(case, label="misaligned")


def test_more_pairs_than_one_round_of_the_grid(dev):
    """the capped grid covers ops.der_pairs_per_round() pairs at once; B * sum T_l exceeds that by at least one block, so waves
    walk a second pair and every block's partial enters the sum"""
    from vilco_amd import ops
    cap = ops.der_pairs_per_round()
    assert cap % 4 == 0 and cap >= 1024
    rows = -(-(cap + 4) // 3)
    levels = (1024, rows - 1024) if rows > 1025 else (rows - 1, 1)
    assert 3 * sum(levels) >= cap + 4
    case = Case(dev, 3, [3, 2, 3], levels=levels, valid=[list(levels), [levels[0], 1], [levels[0] - 1, levels[1]]], seed=60)
    _, N, _ = check(case, label="pairs=%d cap=%d" % (3 * sum(levels), cap))
    assert N == 3 * sum(levels) + 2 * (levels[0] + 1) + 3 * (sum(levels) - 1)


def test_two_calls_give_the_same_bits(dev):
    case = Case(dev, 65, [65, 64, 1], seed=70)
    o1, n1, d1 = case.run(0.5)
    o2, n2, d2 = case.run(0.5)
    assert n1 == n2 > 0 and torch.equal(_bits(o1), _bits(o2)) and torch.equal(_bits(d1), _bits(d2))
    big = Case(dev, 3, [3, 3, 3], levels=(1024, 512), valid=[[1024, 512]] * 3, seed=71)
    o1, n1, d1 = big.run()
    o2, n2, d2 = big.run()
    assert n1 == n2 == 9 * 1536 and torch.equal(_bits(o1), _bits(o2)) and torch.equal(_bits(d1), _bits(d2))


def test_large_differences_stay_finite(dev):
    case = Case(dev, 22, [22, 11, 1], seed=80)
    case.x += 1e4
    torch.cuda.synchronize()
    out, N, dl = check(case, label="|x - z| ~ 1e4")
    assert float(out[0]) > 1e6 and bool(torch.isfinite(dl).all())


def test_op_and_autograd(dev):
    """ops.der_replay: the same numbers as the entry points, a dense gradient that is zero outside the compared elements and
    scaled by the upstream gradient; argument checks"""
    from vilco_amd import ops
    case = Case(dev, 22, [11, None, 22], seed=90)
    out, N, dl = case.run(2.0)
    x = case.x.clone().requires_grad_(True)
    loss, count = ops.der_replay(x, case.level_row, case.levels, case.level_len, case.tab, ALPHA, return_count=True)
    (2.0 * loss).backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and torch.equal(_bits(loss.reshape(1)), _bits(out)) and int(count) == N > 0
    mask = case.want()[3].to(dev)
    assert torch.equal(_bits(x.grad[mask]), _bits(dl[mask])) and bool((x.grad[~mask] == 0).all())
    plain = ops.der_replay(case.x, case.level_row, case.levels, case.level_len, case.tab, ALPHA)
    assert torch.equal(_bits(plain.reshape(1)), _bits(out))
    with pytest.raises(ValueError):
        ops.der_replay(case.x, case.level_row, case.levels, case.level_len[:, :3].contiguous(), case.tab, ALPHA)
    with pytest.raises(ValueError):
        ops.der_replay(case.x, case.level_row, case.levels, case.level_len, case.tab.int(), ALPHA)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.der_replay(case.x.cpu(), case.level_row, case.levels, case.level_len, case.tab, ALPHA)


def test_against_the_tensor_op_body(dev):
    """the A/B reference a CPU model runs (cl_methods.der.der_term), on the device in fp32: same loss to the op test's bound
    plus the fp32 sum's own roundings (N additions)"""
    from vilco_amd import ops
    from vilco_amd.cl_methods import der
    case = Case(dev, 22, [11, 22, 21], seed=95)
    x = case.x.clone().requires_grad_(True)
    body, N = der.der_term(x, case.level_row, case.levels, case.valid, case.records, ALPHA)
    body.backward()
    loss, count = ops.der_replay(case.x, case.level_row, case.levels, case.level_len, case.tab, ALPHA, return_count=True)
    w_loss, w_N, w_grad, mask, _ = case.want()
    assert N == w_N == int(count)
    assert abs(float(loss) - w_loss) <= (gamma(4) + U) * w_loss
    assert abs(float(body) - w_loss) <= gamma(N + 4) * w_loss
    assert torch.allclose(x.grad.double().cpu(), w_grad, rtol=gamma(4), atol=2.0 ** -149)
