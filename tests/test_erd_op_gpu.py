"""Elastic Response Distillation on the device: vilco_erd_select / _select_fill / _fwd / _bwd (csrc/erd.hip) and ops.erd_select /
ops.erd_distill against the float64 restatement tests/erd_restatement.py.

Selection is compared as index sets, exactly; every case asserts first, on the restatement, that each valid response is at least
1e-6 (relative) away from both thresholds, so that the order of the fp64 sums cannot move a position across one.

Values and gradients.  The C entry points are called with every gradient tensor pre-filled with a sentinel, so each case also
checks the footprint: the backward assigns EVERY element.  The tolerance is not a constant: the fp32 tensor-op body
cl_methods.erd.erd_term is evaluated on the same inputs, its distance from the restatement is measured per tensor in max norm
relative to the tensor's largest reference magnitude, and the op may be at most TWICE that far (another summation order, one more
rounding).  The op is never compared with itself; where the reference is exactly zero the op must be exactly zero."""
import ctypes as C

import numpy as np
import pytest
import torch

import erd_restatement as E

pytestmark = pytest.mark.gpu
LEVELS, ROWS, R = (16, 8, 4), (0, 17, 26), 30           # a separator row between the levels (and two unused rows at the end)
VALID = [[16, 8, 4], [11, 6, 3], [5, 3, 2]]
SENTINEL = -777.25
LAM_C, LAM_R = 0.7, 1.3


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def teacher(seed, B=3, Cn=5, levels=LEVELS, peaks=6):
    g = torch.Generator().manual_seed(seed)
    P = sum(levels)
    z = torch.randn(B, P, Cn, generator=g)
    for b in range(B):
        for i in torch.randperm(P, generator=g)[:peaks].tolist():
            z[b, i, 0] += 6.0
    return z, torch.rand(B, P, 2, generator=g) * 3.0


def restated(z, o, levels, valid, n_old, a_c=2.0, a_r=2.0):
    sels = [E.select(z[b].numpy(), o[b].numpy(), levels, valid[b], n_old, a_c, a_r) for b in range(z.shape[0])]
    for s in sels:
        # (sigma == 0: every response IS the threshold; those cases use a dyadic constant, whose sums are exact in any order)
        assert s['sigma'] == 0.0 or E.margin(s) >= 1e-6, "a response within 1e-6 of a threshold: choose other inputs"
    return sels, [E.make_record(z[b].numpy(), o[b].numpy(), s, n_old) for b, s in enumerate(sels)]


def device_select(dev, z, o, levels, valid, n_old, a_c=2.0, a_r=2.0):
    from vilco_amd import ops
    out = ops.erd_select(z.to(dev), o.to(dev), levels, torch.tensor(valid, dtype=torch.int32, device=dev), n_old, a_c, a_r)
    torch.cuda.synchronize()
    return out


def same_selection(got, sels, recs):
    for (mc, mr, vc, vr, kc, kr), s, r in zip(got, sels, recs):
        assert [i for i, v in enumerate(mc.tolist()) if v >= 0] == s['S_cls'] and kc == len(s['S_cls'])
        assert [i for i, v in enumerate(mr.tolist()) if v >= 0] == s['S_reg'] and kr == len(s['S_reg'])
        assert np.array_equal(mc.cpu().numpy(), r['map_cls']) and np.array_equal(mr.cpu().numpy(), r['map_reg'])
        assert np.array_equal(vc[:kc].cpu().numpy(), r['val_cls']) and np.array_equal(vr[:kr].cpu().numpy(), r['val_reg'])


class Case:
    """student x [B, R, C], o [B, R, 2] (raw with `scale`), records = the restatement's (or None per row), uploaded as they are"""

    def __init__(self, dev, x, o, scale, recs, levels=LEVELS, rows=ROWS, valid=VALID):
        from vilco_amd.cl_methods import erd
        self.dev, self.x, self.o, self.scale, self.recs = dev, x, o, scale, recs
        self.levels, self.rows, self.valid = tuple(levels), tuple(rows), valid
        self.host, self.keep, tab = [], [], []
        for r in recs:
            if r is None:
                self.host.append(None)
                tab.append([0] * 5)
                continue
            kc, kr = r['val_cls'].shape[0], r['val_reg'].shape[0]
            vc, vr = torch.zeros(max(kc, 1), r['n_old']), torch.zeros(max(kr, 1), 2)
            vc[:kc], vr[:kr] = torch.from_numpy(r['val_cls']), torch.from_numpy(r['val_reg'])
            h = erd.Record(torch.from_numpy(r['map_cls']), torch.from_numpy(r['map_reg']), vc, vr, kc, kr, r['n_old'], 0, self.levels)
            self.host.append(h)
            bufs = [t.to(dev) for t in h.buffers()]
            self.keep.append(bufs)
            tab.append([t.data_ptr() for t in bufs] + [r['n_old']])
        self.tab = torch.tensor(tab, dtype=torch.int64, device=dev)
        self.level_len = torch.tensor(valid, dtype=torch.int32, device=dev)
        self.xd, self.od = x.to(dev), o.to(dev)
        self.sd = None if scale is None else scale.to(dev)

    def reference(self, g=1.0):
        return E.term(self.x.numpy(), self.o.numpy(), None if self.scale is None else self.scale.numpy(), self.rows, self.levels,
                      self.valid, self.recs, LAM_C, LAM_R, g_out=g)

    def body(self, g=1.0):
        """cl_methods.erd.erd_term in fp32 -> the same dictionary"""
        from vilco_amd.cl_methods import erd
        x, o = self.x.clone().requires_grad_(True), self.o.clone().requires_grad_(True)
        s = None if self.scale is None else self.scale.clone().requires_grad_(True)
        loss, cls, reg, nc, nr = erd.erd_term(x, o, s, self.rows, self.levels, self.valid, self.host, LAM_C, LAM_R)
        (loss * g).backward()
        return dict(loss=loss.detach(), cls=cls.detach(), reg=reg.detach(), N_c=nc, N_r=nr, d_logits=x.grad, d_offsets=o.grad,
                    d_scale=None if s is None else s.grad)

    def run(self, g=1.0):
        """the C entry points -> the same dictionary; gradients pre-filled with the sentinel, the workspace with 0xA5"""
        from vilco_amd import _lib, ops
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        tab = ops._distill_levels(self.rows, self.levels, self.dev)
        d = _lib.ErdDesc()
        d.logits, d.offsets, d.scale = self.xd.data_ptr(), self.od.data_ptr(), (None if self.sd is None else self.sd.data_ptr())
        d.level_row, d.level_T, d.level_dev = C.addressof(tab[0]), C.addressof(tab[1]), tab[2].data_ptr()
        d.level_len, d.erd_tab = self.level_len.data_ptr(), self.tab.data_ptr()
        d.B, d.R, d.C, d.L = self.x.shape[0], self.x.shape[1], self.x.shape[2], len(self.levels)
        d.lambda_cls, d.lambda_reg = LAM_C, LAM_R
        nws = lib.vilco_erd_workspace(d.B * sum(self.levels))
        ws = torch.full((nws,), 0xA5, dtype=torch.uint8, device=self.dev)
        out = torch.full((3,), float('nan'), device=self.dev)
        gd = torch.full((1,), float(g), device=self.dev)
        dl, do = torch.full_like(self.xd, SENTINEL), torch.full_like(self.od, SENTINEL)
        ds = None if self.sd is None else torch.full_like(self.sd, SENTINEL)
        try:
            _lib.check(lib.vilco_erd_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws, st))
            _lib.check(lib.vilco_erd_bwd(C.byref(d), gd.data_ptr(), dl.data_ptr(), do.data_ptr(),
                                         None if ds is None else ds.data_ptr(), ws.data_ptr(), nws, st))
        finally:
            torch.cuda.synchronize()
        off = (-ws.data_ptr()) % 256
        n = ws[off:off + 16].view(torch.int64).tolist()
        return dict(loss=out[0], cls=out[1], reg=out[2], N_c=n[0], N_r=n[1], d_logits=dl, d_offsets=do, d_scale=ds)


def dist(got, ref):
    """max |got - ref| relative to the tensor's largest reference magnitude (absolute where the reference is all zero)"""
    got = torch.as_tensor(got, dtype=None if torch.is_tensor(got) else torch.float64).detach().double().cpu().reshape(-1)
    ref = torch.as_tensor(ref, dtype=None if torch.is_tensor(ref) else torch.float64).detach().double().cpu().reshape(-1)
    top = float(ref.abs().max())
    return float((got - ref).abs().max()) / (top if top > 0 else 1.0)


def check(case, g=1.0, label=""):
    """op within twice the fp32 body's distance from the restatement, tensor by tensor; counts equal; nothing left unassigned"""
    ref, body, op = case.reference(g), case.body(g), case.run(g)
    assert (op['N_c'], op['N_r']) == (ref['N_c'], ref['N_r']) == (body['N_c'], body['N_r'])
    figures = {}
    for k in ('loss', 'cls', 'reg', 'd_logits', 'd_offsets', 'd_scale'):
        if ref[k] is None:
            assert op[k] is None
            continue
        assert not bool((op[k] == SENTINEL).any()) and bool(torch.isfinite(op[k]).all()), k
        figures[k] = (dist(op[k], ref[k]), dist(body[k], ref[k]))
    print(label, "N_c %d N_r %d" % (ref['N_c'], ref['N_r']),
          "  ".join("%s op %.3g body %.3g" % (k, a, b) for k, (a, b) in figures.items()))
    for k, (a, b) in figures.items():
        assert a <= 2.0 * b, (label, k, a, b)
    return ref, op


def student(seed, B=3, Cn=5, rows=R, raw=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, rows, Cn, generator=g)
    return x, (torch.randn(B, rows, 2, generator=g) if raw else torch.rand(B, rows, 2, generator=g) * 3.0)


# ------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("seed,a_r", [(0, 2.0), (1, 1.0), (2, 2.5)])
def test_selection_is_the_restatements(dev, seed, a_r):
    """case 1: the two index sets, the maps and the gathered rows, exactly"""
    z, o = teacher(seed)
    sels, recs = restated(z, o, LEVELS, VALID, 3, 2.0, a_r)
    assert sum(len(s['S_cls']) for s in sels) > 0
    same_selection(device_select(dev, z, o, LEVELS, VALID, 3, 2.0, a_r), sels, recs)


def test_selection_edges(dev):
    """cases 2, 3, 4, 6: constant responses select nothing; the largest response at the first padded position is not selected;
    the last valid position is, and the sets cross a level boundary; a teacher row with offsets (0, 0) is in S_cls only"""
    z, o = teacher(3, peaks=0)
    z[0, :, :3] = 0.25                                          # sigma = 0, strict comparison
    z[1, 11, 1] = 60.0                                          # level 0 of clip 1 is valid below 11
    for i in (10, 16, 26):                                      # last valid of level 0, first of level 1, last of level 2
        z[1, i, 2] += 8.0
    z[2, 25, 0] += 9.0                                          # the last valid position of clip 2
    o[1, 16] = 0.0
    sels, recs = restated(z, o, LEVELS, VALID, 3)
    assert sels[0]['S_cls'] == [] and sels[0]['S_reg'] == [] and sels[0]['sigma'] == 0.0
    assert 11 not in sels[1]['S_cls'] and sels[1]['S_cls'] == [10, 16, 26]
    assert sels[1]['S_reg'] == [10, 26], "a teacher that predicts no extent is not regressed to"
    assert sels[2]['S_cls'] == [25]
    assert 26 == 16 + 8 + VALID[1][2] - 1, "the last valid position of the last level"
    got = device_select(dev, z, o, LEVELS, VALID, 3)
    same_selection(got, sels, recs)
    assert got[0][4] == got[0][5] == 0 and int(got[0][0].max()) == -1 and int(got[0][1].max()) == -1
    assert int(got[1][0][11]) == -1


@pytest.mark.parametrize("n_old,Cn", [(1, 5), (1, 1), (5, 5)])
def test_selection_with_one_old_class_and_one_class(dev, n_old, Cn):
    """case 5"""
    z, o = teacher(4, Cn=Cn)
    sels, recs = restated(z, o, LEVELS, VALID, n_old)
    assert sum(len(s['S_cls']) for s in sels) > 0
    same_selection(device_select(dev, z, o, LEVELS, VALID, n_old), sels, recs)


# ------------------------------------------------------------------------------------------------- the term
def _case(dev, seed=7, has=(1, 1, 1), raw=False, n_old=3, Cn=5, a_r=2.0):
    z, o_hat = teacher(seed, Cn=Cn)
    _, recs = restated(z, o_hat, LEVELS, VALID, n_old, 2.0, a_r)
    x, o = student(seed + 1, Cn=Cn, raw=raw)
    scale = torch.tensor([1.5, 0.75, 2.0]) if raw else None
    return Case(dev, x, o, scale, [r if h else None for r, h in zip(recs, has)])


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("g", [1.0, -0.375])      # (exact in fp32: the op is handed g as an fp32 scalar)
def test_term_and_gradients(dev, raw, g):
    """cases 8 and 12: n_b = 3 < C = 5 leaves the new classes' gradient columns exactly zero; the raw-offset form with the
    per-level Scale, d raw and d scale, next to the finished-offset form"""
    case = _case(dev, raw=raw, a_r=1.0)
    ref, op = check(case, g, "raw=%s g=%g" % (raw, g))
    assert ref['N_c'] > 0 and ref['N_r'] > 0
    assert float(op['d_logits'][:, :, 3:].abs().max()) == 0.0
    gaps = [r for r in range(R) if not any(r0 <= r < r0 + T for r0, T in zip(ROWS, LEVELS))]
    assert len(gaps) == 2 and float(op['d_logits'][:, gaps].abs().max()) == 0.0 and float(op['d_offsets'][:, gaps].abs().max()) == 0.0
    zero = (ref['d_logits'] == 0).to(op['d_logits'].device)
    assert float(op['d_logits'][zero].abs().max()) == 0.0, "where the restatement has no gradient the op assigns an exact zero"


def test_raw_form_is_the_finished_form(dev):
    """case 12: relu(scale_l raw) handed over finished gives the same losses, and d raw = d o * scale_l where the relu passes"""
    case = _case(dev, raw=True, a_r=1.0)
    raw = case.run()
    scale_rows = torch.zeros(R)
    for l, (r0, T) in enumerate(zip(ROWS, LEVELS)):
        scale_rows[r0:r0 + T] = case.scale[l]
    pre = case.o * scale_rows[None, :, None]
    fin = Case(dev, case.x, torch.relu(pre), None, case.recs).run()
    for k in ('loss', 'cls', 'reg'):
        assert torch.equal(raw[k], fin[k]), k
    assert torch.equal(raw['d_logits'], fin['d_logits'])
    want = fin['d_offsets'].double().cpu() * scale_rows[None, :, None].double() * (pre > 0)
    assert dist(raw['d_offsets'], want) <= 2.0 ** -23
    ds = torch.stack([(fin['d_offsets'].double().cpu() * case.o.double() * (pre > 0))[:, r0:r0 + T].sum() for r0, T in zip(ROWS, LEVELS)])
    assert dist(raw['d_scale'], ds) <= 2.0 ** -22


def test_rows_without_a_record_and_batches_without_any(dev):
    """case 7: a row with address 0 contributes nothing; a batch where no row has a record gives an exact 0 and all-zero gradients"""
    case = _case(dev, has=(1, 0, 1), raw=True)
    ref, op = check(case, 1.0, "row 1 without a record")
    assert float(op['d_logits'][1].abs().max()) == 0.0 and float(op['d_offsets'][1].abs().max()) == 0.0
    none = _case(dev, has=(0, 0, 0), raw=True).run()
    assert (none['N_c'], none['N_r']) == (0, 0)
    for k in ('loss', 'cls', 'reg', 'd_logits', 'd_offsets', 'd_scale'):
        assert float(none[k].abs().max()) == 0.0 and not bool(torch.signbit(none[k]).any()), k


def test_student_equal_to_the_record_and_student_zero(dev):
    """cases 9 and 10: offsets equal to the record sit on every min / max tie -- value and gradient are the restatement's there;
    offsets of 0 after the relu against a positive record stay finite"""
    z, o_hat = teacher(7)
    _, recs = restated(z, o_hat, LEVELS, VALID, 3)
    x, o = student(8)
    pos = torch.cat([r0 + torch.arange(T) for r0, T in zip(ROWS, LEVELS)])
    o[:, pos] = o_hat
    ref, op = check(Case(dev, x, o, None, recs), 1.0, "student == record")
    assert ref['reg'] == 0.0 and float(op['reg']) == 0.0 and ref['N_r'] > 0
    # each side of a tie gets half, and the halves cancel: the gradient there is zero up to the restatement's own fp64 rounding
    assert float(ref['d_offsets'].abs().max()) <= 1e-15 and float(op['d_offsets'].abs().max()) <= 1e-15
    raw = -torch.rand(3, R, 2) - 0.5                            # relu gives 0 everywhere
    ref, op = check(Case(dev, x, raw, torch.tensor([1.5, 0.75, 2.0]), recs), 1.0, "student 0")
    assert bool(torch.isfinite(op['d_offsets']).all()) and float(op['d_offsets'].abs().max()) == 0.0 and float(op['d_scale'].abs().max()) == 0.0
    ref, op = check(Case(dev, x, torch.zeros(3, R, 2), None, recs), 1.0, "student 0, finished")
    assert abs(ref['reg'] - LAM_R * 1.25) <= 0.26 * LAM_R and bool(torch.isfinite(op['d_offsets']).all())


def test_more_rows_than_one_round_of_the_grid(dev):
    """case 11: the waves walk further pairs once B * sum T_l exceeds the capped grid"""
    from vilco_amd import ops
    levels, rows = (1536, 512, 130), (0, 1537, 2050)
    Rr, B = 2181, 2
    assert B * sum(levels) > ops.erd_pairs_per_round()
    valid = [[1536, 512, 130], [1201, 401, 101]]
    z, o_hat = teacher(11, B=B, levels=levels, peaks=40)
    sels, recs = restated(z, o_hat, levels, valid, 3)
    same_selection(device_select(dev, z, o_hat, levels, valid, 3), sels, recs)
    x, o = student(12, B=B, rows=Rr, raw=True)
    case = Case(dev, x, o, torch.tensor([1.5, 0.75, 2.0]), recs, levels=levels, rows=rows, valid=valid)
    ref, _ = check(case, 1.0, "2 x 2178 pairs")
    assert ref['N_c'] >= 3 * 40 and ref['N_r'] > 0


def test_two_calls_give_the_same_bits(dev):
    """case 13"""
    case = _case(dev, raw=True, a_r=1.0)
    a, b = case.run(0.875), case.run(0.875)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
    z, o = teacher(0)
    g1, g2 = device_select(dev, z, o, LEVELS, VALID, 3), device_select(dev, z, o, LEVELS, VALID, 3)
    assert all(torch.equal(p, q) for r1, r2 in zip(g1, g2) for p, q in zip(r1[:4], r2[:4]))


@pytest.mark.parametrize("raw", [False, True])
def test_autograd_function_agrees_with_the_restatement(dev, raw):
    """case 14: ops.erd_distill under autograd, with a downstream factor, against the restatement and within twice the body"""
    from vilco_amd import ops
    case = _case(dev, raw=raw, a_r=1.0)
    g = 1.75
    ref, body = case.reference(g), case.body(g)
    x, o = case.xd.clone().requires_grad_(True), case.od.clone().requires_grad_(True)
    s = None if case.sd is None else case.sd.clone().requires_grad_(True)
    loss, cls, reg, counts = ops.erd_distill(x, o, s, ROWS, LEVELS, case.level_len, case.tab, LAM_C, LAM_R, return_counts=True)
    (loss * g).backward()
    torch.cuda.synchronize()
    assert counts.tolist() == [ref['N_c'], ref['N_r']] and not cls.requires_grad and not reg.requires_grad
    got = dict(loss=loss, cls=cls, reg=reg, d_logits=x.grad, d_offsets=o.grad, d_scale=None if s is None else s.grad)
    for k, v in got.items():
        if v is None:
            continue
        a, b = dist(v, ref[k]), dist(body[k], ref[k])
        print("autograd raw=%s %s op %.3g body %.3g" % (raw, k, a, b))
        assert a <= 2.0 * b, (k, a, b)
    direct = case.run(g)
    for k in ('loss', 'd_logits', 'd_offsets'):
        assert torch.equal(_bits(got[k]), _bits(direct[k])), k
