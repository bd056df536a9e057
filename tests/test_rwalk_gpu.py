"""RWalk on the device: the Fisher moving average, the path integral and the checkpointed path scores taken inside the
multi-tensor AdamW / SGD update (vilco_optim_step_rwalk), the three consolidation launches (vilco_rwalk_consolidate) and the
Python layer (FusedOptimizer.attach_rwalk, regularizers.rwalk_begin_task / on_task_rwalk_update) -- against the float64
restatement tests/rwalk_restatement.py.

Kernel tests call the C entry points with hand-built chunk tables over tensors whose element counts sit at the wave and chunk
edges.  Every tensor is a view into a buffer of its own that starts 1 to 4 elements in and ends in a canary word.

Bounds are counted roundings, u = 2^-24, gamma(n) = n u / (1 - n u), never measurements.  One update, started from the fp32 state
the kernel itself left and the fp32 values p0 -> pv the parameter held (gc = g c in float64, gr = fl(g c) the kernel's):
  F' = fl(F + fl(alpha fl(fl(gr gr) - F))):  gr gr = gc^2 (1 + theta_3) (one rounding in gr counted twice, one in the product);
    fl(.. - F) and fl(alpha ..) add two more, so s = alpha [gc^2 (1 + theta_5) - F (1 + theta_2)], |s - alpha (gc^2 - F)| <=
    alpha (gamma(5) gc^2 + gamma(2) |F|) =: e_s; the last add rounds once: |err F'| <= e_s + u (|F'| + e_s)  =: bF.
  w' = fma(-gr, fl(pv - p0), w):  SI's bound (tests/test_si_gpu.py): gamma(3) |gc (pv - p0)| + gamma(2) |w'|  =: bw.
  checkpoint: the kernel forms q = max(w^, 0) / (0.5 F^ d^2 + eps) in double from ITS fp32 w^ in [w' - bw, w' + bw] and F^ in
    [F' - bF, F' + bF] (F^ >= 0: every step of its expression is monotone and alpha <= 1) and d = pv - theta_ck, exact in
    double; q is monotone in both, so q^ lies in [q_lo, q_hi] taken at the interval ends; s' = fl32(s + q^) rounds once, the
    five double operations before it at 2^-53 each (allowed for as 16 * 2^-53):
    |err s'| <= max(q_hi - q, q - q_lo) + (u + 2^-49) (s + q_hi).
Consolidation: s_fl = fl32(s + q), q in double from fp32 inputs: |err| <= (u + 2^-49) |s_fl|.  maxS^ = max of the rounded values:
  relative u off the exact max; s^ / maxS^ = (s / maxS)(1 + theta_2)/(1 - u) <= (1 + gamma(3)); F / maxF has exact operands; the
  sum is formed in double and rounded once: |err importance| <= (u + 2^-49) |importance| + gamma(3) s / maxS."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import optim_restatement as R
import rwalk_restatement as W

U = 2.0 ** -24
DBL = 2.0 ** -49
CHUNK = R.CHUNK
pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
NO_STATE = (2, 6)               # these tensors' address entries are 0; their neighbours have states
LRS, WDS = [1e-2, 2.5e-2], [0.05, 0.0]
BETA1, BETA2, EPS, MOM = 0.9, 0.999, 1e-8, 0.9
ALPHA, RW_EPS = 0.9, 1e-8
CLIP = 0.37
CANARY = 1234.5
ITERS = 7


def gamma(n):
    return n * U / (1 - n * U)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np(x):
    return x.detach().double().cpu().numpy()


class Slot:
    """`n` elements inside a buffer of their own: 1..4 canary words in front, one behind"""

    def __init__(self, values, rot, dev):
        self.n, self.start = values.numel(), 1 + rot % 4
        host = torch.full((self.start + self.n + 1,), CANARY)
        host[self.start:self.start + self.n] = values.float()
        self.buf = host.to(dev)
        self.view = self.buf[self.start:self.start + self.n]
        self.first = self.buf.clone()

    def reset(self):
        self.buf.copy_(self.first)

    def canaries_intact(self):
        s, e = self.start, self.start + self.n
        return bool((self.buf[:s] == CANARY).all()) and bool((self.buf[e:] == CANARY).all())


def _slots(dev, seed, rot, scale=1.0, fn=None, sizes=SIZES):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        x = torch.randn(n, generator=g) * scale
        out.append(Slot(fn(x) if fn else x, i + rot, dev))
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from vilco_amd import _lib as L
    return L, L.load()


def test_the_chunk_is_the_library_s():
    from vilco_amd import ops
    assert ops.ChunkPlan([1], torch.device('cpu')).chunk == CHUNK


# ------------------------------------------------------------------------------------------------- the update kernels
class StepCase:
    def __init__(self, dev, kind, seed):
        self.dev, self.kind, n = dev, kind, len(SIZES)
        self.p = _slots(dev, seed, 0, 1e-2)
        self.g = _slots(dev, seed + 1, 1)
        self.m = _slots(dev, seed + 2, 2, 0.1)
        self.v = _slots(dev, seed + 3, 3, 0.01, fn=torch.abs)
        self.om = _slots(dev, seed + 4, 2, 1e-4)                       # an interval already under way, both signs
        self.fi = _slots(dev, seed + 5, 3, 0.3, fn=torch.abs)
        self.sc = _slots(dev, seed + 6, 0, 2.0, fn=torch.abs)
        self.ck = _slots(dev, seed + 7, 1, 1e-2)
        self.group = [i % 2 for i in range(n)]
        self.table = R.Table(dev, [[s.view.data_ptr() for s in r] for r in (self.p, self.g, self.m, self.v)], SIZES)
        self.tstep = torch.zeros(n, dtype=torch.float32, device=dev)
        self.tgroup = torch.tensor(self.group, dtype=torch.int32).to(dev)
        self.amax = torch.zeros(self.table.nchunks, device=dev)
        self.coef = torch.tensor([7.0, CLIP]).to(dev)
        self.tick = torch.zeros(1, dtype=torch.int32, device=dev)

        def addr(slots):
            return [0 if i in NO_STATE else s.view.data_ptr() for i, s in enumerate(slots)]
        self.si = torch.tensor(addr(self.om), dtype=torch.int64).to(dev)
        self.rw = torch.tensor([addr(self.fi), addr(self.sc), addr(self.ck)], dtype=torch.int64).to(dev)
        self.states = (self.om, self.fi, self.sc, self.ck)

    def reset(self):
        for rows in (self.p, self.m, self.v) + self.states:
            for s in rows:
                s.reset()

    def set_grads(self, call):
        for i, s in enumerate(self.g):
            s.view.copy_(torch.randn(s.n, generator=torch.Generator().manual_seed(7000 + 100 * call + i)).to(self.dev))

    def run(self, step, tick=None, delta_t=None):
        L, lib = _lib()
        lr, wd = (C.c_float * 2)(*LRS), (C.c_float * 2)(*WDS)
        self.tstep.fill_(float(step))
        d = L.OptimDesc(table=self.table.struct(), kind=0 if self.kind == "AdamW" else 1, group=self.tgroup.data_ptr(),
                        lr=C.addressof(lr), wd=C.addressof(wd), ngroups=2, beta1=BETA1, beta2=BETA2, eps=EPS, momentum=MOM,
                        tensor_step=self.tstep.data_ptr(), norm_coef=self.coef.data_ptr(), chunk_amax=self.amax.data_ptr(),
                        lr_dev=None, si_ptrs=self.si.data_ptr())
        try:
            if tick is None:
                L.check(lib.vilco_optim_step(C.byref(d), _stream()))
            else:
                self.tick.fill_(tick)
                rd = L.RwalkStepDesc(optim=d, rw_ptrs=self.rw.data_ptr(), tick=self.tick.data_ptr(), alpha=ALPHA, eps=RW_EPS,
                                     delta_t=delta_t)
                L.check(lib.vilco_optim_step_rwalk(C.byref(rd), _stream()))
        finally:
            torch.cuda.synchronize()


def _check_update(case, i, before, checkpoint, c, tag):
    """tensor i after one call against the restatement started from `before` = (p0, w, F, s, ck) clones"""
    p0, w0, F0, s0, ck0 = before[i]
    pv = case.p[i].view
    gc = _np(case.g[i].view) * c
    F1, s1, w1, ck1, parts = W.update(_np(F0), _np(s0), _np(w0), _np(ck0), gc, _np(p0), _np(pv), ALPHA, RW_EPS, checkpoint)
    a = W.f32(ALPHA)
    e_s = a * (gamma(5) * parts['g2'] + gamma(2) * np.abs(_np(F0)))
    bF = e_s + U * (np.abs(F1) + e_s)
    errF = np.abs(_np(case.fi[i].view) - F1)
    assert np.all(errF <= bF), (tag, "F", float((errF / np.maximum(bF, 1e-300)).max()))
    assert float(_np(case.fi[i].view).min()) >= 0.0
    wc = parts['w_closed']
    bw = gamma(3) * parts['term'] + gamma(2) * np.abs(wc)
    worst = float((errF / np.maximum(bF, 1e-300)).max())
    if not checkpoint:
        errw = np.abs(_np(case.om[i].view) - w1)
        assert np.all(errw <= bw), (tag, "w", float((errw / np.maximum(bw, 1e-300)).max()))
        assert _same_bits(case.sc[i].buf, s0.base_buf) and _same_bits(case.ck[i].buf, ck0.base_buf), (tag, "score / theta_ck touched")
        return worst
    d2 = (_np(pv) - _np(ck0)) ** 2
    eps = W.f32(RW_EPS)
    q = parts['quot']
    q_hi = np.maximum(wc + bw, 0.0) / (0.5 * np.maximum(F1 - bF, 0.0) * d2 + eps)
    q_lo = np.maximum(wc - bw, 0.0) / (0.5 * (F1 + bF) * d2 + eps)
    bs = np.maximum(q_hi - q, q - q_lo) + (U + DBL) * (_np(s0) + q_hi)
    errs = np.abs(_np(case.sc[i].view) - s1)
    assert np.all(errs <= bs), (tag, "s", float((errs / np.maximum(bs, 1e-300)).max()))
    assert bool((_bits(case.om[i].view) == 0).all()), (tag, "w not reset")
    assert _same_bits(case.ck[i].view, pv), (tag, "theta_ck is not the new parameter")
    assert float(_np(case.sc[i].view).min()) >= 0.0 and np.all(_np(case.sc[i].view) >= _np(s0))
    return max(worst, float((errs / np.maximum(bs, 1e-300)).max()))


def _clone_with_buf(slot):
    t = slot.view.clone()
    t.base_buf = slot.buf.clone()
    return t


def _walk(case, schedule, delta_t, reference, check):
    """the calls of `schedule` = [(optimizer step count, tick)] through vilco_optim_step_rwalk from the case's first state.
    reference[k] = (p, m, v rows, amax, omega rows) after call k of the same schedule through vilco_optim_step with si_ptrs."""
    case.reset()
    c = float(case.coef[1])
    first_ckpt = min([k for k, (_, tick) in enumerate(schedule) if tick % delta_t == 0] or [len(schedule)])
    seen = {True: 0, False: 0}
    worst = 0.0
    for k, (step, tick) in enumerate(schedule):
        case.set_grads(k)
        checkpoint = tick % delta_t == 0
        seen[checkpoint] += 1
        before = [tuple(_clone_with_buf(r[i]) for r in (case.p, case.om, case.fi, case.sc, case.ck)) for i in range(len(SIZES))]
        case.run(step, tick=tick, delta_t=delta_t)
        if not check:
            continue
        rows, amax, omegas = reference[k]
        for mine, theirs in zip((case.p, case.m, case.v), rows):
            for i, (s, t) in enumerate(zip(mine, theirs)):
                assert _same_bits(s.view, t), "call %d: the update of tensor %d (numel %d) is not vilco_optim_step's" % (k, i, s.n)
        assert _same_bits(case.amax, amax), "call %d: chunk_amax" % k
        for i in range(len(SIZES)):
            if i in NO_STATE:
                continue
            if k < first_ckpt:
                assert _same_bits(case.om[i].view, omegas[i]), "call %d: omega of tensor %d is not SI's" % (k, i)
            worst = max(worst, _check_update(case, i, before, checkpoint, c, (case.kind, delta_t, k, SIZES[i])))
        for i in NO_STATE:
            assert all(_same_bits(r[i].buf, r[i].first) for r in case.states), "call %d: a state of address-0 tensor %d was touched" % (k, i)
    if check:
        assert all(s.canaries_intact() for rows in (case.p, case.m, case.v) + case.states for s in rows)
        print("%s delta_t %d: max err / bound = %.3f over %d checkpoint and %d plain calls" % (case.kind, delta_t, worst, seen[True], seen[False]))
    return seen, [[s.buf.clone() for s in rows] for rows in (case.p, case.m, case.v) + case.states]


def _si_reference(case, schedule):
    case.reset()
    out = []
    for k, (step, _) in enumerate(schedule):
        case.set_grads(k)
        case.run(step)
        out.append(([[s.view.clone() for s in rows] for rows in (case.p, case.m, case.v)], case.amax.clone(),
                    [s.view.clone() for s in case.om]))
    untouched = all(_same_bits(s.buf, s.first) for rows in (case.fi, case.sc, case.ck) for s in rows)
    assert untouched, "vilco_optim_step knows nothing of fisher, score and theta_ck"
    return out


@pytest.mark.parametrize("delta_t", [1, 3])
@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_step_kernels_keep_the_rwalk_states(dev, kind, delta_t):
    """seven iterations, clip coefficient 0.37, two (lr, wd) groups, tensors 2 and 6 without states.  delta_t = 3: checkpoints at
    iterations 3 and 6, plain updates between, an interval left open after 7; delta_t = 1: every update is a checkpoint.
    Assertions 1-5 of the module's list: the update's bits, each update against the restatement, score / theta_ck untouched by
    plain updates, address-0 tensors untouched, and a second run with identical bits."""
    case = StepCase(dev, kind, 300)
    schedule = [(it, it) for it in range(1, ITERS + 1)]
    reference = _si_reference(case, schedule)
    seen, final = _walk(case, schedule, delta_t, reference, check=True)
    assert seen == ({True: 7, False: 0} if delta_t == 1 else {True: 2, False: 5})
    if delta_t == 3:
        assert any(float(case.om[i].view.abs().max()) > 0 for i in range(len(SIZES)) if i not in NO_STATE), "an open interval"
    _, again = _walk(case, schedule, delta_t, reference, check=False)
    for rows_a, rows_b in zip(final, again):
        assert all(_same_bits(a, b) for a, b in zip(rows_a, rows_b)), "two runs differ"


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_a_tensor_listed_twice_takes_every_update_twice(dev, kind):
    """what FusedOptimizer launches for a parameter listed twice: two calls per iteration with the SAME tick (AdamW: consecutive
    step counts; SGD: pass 0's count for both).  Every call is the restatement's update: F and w advance in both passes, and on a
    checkpoint iteration (tick 2, 4 with delta_t = 2) both passes close an interval -- the second one the one-pass interval."""
    case = StepCase(dev, kind, 400)
    schedule = []
    for it in range(1, 5):
        schedule += [((2 * it - 1) if kind == "AdamW" else it, it), ((2 * it) if kind == "AdamW" else it, it)]
    reference = _si_reference(case, schedule)
    seen, _ = _walk(case, schedule, 2, reference, check=True)
    assert seen == {True: 4, False: 4}


# ------------------------------------------------------------------------------------------------- the consolidation
def _consolidate(dev, rows, outs, numels, eps=RW_EPS):
    L, lib = _lib()
    tb = R.Table(dev, [[s.view.data_ptr() for s in r] for r in rows], numels)
    out_ptrs = torch.tensor([[s.view.data_ptr() for s in r] for r in outs], dtype=torch.int64).to(dev)
    partial = torch.full((2 * tb.nchunks + 1,), CANARY, device=dev)
    out = torch.full((3,), CANARY, device=dev)
    d = L.RwalkDesc(table=tb.struct(), out_ptrs=out_ptrs.data_ptr(), partial=partial.data_ptr(), out=out.data_ptr(), eps=eps)
    try:
        L.check(lib.vilco_rwalk_consolidate(C.byref(d), _stream()))
    finally:
        torch.cuda.synchronize()
    assert float(partial[-1]) == CANARY and float(out[2]) == CANARY
    return out[:2].clone(), partial[:-1].clone(), tb


def _consolidation_case(dev, seed):
    p = _slots(dev, seed, 0, 1e-2)
    fi = _slots(dev, seed + 1, 1, 0.3, fn=torch.abs)
    sc = _slots(dev, seed + 2, 2, 2.0, fn=torch.abs)
    om = _slots(dev, seed + 3, 3, 1e-4)
    ck = _slots(dev, seed + 4, 0, 1e-2)
    imp = _slots(dev, seed + 5, 1, 1.0, fn=lambda x: x * float('nan'))        # written, never read
    opt = _slots(dev, seed + 6, 2, 1.0, fn=lambda x: x * float('nan'))
    with torch.no_grad():
        for i in range(len(SIZES)):
            ck[i].view[::2] = p[i].view[::2]                                  # d = 0: the denominator is eps alone
    return p, fi, sc, om, ck, imp, opt


def _check_consolidation(rows, outs, before, maxes, tag):
    p, fi, sc, om, ck = rows
    imp, opt = outs
    p0, F0, s0, w0, ck0 = before
    want = W.consolidate(p0, F0, s0, w0, ck0, RW_EPS)
    worst = 0.0
    for i, n in enumerate(SIZES):
        got = _np(imp[i].view)
        bound = (U + DBL) * np.abs(want['importance'][i]) + gamma(3) * want['term_s'][i]
        err = np.abs(got - want['importance'][i])
        assert np.all(np.isfinite(got)) and got.min() >= 0 and got.max() <= 2 * (1 + 4 * U), (tag, n)
        assert np.all(err <= bound), (tag, n, "importance", float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        fl = want['s_flushed'][i]
        err = np.abs(2.0 * _np(sc[i].view) - fl)                               # the halving is exact
        assert np.all(err <= (U + DBL) * np.abs(fl)), (tag, n, "s")
        assert _same_bits(opt[i].view, p0[i]) and _same_bits(ck[i].view, p0[i]) and _same_bits(p[i].view, p0[i]), (tag, n)
        assert bool((_bits(om[i].view) == 0).all()) and _same_bits(fi[i].view, F0[i]), (tag, n)
    assert abs(float(maxes[0]) - want['maxF']) == 0.0, (tag, "max F is a maximum of fp32 values: exact")
    assert abs(float(maxes[1]) - want['maxS']) <= (U + DBL) * want['maxS'], (tag, "max s")
    assert all(s.canaries_intact() for r in rows + outs for s in r)
    print("%s: importance max err / bound = %.3f, maxF %.6g maxS %.6g" % (tag, worst, float(maxes[0]), float(maxes[1])))
    return want


def test_consolidation_kernels_with_the_maxima_at_the_far_ends(dev):
    """max F in the last element of the last chunk of the last tensor, max s in element 0 of the first tensor (a one-element tensor:
    its block has 255 idle threads); omega of both signs, every other element with d = 0."""
    p, fi, sc, om, ck, imp, opt = _consolidation_case(dev, 500)
    with torch.no_grad():
        fi[-1].view[-1] = 77.0
        sc[0].view[0] = 1e6
    before = [[s.view.clone() for s in r] for r in (p, fi, sc, om, ck)]
    assert any(bool((w < 0).any()) for w in before[3]) and any(bool((w > 0).any()) for w in before[3])
    maxes, partial, tb = _consolidate(dev, (p, fi, sc, om, ck), (imp, opt), SIZES)
    want = _check_consolidation((p, fi, sc, om, ck), (imp, opt), before, maxes, "far ends")
    assert want['maxF'] == 77.0 and float(maxes[0]) == 77.0 and float(partial[tb.nchunks - 1]) == 77.0
    assert float(maxes[1]) >= 1e6 and float(partial[tb.nchunks]) == float(maxes[1])
    assert float(_np(imp[-1].view)[-1]) >= 1.0 and float(_np(imp[0].view)[0]) >= 1.0


def test_consolidation_with_an_all_zero_score(dev):
    """s = 0 everywhere and no positive omega: max s = 0, the score term contributes an exact 0 and the importance is F / maxF"""
    p, fi, sc, om, ck, imp, opt = _consolidation_case(dev, 600)
    with torch.no_grad():
        for i in range(len(SIZES)):
            sc[i].view.zero_()
            om[i].view.copy_(-om[i].view.abs())
    before = [[s.view.clone() for s in r] for r in (p, fi, sc, om, ck)]
    maxes, _, _ = _consolidate(dev, (p, fi, sc, om, ck), (imp, opt), SIZES)
    want = _check_consolidation((p, fi, sc, om, ck), (imp, opt), before, maxes, "zero score")
    assert float(maxes[1]) == 0.0 and want['maxS'] == 0.0
    assert all(bool((_bits(s.view) == 0).all()) for s in sc)
    top = max(float(_np(s.view).max()) for s in imp)
    assert top == 1.0


@pytest.mark.parametrize("where", ["fisher", "score"])
def test_a_nan_reaches_the_maximum_and_every_importance(dev, where):
    """one NaN in F (or s) in the middle of the second chunk of the last tensor: fmaxf would drop it and the importance would look
    healthy; the reduction hands it on, so out and every importance are NaN"""
    p, fi, sc, om, ck, imp, opt = _consolidation_case(dev, 700)
    with torch.no_grad():
        (fi if where == "fisher" else sc)[-1].view[CHUNK + 1000] = float('nan')
    maxes, _, _ = _consolidate(dev, (p, fi, sc, om, ck), (imp, opt), SIZES)
    # (a NaN F also poisons the score it divides: both maxima; a NaN s leaves max F alone)
    assert bool(torch.isnan(maxes[1])) and bool(torch.isnan(maxes[0])) == (where == "fisher")
    assert all(bool(torch.isnan(s.view).all()) for s in imp)
    assert all(bool(torch.isfinite(s.view).all()) for s in opt)


# ------------------------------------------------------------------------------------------------- the Python layer
class _Net(torch.nn.Module):
    """parameters at the chunk edges; `head` is the class head (rows = classes); 'scale' is not regularised"""

    def __init__(self, dev, rows=4, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)

        def mk(*shape):
            return torch.nn.Parameter((0.05 * torch.randn(*shape, generator=g)).to(dev))
        self.a, self.b, self.c = mk(CHUNK + 1), mk(65), mk(3)
        self.big = mk(2 * CHUNK + 3)
        self.head = mk(rows, 65)
        self.frozen = mk(40)
        self.frozen.requires_grad = False
        self.scale = mk(1)
        self.reg_params = {}


def _set_grads(net, it):
    for i, (name, p) in enumerate(net.named_parameters()):
        if p.requires_grad:
            p.grad = torch.randn(p.shape, generator=torch.Generator().manual_seed(1000 * it + i)).to(p.device)


def test_two_tasks_through_the_python_layer_with_a_grown_head(dev):
    """FusedOptimizer over a small net (`b` listed twice), two tasks with delta_t = 2: three clipped steps (a checkpoint at
    iteration 2, an open interval after 3), on_task_rwalk_update against the restatement; the head grows by two rows, a new
    optimizer, rwalk_begin_task carries F and the halved s on their prefix and zeroes the new rows; the same again."""
    from vilco_amd.cl_methods import regularizers
    from vilco_amd.utils.train_utils import FusedOptimizer
    net = _Net(dev)
    tracked = ['a', 'b', 'c', 'big', 'head']
    keys = ('fisher', 'score', 'omega', 'theta_ck')
    carried = None
    for task in range(2):
        if task == 1:
            with torch.no_grad():
                grown = torch.cat([net.head.detach(), 0.05 * torch.randn(2, 65, device=dev)])
            net.head = torch.nn.Parameter(grown)
        params = dict(net.named_parameters())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            opt = FusedOptimizer([{"params": [params['a'], params['b'], params['head'], params['b']], "weight_decay": 0.05},
                                  {"params": [params['c'], params['big'], params['scale']], "weight_decay": 0.0}], lr=1e-2)
        sd_keys = sorted(opt.state_dict())
        state = regularizers.rwalk_begin_task(net, opt, alpha=ALPHA, delta_t=2, eps=RW_EPS)
        assert sorted(state) == sorted(tracked) and sorted(opt.state_dict()) == sd_keys and int(opt.rwalk_tick) == 0
        for n in tracked:
            assert float(state[n]['omega'].abs().max()) == 0.0 and _same_bits(state[n]['theta_ck'], params[n])
            assert all(state[n][k].shape == params[n].shape for k in keys)
            if carried is None:
                assert float(state[n]['fisher'].abs().max()) == 0.0 and float(state[n]['score'].abs().max()) == 0.0
            else:
                old_f, old_s = carried[n]
                k = old_f.numel()
                assert _same_bits(state[n]['fisher'].view(-1)[:k], old_f.view(-1)) and _same_bits(state[n]['score'].view(-1)[:k], old_s.view(-1))
                assert float(state[n]['fisher'].view(-1)[k:].abs().sum()) == 0.0 and float(state[n]['score'].view(-1)[k:].abs().sum()) == 0.0
        if carried is not None:
            assert state['head']['fisher'].shape[0] == 6 and carried['head'][0].shape[0] == 4
        for it in range(3):
            _set_grads(net, 10 * task + it)
            s_before = {n: state[n]['score'].clone() for n in tracked}
            opt.step(clip_grad_l2norm=1.0)
            torch.cuda.synchronize()
            assert int(opt.rwalk_tick) == it + 1, "one tick per iteration, whatever the number of passes"
            assert float(opt.last_grad_norm[1]) < 1.0
            moved = [not torch.equal(state[n]['score'], s_before[n]) for n in tracked]
            assert all(moved) if it == 1 else not any(moved), (task, it, moved)
        assert all(float(state[n]['omega'].abs().max()) > 0 and float(state[n]['fisher'].min()) >= 0 for n in tracked)
        if task == 1:
            pen = regularizers.apply_penalty(net, 0.5, kind='rwalk')
            assert pen is not None and float(pen) > 0
        order = [n for n, _ in net.named_parameters() if n in tracked]
        snap = [[t.detach().clone() for t in col] for col in
                zip(*[(params[n], state[n]['fisher'], state[n]['score'], state[n]['omega'], state[n]['theta_ck']) for n in order])]
        reg, maxes = regularizers.on_task_rwalk_update(net, opt, eps=RW_EPS, return_max=True)
        torch.cuda.synchronize()
        assert sorted(reg) == ['importance', 'optpar'] and len(reg['importance']) == len(reg['optpar']) == 1
        assert sorted(reg['importance'][0]) == sorted(tracked) == sorted(reg['optpar'][0])
        want = W.consolidate(*snap, RW_EPS)
        assert float(maxes[0]) == want['maxF'] and abs(float(maxes[1]) - want['maxS']) <= (U + DBL) * want['maxS'] and want['maxS'] > 0
        for i, n in enumerate(order):
            got = _np(reg['importance'][0][n])
            assert got.shape == tuple(params[n].shape) and got.min() >= 0 and got.max() <= 2 * (1 + 4 * U)
            bound = (U + DBL) * np.abs(want['importance'][i]) + gamma(3) * want['term_s'][i]
            assert np.all(np.abs(got - want['importance'][i]) <= bound), (task, n)
            assert np.all(np.abs(2.0 * _np(state[n]['score']) - want['s_flushed'][i]) <= (U + DBL) * want['s_flushed'][i]), (task, n)
            assert _same_bits(reg['optpar'][0][n], snap[0][i]) and _same_bits(state[n]['theta_ck'], snap[0][i])
            assert float(state[n]['omega'].abs().max()) == 0.0 and _same_bits(state[n]['fisher'], snap[1][i])
        carried = {n: (state[n]['fisher'].clone(), state[n]['score'].clone()) for n in tracked}
    sd = regularizers.rwalk_state_dict(net)
    assert sorted(sd['fisher']) == sorted(tracked) and torch.equal(sd['score']['head'], state['head']['score'].cpu())
    with pytest.raises(RuntimeError):
        opt.attach_si({params['a']: torch.zeros_like(params['a'])})
    opt.attach_rwalk(None)
    _set_grads(net, 99)
    opt.step()
    torch.cuda.synchronize()
    assert all(float(state[n]['omega'].abs().max()) == 0.0 for n in tracked), "detached: the states are no longer advanced"


def test_a_model_without_regularised_parameters_steps_plainly(dev):
    """only a 'scale' parameter is trained: rwalk_begin_task finds nothing to track and leaves NOTHING attached -- the update
    kernel reads the tick word in every block, so an attachment without a device word must not exist -- and the step is the
    plain update, bit for bit."""
    from vilco_amd.cl_methods import regularizers
    from vilco_amd.utils.train_utils import FusedOptimizer

    class OnlyScale(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.scale = torch.nn.Parameter(torch.linspace(0.5, 1.5, 65).to(dev))
            self.reg_params = {}
    got = []
    for with_rwalk in (False, True):
        m = OnlyScale()
        opt = FusedOptimizer([m.scale], lr=1e-2)
        if with_rwalk:
            assert regularizers.rwalk_begin_task(m, opt) == {}
            assert opt._rwalk is None and opt.rwalk_tick is None
        m.scale.grad = torch.randn(65, generator=torch.Generator().manual_seed(5)).to(dev)
        opt.step(clip_grad_l2norm=1.0)
        torch.cuda.synchronize()
        assert all(pl['rw'] is None for pl in opt._plans)
        got.append(m.scale.detach().clone())
        if with_rwalk:
            assert regularizers.on_task_rwalk_update(m, opt) == {'importance': [{}], 'optpar': [{}]}
            assert regularizers.apply_penalty(m, 1.0, kind='rwalk') is None
    assert _same_bits(got[0], got[1])
