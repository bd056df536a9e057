"""Synaptic Intelligence on the device: the path integral taken inside the multi-tensor AdamW / SGD update
(vilco_optim_desc.si_ptrs), the consolidation launch (vilco_si_consolidate), the penalty, the Python layer
(FusedOptimizer.attach_si, regularizers.si_begin_task / on_task_si_update), replayed steps and a two-task episode -- against
the float64 restatement tests/si_restatement.py.

Kernel tests call the C entry points with hand-built chunk tables over tensors whose element counts sit at the chunk edges.
Every tensor is a view into a buffer of its own that starts 1 to 4 elements in (no 16-byte alignment, different between the
streams of one tensor) and ends in a canary word.

Bounds are counted roundings, u = 2^-24, never measurements.
  omega, one call:  gr = fl(g c) (u), d = fl(p_new - p_old) on the stored values (u), omega' = fl(omega - gr d) as one fused
    multiply-add (u on the result):  |err| <= gamma(3) |gr d| + gamma(2) |omega'|   per element, with the exact product and sum.
  omega, K calls:  the sum of the K one-call bounds (each call starts from the fp32 value the one before left).
  Omega:  quotient and sum formed in double, one rounding to fp32; the issue's allowance is one rounding for the division and one
    for the add:  |err| <= u |q| + u |Omega|."""
import ctypes as C
import os
import random
import warnings

import pytest
import torch

import si_restatement as S

R = S.R
U = 2.0 ** -24
CHUNK = R.CHUNK
pytestmark = pytest.mark.gpu

SIZES = [1, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
NO_OMEGA = 4                    # this tensor's table entry is 0; its neighbours 3 and 5 have an omega
STEP_COUNTS = [1.0, 2.0, 1000.0]
LRS, WDS = [1e-2, 2.5e-2, 4e-3], [0.05, 0.0, 0.2]
BETA1, BETA2, EPS, MOM = 0.9, 0.999, 1e-8, 0.9
CANARY = 1234.5


def gamma(n):
    return n * U / (1 - n * U)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class Slot:
    """`n` elements inside a buffer of their own: `start` = 1..4 canary words in front, one canary word behind"""

    def __init__(self, values, rot, dev):
        self.n, self.start = values.numel(), 1 + rot % 4
        host = torch.full((self.start + self.n + 1,), CANARY)
        host[self.start:self.start + self.n] = values.float()
        self.buf = host.to(dev)
        self.view = self.buf[self.start:self.start + self.n]
        self.before = self.buf.clone()

    def snap(self):
        self.before = self.buf.clone()

    def restore(self):
        self.buf.copy_(self.before)

    def old(self):
        return self.before[self.start:self.start + self.n]

    def canaries_intact(self):
        s, e = self.start, self.start + self.n
        return bool((self.buf[:s] == CANARY).all()) and bool((self.buf[e:] == CANARY).all())

    def untouched(self):
        return _same_bits(self.buf, self.before)


def _slots(dev, seed, stream, scale=1.0, fn=None, sizes=SIZES):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        x = torch.randn(n, generator=g) * scale
        out.append(Slot(fn(x) if fn else x, i + stream, dev))
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from vilco_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------- the update kernels
class StepCase:
    def __init__(self, dev, kind, ngroups, seed):
        self.dev, self.kind, self.ngroups, n = dev, kind, ngroups, len(SIZES)
        self.p = _slots(dev, seed, 0, 1e-2)
        self.g = _slots(dev, seed + 1, 1)
        self.m = _slots(dev, seed + 2, 2, 0.1)
        self.v = _slots(dev, seed + 3, 3, 0.01, fn=torch.abs)
        self.om = _slots(dev, seed + 4, 2, 1e-4)                 # a path integral already under way, both signs
        self.steps = [STEP_COUNTS[i % 3] for i in range(n)]
        self.group = [(2 * i + i // 3) % ngroups for i in range(n)]        # every (group, step count) pair occurs
        if kind == "SGD":
            with torch.no_grad():
                for i, t in enumerate(self.steps):
                    if t <= 1:
                        self.m[i].view.fill_(float('nan'))       # first step: the buffer is not read
        for s in self.p + self.m + self.v:
            s.snap()
        self.table = R.Table(dev, [[s.view.data_ptr() for s in r] for r in (self.p, self.g, self.m, self.v)], SIZES)
        self.tstep = torch.tensor(self.steps, dtype=torch.float32).to(dev)
        self.tgroup = torch.tensor(self.group, dtype=torch.int32).to(dev)
        self.amax = torch.zeros(self.table.nchunks, device=dev)
        self.si = torch.tensor([0 if i == NO_OMEGA else s.view.data_ptr() for i, s in enumerate(self.om)], dtype=torch.int64).to(dev)

    def run(self, coef, with_si):
        L, lib = _lib()
        lr, wd = (C.c_float * 3)(*LRS), (C.c_float * 3)(*WDS)
        d = L.OptimDesc(table=self.table.struct(), kind=0 if self.kind == "AdamW" else 1, group=self.tgroup.data_ptr(),
                        lr=C.addressof(lr), wd=C.addressof(wd), ngroups=self.ngroups,
                        beta1=BETA1, beta2=BETA2, eps=EPS, momentum=MOM, tensor_step=self.tstep.data_ptr(),
                        norm_coef=None if coef is None else coef.data_ptr(), chunk_amax=self.amax.data_ptr(), lr_dev=None,
                        si_ptrs=self.si.data_ptr() if with_si else None)
        try:
            L.check(lib.vilco_optim_step(C.byref(d), _stream()))
        finally:
            torch.cuda.synchronize()


@pytest.mark.parametrize("clip", [1.0, 0.37], ids=["noclip", "clip"])
@pytest.mark.parametrize("ngroups", [2, 3])
@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_step_kernels_take_the_path_integral(dev, kind, ngroups, clip):
    """numel 1 .. 2 chunks + 5, step counts 1 / 2 / 1000 and two or three (lr, wd) groups mixed over one call, clip coefficient
    1 (no norm_coef) or 0.37; tensor NO_OMEGA has no omega.  Two calls with SI on top of each other, each checked from the
    device's own state before it; p and the optimizer state must carry the bits of the same calls without SI."""
    case = StepCase(dev, kind, ngroups, 100)
    coef = None if clip == 1.0 else torch.tensor([7.0, clip]).to(dev)
    c = 1.0 if coef is None else R.f32(clip)
    assert sorted(set(case.steps)) == STEP_COUNTS and len(set(case.group)) == ngroups
    written = (case.p, case.m) + ((case.v,) if kind == "AdamW" else ())
    # the same two calls without SI
    plain = []
    for call in range(2):
        case.run(coef, with_si=False)
        plain.append([[s.view.clone() for s in rows] for rows in written])
    assert all(s.untouched() for s in case.om), "si_ptrs = NULL must not touch any omega"
    for s in case.p + case.m + case.v:
        s.restore()
    total_term = [torch.zeros(n, dtype=torch.float64) for n in SIZES]
    total_bound = [torch.zeros(n, dtype=torch.float64) for n in SIZES]
    start = [s.view.double().cpu() for s in case.om]
    for call in range(2):
        p_old = [s.view.clone() for s in case.p]
        om_old = [s.view.clone() for s in case.om]
        case.run(coef, with_si=True)
        for rows, kept in zip(written, plain[call]):
            for i, (s, k) in enumerate(zip(rows, kept)):
                assert _same_bits(s.view, k), "call %d: SI changed the update of tensor %d (numel %d)" % (call, i, s.n)
        worst = 0.0
        for i, n in enumerate(SIZES):
            if i == NO_OMEGA:
                continue
            want, term = S.path_integral(om_old[i], case.g[i].view, c, p_old[i], case.p[i].view)
            err = (case.om[i].view.double().cpu() - want).abs()
            bound = gamma(3) * term + gamma(2) * want.abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (call, n, case.steps[i], float((err / bound.clamp_min(1e-300)).max()))
            assert float(term.max()) > 0 and not _same_bits(case.om[i].view, om_old[i])
            total_term[i] += (case.g[i].view.double().cpu() * c) * (case.p[i].view.double().cpu() - p_old[i].double().cpu())
            total_bound[i] += bound
        print("%s groups %d clip %g call %d: omega max err / bound = %.3f" % (kind, ngroups, clip, call, worst))
    for i, n in enumerate(SIZES):
        if i != NO_OMEGA:      # both calls together, against the float64 sum of the two products
            err = (case.om[i].view.double().cpu() - (start[i] - total_term[i])).abs()
            assert bool((err <= total_bound[i]).all()), n
    assert case.om[NO_OMEGA].untouched(), "a tensor whose table entry is 0 has no omega to write"
    assert all(s.canaries_intact() for s in case.om + case.p + case.m + case.v)
    assert all(s.untouched() for s in case.g)
    if kind == "SGD":
        assert all(s.untouched() for s in case.v)


# ------------------------------------------------------------------------------------------------- the consolidation
def _consolidate(dev, rows, numels, numel_old, xi):
    L, lib = _lib()
    tb = R.Table(dev, [[s.view.data_ptr() for s in r] for r in rows], numels)
    t_o = torch.tensor(numel_old, dtype=torch.int64).to(dev)
    d = L.SiDesc(table=tb.struct(), numel_old=t_o.data_ptr(), xi=xi)
    try:
        L.check(lib.vilco_si_consolidate(C.byref(d), _stream()))
    finally:
        torch.cuda.synchronize()


def _prefix(n, mode):
    """numel_old: 0, a strict prefix (for 2 CHUNK + 5 it ends inside the second chunk), all"""
    return (0, n - n // 3 - 1 if n > 1 else 0, n)[mode]


def test_consolidation_kernel(dev):
    """every edge size with numel_old = 0, a strict prefix and the full tensor (3 x 9 tensors, one launch); omega of both
    signs (negative: clamped, the importance keeps its old value), theta == theta_start on every other element (denominator
    xi); importance behind numel_old is NaN before the call: it must be written without being read."""
    xi = 0.1
    sizes = [n for n in SIZES for _ in range(3)]
    modes = [k % 3 for k in range(len(sizes))]
    n_old = [_prefix(n, m) for n, m in zip(sizes, modes)]
    assert any(0 < o < n for o, n in zip(n_old, sizes)) and any(CHUNK < o < 2 * CHUNK for o in n_old)
    p = _slots(dev, 200, 0, 1e-2, sizes=sizes)
    om = _slots(dev, 201, 1, 1e-4, sizes=sizes)
    ts = _slots(dev, 202, 2, 1e-2, sizes=sizes)
    imp = _slots(dev, 203, 3, 1.0, fn=torch.abs, sizes=sizes)
    opt = _slots(dev, 204, 0, 1.0, sizes=sizes)
    with torch.no_grad():
        for i, n in enumerate(sizes):
            ts[i].view[::2] = p[i].view[::2]
            imp[i].view[n_old[i]:] = float('nan')
    for s in p + om + ts + imp:
        s.snap()
    assert any(bool((s.old() < 0).any()) for s in om)
    _consolidate(dev, [p, om, ts, imp, opt], sizes, n_old, xi)
    worst = 0.0
    for i, n in enumerate(sizes):
        old = None if n_old[i] == 0 else imp[i].old()[:n_old[i]]
        want, _, _, _, (a_old, quot) = S.consolidate(p[i].old(), om[i].old(), ts[i].old(), old, xi)
        got = imp[i].view.double().cpu()
        assert bool(torch.isfinite(got).all()) and bool((got >= 0).all()), (n, n_old[i])
        err, bound = (got - want).abs(), U * quot + U * want
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (n, n_old[i], float((err / bound.clamp_min(1e-300)).max()))
        neg = (om[i].old() <= 0).cpu()
        assert torch.equal(got[neg], a_old[neg])                       # clamped: exactly the old importance (0 behind numel_old)
        assert _same_bits(opt[i].view, p[i].old()) and _same_bits(ts[i].view, p[i].old()), n
        assert bool((_bits(om[i].view) == 0).all()), n
    print("consolidation: importance max err / bound = %.3f" % worst)
    assert all(s.untouched() for s in p)
    assert all(s.canaries_intact() for s in om + ts + imp + opt)


# ------------------------------------------------------------------------------------------------- penalty, Python layer
class _Net(torch.nn.Module):
    """parameters at the chunk edges; `head` is the class head (rows = classes); 'scale' is not regularised"""

    def __init__(self, dev, rows=4, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)

        def mk(*shape):
            return torch.nn.Parameter((0.05 * torch.randn(*shape, generator=g)).to(dev))
        self.a, self.b, self.c = mk(CHUNK + 1), mk(257), mk(3)
        self.big = mk(2 * CHUNK + 5)
        self.head = mk(rows, 65)
        self.frozen = mk(40)
        self.frozen.requires_grad = False
        self.scale = mk(1)
        self.reg_params = {}


def _set_grads(net, it):
    for i, (name, p) in enumerate(net.named_parameters()):
        if p.requires_grad:
            g = torch.randn(p.shape, generator=torch.Generator().manual_seed(1000 * it + i))
            p.grad = g.to(p.device)


def test_penalty_si_is_the_mas_penalty(dev):
    from vilco_amd.cl_methods import regularizers
    net = _Net(dev)
    gen = torch.Generator().manual_seed(3)
    imp = {n: torch.rand(p.shape, generator=gen).to(dev) for n, p in net.named_parameters() if n != 'frozen'}
    imp['head'] = imp['head'][:3].contiguous()                          # consolidated when the head had three rows
    opt = {n: torch.randn(v.shape, generator=gen).to(dev) for n, v in imp.items()}
    net.reg_params = {'importance': [imp], 'optpar': [opt]}
    out = {}
    for kind in ('mas', 'si'):
        _set_grads(net, 0)
        val = regularizers.apply_penalty(net, 0.37, kind=kind)
        torch.cuda.synchronize()
        out[kind] = (val.clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    assert float(out['si'][0]) > 0 and _same_bits(out['si'][0], out['mas'][0])
    assert all(_same_bits(out['si'][1][n], g) for n, g in out['mas'][1].items())
    want = S.penalty([p for _, p in net.named_parameters()],
                     [(i, imp[n], opt[n]) for i, (n, _) in enumerate(net.named_parameters()) if n in imp and 'scale' not in n], 0.37)
    assert abs(float(out['si'][0]) - want) <= gamma(74) * want           # the value bound of tests/test_optim_edges_gpu.py


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_attach_begin_task_and_consolidate_through_the_python_layer(dev, kind):
    """FusedOptimizer over a small net, two tasks: si_begin_task, three clipped steps with changing gradients (omega against
    the float64 path integral over the values the parameters held), on_task_si_update (reg_params against the restatement);
    then the head grows, a new optimizer, the same again: importance of the new shape, the old importance on its prefix."""
    from vilco_amd.cl_methods import regularizers
    from vilco_amd.utils.train_utils import FusedOptimizer
    net = _Net(dev)
    xi = 0.1
    tracked = ['a', 'b', 'c', 'big', 'head']
    prev_imp = None
    for task in range(2):
        if task == 1:                                   # the class head gains two rows (a new tensor, as augment_classification)
            with torch.no_grad():
                grown = torch.cat([net.head.detach(), 0.05 * torch.randn(2, 65, device=dev)])
            net.head = torch.nn.Parameter(grown)
        params = dict(net.named_parameters())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            opt = FusedOptimizer([{"params": [params['a'], params['b'], params['head'], params['b']], "weight_decay": 0.05},
                                  {"params": [params['c'], params['big'], params['scale']], "weight_decay": 0.0}],
                                 lr=1e-2, kind=kind)     # `b` is listed twice: two updates per step, both on its path
        sd_keys = sorted(opt.state_dict())
        state = regularizers.si_begin_task(net, opt)
        assert sorted(state) == sorted(tracked) and sorted(opt.state_dict()) == sd_keys
        assert all(float(state[n]['omega'].abs().max()) == 0.0 and _same_bits(state[n]['theta_start'], params[n]) for n in tracked)
        want = {n: torch.zeros(params[n].shape, dtype=torch.float64) for n in tracked}
        bound = {n: torch.zeros(params[n].shape, dtype=torch.float64) for n in tracked}
        for it in range(3):
            _set_grads(net, 10 * task + it)
            before = {n: params[n].detach().clone() for n in tracked}
            opt.step(clip_grad_l2norm=1.0)
            torch.cuda.synchronize()
            c = float(opt.last_grad_norm[1])
            assert c < 1.0
            for n in tracked:
                if n == 'b':         # two updates per step: the value between them is not observable from here
                    continue
                w, term = S.path_integral(want[n], params[n].grad, c, before[n], params[n])
                bound[n] += gamma(3) * term + gamma(2) * w.abs()
                want[n] = w
        for n in tracked:
            if n == 'b':
                assert float(state[n]['omega'].abs().max()) > 0
                continue
            err = (state[n]['omega'].double().cpu() - want[n]).abs()
            assert bool((err <= bound[n]).all()), (task, n, float((err / bound[n].clamp_min(1e-300)).max()))
        assert 'scale' not in state and 'frozen' not in state
        snap = {n: (params[n].detach().clone(), state[n]['omega'].clone(), state[n]['theta_start'].clone()) for n in tracked}
        reg = regularizers.on_task_si_update(net, opt, xi=xi)
        torch.cuda.synchronize()
        assert sorted(reg) == ['importance', 'optpar'] and len(reg['importance']) == len(reg['optpar']) == 1
        assert sorted(reg['importance'][0]) == sorted(tracked) == sorted(reg['optpar'][0])
        for n in tracked:
            th, om, ts = snap[n]
            old = None if prev_imp is None else prev_imp[n]
            w, _, _, _, (a_old, quot) = S.consolidate(th, om, ts, old, xi)
            got = reg['importance'][0][n]
            assert got.shape == params[n].shape
            err = (got.double().cpu() - w).abs()
            assert bool((err <= U * quot + U * w).all()), (task, n)
            assert _same_bits(reg['optpar'][0][n], th) and _same_bits(state[n]['theta_start'], th)
            assert float(state[n]['omega'].abs().max()) == 0.0
            assert float(got.max()) > 0 and float(got.min()) >= 0
        if task == 1:      # the two new rows: Omega_old counts as zero there
            th, om, ts = snap['head']
            fresh = S.consolidate(th[4:], om[4:], ts[4:], None, xi)[0]
            err = (reg['importance'][0]['head'][4:].double().cpu() - fresh).abs()
            assert bool((err <= 2 * U * fresh).all())
        prev_imp = {n: v.clone() for n, v in reg['importance'][0].items()}
        assert regularizers.apply_penalty(net, 0.5, kind='si') is not None
    with pytest.raises(RuntimeError):
        opt.attach_si({params['a']: torch.zeros(3, device=dev)})
    opt.attach_si(None)
    _set_grads(net, 99)
    opt.step()
    torch.cuda.synchronize()
    assert all(float(state[n]['omega'].abs().max()) == 0.0 for n in tracked), "detached: omega is no longer advanced"


# ------------------------------------------------------------------------------------------------- replayed steps
def _episode_model(dev):
    import vilco_amd.modeling as vm
    from parity_util import cases, episode_full_state, load_episode_golden
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_episode_golden()
    cfg = make_config(**gold['overrides'])
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    model.load_state_dict(episode_full_state(gold['init_state']), strict=True)
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    return cfg, model


@pytest.fixture
def seed_word_zero():
    from vilco_amd import _lib
    yield
    _lib.check(_lib.load().vilco_seed_word_set(0, None))
    torch.cuda.synchronize()


def test_replayed_steps_advance_omega_like_eager_steps(dev, seed_word_zero):
    """the episode model of tests/test_graph_gpu.py (adapters listed twice, prompts, an XLNet layer; no dropout), four changing
    batches per epoch.  Epoch 0 without SI, then si_begin_task, epoch 1 with it -- eagerly, and through a GraphedStep (first
    iteration of each epoch eager, three replayed).  The graph captured before attach_si must not be reused after it, and
    the omegas of the two runs must be the same bits: the replayed update is the eager update's launch, and the step is
    deterministic on this model (as tests/test_graph_gpu.py holds for the parameters, with the same proviso for the
    gaussian-weight parameters, whose gradients loss.hip accumulates with float atomics)."""
    from parity_util import cases
    from vilco_amd.cl_methods import regularizers
    from vilco_amd.graph import GraphedStep
    from vilco_amd.utils.train_utils import make_optimizer, make_scheduler, train_one_epoch
    runs = []
    for use_graph in (False, True):
        cfg, model = _episode_model(dev)
        clip = cfg['train_cfg']['clip_grad_l2norm']
        opt = make_optimizer(model, cfg['opt'])
        sch = make_scheduler(opt, cfg['opt'], len(cases.episode_batches(0)))
        graph = GraphedStep(model, opt, clip_grad_l2norm=clip, eager_steps=1) if use_graph else None
        mid = None
        for epoch in range(2):
            if epoch == 1:
                state = regularizers.si_begin_task(model, opt)
                mid = dict(graph.stats) if use_graph else None
            model.pre_train_epoch(task_id=0, current_epoch=epoch)
            train_one_epoch(cases.episode_batches(0), model, opt, sch, epoch, 1, clip_grad_l2norm=clip, cl_name='si',
                            reg_lambda=1.0, prev_out_cls_logits_dict={}, current_task_id=0, graph=graph)
        torch.cuda.synchronize()
        if use_graph:
            assert mid['captured'] == 1 and mid['replayed'] == 3 and mid['dropped'] == 0, mid
            assert graph.stats['dropped'] == 1 and graph.stats['captured'] == 2 and graph.stats['replayed'] == 6, graph.stats
            assert graph.stats['eager'] == 2, graph.stats
        runs.append({n: s['omega'].clone() for n, s in state.items()})
    eager, replayed = runs
    assert sorted(eager) == sorted(replayed) and len(eager) > 50
    moved = 0
    for n in eager:
        moved += float(eager[n].abs().max()) > 0
        assert torch.equal(eager[n], replayed[n]) or (any(t in n for t in ("mu", "sigma")) and
                                                      torch.allclose(eager[n], replayed[n], rtol=1e-5, atol=1e-12)), n
    assert moved > 50, moved


# ------------------------------------------------------------------------------------------------- episode
def _task_data(task):
    from parity_util import cases
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_task_episode_under_si(dev, tmp_path, monkeypatch, seed_word_zero, use_graph):
    """run_episodes with cl_cfg.name = 'si' over the two-task in-memory stream: task 0 trains without a penalty and leaves
    importance / optpar for every regularised parameter; task 1 pays a positive penalty in every iteration; a consolidation
    after task 1 gives the grown class head an importance of its new shape, the new rows without an old part."""
    from parity_util import cases
    from vilco_amd.cl_methods import regularizers
    from vilco_amd.train_cl import run_episodes
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    cfg, model = _episode_model(dev)
    cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], name='si', reg_lambda=1.0, si_xi=0.1, path_memory='memory.pkl')
    stream = InMemoryQILStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
    random.seed(0)
    pens, real = [], regularizers.apply_penalty

    def spy(m, lam, kind='ewc'):
        out = real(m, lam, kind=kind)
        pens.append((kind, None if out is None else out.detach().clone(), len(m.reg_params.get('importance', []))))
        return out
    monkeypatch.setattr(regularizers, 'apply_penalty', spy)
    with pytest.raises(ValueError, match="start_epoch"):
        run_episodes(cfg, model, stream, ckpt_folder=None, start_epoch=1)
    calls = []

    def validate(m, epoch, task):
        # the first of a task's two epochs scores best: the reload puts the model back to it, while SI has consolidated (and
        # anchored theta*) at the end of the second -- so task 1 starts away from theta* and pays from its first iteration
        calls.append(task)
        return 1.0 if calls.count(task) == 2 else 0.1             # (a task's first call validates the incoming model)
    model, opt, sch, log = run_episodes(cfg, model, stream, validate=validate, ckpt_folder=str(tmp_path), gpu_id=0,
                                        use_graph=use_graph, keep_history=True)
    torch.cuda.synchronize()
    assert [e['best_epoch'] for e in log] == [0, 0]
    n0, n1 = (sum(len(ep) for ep in e['history']) for e in log)
    assert len(pens) == n0 + n1 and n0 > 0 and n1 > 0 and {k for k, _, _ in pens} == {'si'}
    assert all(v is None for _, v, _ in pens[:n0]), "no task consolidated yet: no penalty in task 0"
    assert all(v is not None and float(v) > 0 and k == 1 for _, v, k in pens[n0:]), "task 1 pays a positive penalty"
    hist1 = [h for ep in log[1]['history'] for h in ep]
    assert all(bool(torch.isfinite(h['final_loss'])) for h in hist1)
    # what task 0 left (the best checkpoint of task 1 carries it through the reload)
    reg = model.reg_params
    assert sorted(reg) == ['importance', 'optpar'] and len(reg['importance']) == 1
    imp0, opt0 = reg['importance'][0], reg['optpar'][0]
    params = dict(model.named_parameters())
    names = sorted(imp0)          # what was trainable when task 0 began (a parameter unfrozen later has no omega: table entry 0)
    assert set(imp0) == set(opt0) and len(imp0) > 50 and all(n in params and 'scale' not in n for n in names)
    total = 0.0
    for n in names:
        assert imp0[n].shape == opt0[n].shape and imp0[n].shape[1:] == params[n].shape[1:], n
        assert bool(torch.isfinite(imp0[n]).all()) and float(imp0[n].min()) >= 0, n
        total += float(imp0[n].sum())
    assert total > 0
    head = 'cls_head.cls_head.conv.weight'
    assert imp0[head].shape[0] == cases.EP_NCLS0 and params[head].shape[0] == cases.EP_NCLS0 + cases.EP_NEW
    ck = torch.load(os.path.join(str(tmp_path), 'best_task_001_performance.pth.tar'), weights_only=False)
    assert sorted(ck['reg_params']) == ['importance', 'optpar'] and 'si_state' not in ck
    assert torch.equal(ck['reg_params']['importance'][0][head].to(dev), imp0[head])
    ck0 = torch.load(os.path.join(str(tmp_path), 'best_task_000_performance.pth.tar'), weights_only=False)
    assert not ck0['reg_params'], "task 0's checkpoints were written before anything was consolidated"
    moved = [n for n in names if not torch.equal(opt0[n], ck0['state_dict'][n].to(dev))]
    assert len(moved) > 50, "theta* is the state at the END of task 0's training, not the reloaded best epoch"
    # a consolidation after task 1: the head's importance takes the new shape
    state = model.si_state
    snap = {n: (params[n].detach().clone(), state[n]['omega'].clone(), state[n]['theta_start'].clone(), imp0[n].clone())
            for n in (head, next(k for k in names if k != head and k in state))}
    assert float(state[head]['omega'].abs().max()) > 0
    reg = regularizers.on_task_si_update(model, opt, xi=0.1)
    torch.cuda.synchronize()
    for n, (th, om, ts, old) in snap.items():
        want, _, _, _, (a_old, quot) = S.consolidate(th, om, ts, old, 0.1)
        got = reg['importance'][0][n]
        assert got.shape == params[n].shape, n
        err = (got.double().cpu() - want).abs()
        assert bool((err <= U * quot + U * want).all()), n
    th, om, ts, old = snap[head]
    new_rows = reg['importance'][0][head][cases.EP_NCLS0:].double().cpu()
    fresh = S.consolidate(th[cases.EP_NCLS0:], om[cases.EP_NCLS0:], ts[cases.EP_NCLS0:], None, 0.1)[0]
    assert bool(((new_rows - fresh).abs() <= 2 * U * fresh).all()), "new rows: the old importance counts as zero"
    assert float(state[head]['omega'].abs().max()) == 0.0 and _same_bits(reg['optpar'][0][head], th)
