"""A-GEM on the device: vilco_agem_project (csrc/optim.hip) at the chunk edges, `ops.agem_project`, `cl_methods.agem.AGEM` on a
small net and a two-task episode, eager and replayed -- against the float64 restatement tests/agem_restatement.py.

Kernel tests call the C entry point with a hand-built chunk table over tensors whose element counts sit at the chunk edges.
Every tensor is a view into a buffer of its own that starts 1 to 4 elements in and ends in a canary word (the `Slot` of
tests/test_si_gpu.py, copied); grad and ref of a tensor start at the SAME offset for six of the nine sizes (the 16-byte path of
the apply kernel, with a scalar head of 0 to 3 elements) and at different offsets for three (its all-scalar path).

Bounds are counted roundings, u = 2^-24, never measurements.
  g.r and r.r:  the dot kernel is sqnorm_kernel's loop with two accumulators: a thread adds at most CHUNK / 256 = 64 products
    (one rounding for the product, one for the add, or one for both when the compiler fuses them: 65 at most along the chain of
    one accumulator), the wave tree adds 6 levels, the block tree 2; the double sum over the partials is exact to 2^-53 and
    its rounding to fp32 is the u |sum| term:  |out - sum| <= gamma(74) sum|terms| + u |sum|   (74 >= 65 + 6 + 2: the constant of
    the penalty test in tests/test_si_gpu.py, whose kernel has the same reduction).
  alpha = fl(dot_d / rr_d) with the double sums: relative error <= (e_dot + e_rr + u) / (1 - e_rr), e_* the relative bounds
    above without their u term.
  elements:  g' = fmaf(-alpha, r, g), one rounding:  |g' - (g - alpha r)| <= u |g - alpha r| (+ u |alpha r|, the allowance for
    an unfused product, which the kernel as built does not use), alpha = the device's own out[2]."""
import random

import pytest
import torch

import agem_restatement as A

R = A.R
U = 2.0 ** -24
CHUNK = A.CHUNK
pytestmark = pytest.mark.gpu

SIZES = [1, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
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

    def restore(self):
        self.buf.copy_(self.before)

    def old(self):
        return self.before[self.start:self.start + self.n]

    def canaries_intact(self):
        s, e = self.start, self.start + self.n
        return bool((self.buf[:s] == CANARY).all()) and bool((self.buf[e:] == CANARY).all())

    def untouched(self):
        return _same_bits(self.buf, self.before)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """grad slot i starts 1 + i % 4 words in; ref slot i one word further for i = 0, 3, 6 (unequal misalignment) and at the
    same offset otherwise"""

    def __init__(self, dev, k, seed=11, zero_ref=False, sizes=SIZES):
        gs, rs = A.inputs(sizes, k, seed)
        if zero_ref:
            rs = [torch.zeros_like(r) for r in rs]
        self.sizes = list(sizes)
        self.g = [Slot(x, i, dev) for i, x in enumerate(gs)]
        self.r = [Slot(x, i + (1 if i % 3 == 0 else 0), dev) for i, x in enumerate(rs)]
        self.table = R.Table(dev, [[s.view.data_ptr() for s in row] for row in (self.g, self.r)], self.sizes)
        self.partial = torch.full((2 * max(self.table.nchunks, 1),), float('nan'), device=dev)
        self.out = torch.full((3,), float('nan'), device=dev)

    def misalignments(self):
        return [(s.view.data_ptr() & 15, t.view.data_ptr() & 15) for s, t in zip(self.g, self.r)]

    def run(self):
        from vilco_amd import _lib as L
        import ctypes as C
        try:
            L.check(L.load().vilco_agem_project(C.byref(self.table.struct()), self.partial.data_ptr(), self.out.data_ptr(), _stream()))
        finally:
            torch.cuda.synchronize()
        return self.out.double().cpu().tolist()


def _sum_bounds(gs, rs):
    """(dot, rr, alpha, projected, bound of out[0], bound of out[1], relative bound of alpha)"""
    dot, rr, alpha, proj, abs_dot = A.project(gs, rs)
    b_dot, b_rr = gamma(74) * abs_dot + U * abs(dot), gamma(74) * rr + U * rr
    e_d = gamma(74) * abs_dot / abs(dot) if dot != 0 else 0.0
    e_r = gamma(74)
    return dot, rr, alpha, proj, b_dot, b_rr, (e_d + e_r + U) / (1 - e_r)


def _check_elements(g_old, r, g_new, alpha_dev):
    """every element against g - alpha r in float64 with the DEVICE's alpha; -> (the float64 reference, its bound)"""
    g_old, r, g_new = (x.detach().double().cpu() for x in (g_old, r, g_new))
    want = g_old - alpha_dev * r
    bound = U * want.abs() + U * (alpha_dev * r).abs()
    err = (g_new - want).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    return want, bound


def test_conflicting_gradient_is_projected(dev):
    case = Case(dev, -0.5)
    mis = case.misalignments()
    assert any(a == b for a, b in mis) and any(a != b for a, b in mis), mis
    assert {a for a, b in mis if a == b} == {0, 4, 8, 12}, "the 16-byte path with every head length"
    assert mis[8][0] == mis[8][1] and mis[6][0] != mis[6][1], "two chunks on the wide path, a full chunk on the scalar path"
    gs, rs = [s.old() for s in case.g], [s.old() for s in case.r]
    dot, rr, alpha, _, b_dot, b_rr, e_alpha = _sum_bounds(gs, rs)
    assert dot < 0 and abs(dot) > 100 * b_dot, (dot, b_dot)
    o_dot, o_rr, o_alpha = case.run()
    print("conflict: |out0 - dot| / bound = %.3f, |out1 - rr| / bound = %.3f, alpha rel err / bound = %.3f"
          % (abs(o_dot - dot) / b_dot, abs(o_rr - rr) / b_rr, abs(o_alpha - alpha) / (e_alpha * abs(alpha))))
    assert abs(o_dot - dot) <= b_dot and abs(o_rr - rr) <= b_rr
    assert o_alpha < 0 and abs(o_alpha - alpha) <= e_alpha * abs(alpha)
    # elements, and g'.r in float64: g' = g - alpha_dev r + delta gives  g'.r = (dot - alpha_dev rr) + delta.r  with
    # |dot - alpha_dev rr| = |alpha - alpha_dev| rr <= e_alpha |dot|
    gr_new, gr_bound = 0.0, e_alpha * abs(dot)
    for i, n in enumerate(SIZES):
        _, bound = _check_elements(gs[i], rs[i], case.g[i].view, o_alpha)
        rd = rs[i].double().cpu()
        gr_new += float((case.g[i].view.double().cpu() * rd).sum())
        gr_bound += float((bound * rd.abs()).sum())
        assert not _same_bits(case.g[i].view, gs[i]), n
    print("conflict: |g'.r| / bound = %.3f (|g.r| was %.1f)" % (abs(gr_new) / gr_bound, abs(dot)))
    assert abs(gr_new) <= gr_bound < 1e-3 * abs(dot)
    assert all(s.untouched() for s in case.r), "ref is read only"
    assert all(s.canaries_intact() for s in case.g + case.r)


def test_agreeing_gradient_keeps_its_bits(dev):
    case = Case(dev, +0.5)
    dot, rr, _, _, b_dot, b_rr, _ = _sum_bounds([s.old() for s in case.g], [s.old() for s in case.r])
    assert dot > 100 * b_dot
    o_dot, o_rr, o_alpha = case.run()
    assert abs(o_dot - dot) <= b_dot and abs(o_rr - rr) <= b_rr
    assert o_alpha == 0.0 and int(_bits(case.out)[2]) == 0
    assert all(s.untouched() for s in case.g + case.r)


def test_zero_reference_gradient_writes_nothing(dev):
    case = Case(dev, -0.5, zero_ref=True)
    out = case.run()
    assert out == [0.0, 0.0, 0.0] and not bool(torch.isnan(case.out).any())
    assert all(s.untouched() for s in case.g + case.r)
    assert not any(bool(torch.isnan(s.buf).any()) for s in case.g)


def test_no_tensors(dev):
    case = Case(dev, -0.5, sizes=[])
    assert case.table.nchunks == 0 and case.table.n == 0
    assert case.run() == [0.0, 0.0, 0.0]


def test_two_calls_give_the_same_bits(dev):
    case = Case(dev, -0.5, seed=12)
    case.run()
    first_out = case.out.clone()
    first = [s.buf.clone() for s in case.g]
    for s in case.g:
        s.restore()
    case.partial.fill_(float('nan'))
    case.out.fill_(float('nan'))
    case.run()
    assert _same_bits(case.out, first_out) and float(case.out[2]) < 0
    assert all(_same_bits(s.buf, f) for s, f in zip(case.g, first))


# ------------------------------------------------------------------------------------------------- op and Python layer
class _Net(torch.nn.Module):
    """the net of tests/test_si_gpu.py (parameters at the chunk edges, a frozen one) with a loss: linear in every parameter
    but `scale`, which the loss does not reach -- so `scale` never has a reference gradient"""

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

    def forward(self, batch, task_id=0):
        """batch: {parameter name: tensor of its shape}; d loss / d p = batch[name]"""
        loss = self.frozen.sum() * 0.0
        for n in ('a', 'b', 'c', 'big', 'head'):
            loss = loss + (getattr(self, n) * batch[n]).sum()
        return {'final_loss': loss}


def _ref_batch(net):
    gen = torch.Generator().manual_seed(77)
    return {n: torch.randn(p.shape, generator=gen).to(p.device) for n, p in net.named_parameters()}


def test_op_and_agem_project_on_a_small_net(dev):
    """reference_pass leaves r = the batch's tensors and every p.grad None.  Then: `c` has no current gradient (left out of both
    sums), `scale` has a gradient but no reference gradient (keeps its bits), `frozen` has neither; a, b, big, head are
    projected as ONE vector.  The fused optimizer's clip afterwards sees the projected gradient."""
    from vilco_amd import ops
    from vilco_amd.cl_methods.agem import AGEM
    from vilco_amd.utils.train_utils import FusedOptimizer
    net = _Net(dev)
    batch = _ref_batch(net)
    params = dict(net.named_parameters())
    agem = AGEM(net, iter(lambda: batch, None), trace=[])
    params['a'].grad = torch.ones_like(params['a'])          # whatever is there is cleared
    agem.reference_pass(0)
    assert all(p.grad is None for p in net.parameters())
    assert {id(p) for p, _ in agem.ref.values()} == {id(params[n]) for n in ('a', 'b', 'c', 'big', 'head')}
    assert all(torch.equal(agem.ref[id(params[n])][1], batch[n]) for n in ('a', 'b', 'c', 'big', 'head'))
    proj = ['a', 'b', 'big', 'head']
    gen = torch.Generator().manual_seed(5)
    for n in proj + ['scale']:
        noise = torch.randn(params[n].shape, generator=gen).to(dev)
        params[n].grad = noise - 0.5 * batch[n] if n != 'scale' else noise
    before = {n: params[n].grad.clone() for n in proj + ['scale']}
    out = agem.project()
    torch.cuda.synchronize()
    assert len(agem.trace) == 1 and agem.trace[0] is out and tuple(out.shape) == (3,) and out.device == dev
    dot, rr, alpha, _, b_dot, b_rr, e_alpha = _sum_bounds([before[n] for n in proj], [batch[n] for n in proj])
    o_dot, o_rr, o_alpha = out.double().cpu().tolist()
    assert dot < 0 and abs(dot) > 100 * b_dot
    assert abs(o_dot - dot) <= b_dot and abs(o_rr - rr) <= b_rr, "c's reference gradient is in neither sum"
    assert o_alpha < 0 and abs(o_alpha - alpha) <= e_alpha * abs(alpha)
    for n in proj:
        _check_elements(before[n], batch[n], params[n].grad, o_alpha)
        assert torch.equal(agem.ref[id(params[n])][1], batch[n])
    assert _same_bits(params['scale'].grad, before['scale']), "no reference gradient: the gradient stays as it is"
    assert params['c'].grad is None and params['frozen'].grad is None
    # the op on its own: the same call gives the same bits; an agreeing pair is left alone
    again = [before[n].clone() for n in proj]
    out2 = ops.agem_project(again, [batch[n] for n in proj])
    assert _same_bits(out2, out) and all(_same_bits(x, params[n].grad) for x, n in zip(again, proj))
    agree = [-before[n] for n in proj]
    kept = [x.clone() for x in agree]
    out3 = ops.agem_project(agree, [batch[n] for n in proj])
    assert float(out3[2]) == 0.0 and float(out3[0]) > 0 and all(_same_bits(x, k) for x, k in zip(agree, kept))
    assert ops.agem_project([], []).tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(RuntimeError):
        ops.agem_project([again[0]], [batch['b']])
    with pytest.raises(RuntimeError):
        ops.agem_project([again[0].double()], [batch['a']])
    # clip + update over what p.grad holds now
    held = [params[n].grad.double().cpu() for n in proj + ['scale']]
    want = float(sum(float((x * x).sum()) for x in held)) ** 0.5
    unprojected = float(sum(float((before[n].double() ** 2).sum()) for n in proj + ['scale'])) ** 0.5
    opt = FusedOptimizer([{"params": [params[n] for n in ('a', 'b', 'c', 'big', 'head', 'scale')], "weight_decay": 0.0}], lr=1e-3)
    opt.step(clip_grad_l2norm=1.0)
    torch.cuda.synchronize()
    norm = float(opt.last_grad_norm[0])
    assert abs(norm - want) <= gamma(74) * want and want < 0.95 * unprojected


# ------------------------------------------------------------------------------------------------- episode
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


def _task_data(task):
    from parity_util import cases
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


@pytest.fixture(scope="module")
def episodes(dev, tmp_path_factory):
    """run_episodes with cl_cfg.name = 'agem' over the two-task in-memory stream of tests/test_si_gpu.py, eagerly and with
    replayed steps: {use_graph: (log, final parameters, stats of every GraphedStep made)}"""
    from vilco_amd import _lib
    from vilco_amd import graph as graph_mod
    from vilco_amd.train_cl import run_episodes
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    runs = {}
    real = graph_mod.GraphedStep
    made = []

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    mp = pytest.MonkeyPatch()
    mp.setattr(graph_mod, 'GraphedStep', Spy)
    try:
        for use_graph in (False, True):
            del made[:]
            cfg, model = _episode_model(dev)
            cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))
            cfg['cl_cfg'] = dict(cfg['cl_cfg'], name='agem', path_memory='memory.pkl')
            stream = InMemoryQILStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
            random.seed(0)                      # the memory's random selection
            torch.manual_seed(0)                # the new rows of the class head (augment_classification)
            torch.cuda.manual_seed_all(0)
            calls = []

            def validate(m, epoch, task):
                calls.append(task)
                return 1.0 if calls.count(task) == 2 else 0.1
            model, opt, sch, log = run_episodes(cfg, model, stream, validate=validate,
                                                ckpt_folder=str(tmp_path_factory.mktemp("agem%d" % use_graph)), gpu_id=0,
                                                use_graph=use_graph, keep_history=True)
            torch.cuda.synchronize()
            runs[use_graph] = (log, {n: p.detach().clone() for n, p in model.named_parameters()}, [dict(g.stats) for g in made])
    finally:
        mp.undo()
        _lib.check(_lib.load().vilco_seed_word_set(0, None))
        torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_task_episode_under_agem(episodes, use_graph):
    """task 0 finds the memory empty and trains plainly; task 1 takes a reference gradient and projects in every iteration"""
    log, params, stats = episodes[use_graph]
    assert len(log) == 2 and not log[0].get('agem')
    hist1 = [h for ep in log[1]['history'] for h in ep]
    recs = log[1]['agem']
    assert len(recs) == len(hist1) > 0
    alphas = []
    for o in recs:
        assert tuple(o.shape) == (3,) and bool(torch.isfinite(o).all())
        dot, rr, alpha = o.tolist()
        assert rr > 0 and alpha <= 0 and (alpha < 0) == (dot < 0)
        alphas.append(alpha)
    print("use_graph=%s: alpha per iteration of task 1: %s" % (use_graph, ["%.3g" % a for a in alphas]))
    for e in log:
        assert all(bool(torch.isfinite(h['final_loss'])) for ep in e['history'] for h in ep)
    assert all(bool(torch.isfinite(p).all()) for p in params.values())
    if use_graph:
        assert len(stats) == 2, "a GraphedStep per task"
        print("replay counters:", stats)
        assert stats[1]['replayed'] > 0 and stats[1]['captured'] > 0, stats
        assert stats[1]['replayed'] + stats[1]['eager'] == len(hist1)
    else:
        assert stats == []


def test_replayed_episode_ends_where_the_eager_one_does(episodes):
    """the replayed update is the eager update's launch and the projection runs on the same values: equal bits, with the proviso
    tests/test_si_gpu.py makes for the gaussian-weight parameters (loss.hip accumulates their gradients with float atomics)"""
    eager, replayed = episodes[False][1], episodes[True][1]
    assert sorted(eager) == sorted(replayed) and len(eager) > 50
    a0 = [float(o[2]) for o in episodes[False][0][1]['agem']]
    a1 = [float(o[2]) for o in episodes[True][0][1]['agem']]
    assert len(a0) == len(a1)
    worst = {}
    for n in eager:
        if not torch.equal(eager[n], replayed[n]):
            d = (eager[n].double() - replayed[n].double()).abs()
            worst[n] = (float(d.max()), float((d / eager[n].double().abs().clamp_min(1e-300)).max()))
    print("parameters that are not bit-equal (max abs, max rel difference):", worst)
    for n in eager:
        assert torch.equal(eager[n], replayed[n]) or (any(t in n for t in ("mu", "sigma")) and
                                                      torch.allclose(eager[n], replayed[n], rtol=1e-5, atol=1e-12)), (n, worst[n])


def test_replayed_steps_project_like_eager_steps_when_the_gradients_conflict(dev):
    """the episode's memory batches never conflict with its task batches, so here the reference gradient is turned round (r = minus
    the gradient of a memory batch): the projection fires -- in eager steps and between the two graphs of a
    replayed step (first two iterations of the epoch eager, the others replayed), with the same bits in out and in the parameters"""
    from parity_util import cases
    from vilco_amd import _lib
    from vilco_amd.cl_methods.agem import AGEM, MemorySampler
    from vilco_amd.graph import GraphedStep
    from vilco_amd.utils.train_utils import make_optimizer, make_scheduler, train_one_epoch

    class Opposed(AGEM):
        def reference_pass(self, task_id):
            out = super().reference_pass(task_id)
            torch._foreach_neg_([r for _, r in self.ref.values()])
            return out
    runs = []
    try:
        for use_graph in (False, True):
            cfg, model = _episode_model(dev)
            clip = cfg['train_cfg']['clip_grad_l2norm']
            opt = make_optimizer(model, cfg['opt'])
            sch = make_scheduler(opt, cfg['opt'], len(cases.episode_batches(0)))
            graph = GraphedStep(model, opt, clip_grad_l2norm=clip, eager_steps=1) if use_graph else None
            agem = Opposed(model, MemorySampler(_task_data(0), 2, seed=1), trace=[])
            for epoch in range(2):
                model.pre_train_epoch(task_id=0, current_epoch=epoch)
                train_one_epoch(cases.episode_batches(0), model, opt, sch, epoch, 1, clip_grad_l2norm=clip, cl_name='agem',
                                prev_out_cls_logits_dict={}, current_task_id=0, graph=graph, agem=agem)
            torch.cuda.synchronize()
            if use_graph:
                assert graph.stats['replayed'] >= 4 and graph.stats['replayed'] + graph.stats['eager'] == 8, graph.stats
            runs.append((torch.stack(agem.trace).cpu(), {n: p.detach().clone() for n, p in model.named_parameters()}))
    finally:
        _lib.check(_lib.load().vilco_seed_word_set(0, None))
        torch.cuda.synchronize()
    (t0, p0), (t1, p1) = runs
    print("alpha per iteration:", ["%.3g" % a for a in t0[:, 2].tolist()])
    assert t0.shape == (8, 3) and bool(torch.isfinite(t0).all()) and bool((t0[:, 2] <= 0).all())
    assert int((t0[:, 2] < 0).sum()) >= 4, "the opposed reference gradient conflicts with most task batches"
    assert torch.equal(t0, t1)
    for n in p0:
        assert torch.equal(p0[n], p1[n]) or (any(t in n for t in ("mu", "sigma")) and
                                             torch.allclose(p0[n], p1[n], rtol=1e-5, atol=1e-12)), n
