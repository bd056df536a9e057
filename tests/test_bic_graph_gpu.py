"""A BiC stage-1 step with n_known > 0 -- the bias layers of MQ/libs/modeling/meta_archs.py:821-836 through ops.bic_correct, the
fused label / loss kernels, the distillation term of :1482-1499 through ops.cl_distill -- is the step the unfused path runs, and
replayed as hipGraphs (vilco_amd/graph.py) it is the step the eager path runs: the targets travel in StepInputs.dist_tgt, alpha
and beta are read from the layers' memory by every replay.  The reference has no counterpart of the replay (eager PyTorch).

(The helpers are those of tests/test_distill_graph_gpu.py, copied.)"""
import random

import numpy as np
import pytest
import torch

from parity_util import GRAD_FLOOR, cases, episode_full_state, load_episode_golden, rel_err

pytestmark = pytest.mark.gpu

N_KNOWN = 2
LAYERS = ((0.9, 0.05), (1.2, -0.1))          # (alpha, beta) of the two bias layers


@pytest.fixture
def seed_word_zero():
    """the dropout step word is process-wide device state: leave it at 0 for the other tests"""
    from vilco_amd import _lib
    yield
    _lib.check(_lib.load().vilco_seed_word_set(0, None))
    torch.cuda.synchronize()


def _bic_model(dev, splits=None, cl_cfg_name=None):
    """the small model of tests/test_graph_gpu.py (BASELINE configs[2] scaled down) as a BiC model after its first task: the
    first N_KNOWN classes known, two frozen bias layers over the columns [0, N_KNOWN) and [N_KNOWN, EP_NCLS0)"""
    import vilco_amd.modeling as vm
    from vilco_amd.core.config import make_config
    from vilco_amd.train_cl import _bias_layer
    from ref_import import xlnet_json
    gold = load_episode_golden()
    o = dict(gold['overrides'])
    if cl_cfg_name is not None:
        o['cl_cfg'] = dict(o['cl_cfg'], name=cl_cfg_name)
    cfg = make_config(**o)
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    model.load_state_dict(episode_full_state(gold['init_state']), strict=True)
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    if cl_cfg_name is None:
        model.cl_name, model.n_known = 'bic', N_KNOWN
        model.list_splits = list(splits) if splits is not None else [N_KNOWN, cases.EP_NCLS0]
        model.list_bias_layers = [_bias_layer(dev) for _ in LAYERS]
        for l, (a, b) in zip(model.list_bias_layers, LAYERS):
            l.alpha.data.fill_(a)
            l.beta.data.fill_(b)
    return cfg, model


def _targets(model, dev, as_numpy):
    """{video_id: per-level list}: every clip its own seeded softmax(. / 2)-style targets over the known classes, the levels
    views of one device buffer as train_cl.cache_prev_logits(kind='softmax_T2') stores them (or the reference's NumPy arrays)"""
    level_T = [model.max_seq_len // s for s in model.fpn_strides]
    out = {}
    for batch in cases.episode_batches(0):
        for clip in batch:
            r = np.random.RandomState(int(clip['video_id'][2:]) + 77)
            host = r.uniform(0.02, 0.98, (sum(level_T), N_KNOWN))
            host = (host / host.sum(1, keepdims=True)).astype(np.float32)
            if as_numpy:
                out[clip['video_id']] = [np.ascontiguousarray(a) for a in np.split(host, np.cumsum(level_T)[:-1])]
            else:
                out[clip['video_id']] = list(torch.from_numpy(host).to(dev).split(level_T))
    return out


def _train(dev, use_graph, as_numpy=False, splits=None, epochs=2, more=False):
    """`epochs` epochs of four iterations; more: then alpha / beta of the newest layer are changed in place and two further
    iterations run.  -> (losses, state, stats[, further losses, state after them])"""
    from vilco_amd.graph import GraphedStep
    from vilco_amd.utils.train_utils import make_optimizer, make_scheduler, train_one_epoch
    cfg, model = _bic_model(dev, splits)
    opt = make_optimizer(model, cfg['opt'])
    sch = make_scheduler(opt, cfg['opt'], len(cases.episode_batches(0)))
    clip = cfg['train_cfg']['clip_grad_l2norm']
    graph = GraphedStep(model, opt, clip_grad_l2norm=clip, eager_steps=1) if use_graph else None
    prev = _targets(model, dev, as_numpy)

    def run(batches, epoch):
        model.pre_train_epoch(task_id=0, current_epoch=epoch)
        hist = train_one_epoch(batches, model, opt, sch, epoch, 1, clip_grad_l2norm=clip, cl_name='bic', reg_lambda=0.0,
                               prev_out_cls_logits_dict=prev, current_task_id=0, graph=graph)
        return [{k: v.detach().clone() for k, v in h.items()} for h in hist]
    losses = []
    for epoch in range(epochs):
        losses += run(cases.episode_batches(0), epoch)
    torch.cuda.synchronize()
    out = (losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, (dict(graph.stats) if use_graph else None))
    if more:
        model.list_bias_layers[-1].alpha.data.fill_(0.7)
        model.list_bias_layers[-1].beta.data.fill_(0.3)
        further = run(cases.episode_batches(0)[:2], epochs)
        torch.cuda.synchronize()
        out += (further, {k: v.detach().clone() for k, v in model.state_dict().items()}, (dict(graph.stats) if use_graph else None))
    return out


@pytest.fixture(scope="module")
def eager_run(dev):
    """the twin stepped eagerly for 8 + 2 iterations: computed once, shared, left unchanged"""
    return _train(dev, use_graph=False, more=True)


def _same_run(a, b, n=8):
    """the bar of test_graph_gpu.test_graphed_training_equals_eager_training: losses bit for bit; parameters bit for bit, the
    gaussian weights and regression scales up to the order of their gradient sums"""
    (la, sa), (lb, sb) = a[:2], b[:2]
    assert len(la) == len(lb) == n
    for i, (x, y) in enumerate(zip(la, lb)):
        assert set(x) == set(y) and 'dist_loss' in x
        assert torch.equal(x['dist_loss'], y['dist_loss']), (i, float(x['dist_loss']), float(y['dist_loss']))
        for k in x:
            assert float(x[k]) == float(y[k]), (i, k, float(x[k]), float(y[k]))
    for k in sa:
        assert torch.equal(sa[k], sb[k]) or (any(t in k for t in ("mu", "sigma", "scale")) and
                                             torch.allclose(sa[k], sb[k], rtol=1e-5, atol=1e-9)), k


def test_fused_bic_step_equals_the_unfused_step(dev):
    """(a) one eager step through ops.bic_correct + ops.mq_loss + ops.cl_distill against the same step with fused_loss = False
    (label_points + losses over the corrected per-level lists).  The bar between the fused and the tensor-expression loss path
    of the whole model: tests/test_loss_gpu.py:140-145 (losses 1e-5, gradients 1e-4 over a floor of GRAD_FLOOR, the
    analytically-zero key biases left out); tests/test_model_gpu.py:253-258 holds its two evaluations of the unfused losses to
    the same 1e-5 on the losses."""
    batch = cases.episode_batches(0)[0]
    outs = []
    for fused in (True, False):
        cfg, model = _bic_model(dev)
        model.train()
        model.fused_loss = fused
        prev = _targets(model, dev, False)[batch[-1]['video_id']]
        model.pre_train_epoch(task_id=0, current_epoch=0)
        losses = model(batch, task_id=0, prev_out_cls_logits=prev)
        losses['final_loss'].backward()
        outs.append(({k: v.detach().clone() for k, v in losses.items()},
                     {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    (la, ga), (lb, gb) = outs
    assert set(la) == set(lb) and 'dist_loss' in la and float(la['dist_loss']) > 0.0
    worst_l = max((rel_err(la[k], lb[k]), k) for k in la)
    assert sorted(ga) == sorted(gb)
    worst_g = max((rel_err(ga[k], gb[k], GRAD_FLOOR), k) for k in ga if not k.endswith(('key_norm.bias', '.key.bias')))
    print("fused vs unfused BiC step: worst loss %.3e (%s), worst gradient %.3e (%s)" % (worst_l + worst_g))
    assert worst_l[0] < 1e-5, worst_l
    assert worst_g[0] < 1e-4, worst_g


def test_replayed_bic_steps_equal_eager_and_follow_changed_bias_values(dev, seed_word_zero, eager_run):
    """(b) 8 iterations over 2 epochs, eager_steps = 1: one capture, seven replays, the eager twin's numbers.
    (c) alpha / beta of the newest layer changed in place after the capture: two further replays of the SAME graph equal the
    eager twin's two further steps"""
    run = _train(dev, use_graph=True, more=True)
    stats = run[2]
    assert stats['captured'] == 1 and stats['replayed'] == 7 and stats['eager'] == 1, stats
    dist = [float(l['dist_loss']) for l in run[0]]
    assert len(set(dist[:4])) == 4 and min(dist) > 0.0, dist          # consecutive batches carry different targets
    _same_run(run, eager_run)
    after = run[5]
    assert after['captured'] == 1 and after['replayed'] == 9 and after['eager'] == 1 and after['dropped'] == 0, after
    _same_run(run[3:5], eager_run[3:5], n=2)


def test_numpy_targets_stay_eager_and_give_the_same_losses(dev, seed_word_zero, eager_run):
    """(d) host-side targets are uploaded per step: nothing a replay could carry"""
    run = _train(dev, use_graph=True, as_numpy=True)
    assert run[2]['captured'] == 0 and run[2]['replayed'] == 0 and run[2]['eager'] == 8, run[2]
    _same_run(run, eager_run)


def test_a_split_table_the_op_does_not_take_stays_eager(dev, seed_word_zero):
    """(d) splits that do not end at the head's class count: the reference's slice-and-concatenate loop and the unfused losses,
    as before -- with and without a GraphedStep around them.  (A table that ends BELOW the class count leaves the loop's
    output narrower than the labels and the reference's focal loss refuses the shapes; the table here ends above it, where
    the last slice is clamped, so that the step runs.)"""
    splits = [N_KNOWN, cases.EP_NCLS0 + 1]
    graphed = _train(dev, use_graph=True, splits=splits, epochs=1)
    assert graphed[2]['captured'] == 0 and graphed[2]['replayed'] == 0 and graphed[2]['eager'] == 4, graphed[2]
    _same_run(graphed, _train(dev, use_graph=False, splits=splits, epochs=1), n=4)
    _, model = _bic_model(dev, [N_KNOWN])
    model.train()
    batch = cases.episode_batches(0)[0]
    inp = model.prepare(batch, True, gt_pad=8)
    inp.dist_tgt, inp.dist_lens = model.distill_target(_targets(model, dev, False)[batch[-1]['video_id']])
    inp.dist_kind = 'bic'
    assert not model._bic_op_ready() and not model.capturable(inp, 0, None)


def test_what_decides_that_a_bic_step_is_capturable(dev):
    """(d) a batch without a cached clip has no target and stays eager (where the distillation term then refuses the empty
    list, as it did before); the other conditions one by one"""
    from vilco_amd.graph import GraphedStep
    from vilco_amd.modeling.meta_archs import BiasLayer
    _, model = _bic_model(dev)
    model.train()
    batch = cases.episode_batches(0)[0]
    prev = _targets(model, dev, False)[batch[-1]['video_id']]
    g = GraphedStep(model, None)
    inp = g._prepare(batch, prev)
    assert inp.dist_kind == 'bic' and inp.dist_tgt.data_ptr() == prev[0].data_ptr()        # the cached clip's buffer, not a copy
    assert isinstance(model.distill_target(prev), tuple) and len(model.distill_target(prev)) == 2
    assert model.capturable(inp, 0, prev)
    assert ("dist_kind", 'bic') in inp.signature()
    bare = g._prepare(batch, [])
    assert bare.dist_tgt is None and bare.dist_kind is None and not model.capturable(bare, 0, [])
    with pytest.raises(ValueError, match="distillation targets of 0 levels"):
        model(batch, task_id=0, prev_out_cls_logits=[])
    assert model.distill_target(_targets(model, dev, True)[batch[-1]['video_id']]) is None
    by_hand = model.prepare(batch, True, gt_pad=8)
    by_hand.dist_tgt, by_hand.dist_lens = model.distill_target(prev)
    assert not model.capturable(by_hand, 0, prev)                                          # not attached for BiC
    key = g._bic_sig()
    model.list_bias_layers[-1].alpha.data.fill_(3.0)
    assert g._bic_sig() == key                                                             # values are not in the key
    layers, splits = model.list_bias_layers, model.list_splits
    model.list_splits = [1, N_KNOWN, cases.EP_NCLS0]
    assert g._bic_sig() != key and not model.capturable(inp, 0, prev)                      # more splits than layers
    model.list_splits, model.list_bias_layers = splits, [layers[0], BiasLayer()]          # a layer on the host
    assert g._bic_sig() != key and not model.capturable(inp, 0, prev)
    model.list_bias_layers = []
    assert not model.capturable(inp, 0, prev)
    model.list_bias_layers = layers
    assert model.capturable(inp, 0, prev)
    model.bic_raw_logits = True
    assert not model.capturable(inp, 0, prev)


def _task_data(task):
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


def test_driver_with_graphs_equals_driver_without(dev, seed_word_zero, monkeypatch):
    """(e) run_episodes_bic over the two-task stream of tests/test_bic_gpu.py: with use_graph the second task replays, and its
    stage 2 ends where the eager driver's does (the bar of _same_run: bit for bit, or within the allowance that bar gives the
    parameters whose gradient sums depend on the order)"""
    import vilco_amd.graph as G
    from vilco_amd.train_cl import run_episodes_bic
    from vilco_amd.utils.cl_stream import InMemoryBiCStream
    made = []

    class Recording(G.GraphedStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(G, "GraphedStep", Recording)
    logs = {}
    for use_graph in (False, True):
        cfg, model = _bic_model(dev, cl_cfg_name='bic')
        cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))           # two epochs per stage
        stream = InMemoryBiCStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
        random.seed(0)
        torch.manual_seed(0)                                                       # augment_classification draws the new head rows
        model, _, _, log = run_episodes_bic(cfg, model, stream, validate=None, ckpt_folder=None, gpu_id=0, use_graph=use_graph)
        assert len(log) == 2 and 'bic' in log[1] and len(model.list_bias_layers) == 2
        logs[use_graph] = log
    assert len(made) == 2, len(made)                                                # one GraphedStep per optimizer, graphs only
    print("driver: task 0 %s, task 1 %s" % (made[0].stats, made[1].stats))
    assert made[1].stats['captured'] >= 1 and made[1].stats['replayed'] >= 1, made[1].stats
    a, b = logs[False][1]['bic'], logs[True][1]['bic']
    for k in ('alpha', 'beta'):
        assert a[k] == b[k] or abs(a[k] - b[k]) <= 1e-5 * abs(a[k]) + 1e-9, (k, a[k], b[k])
    assert a['losses'].shape == b['losses'].shape
    assert torch.equal(a['losses'], b['losses']) or torch.allclose(a['losses'], b['losses'], rtol=1e-5, atol=1e-9), \
        (a['losses'] - b['losses']).abs().max()
    ha = [h for ep in logs[False][1]['history'] for h in ep]
    hb = [h for ep in logs[True][1]['history'] for h in ep]
    assert len(ha) == len(hb) and all('dist_loss' in h for h in hb)
    for i, (x, y) in enumerate(zip(ha, hb)):
        for k in x:
            assert float(x[k]) == float(y[k]), (i, k, float(x[k]), float(y[k]))
