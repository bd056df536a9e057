"""An iCaRL step with n_known > 0 -- the distillation term of MQ/libs/modeling/meta_archs.py:1501-1519 through ops.cl_distill --
replayed as hipGraphs (vilco_amd/graph.py) is the step the eager path runs: the targets travel in StepInputs.dist_tgt and
every replay distils against ITS batch's cached clip.  The reference has no counterpart of the replay (eager PyTorch)."""
import numpy as np
import pytest
import torch

from parity_util import cases, episode_full_state, load_episode_golden

pytestmark = pytest.mark.gpu

N_KNOWN = 2


@pytest.fixture
def seed_word_zero():
    """the dropout step word is process-wide device state: leave it at 0 for the other tests"""
    from vilco_amd import _lib
    yield
    _lib.check(_lib.load().vilco_seed_word_set(0, None))
    torch.cuda.synchronize()


def _icarl_model(dev, cl_name='icarl'):
    """the small model of tests/test_graph_gpu.py (BASELINE configs[2] scaled down), distilling its first N_KNOWN classes"""
    import vilco_amd.modeling as vm
    from vilco_amd.core.config import make_config
    from ref_import import xlnet_json
    gold = load_episode_golden()
    cfg = make_config(**gold['overrides'])
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    model.load_state_dict(episode_full_state(gold['init_state']), strict=True)
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    model.cl_name, model.n_known = cl_name, N_KNOWN
    return cfg, model


def _targets(model, dev, as_numpy):
    """{video_id: per-level list}: every clip its own seeded targets, the levels views of one device buffer as
    train_cl.cache_prev_logits stores them (or the reference's NumPy arrays)"""
    level_T = [model.max_seq_len // s for s in model.fpn_strides]
    out = {}
    for batch in cases.episode_batches(0):
        for clip in batch:
            r = np.random.RandomState(int(clip['video_id'][2:]) + 77)
            host = r.uniform(0.02, 0.98, (sum(level_T), cases.EP_NCLS0)).astype(np.float32)
            if as_numpy:
                out[clip['video_id']] = [np.ascontiguousarray(a) for a in np.split(host, np.cumsum(level_T)[:-1])]
            else:
                out[clip['video_id']] = list(torch.from_numpy(host).to(dev).split(level_T))
    return out


def _train(dev, use_graph, as_numpy=False):
    from vilco_amd.graph import GraphedStep
    from vilco_amd.utils.train_utils import make_optimizer, make_scheduler, train_one_epoch
    cfg, model = _icarl_model(dev)
    opt = make_optimizer(model, cfg['opt'])
    sch = make_scheduler(opt, cfg['opt'], len(cases.episode_batches(0)))
    clip = cfg['train_cfg']['clip_grad_l2norm']
    graph = GraphedStep(model, opt, clip_grad_l2norm=clip, eager_steps=1) if use_graph else None
    prev = _targets(model, dev, as_numpy)
    losses = []
    for epoch in range(2):
        model.pre_train_epoch(task_id=0, current_epoch=epoch)
        hist = train_one_epoch(cases.episode_batches(0), model, opt, sch, epoch, 1, clip_grad_l2norm=clip, cl_name='icarl',
                               reg_lambda=0.0, prev_out_cls_logits_dict=prev, current_task_id=0, graph=graph)
        losses += [{k: v.detach().clone() for k, v in h.items()} for h in hist]
    torch.cuda.synchronize()
    return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, (graph.stats if use_graph else None)


@pytest.fixture(scope="module")
def eager_run(dev):
    """the twin stepped eagerly for 8 iterations: computed once, shared, left unchanged"""
    return _train(dev, use_graph=False)


def _same_run(a, b):
    """the bar of test_graph_gpu.test_graphed_training_equals_eager_training: losses bit for bit; parameters bit for bit, the
    gaussian weights and regression scales up to the order of their gradient sums"""
    (la, sa, _), (lb, sb, _) = a, b
    assert len(la) == len(lb) == 8
    for i, (x, y) in enumerate(zip(la, lb)):
        assert set(x) == set(y) and 'dist_loss' in x
        assert torch.equal(x['dist_loss'], y['dist_loss']), (i, float(x['dist_loss']), float(y['dist_loss']))
        for k in x:
            assert float(x[k]) == float(y[k]), (i, k, float(x[k]), float(y[k]))
    for k in sa:
        assert torch.equal(sa[k], sb[k]) or (any(t in k for t in ("mu", "sigma", "scale")) and
                                             torch.allclose(sa[k], sb[k], rtol=1e-5, atol=1e-9)), k


def test_replayed_icarl_steps_distil_against_their_own_batch(dev, seed_word_zero, eager_run):
    run = _train(dev, use_graph=True)
    stats = run[2]
    assert stats['captured'] == 1 and stats['replayed'] == 7 and stats['eager'] == 1, stats
    dist = [float(l['dist_loss']) for l in run[0]]
    assert len(set(dist[:4])) == 4 and min(dist) > 0.0, dist          # consecutive batches carry different targets
    _same_run(run, eager_run)


def test_numpy_targets_stay_eager_and_give_the_same_losses(dev, seed_word_zero, eager_run):
    run = _train(dev, use_graph=True, as_numpy=True)
    assert run[2]['captured'] == 0 and run[2]['replayed'] == 0 and run[2]['eager'] == 8, run[2]
    _same_run(run, eager_run)


def test_bic_and_targetless_steps_are_not_capturable(dev):
    _, model = _icarl_model(dev)
    model.train()
    batch = cases.episode_batches(0)[0]
    prev = _targets(model, dev, False)
    inp = model.prepare(batch, True, gt_pad=8)
    assert not model.capturable(inp, 0, [prev[batch[0]['video_id']]])          # no target buffer among the inputs
    inp.dist_tgt, inp.dist_lens = model.distill_target([prev[v['video_id']] for v in batch])
    assert inp.dist_tgt.data_ptr() == prev[batch[0]['video_id']][0].data_ptr()  # the first cached clip's buffer, not a copy
    assert model.capturable(inp, 0, [prev[v['video_id']] for v in batch])
    assert ("dist_tgt", tuple(inp.dist_tgt.shape)) in inp.signature()
    assert model.distill_target([]) is None and model.distill_target(_targets(model, dev, True)[batch[0]['video_id']]) is None
    model.cl_name = 'bic'
    assert not model.capturable(inp, 0, prev[batch[0]['video_id']])
    assert not model.capturable(inp, 0, None)
