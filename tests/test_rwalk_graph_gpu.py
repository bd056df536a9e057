"""RWalk in replayed steps and in the episode driver, on the episode fixture model of tests/test_graph_gpu.py (adapters listed
twice, prompts, an XLNet layer; no dropout, no stochastic depth).

Equal bits between two runs are asked of every parameter and every RWalk state, with the proviso tests/test_graph_gpu.py makes:
loss.hip accumulates the gradients of the gaussian-weight parameters and regression scales ('mu', 'sigma', 'scale') with float
atomics, so those tensors (matched by their exact names, `_atomic`) -- and the states that follow their gradients -- are held to
rtol 1e-5 instead."""
import copy
import ctypes
import os
import pickle
import random
import re

import pytest
import torch

from parity_util import cases, episode_full_state, load_episode_golden

pytestmark = pytest.mark.gpu
DELTA_T = 3
KEYS = ('fisher', 'score', 'omega', 'theta_ck')


# the parameters whose gradients loss.hip accumulates with float atomics (dgauss, dscale): the model's six gaussian-weight
# parameters and the regression head's per-level scales, by their exact names
ATOMIC_NAMES = {'mu', 'sigma', 'mu_reg_left', 'sigma_reg_left', 'mu_reg_right', 'sigma_reg_right'}
ATOMIC_SCALE = re.compile(r'^reg_head\.scale\.\d+\.scale$')


def _atomic(name):
    return name in ATOMIC_NAMES or ATOMIC_SCALE.match(name) is not None


def _equal(name, a, b):
    return torch.equal(a, b) or (_atomic(name) and torch.allclose(a, b, rtol=1e-5, atol=1e-12))


def _episode_model(dev, **cl):
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_episode_golden()
    over = dict(gold['overrides'])
    over['cl_cfg'] = dict(over.get('cl_cfg', {}), **cl)
    cfg = make_config(**over)
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


def test_replayed_steps_keep_the_rwalk_states_of_eager_steps(dev, seed_word_zero):
    """one epoch (four batches) without RWalk, then rwalk_begin_task and 2 delta_t + 1 = 7 iterations on changing batches, then the
    consolidation -- eagerly, and through a GraphedStep (first iteration of each stretch eager, the others replayed).  The graph
    captured before attach_rwalk must not be replayed after it; the tick word, every state, the importance and every parameter
    of the two runs carry the same bits."""
    from vilco_amd.cl_methods import regularizers
    from vilco_amd.graph import GraphedStep
    from vilco_amd.utils.train_utils import make_optimizer, make_scheduler, train_one_epoch
    n_iters = 2 * DELTA_T + 1
    stretch = (cases.episode_batches(0) + cases.episode_batches(0))[:n_iters]
    runs = []
    for use_graph in (False, True):
        cfg, model = _episode_model(dev)
        clip = cfg['train_cfg']['clip_grad_l2norm']
        opt = make_optimizer(model, cfg['opt'])
        sch = make_scheduler(opt, cfg['opt'], n_iters)          # 4 + 7 iterations stay inside its 2 * 7 steps
        graph = GraphedStep(model, opt, clip_grad_l2norm=clip, eager_steps=1) if use_graph else None
        model.pre_train_epoch(task_id=0, current_epoch=0)
        train_one_epoch(cases.episode_batches(0), model, opt, sch, 0, 1, clip_grad_l2norm=clip, cl_name='rwalk', reg_lambda=1.0,
                        prev_out_cls_logits_dict={}, current_task_id=0, graph=graph)
        mid = dict(graph.stats) if use_graph else None
        gen = opt.rwalk_gen
        state = regularizers.rwalk_begin_task(model, opt, alpha=0.9, delta_t=DELTA_T, eps=1e-8)
        assert opt.rwalk_gen == gen + 1
        model.pre_train_epoch(task_id=0, current_epoch=1)
        train_one_epoch(stretch, model, opt, sch, 1, 1, clip_grad_l2norm=clip, cl_name='rwalk', reg_lambda=1.0,
                        prev_out_cls_logits_dict={}, current_task_id=0, graph=graph)
        torch.cuda.synchronize()
        assert int(opt.rwalk_tick) == n_iters
        if use_graph:
            assert mid['captured'] == 1 and mid['replayed'] == 3 and mid['dropped'] == 0, mid
            st = graph.stats
            assert st['dropped'] == 1 and st['captured'] == 2 and st['replayed'] == 3 + n_iters - 1 and st['eager'] == 2, st
        open_interval = sum(float(s['omega'].abs().max()) > 0 for s in state.values())
        scored = sum(float(s['score'].max()) > 0 for s in state.values())
        assert open_interval > 50 and scored > 50, (open_interval, scored)
        before = {n: {k: s[k].clone() for k in KEYS} for n, s in state.items()}
        reg = regularizers.on_task_rwalk_update(model, opt, eps=1e-8)
        torch.cuda.synchronize()
        runs.append(dict(before=before, after={n: {k: s[k].clone() for k in KEYS} for n, s in state.items()},
                         imp={n: t.clone() for n, t in reg['importance'][0].items()},
                         params={n: p.detach().clone() for n, p in model.named_parameters()}))
    eager, replayed = runs
    assert sorted(eager['before']) == sorted(replayed['before']) and len(eager['before']) > 50
    for n in eager['before']:
        for k in KEYS:
            assert _equal(n, eager['before'][n][k], replayed['before'][n][k]), (n, k, "before the consolidation")
            assert _equal(n, eager['after'][n][k], replayed['after'][n][k]), (n, k, "after the consolidation")
    # the importance is normalised by maxima over ALL tensors: the proviso's tensors can move them by a rounding
    exact = all(torch.equal(eager['before'][n][k], replayed['before'][n][k]) for n in eager['before'] for k in KEYS)
    for n in eager['imp']:
        assert torch.equal(eager['imp'][n], replayed['imp'][n]) or (not exact and torch.allclose(eager['imp'][n], replayed['imp'][n], rtol=1e-5, atol=1e-12)), n
        assert bool(torch.isfinite(eager['imp'][n]).all()) and float(eager['imp'][n].min()) >= 0 and float(eager['imp'][n].max()) <= 2.0001
    for n in eager['params']:
        assert _equal(n, eager['params'][n], replayed['params'][n]), n


# ------------------------------------------------------------------------------------------------- episode
def _task_data(task):
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


def _validate(calls, hook=None):
    def validate(m, epoch, task):
        # the first of a task's two epochs scores best: the reload puts the model back to it, while RWalk has consolidated (and
        # anchored theta*) at the end of the second -- task 1 starts away from theta* and pays from its first iteration
        calls.append(task)
        if hook is not None and calls.count(task) == 1:
            hook(m, task)                                   # (a task's first call validates the incoming model)
        return 1.0 if calls.count(task) == 2 else 0.1
    return validate


def test_two_task_episode_under_rwalk_and_a_rerun_from_the_task_boundary(dev, tmp_path, monkeypatch, seed_word_zero):
    """run_episodes with cl_cfg.name = 'rwalk' over the two-task in-memory stream: task 0 pays no penalty and leaves ONE finite
    importance dictionary with values in [0, 2] and rwalk_state.pt next to the memory pickle; task 1 pays a positive penalty.
    Then task 1 again from what the boundary left (the model as task 1 met it, the memory as it was pickled then, rwalk_state.pt):
    the same losses, parameters and RWalk states as the uninterrupted run."""
    from vilco_amd import _lib
    from vilco_amd.cl_methods import regularizers
    from vilco_amd.train_cl import RWALK_STATE_FILE, run_episodes
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    lib = _lib.load()

    def config():
        cfg, model = _episode_model(dev)
        cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))
        cfg['cl_cfg'] = dict(cfg['cl_cfg'], name='rwalk', reg_lambda=1.0, rwalk_delta_t=DELTA_T, path_memory='memory.pkl')
        return cfg, model
    cfg, model = config()
    assert cfg['cl_cfg']['rwalk_alpha'] == 0.9 and cfg['cl_cfg']['rwalk_eps'] == 1e-8
    stream = InMemoryQILStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
    random.seed(0)
    torch.manual_seed(0)
    torch.cuda.manual_seed_all(0)
    pens, real = [], regularizers.apply_penalty

    def spy(m, lam, kind='ewc'):
        out = real(m, lam, kind=kind)
        pens.append((kind, None if out is None else out.detach().clone(), len(m.reg_params.get('importance', []))))
        return out
    monkeypatch.setattr(regularizers, 'apply_penalty', spy)
    with pytest.raises(ValueError, match="start_epoch"):
        run_episodes(cfg, model, stream, ckpt_folder=None, start_epoch=1)
    boundary = {}

    def at_task_start(m, task):
        if task == 1:
            word = ctypes.c_uint32()
            _lib.check(lib.vilco_seed_word_get(ctypes.byref(word)))
            boundary.update(state={k: v.detach().clone() for k, v in m.state_dict().items()},
                            loss_norm=copy.deepcopy(m.loss_normalizer), n_known=m.n_known, word=word.value,
                            memory=pickle.dumps(m.memory),      # memory.pkl as it stood then: task 1's end rewrites the file
                            rng=(random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(dev)))
    folder = str(tmp_path)
    model, opt, sch, log = run_episodes(cfg, model, stream, validate=_validate([], at_task_start), ckpt_folder=folder, gpu_id=0,
                                        use_graph=True, keep_history=True)
    torch.cuda.synchronize()
    n0, n1 = (sum(len(ep) for ep in e['history']) for e in log)
    assert len(pens) == n0 + n1 and n0 > DELTA_T and n1 > DELTA_T and {k for k, _, _ in pens} == {'rwalk'}
    assert all(v is None for _, v, _ in pens[:n0]), "no task consolidated yet: no penalty in task 0"
    assert all(v is not None and float(v) > 0 and k == 1 for _, v, k in pens[n0:]), "task 1 pays a positive penalty"
    hist1 = [h for ep in log[1]['history'] for h in ep]
    assert all(bool(torch.isfinite(h['final_loss'])) for h in hist1)
    reg = model.reg_params
    assert sorted(reg) == ['importance', 'optpar'] and len(reg['importance']) == len(reg['optpar']) == 1
    imp0, opt0 = reg['importance'][0], reg['optpar'][0]
    params = dict(model.named_parameters())
    assert set(imp0) == set(opt0) and len(imp0) > 50 and all(n in params and 'scale' not in n for n in imp0)
    top = 0.0
    for n in imp0:
        assert imp0[n].shape == opt0[n].shape and imp0[n].shape[1:] == params[n].shape[1:], n
        assert bool(torch.isfinite(imp0[n]).all()) and float(imp0[n].min()) >= 0 and float(imp0[n].max()) <= 2.0001, n
        top = max(top, float(imp0[n].max()))
    assert top >= 1.0, "the element that holds a maximum has a term of exactly 1"
    head = 'cls_head.cls_head.conv.weight'
    assert imp0[head].shape[0] == cases.EP_NCLS0 and params[head].shape[0] == cases.EP_NCLS0 + cases.EP_NEW
    path = os.path.join(folder, RWALK_STATE_FILE)
    assert os.path.exists(path) and os.path.exists(os.path.join(folder, 'memory.pkl'))
    saved = torch.load(path, weights_only=False)
    assert sorted(saved) == ['fisher', 'importance', 'optpar', 'score'] and set(saved['fisher']) == set(imp0)
    assert torch.equal(saved['importance'][head].to(dev), imp0[head]) and saved['fisher'][head].shape[0] == cases.EP_NCLS0
    state = model.rwalk_state
    assert state[head]['fisher'].shape[0] == cases.EP_NCLS0 + cases.EP_NEW
    assert float(state[head]['fisher'][cases.EP_NCLS0:].max()) > 0, "the new rows have gathered their own Fisher average in task 1"
    first = {'hist': [{k: v.clone() for k, v in h.items()} for h in hist1],
             'params': {n: p.detach().clone() for n, p in model.named_parameters()},
             'state': {n: {k: s[k].clone() for k in KEYS} for n, s in state.items()}}

    # ---- task 1 again, from the boundary
    class _ResumedStream(InMemoryQILStream):
        def __iter__(self):                                 # iter() empties the memory: a resumed stream keeps what was loaded into it
            memory = self.memory
            super().__iter__()
            self.memory = memory
            return self
    cfg2, model2 = config()
    model2.augment_classification(cases.EP_NEW, dev)
    model2.load_state_dict(boundary['state'], strict=True)
    model2.loss_normalizer = boundary['loss_norm']
    model2.memory = pickle.loads(boundary['memory'])
    model2.n_known = boundary['n_known']
    stream2 = _ResumedStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
    stream2.memory = model2.memory
    with pytest.raises(ValueError, match="rwalk_state.pt"):
        run_episodes(cfg2, model2, stream2, ckpt_folder=None, start_task=1)
    random.setstate(boundary['rng'][0])
    torch.set_rng_state(boundary['rng'][1])
    torch.cuda.set_rng_state(boundary['rng'][2], dev)
    _lib.check(lib.vilco_seed_word_set(boundary['word'], None))
    stream2 = _ResumedStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
    stream2.memory = model2.memory
    folder2 = str(tmp_path / "again")
    os.makedirs(folder2)
    with open(os.path.join(folder, RWALK_STATE_FILE), 'rb') as src, open(os.path.join(folder2, RWALK_STATE_FILE), 'wb') as dst:
        dst.write(src.read())                               # (written at the boundary only: task 1 is the last task)
    model2, _, _, log2 = run_episodes(cfg2, model2, stream2, validate=_validate([]), ckpt_folder=folder2, gpu_id=0, start_task=1,
                                      use_graph=True, keep_history=True)
    torch.cuda.synchronize()
    hist2 = [h for ep in log2[0]['history'] for h in ep]
    assert len(hist2) == len(first['hist'])
    for a, b in zip(first['hist'], hist2):
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, float(a[k]), float(b[k]))
    for n, p in model2.named_parameters():
        assert _equal(n, first['params'][n], p.detach()), n
    for n, s in model2.rwalk_state.items():
        for k in KEYS:
            assert _equal(n, first['state'][n][k], s[k]), (n, k)
