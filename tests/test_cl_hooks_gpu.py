"""The order of events of an episode, per method: the hook points of cl_methods/hooks.py and the calls they wrap, between the
driver's own steps (optimizers, memory pickle, best-checkpoint reload, head growth), recorded over two tasks of two epochs and
compared with a literal list.  The position of a method's consolidation between "training ends", "best checkpoint reloaded",
"head grown" and "new optimizer" is its semantics; this is where it is written down."""
import os
import random
import types

import pytest
import torch

from test_si_gpu import _episode_model, _task_data, seed_word_zero  # noqa: F401  (the tiny MQ episode model and its stream)

pytestmark = pytest.mark.gpu

POINTS = ('begin_run', 'begin_task', 'end_training', 'save_state', 'after_reload', 'before_next_task')


def _record(monkeypatch, events, owner, name, label=None):
    """wrap `owner.name` so that a call appends `label` to `events`, then goes through"""
    real = getattr(owner, name)
    label = label or name

    def wrapper(*a, **k):
        events.append(label)
        return real(*a, **k)
    monkeypatch.setattr(owner, name, wrapper)


def _record_run(monkeypatch, events, hook_cls, model, tu, state_file=None):
    """the six points of `hook_cls`, the drivers' own steps and the regularizers' task-boundary calls -> `events`"""
    import pickle
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import hooks, regularizers
    for point in POINTS:
        _record(monkeypatch, events, hook_cls, point, '%s.%s' % (hook_cls.__name__, point))
    _record(monkeypatch, events, tu, 'make_optimizer')
    _record(monkeypatch, events, train_cl, 'load_best_checkpoint')
    _record(monkeypatch, events, model, 'augment_classification')
    for fn in ('si_begin_task', 'on_task_si_update', 'on_task_update', 'rwalk_begin_task', 'on_task_rwalk_update'):
        _record(monkeypatch, events, regularizers, fn)

    def dump(obj, fh):
        events.append('memory pickle')
        return pickle.dump(obj, fh)
    monkeypatch.setattr(train_cl, 'pickle', types.SimpleNamespace(dump=dump))
    if state_file is not None:
        real_save = torch.save

        def save(obj, f, *a, **k):
            if isinstance(f, str) and os.path.basename(f) == state_file:
                events.append('write ' + state_file)
            return real_save(obj, f, *a, **k)
        monkeypatch.setattr(hooks.torch, 'save', save)


def _mq_episode(dev, name, **cl):
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    cfg, model = _episode_model(dev)
    cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], name=name, reg_lambda=1.0, path_memory='memory.pkl', **cl)
    random.seed(0)
    return cfg, model, InMemoryQILStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)


def test_order_of_events_under_si(dev, tmp_path, monkeypatch, seed_word_zero):  # noqa: F811
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import hooks
    cfg, model, stream = _mq_episode(dev, 'si', si_xi=0.1)
    events = []
    _record_run(monkeypatch, events, hooks.SI, model, train_cl)
    model, _, _, log = train_cl.run_episodes(cfg, model, stream, ckpt_folder=str(tmp_path), gpu_id=0)
    torch.cuda.synchronize()
    assert len(log) == 2 and [len(e['history']) for e in log] == [2, 2]
    assert events == [
        'SI.begin_run', 'make_optimizer',
        # task 0: the path integral is attached to the task's optimizer; SI consolidates where training ends, BEFORE the memory
        # pickle and the reload, and installs what it held AFTER the reload and the head growth, before the next optimizer
        'SI.begin_task', 'si_begin_task',
        'SI.end_training', 'on_task_si_update',
        'memory pickle', 'SI.save_state', 'load_best_checkpoint', 'SI.after_reload',
        'augment_classification', 'SI.before_next_task', 'make_optimizer',
        # task 1, the last: nothing follows, nothing is consolidated
        'SI.begin_task', 'si_begin_task',
        'SI.end_training',
        'memory pickle', 'SI.save_state', 'load_best_checkpoint', 'SI.after_reload',
    ], events
    assert len(model.reg_params['importance']) == 1


def test_order_of_events_under_rwalk(dev, tmp_path, monkeypatch, seed_word_zero):  # noqa: F811
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import hooks
    cfg, model, stream = _mq_episode(dev, 'rwalk', rwalk_delta_t=2)
    events = []
    _record_run(monkeypatch, events, hooks.RWalk, model, train_cl, state_file=train_cl.RWALK_STATE_FILE)
    model, _, _, log = train_cl.run_episodes(cfg, model, stream, ckpt_folder=str(tmp_path), gpu_id=0)
    torch.cuda.synchronize()
    assert len(log) == 2 and [len(e['history']) for e in log] == [2, 2]
    assert events == [
        'RWalk.begin_run', 'make_optimizer',
        # task 0: as SI, and the state the next task starts from is written between the memory pickle and the reload
        'RWalk.begin_task', 'rwalk_begin_task',
        'RWalk.end_training', 'on_task_rwalk_update',
        'memory pickle', 'RWalk.save_state', 'write rwalk_state.pt', 'load_best_checkpoint', 'RWalk.after_reload',
        'augment_classification', 'RWalk.before_next_task', 'make_optimizer',
        # task 1, the last: no consolidation, no state file
        'RWalk.begin_task', 'rwalk_begin_task',
        'RWalk.end_training',
        'memory pickle', 'RWalk.save_state', 'load_best_checkpoint', 'RWalk.after_reload',
    ], events
    assert os.path.exists(os.path.join(str(tmp_path), 'rwalk_state.pt')) and len(model.reg_params['importance']) == 1


def test_order_of_events_under_mas_in_the_nlq_driver(dev, tmp_path, monkeypatch):
    import vilco_amd.modeling_nlq as nlq
    from parity_util import cases
    from test_nlq import _gold_episode, _Recorder, _ValTasks
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import hooks
    from vilco_amd.utils import train_utils_nlq as tu
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    mcfg = cases.nlq_model_cfg()
    cfg = {'opt': cases.nlq_episode_opt(0.5), 'train_cfg': mcfg['train_cfg'],
           'cl_cfg': dict(mcfg['cl_cfg'], name='mas', reg_lambda=1.0, memory_size=cases.NLQ_EP_MEMORY, path_memory='mem.pkl')}
    assert cfg['opt']['epochs'] + cfg['opt']['warmup_epochs'] == 2
    model = nlq.make_meta_arch('LocPointTransformer', **mcfg)
    model.load_state_dict(_gold_episode()['init_state'], strict=True)
    model = model.to(dev)
    model.augment_classification = lambda *a, **k: None          # (the NLQ head does not grow: the driver must not ask)
    stream = InMemoryQILStream([cases.nlq_episode_data(j) for j in range(2)], batch_size=cases.NLQ_EP_BATCH, shuffle=False)
    random.seed(0)
    events = []
    _record_run(monkeypatch, events, hooks.Importance, model, tu)
    model, _, _, log = train_cl.run_episodes_nlq(cfg, model, stream, _ValTasks(), _Recorder(), ckpt_folder=str(tmp_path), ckpt_freq=2)
    torch.cuda.synchronize()
    assert len(log) == 2 and [len(e['history']) for e in log] == [2, 2]
    assert events == [
        'Importance.begin_run', 'make_optimizer',
        # task 0: MAS consolidates over the task's loader from the RELOADED best state, before the next optimizer
        'Importance.begin_task',
        'Importance.end_training',
        'memory pickle', 'Importance.save_state', 'load_best_checkpoint', 'Importance.after_reload',
        'Importance.before_next_task', 'on_task_update', 'make_optimizer',
        # task 1, the last
        'Importance.begin_task',
        'Importance.end_training',
        'memory pickle', 'Importance.save_state', 'load_best_checkpoint', 'Importance.after_reload',
    ], events
    assert len(model.reg_params['importance']) == 1 and len(model.reg_params['optpar']) == 1
