"""RWalk without a GPU: the float64 restatement (tests/rwalk_restatement.py) has the properties that define the method, the two C
entry points (vilco_optim_step_rwalk, vilco_rwalk_consolidate) refuse bad arguments before they touch memory, and the Python
layer validates its options, keeps SI and RWalk apart and refuses the resumes it cannot serve."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rwalk_restatement as W
import si_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- the restatement
def _zeros(n):
    return np.zeros(n)


def test_fisher_average_tends_to_the_squared_gradient():
    g = np.array([0.5, -2.0, 0.0, 1e-3])
    F = np.array([3.0, 0.0, 1.0, 0.0])
    for alpha in (0.9, 0.25, 1.0):
        Fk = F
        for k in range(200):
            Fk = W.update(Fk, _zeros(4), _zeros(4), _zeros(4), g, _zeros(4), _zeros(4), alpha, 1e-8, False)[0]
        # F_k - g^2 = (1 - alpha)^k (F_0 - g^2): a geometric approach (exact but for the roundings of 200 double steps)
        left = (1.0 - W.f32(alpha)) ** 200 * np.abs(F - g * g)
        assert np.all(np.abs(Fk - g * g) <= left * (1 + 1e-9) + 1e-13 * g * g), alpha
        assert left.max() < 1e-24
    one = W.update(F, _zeros(4), _zeros(4), _zeros(4), g, _zeros(4), _zeros(4), 1.0, 1e-8, False)[0]
    assert np.array_equal(one, g * g)                    # alpha = 1: the new squared gradient alone


def test_path_integral_is_the_one_of_synaptic_intelligence():
    rng = np.random.default_rng(0)
    w, g, p0, pv = (rng.standard_normal(33) for _ in range(4))
    c = 0.37
    got = W.update(_zeros(33), _zeros(33), w, p0, g * c, p0, pv, 0.9, 1e-8, False)[2]
    want, term = S.path_integral(torch.tensor(w), torch.tensor(g), c, torch.tensor(p0), torch.tensor(pv))
    assert np.allclose(got, want.numpy(), rtol=1e-15, atol=0)
    # a checkpoint scores that very value, then starts the next interval from zero at the new parameter
    F1, s1, w1, ck1, parts = W.update(np.ones(33), np.ones(33), w, p0 - 1.0, g * c, p0, pv, 0.9, 1e-8, True)
    assert np.allclose(parts['w_closed'], want.numpy(), rtol=1e-15, atol=0)
    assert np.array_equal(w1, _zeros(33)) and np.array_equal(ck1, pv)
    assert np.allclose(s1, 1.0 + np.maximum(want.numpy(), 0) / (0.5 * F1 * (pv - p0 + 1.0) ** 2 + W.f32(1e-8)), rtol=1e-14)


def test_scores_are_non_negative_and_untouched_between_checkpoints():
    rng = np.random.default_rng(1)
    n = 64
    F, s, w, ck = _zeros(n), _zeros(n), _zeros(n), rng.standard_normal(n)
    p = ck.copy()
    for it in range(1, 13):
        g = rng.standard_normal(n)
        pv = p + 0.1 * rng.standard_normal(n)               # both signs of gr (pv - p): w takes both signs
        s_before, ck_before = s.copy(), ck.copy()
        F, s, w, ck, _ = W.update(F, s, w, ck, g, p, pv, 0.9, 1e-8, it % 3 == 0)
        p = pv
        if it % 3:
            assert np.array_equal(s, s_before) and np.array_equal(ck, ck_before)
        else:
            assert np.all(s >= s_before) and np.array_equal(w, _zeros(n)) and np.array_equal(ck, p)
        assert np.all(s >= 0) and np.all(F >= 0) and np.all(np.isfinite(s))
    assert s.max() > 0 and (s == 0).sum() < n


def test_consolidation_normalises_into_0_2_and_halves_the_score():
    rng = np.random.default_rng(2)
    sizes = [5, 1, 40]
    ps = [rng.standard_normal(k) for k in sizes]
    Fs = [rng.random(k) for k in sizes]
    ss = [rng.random(k) * 3 for k in sizes]
    ws = [rng.standard_normal(k) for k in sizes]
    cks = [p + 0.1 * rng.standard_normal(p.shape) for p in ps]
    out = W.consolidate(ps, Fs, ss, ws, cks, 1e-8)
    imp = np.concatenate(out['importance'])
    assert imp.min() >= 0 and imp.max() <= 2 and np.isfinite(imp).all()
    assert np.concatenate(out['term_F']).max() == 1.0 and np.concatenate(out['term_s']).max() == 1.0
    for i in range(3):
        assert np.array_equal(out['s'][i], 0.5 * out['s_flushed'][i])                      # halved AFTER the open interval was closed
        assert np.all(out['s_flushed'][i] >= ss[i]) and np.array_equal(out['w'][i], np.zeros(sizes[i]))
        assert np.array_equal(out['optpar'][i], ps[i]) and np.array_equal(out['theta_ck'][i], ps[i])
        assert np.array_equal(out['F'][i], Fs[i])                                          # the moving average runs on
    assert out['maxF'] == max(F.max() for F in Fs)


def test_all_zero_score_contributes_a_finite_zero():
    ps = [np.array([1.0, 2.0]), np.array([3.0])]
    Fs = [np.array([0.5, 0.25]), np.array([1.0])]
    zeros = [np.zeros(2), np.zeros(1)]
    neg = [np.array([-1.0, 0.0]), np.array([-0.5])]          # nothing positive left in the open interval either
    out = W.consolidate(ps, Fs, zeros, neg, ps, 1e-8)
    assert out['maxS'] == 0.0
    assert all(np.array_equal(t, np.zeros_like(t)) for t in out['term_s'])
    assert np.array_equal(np.concatenate(out['importance']), np.array([0.5, 0.25, 1.0]))
    none = W.consolidate(ps, [np.zeros(2), np.zeros(1)], zeros, neg, ps, 1e-8)
    assert np.array_equal(np.concatenate(none['importance']), np.zeros(3))                # 0/0 in neither term


# ------------------------------------------------------------------------------------------------------- C ABI
FAKE = 4096          # a non-null address: every check below fails before anything is dereferenced or launched


def _table(rows, kw):
    from vilco_amd import _lib
    d = dict(ptrs=FAKE, numel=FAKE, chunk_tensor=FAKE, chunk_off=FAKE, rows=rows, n=1, nchunks=1, chunk=S.R.CHUNK)
    d.update({k: kw.pop(k) for k in list(kw) if k in d})
    return _lib.ChunkTable(**d)


def test_optim_step_rwalk_rejects_bad_arguments_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()
    lr = (ctypes.c_float * 1)(1e-3)

    def desc(**kw):
        rw = dict(rw_ptrs=FAKE, tick=FAKE, alpha=0.9, eps=1e-8, delta_t=10)
        rw.update({k: kw.pop(k) for k in list(kw) if k in rw})
        o = dict(table=_table(4, kw), kind=0, group=FAKE, lr=ctypes.addressof(lr), wd=ctypes.addressof(lr), ngroups=1, beta1=0.9,
                 beta2=0.999, eps=1e-8, momentum=0.9, tensor_step=FAKE, si_ptrs=FAKE)
        o.update(kw)
        return _lib.RwalkStepDesc(optim=_lib.OptimDesc(**o), **rw)
    call = lambda d: lib.vilco_optim_step_rwalk(ctypes.byref(d), None)      # noqa: E731
    assert lib.vilco_optim_step_rwalk(None, None) == -1
    for alpha in (0.0, -0.1, 1.5, float('nan')):
        assert call(desc(alpha=alpha)) == -1, alpha
    d = desc()
    d.eps = 0.0
    assert call(d) == -1
    d.eps = -1e-8
    assert call(d) == -1
    d.eps = float('nan')
    assert call(d) == -1
    for dt in (0, -3):
        assert call(desc(delta_t=dt)) == -1, dt
    for missing in ('rw_ptrs', 'tick', 'si_ptrs', 'ptrs', 'numel', 'chunk_tensor', 'chunk_off', 'group', 'tensor_step'):
        assert call(desc(**{missing: None})) == -1, missing
    for bad in (dict(n=-1), dict(chunk=0), dict(kind=2), dict(ngroups=0), dict(rows=3), dict(kind=1, rows=2)):
        assert call(desc(**bad)) == -1, bad
    assert call(desc(nchunks=0)) == 0 and call(desc(alpha=1.0, delta_t=1, nchunks=0)) == 0      # legal, nothing to launch
    assert ctypes.sizeof(_lib.RwalkStepDesc) == lib.vilco_abi_sizeof(b"vilco_rwalk_step_desc") > ctypes.sizeof(_lib.OptimDesc)
    assert _lib.RwalkStepDesc._fields_[0] == ("optim", _lib.OptimDesc) and _lib.OptimDesc._fields_[-1][0] == "si_ptrs"


def test_rwalk_consolidate_rejects_bad_arguments_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()

    def desc(**kw):
        f = dict(out_ptrs=FAKE, partial=FAKE, out=FAKE, eps=1e-8)
        f.update({k: kw.pop(k) for k in list(kw) if k in f})
        return _lib.RwalkDesc(table=_table(5, kw), **f)
    call = lambda d: lib.vilco_rwalk_consolidate(ctypes.byref(d), None)      # noqa: E731
    assert lib.vilco_rwalk_consolidate(None, None) == -1
    for missing in ('ptrs', 'numel', 'chunk_tensor', 'chunk_off', 'out_ptrs', 'partial', 'out'):
        assert call(desc(**{missing: None})) == -1, missing
    for eps in (0.0, -1.0, float('nan')):
        assert call(desc(eps=eps)) == -1, eps
    for bad in (dict(n=0), dict(n=-1), dict(chunk=0), dict(nchunks=-1), dict(rows=4)):
        assert call(desc(**bad)) == -1, bad
    assert call(desc(nchunks=0)) == 0
    assert ctypes.sizeof(_lib.RwalkDesc) == lib.vilco_abi_sizeof(b"vilco_rwalk_desc") > 0
    assert _lib.RwalkDesc._fields_[0] == ("table", _lib.ChunkTable)


def test_header_and_ctypes_table_agree_on_the_new_entries():
    from vilco_amd import _lib
    text = open(os.path.join(ROOT, "include", "vilco_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, mirror in (("vilco_rwalk_step_desc", _lib.RwalkStepDesc), ("vilco_rwalk_desc", _lib.RwalkDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        fields = [re.split(r"[\s*]+", decl.strip())[-1] for decl in body.split(";") if decl.strip()]
        assert fields == [f for f, _ in mirror._fields_], name
    assert re.search(r"int vilco_optim_step_rwalk\(const vilco_rwalk_step_desc\* d, void\* stream\);", text)
    assert re.search(r"int vilco_rwalk_consolidate\(const vilco_rwalk_desc\* d, void\* stream\);", text)
    assert "vilco_optim_step_rwalk" in _lib.SIGNATURES and "vilco_rwalk_consolidate" in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "vilco_optim_step_rwalk") and hasattr(lib, "vilco_rwalk_consolidate")


# ------------------------------------------------------------------------------------------------------- Python layer
def test_defaults_live_in_extra_defaults():
    from vilco_amd.core import config as c
    want = {'rwalk_alpha': 0.9, 'rwalk_delta_t': 10, 'rwalk_eps': 1e-8}
    for k, v in want.items():
        assert c.EXTRA_DEFAULTS['cl_cfg'][k] == v and k not in c.DEFAULTS['cl_cfg']
    ref_defaults = torch.load(os.path.join(ROOT, "tests", "golden", "config_defaults.pt"), weights_only=False)
    assert c.DEFAULTS == ref_defaults
    got = c.make_config(cl_cfg=dict(name='rwalk', rwalk_delta_t=3))['cl_cfg']
    assert got['rwalk_delta_t'] == 3 and got['rwalk_alpha'] == 0.9 and got['rwalk_eps'] == 1e-8


def test_rwalk_options_validate_early():
    from vilco_amd.cl_methods import regularizers as reg
    assert reg.rwalk_options({}) == dict(alpha=0.9, delta_t=10, eps=1e-8)
    assert reg.rwalk_options({'rwalk_alpha': 1.0, 'rwalk_delta_t': 1, 'rwalk_eps': 0.5}) == dict(alpha=1.0, delta_t=1, eps=0.5)
    for bad in ({'rwalk_alpha': 0.0}, {'rwalk_alpha': 1.01}, {'rwalk_alpha': float('nan')}, {'rwalk_delta_t': 0},
                {'rwalk_delta_t': 2.5}, {'rwalk_delta_t': True}, {'rwalk_eps': 0.0}, {'rwalk_eps': -1e-8}, {'rwalk_eps': float('nan')}):
        with pytest.raises(ValueError, match="rwalk_"):
            reg.rwalk_options(bad)


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.body = torch.nn.Linear(3, 2)
        self.head = torch.nn.Linear(3, 5)
        self.scale = torch.nn.Parameter(torch.ones(1))
        self.reg_params = {}


def test_entries_accept_the_kind_rwalk():
    from vilco_amd.cl_methods import regularizers as reg
    m = _Stub()
    assert reg._entries(m, 'rwalk') == []
    imp = {'body.weight': torch.rand(2, 3), 'head.weight': torch.rand(4, 3), 'scale': torch.rand(1)}
    m.reg_params = {'importance': [imp], 'optpar': [{k: torch.randn_like(v) for k, v in imp.items()}]}
    got = reg._entries(m, 'rwalk')
    assert [p is q for (p, _, _), q in zip(got, (m.body.weight, m.head.weight))] == [True, True] and len(got) == 2
    assert len(reg._entries(m, 'si')) == 2
    with pytest.raises(ValueError):
        reg._entries(m, 'rwalks')


def test_si_and_rwalk_do_not_attach_together():
    from vilco_amd.utils.train_utils import FusedOptimizer
    p = torch.nn.Parameter(torch.zeros(3))
    opt = FusedOptimizer([p], lr=1e-3)
    gen = (opt.si_gen, opt.rwalk_gen)
    opt.attach_si({})
    with pytest.raises(RuntimeError, match="Synaptic Intelligence"):
        opt.attach_rwalk({})
    opt.attach_si(None)
    # nothing to track is a detach: the update kernel dereferences the tick in every block, so an attachment must own a DEVICE
    # word, and without a state tensor there is no device to put one on -- no host address may ever reach the launch
    opt.attach_rwalk({}, alpha=0.5, delta_t=2, eps=1e-6)
    assert opt._rwalk is None and opt.rwalk_tick is None, "an empty attachment must leave nothing attached"
    assert opt.rwalk_gen == gen[1] + 1 and opt.si_gen == gen[0] + 2
    assert 'rwalk' not in str(sorted(opt.state_dict()))
    for bad in (dict(alpha=0.0), dict(delta_t=0), dict(eps=0.0)):
        with pytest.raises(ValueError):
            opt.attach_rwalk({}, **bad)
    # state tensors in host memory are refused before anything is attached
    host = {p: {k: torch.zeros(3) for k in ('fisher', 'score', 'omega', 'theta_ck')}}
    with pytest.raises(RuntimeError, match="device tensor"):
        opt.attach_rwalk(host)
    assert opt._rwalk is None and opt.rwalk_tick is None
    opt.attach_rwalk(None)
    assert opt.rwalk_tick is None and opt.rwalk_gen == gen[1] + 2
    opt.attach_si({})                                      # detached: SI may attach again


def test_a_model_without_regularised_parameters_attaches_nothing():
    from vilco_amd.cl_methods import regularizers as reg
    from vilco_amd.utils.train_utils import FusedOptimizer

    class OnlyScale(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.scale = torch.nn.Parameter(torch.ones(2))
            self.frozen = torch.nn.Parameter(torch.ones(2), requires_grad=False)
            self.reg_params = {}
    m = OnlyScale()
    opt = FusedOptimizer([m.scale], lr=1e-3)
    assert reg.rwalk_begin_task(m, opt) == {} and opt._rwalk is None and opt.rwalk_tick is None
    out = reg.on_task_rwalk_update(m, opt)
    assert out == {'importance': [{}], 'optpar': [{}]} and reg._entries(m, 'rwalk') == []
    with pytest.raises(RuntimeError, match="rwalk_begin_task"):
        reg.on_task_rwalk_update(OnlyScale())


def test_driver_refuses_the_resumes_it_cannot_serve(tmp_path):
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import hooks

    def rwalk_check(cfg, start_epoch, model=None, start_task=0, ckpt_folder=None):
        """RWalk's hook through begin_run -> its options; None when cl_cfg names another method"""
        if cfg['cl_cfg']['name'] != 'rwalk':
            return None
        hook = hooks.RWalk(cfg)
        hook.begin_run(model, None, start_task, start_epoch, ckpt_folder)
        return hook.opts
    cfg = {'cl_cfg': {'name': 'rwalk'}}
    assert [type(h) for h in hooks.make_hooks(cfg, 'run_episodes')] == [hooks.RWalk]
    assert rwalk_check(cfg, 0) == dict(alpha=0.9, delta_t=10, eps=1e-8)
    assert rwalk_check({'cl_cfg': {'name': 'si'}}, 3) is None
    assert not any(isinstance(h, hooks.RWalk) for h in hooks.make_hooks({'cl_cfg': {'name': 'si'}}, 'run_episodes'))
    with pytest.raises(ValueError, match="start_epoch"):
        rwalk_check(cfg, 1)
    with pytest.raises(ValueError, match="rwalk_delta_t"):
        rwalk_check({'cl_cfg': {'name': 'rwalk', 'rwalk_delta_t': 0}}, 0)
    # a resume at a later task needs the Fisher average and the scores of the earlier ones
    assert train_cl.RWALK_STATE_FILE == 'rwalk_state.pt'
    for folder in (None, str(tmp_path)):
        with pytest.raises(ValueError, match="rwalk_state.pt"):
            rwalk_check(cfg, 0, model=_Stub(), start_task=1, ckpt_folder=folder)
    with pytest.raises(ValueError, match="rwalk_state.pt"):
        train_cl.run_episodes(cfg, _Stub(), None, ckpt_folder=str(tmp_path), start_task=1)
    with pytest.raises(ValueError, match="start_epoch"):
        train_cl.run_episodes(cfg, _Stub(), None, start_epoch=2)
    with pytest.raises(ValueError, match="run_episodes_bic"):
        train_cl.run_episodes_bic(cfg, _Stub(), None)
    # with the file the state comes back, to be carried by the next rwalk_begin_task
    from vilco_amd.cl_methods import regularizers as reg
    m = _Stub()
    m.rwalk_state = {'body.weight': {'fisher': torch.rand(2, 3), 'score': torch.rand(2, 3), 'omega': torch.zeros(2, 3),
                                     'theta_ck': torch.zeros(2, 3)}}
    sd = reg.rwalk_state_dict(m)
    assert sorted(sd) == ['fisher', 'score'] and sorted(sd['fisher']) == ['body.weight']
    torch.save(sd, os.path.join(str(tmp_path), 'rwalk_state.pt'))
    m2 = _Stub()
    m2.device = torch.device('cpu')
    assert rwalk_check(cfg, 0, model=m2, start_task=1, ckpt_folder=str(tmp_path))['delta_t'] == 10
    assert torch.equal(m2.rwalk_state['body.weight']['fisher'], m.rwalk_state['body.weight']['fisher'])
    assert torch.equal(m2.rwalk_state['body.weight']['score'], m.rwalk_state['body.weight']['score'])
    with pytest.raises(ValueError):
        reg.load_rwalk_state(m2, {'fisher': {}})
