"""CPU: pooled feature distillation's Python layer (vilco_amd/cl_methods/pod.py) -- the tensor-op body of the term against the
float64 restatement (tests/pod_restatement.py) and against finite differences, the bank's bookkeeping, what the hooks accept and
refuse, the model's 'pod' branch on CPU tensors, the C ABI rows and the host-side argument checks of vilco_pod_* (they come
before any device work, so dummy addresses do)."""
import ctypes
import os
import types

import pytest
import torch

import pod_restatement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (8, 4, 2, 1)
VALID = [[8, 4, 2, 1], [5, 3, 1, 0], [3, 0, 0, 0]]


def _clip(vid, length=13, labels=(0,)):
    return {'video_id': vid, 'feats': torch.zeros(4, length), 'labels': torch.tensor(labels)}


def _case(C, seed=0, dtype=torch.float64):
    """B = 3 over LEVELS: rows 0 and 2 have independent random (normalised, non-negative) records, row 1 has none"""
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(3, T, C, generator=g, dtype=torch.float64).to(dtype) for T in LEVELS]
    recs = []
    for b in range(3):
        other = [torch.randn(T, C, generator=g, dtype=torch.float64) for T in LEVELS]
        recs.append(P.make_record(other, VALID[b]).to(dtype))
    recs[1] = None
    return feats, recs


@pytest.mark.parametrize("C", [1, 5, 22])
def test_tensor_op_body_equals_the_restatement(C):
    from vilco_amd.cl_methods import pod
    feats, recs = _case(C, seed=C)
    want = P.pod_term(feats, VALID, recs, 1.7, g_out=1.0)
    xs = [f.clone().requires_grad_(True) for f in feats]
    loss, n = pod.pod_term(xs, torch.tensor(VALID, dtype=torch.int32), recs, 1.7)
    loss.backward()
    assert n == want['n_rec'] == 2 and want['loss'] > 0
    assert abs(float(loss) - want['loss']) <= 1e-12 * want['loss']
    for x, g, m in zip(xs, want['grads'], want['compared']):
        assert torch.allclose(x.grad, g, rtol=1e-10, atol=1e-14)
        assert bool((x.grad[~m] == 0).all())
    assert any(bool((x.grad != 0).any()) for x in xs)
    # fp32, as a CPU model would run it
    x32 = [f.float().requires_grad_(True) for f in feats]
    loss32, _ = pod.pod_term(x32, VALID, [None if r is None else r.float() for r in recs], 1.7)
    loss32.backward()
    assert abs(float(loss32) - want['loss']) <= 1e-5 * want['loss']
    # nothing to compare: an exact zero that still backpropagates (zeros)
    zero, n0 = pod.pod_term(xs, VALID, [None, None, None], 1.7)
    assert float(zero) == 0.0 and n0 == 0 and zero.requires_grad
    none = P.pod_term(feats, VALID, [None, None, None], 1.7)
    assert none['loss'] == 0.0 and none['n_rec'] == 0 and all(bool((g == 0).all()) for g in none['grads'])


def test_tensor_op_body_against_finite_differences():
    from vilco_amd.cl_methods import pod
    feats, recs = _case(3, seed=7)
    xs = [f.clone().requires_grad_(True) for f in feats]
    assert torch.autograd.gradcheck(lambda *a: pod.pod_term(list(a), VALID, recs, 0.9)[0], xs, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_a_clip_against_its_own_record_has_zero_distance_and_gradient():
    from vilco_amd.cl_methods import pod
    feats, _ = _case(5, seed=9)
    lens = torch.tensor(VALID, dtype=torch.int32)
    rec = pod.pooled_records(feats, lens)
    for b in range(3):
        assert torch.allclose(rec[b], P.make_record([f[b] for f in feats], VALID[b]), rtol=1e-12, atol=0.0)
    xs = [f.clone().requires_grad_(True) for f in feats]
    loss, n = pod.pod_term(xs, lens, list(rec), 2.0)
    loss.backward()
    assert n == 3 and float(loss) == 0.0
    assert all(bool((x.grad == 0).all()) and bool(torch.isfinite(x.grad).all()) for x in xs)
    want = P.pod_term(feats, VALID, list(rec), 2.0)
    assert want['loss'] == 0.0 and all(bool((g == 0).all()) for g in want['grads'])


def test_bank_keep_skip_and_length_mismatch_rules():
    from vilco_amd.cl_methods.pod import PODBank, empty_table
    C = 5
    W = sum(C + T for T in LEVELS)
    bank = PODBank()
    va = torch.arange(W, dtype=torch.float32)
    bank.record('a', va, 13, LEVELS, C)
    bank.record('c', torch.ones(W), 13, LEVELS, C)
    assert len(bank) == 2 and 'a' in bank and 'x' not in bank
    buf, n, lv, c = bank.get('a')
    assert buf.data_ptr() != va.data_ptr() and torch.equal(buf, va) and (n, lv, c) == (13, LEVELS, C)
    assert buf.dtype == torch.float32 and buf.is_contiguous() and buf.dim() == 1
    batch = [_clip('a'), _clip('x'), _clip('c')]
    tab = bank.table_for(batch, [13, 13, 13])
    assert tab.dtype == torch.int64 and tuple(tab.shape) == (3,)
    assert tab.tolist() == [bank.get('a')[0].data_ptr(), 0, bank.get('c')[0].data_ptr()]
    assert bank.skipped == 0, "a clip that is not in the bank is not a skipped record"
    tab = bank.table_for(batch, [13, 13, 12])                     # a re-cropped clip: another length in this step
    assert tab[2] == 0 and tab[0] != 0 and bank.skipped == 1
    assert bank.table_for(batch, [13, 13, 13], level_T=(8, 4, 2, 2)).tolist() == [0, 0, 0] and bank.skipped == 3
    assert bank.table_for(batch, [13, 13, 13], level_T=LEVELS, C=C + 1).tolist() == [0, 0, 0] and bank.skipped == 5
    assert bank.table_for(batch, [13, 13, 13], level_T=LEVELS, C=C)[0] != 0 and bank.skipped == 5
    with pytest.raises(ValueError):
        bank.record('d', torch.ones(W - 1), 13, LEVELS, C)
    ptr = bank.get('c')[0].data_ptr()
    bank.record('a', torch.zeros(W), 13, LEVELS, C)               # recorded again (the next task): replaced, the others stay put
    assert bank.get('c')[0].data_ptr() == ptr and float(bank.get('a')[0].sum()) == 0.0
    bank.clear()
    assert len(bank) == 0
    assert empty_table(4, 'cpu').tolist() == [0, 0, 0, 0]


def test_step_table_is_all_zero_without_known_classes_or_bank():
    from vilco_amd.cl_methods import pod
    C = 3
    bank = pod.PODBank()
    bank.record('a', torch.ones(sum(C + T for T in LEVELS)), 13, LEVELS, C)
    batch = [_clip('a'), _clip('u', labels=()), _clip('x')]          # the unlabelled clip is no row of the step
    model = types.SimpleNamespace(pod_bank=bank, n_known=0, device=torch.device('cpu'), _der_levels=lambda: LEVELS)
    assert pod.step_table(model, batch).tolist() == [0, 0]
    model.n_known = 2
    assert pod.step_table(model, batch).tolist() == [bank.get('a')[0].data_ptr(), 0]
    model.pod_bank = None
    assert pod.step_table(model, batch).tolist() == [0, 0]


def test_adaptive_scale():
    from vilco_amd.cl_methods import pod
    assert pod.adaptive_scale(1.0, 4, 0) == 1.0
    assert abs(pod.adaptive_scale(3.0, 8, 6) - 6.0) < 1e-15
    with pytest.raises(ValueError):
        pod.adaptive_scale(1.0, 4, 4)


def _cfg(**cl):
    from vilco_amd.core.config import make_config
    cfg = make_config()
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], name='pod', type_sampling='random', **cl)
    return cfg


def test_make_hooks_accepts_pod_under_run_episodes_and_refuses_the_rest():
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import hooks, pod
    from vilco_amd.core import config as c
    assert c.EXTRA_DEFAULTS['cl_cfg']['pod_lambda'] == 1.0 and 'pod_lambda' not in c.DEFAULTS['cl_cfg']
    assert hooks.support('pod') == hooks.SUPPORT_MORE['pod'] == ({hooks.MQ: hooks.HOOKS}, False) and hooks.NAMED['pod'] is hooks.POD
    assert hooks.support('der') is hooks.SUPPORT['der'] and 'pod' not in hooks.SUPPORT
    made = hooks.make_hooks(_cfg(), 'run_episodes')
    assert len(made) == 1 and isinstance(made[0], hooks.POD)
    for driver in ('run_episodes_bic', 'run_episodes_nlq'):
        with pytest.raises(ValueError, match=driver):
            hooks.make_hooks(_cfg(), driver)
        assert pod.check_supported('der', driver=driver) is False, "other methods are not this module's business"
    with pytest.raises(ValueError, match="run_episodes_bic"):
        train_cl.run_episodes_bic(_cfg(), None, None)
    with pytest.raises(ValueError, match="run_episodes_nlq"):
        train_cl.run_episodes_nlq(_cfg(), None, None, None, None)
    model = types.SimpleNamespace(pod_lambda=1.0, pod_bank=None)
    with pytest.raises(ValueError, match="data parallelism"):
        train_cl.run_episodes(_cfg(), model, None, reducer=object())
    with pytest.raises(ValueError, match="icarl"):
        train_cl.run_episodes(dict(_cfg(), cl_cfg=dict(_cfg()['cl_cfg'], type_sampling='icarl')), model, None)
    with pytest.raises(ValueError, match="start_epoch"):
        train_cl.run_episodes(_cfg(), model, None, start_epoch=1)
    with pytest.raises(ValueError, match="pod_lambda"):
        hooks.POD(_cfg(pod_lambda=-1.0)).begin_run(model, None)
    assert model.pod_bank is None, "a refused run leaves the model alone"
    h = hooks.POD(_cfg(pod_lambda=0.5))
    h.begin_run(model, None, start_task=1)                          # a resume at a task boundary needs no state file
    assert model.pod_lambda == 0.5 and isinstance(model.pod_bank, pod.PODBank)


def test_begin_task_records_only_with_known_classes(monkeypatch):
    from vilco_amd.cl_methods import hooks, pod
    calls = []
    monkeypatch.setattr(pod, 'record_clips', lambda model, bank, loader, j: calls.append((len(bank), loader, j)) or 7)
    bank = pod.PODBank()
    bank.record('old', torch.ones(4), 3, (1,), 3)
    model = types.SimpleNamespace(pod_lambda=1.0, pod_bank=bank, n_known=0)
    h = hooks.POD(_cfg())
    entry = {}
    assert h.begin_task(0, model, None, 'loader0', entry) is None and entry == {} and calls == [] and len(bank) == 1
    model.n_known = 2
    h.begin_task(1, model, None, 'loader1', entry)
    assert entry == {'pod_recorded': 7} and calls == [(0, 'loader1', 1)], "the bank is cleared before the task's clips are recorded"


def test_model_branch_on_cpu_tensors_goes_through_the_bank():
    """PtTransformer._cl_terms' 'pod' branch on CPU tensors: records looked up by video_id, another length skipped, the
    adaptive factor from the head's width; equal to pod_term"""
    from vilco_amd.cl_methods import pod
    from vilco_amd.modeling.meta_archs import PtTransformer
    C = 5
    feats, recs = _case(C, seed=3, dtype=torch.float32)
    bank = pod.PODBank()
    bank.record('a', recs[0], 13, LEVELS, C)
    bank.record('c', recs[2], 13, LEVELS, C)
    batch = [_clip('a'), _clip('x'), _clip('c')]
    head = types.SimpleNamespace(cls_head=types.SimpleNamespace(conv=types.SimpleNamespace(out_channels=8)))
    stub = types.SimpleNamespace(pod_bank=bank, pod_lambda=0.5, n_known=6, cl_name='pod', cls_head=head, _pod_tab_step=(None, batch))
    stub._pod_loss = types.MethodType(PtTransformer._pod_loss, stub)
    lens = torch.tensor(VALID, dtype=torch.int32)
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), [], [], None, level_len=lens, fpn_feats=feats)
    scale = 0.5 * 2.0
    body = float(pod.pod_term(feats, lens, recs, scale)[0])
    want = P.pod_term(feats, VALID, recs, scale)['loss']
    assert float(out['pod_loss']) == body and abs(body - want) <= 1e-5 * want
    assert abs(float(out['final_loss']) - 1.0 - want) <= 1e-5
    batch[2] = _clip('c', 12)
    stub._pod_tab_step = (None, batch)
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), [], [], None, level_len=lens, fpn_feats=feats)
    want = P.pod_term(feats, VALID, [recs[0], None, None], scale)['loss']
    assert abs(float(out['pod_loss']) - want) <= 1e-5 * want and bank.skipped == 1
    stub.n_known = 0                                                # without known classes the method adds nothing
    assert 'pod_loss' not in PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), [], [], None, level_len=lens, fpn_feats=feats)


def test_step_inputs_carry_the_table_slot():
    from vilco_amd.modeling.meta_archs import StepInputs
    assert "pod_tab" in StepInputs.__slots__ and "pod_tab" not in StepInputs.HOST
    inp = StepInputs()
    for k in StepInputs.__slots__:
        setattr(inp, k, None)
    inp.feats_cf, inp.pod_tab = torch.zeros(2, 4, 8), torch.zeros(2, dtype=torch.int64)
    assert [k for k, _ in inp.tensors()] == ["feats_cf", "pod_tab"] and ("pod_tab", (2,)) in inp.signature()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from vilco_amd import ops
    feats, _ = _case(3, dtype=torch.float32)
    lens = torch.tensor(VALID, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pod_distill(feats, lens, torch.zeros(3, dtype=torch.int64), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pod_record(feats, lens)
    with pytest.raises(ValueError, match="1 to 16 levels"):
        ops.pod_distill([], lens, torch.zeros(3, dtype=torch.int64), 1.0)
    with pytest.raises(ValueError, match="1 to 16 levels"):
        ops.pod_record(feats * 5, lens)
    assert ops.pod_record_width(LEVELS, 3) == 4 * 3 + sum(LEVELS)


def test_cabi_rows_exist():
    from vilco_amd import _lib
    text = open(os.path.join(ROOT, "include", "vilco_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("vilco_pod_workspace", "vilco_pod_fwd", "vilco_pod_bwd", "vilco_pod_record", "vilco_pod_tile_rows"):
        assert n in _lib.SIGNATURES and n + "(" in text and hasattr(lib, n), n
    assert _lib.PodDesc._cname_ == "vilco_pod_desc" and "} vilco_pod_desc;" in text
    assert ctypes.sizeof(_lib.PodDesc) == _lib.load().vilco_abi_sizeof(b"vilco_pod_desc") == 56
    assert _lib.load().vilco_pod_tile_rows() >= 1


def test_entry_points_validate_on_the_host():
    """null pointers, L outside 1..16, B < 1, C < 1, T_l < 1, a short workspace: refused before anything is enqueued"""
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                                             # dummy, suitably aligned addresses
    lens = (ctypes.c_int32 * 17)(*([8, 4] + [1] * 15))
    ptrs = (_lib.c_fp * 17)(*([x] * 17))
    ok = dict(feats=ctypes.addressof(ptrs), level_T=ctypes.addressof(lens), level_len=x, pod_tab=x, B=3, C=5, L=2, scale=1.0)
    nws = lib.vilco_pod_workspace(lens, 2, 3, 5)
    assert nws >= 256 + 8 + 8 * 3 * 2 + 8 * 3 * (2 * 5 + 12)
    assert lib.vilco_pod_workspace(lens, 0, 3, 5) == 0 and lib.vilco_pod_workspace(lens, 17, 3, 5) == 0
    assert lib.vilco_pod_workspace(lens, 2, 0, 5) == 0 and lib.vilco_pod_workspace(lens, 2, 3, 0) == 0
    assert lib.vilco_pod_workspace(None, 2, 3, 5) == 0 and lib.vilco_pod_workspace(lens, 16, 3, 5) > nws

    def fwd(ws=x, out=x, nbytes=nws, **kw):
        return lib.vilco_pod_fwd(ctypes.byref(_lib.PodDesc(**dict(ok, **kw))), out, ws, nbytes, None)

    def bwd(ws=x, g=x, dl=ptrs, nbytes=nws, **kw):
        return lib.vilco_pod_bwd(ctypes.byref(_lib.PodDesc(**dict(ok, **kw))), g, dl, ws, nbytes, None)

    def rec(ws=x, out=x, nbytes=nws, **kw):
        return lib.vilco_pod_record(ctypes.byref(_lib.PodDesc(**dict(ok, **kw))), out, ws, nbytes, None)
    zero = (ctypes.c_int32 * 2)(8, 0)
    hole = (_lib.c_fp * 2)(x, 0)
    for call in (fwd, bwd, rec):
        for bad in (dict(feats=None), dict(level_T=None), dict(level_len=None), dict(L=0), dict(L=-1), dict(L=17), dict(B=0),
                    dict(B=-2), dict(C=0), dict(ws=None), dict(level_T=ctypes.addressof(zero)), dict(feats=ctypes.addressof(hole))):
            assert call(**bad) == -1, (call.__name__, bad)
        assert call(nbytes=nws - 1) == -4, call.__name__
    assert fwd(pod_tab=None) == -1 and bwd(pod_tab=None) == -1
    assert lib.vilco_pod_fwd(None, x, x, nws, None) == -1 and lib.vilco_pod_record(None, x, x, nws, None) == -1
    assert lib.vilco_pod_bwd(None, x, ptrs, x, nws, None) == -1
    assert fwd(out=None) == -1 and rec(out=None) == -1 and bwd(g=None) == -1 and bwd(dl=None) == -1 and bwd(dl=hole) == -1
