"""CPU: Dark Experience Replay's Python layer (vilco_amd/cl_methods/der.py) -- what it refuses, the bank's bookkeeping, the
config default, the tensor-op body of the term against the float64 restatement (tests/der_restatement.py), the C ABI rows and
the host-side argument checks of vilco_der_fwd / _bwd (they come before any device work, so dummy addresses do)."""
import ctypes
import os
import types

import pytest
import torch

import der_restatement as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (8, 4, 2, 1)


def _clip(vid, length=13, labels=(0,)):
    return {'video_id': vid, 'feats': torch.zeros(4, length), 'labels': torch.tensor(labels)}


def _record(n, seed=0, rows=sum(LEVELS)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, n, generator=g)


def test_check_supported_refusals():
    from vilco_amd.cl_methods import der
    assert der.check_supported('icarl') is False and der.check_supported(None) is False
    assert der.check_supported('der') is True
    assert der.check_supported('der', type_sampling='random') is True
    for driver in ('run_episodes_bic', 'run_episodes_nlq'):
        with pytest.raises(ValueError, match=driver):
            der.check_supported('der', driver=driver)
        assert der.check_supported('agem', driver=driver) is False, "other methods are not this module's business"
    with pytest.raises(ValueError, match="data parallelism"):
        der.check_supported('der', reducer=object())
    with pytest.raises(ValueError, match="icarl"):
        der.check_supported('der', type_sampling='icarl')


def test_drivers_refuse_der_before_touching_the_stream():
    from vilco_amd import train_cl
    from vilco_amd.core.config import make_config
    cfg = make_config()
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], name='der', type_sampling='random')
    with pytest.raises(ValueError, match="run_episodes_bic"):
        train_cl.run_episodes_bic(cfg, None, None)
    with pytest.raises(ValueError, match="run_episodes_nlq"):
        train_cl.run_episodes_nlq(cfg, None, None, None, None)
    with pytest.raises(ValueError, match="icarl"):
        train_cl.run_episodes(dict(cfg, cl_cfg=dict(cfg['cl_cfg'], type_sampling='icarl')), None, None)
    with pytest.raises(ValueError, match="data parallelism"):
        train_cl.run_episodes(cfg, None, None, reducer=object())


def test_resume_without_a_bank_file_raises(tmp_path):
    from vilco_amd import train_cl
    from vilco_amd.core.config import make_config
    cfg = make_config()
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], name='der', type_sampling='random')
    model = types.SimpleNamespace(der_alpha=0.1, der_bank=None)
    for folder in (None, str(tmp_path)):
        with pytest.raises(ValueError, match="recorded logits"):
            train_cl.run_episodes(cfg, model, None, ckpt_folder=folder, start_task=1)


def test_config_defaults_carry_der_alpha():
    from vilco_amd.core import config as c
    cfg = c.make_config()
    assert cfg['cl_cfg']['der_alpha'] == 0.1 and cfg['model']['cl_cfg']['der_alpha'] == 0.1
    assert c.make_config(cl_cfg=dict(der_alpha=0.5))['cl_cfg']['der_alpha'] == 0.5
    assert c.EXTRA_DEFAULTS['cl_cfg']['der_alpha'] == 0.1 and 'der_alpha' not in c.DEFAULTS['cl_cfg']


def test_bank_keeps_records_across_tasks_and_drops_evicted_clips():
    from vilco_amd.cl_methods.der import DERBank
    bank = DERBank()
    a, b, c = _clip('a'), _clip('b', 9), _clip('c')
    za = _record(2, 1)
    assert bank.record('a', za, 13, LEVELS) is True
    assert bank.record('b', list(_record(2, 2).split(list(LEVELS))), 9, LEVELS) is True, "the per-level list is taken too"
    assert len(bank) == 2 and 'a' in bank and 'c' not in bank
    ptr = bank.get('a')[0].data_ptr()
    assert ptr != za.data_ptr(), "the bank owns its buffers"
    # a later task (the head has grown to 3 classes): the clip recorded earlier keeps its record
    assert bank.record('a', _record(3, 3), 13, LEVELS) is False
    assert bank.get('a')[0].data_ptr() == ptr and torch.equal(bank.get('a')[0], za) and bank.get('a')[0].shape[1] == 2
    assert bank.record('c', _record(3, 4), 13, LEVELS) is True
    # eviction: 'b' left the memory
    assert bank.drop_missing({0: [a], 1: [c, a]}) == 1
    assert sorted(bank.records) == ['a', 'c'] and bank.get('a')[0].data_ptr() == ptr
    assert bank.drop_missing({0: [a], 1: [c]}) == 0
    with pytest.raises(ValueError):
        bank.record('d', _record(2, 5, rows=7), 13, LEVELS)


def test_table_names_records_and_skips_another_length():
    from vilco_amd.cl_methods.der import DERBank
    bank = DERBank()
    bank.record('a', _record(2, 1), 13, LEVELS)
    bank.record('c', _record(3, 4), 13, LEVELS)
    batch = [_clip('a'), _clip('x'), _clip('c')]
    tab = bank.table_for(batch, [13, 13, 13])
    assert tab.dtype == torch.int64 and tuple(tab.shape) == (3, 2)
    assert tab.tolist() == [[bank.get('a')[0].data_ptr(), 2], [0, 0], [bank.get('c')[0].data_ptr(), 3]]
    assert bank.skipped == 0, "a clip that is not in the bank is not a skipped record"
    # a re-cropped long clip: another length in this step -> address 0, counted
    tab = bank.table_for(batch, [13, 13, 12])
    assert tab[2].tolist() == [0, 0] and tab[0, 0] != 0 and bank.skipped == 1
    # records made with another level layout are not usable either
    tab = bank.table_for(batch, [13, 13, 13], level_T=(8, 4, 2, 2))
    assert tab[:, 0].tolist() == [0, 0, 0] and bank.skipped == 3
    assert bank.table_for(batch, [13, 13, 13], level_T=LEVELS)[:, 1].tolist() == [2, 0, 3] and bank.skipped == 3


def test_step_table_is_all_zero_without_known_classes_or_bank():
    from vilco_amd.cl_methods import der
    bank = der.DERBank()
    bank.record('a', _record(2, 1), 13, LEVELS)
    batch = [_clip('a'), _clip('u', labels=()), _clip('x')]          # the unlabelled clip is no row of the step
    model = types.SimpleNamespace(der_bank=bank, n_known=0, device=torch.device('cpu'))
    assert der.step_table(model, batch).tolist() == [[0, 0], [0, 0]]
    model.n_known = 2
    assert der.step_table(model, batch).tolist() == [[bank.get('a')[0].data_ptr(), 2], [0, 0]]
    model.der_bank = None
    assert der.step_table(model, batch).tolist() == [[0, 0], [0, 0]]
    assert bank.skipped == 0


def test_state_dict_round_trip():
    from vilco_amd.cl_methods.der import DERBank
    bank = DERBank()
    bank.record('a', _record(2, 1), 13, LEVELS)
    bank.record('c', _record(3, 4), 11, LEVELS)
    bank.table_for([_clip('a')], [5])
    state = bank.state_dict()
    import io
    f = io.BytesIO()
    torch.save(state, f)
    f.seek(0)
    other = DERBank().load_state_dict(torch.load(f, weights_only=False))
    assert sorted(other.records) == ['a', 'c'] and other.skipped == bank.skipped == 1
    for k in bank.records:
        (b0, n0, l0), (b1, n1, l1) = bank.get(k), other.get(k)
        assert torch.equal(b0, b1) and b0.data_ptr() != b1.data_ptr() and (n0, l0) == (n1, l1)
        assert b1.dtype == torch.float32 and b1.is_contiguous()


def _case(C, seed=0):
    """B = 3 over LEVELS with separator rows: row 0 a full record of C - 1 (or 1) classes, row 1 none, row 2 a record of C classes
    on a clip so short that only the first two levels have valid positions"""
    g = torch.Generator().manual_seed(seed)
    level_row, r = [], 0
    for T in LEVELS:
        level_row.append(r)
        r += T + 1                        # one separator row behind every level
    x = torch.randn(3, r, C, generator=g)
    records = [torch.randn(sum(LEVELS), max(C - 1, 1), generator=g), None, torch.randn(sum(LEVELS), C, generator=g)]
    valid = [[8, 4, 2, 1], [8, 4, 2, 1], [3, 1, 0, 0]]
    return x, level_row, records, valid


@pytest.mark.parametrize("C", [1, 3, 22])
def test_tensor_op_body_equals_the_restatement(C):
    from vilco_amd.cl_methods import der
    x, level_row, records, valid = _case(C)
    want_loss, want_N, want_grad, mask, _ = D.der_term(x, level_row, LEVELS, valid, records, 0.1)
    xd = x.double().requires_grad_(True)
    loss, N = der.der_term(xd, level_row, LEVELS, torch.tensor(valid, dtype=torch.int32), records, 0.1)
    loss.backward()
    assert N == want_N > 0
    assert abs(float(loss) - want_loss) <= 1e-12 * want_loss
    assert torch.allclose(xd.grad, want_grad, rtol=1e-12, atol=0.0)
    assert bool((xd.grad[~mask] == 0).all()) and bool((xd.grad[mask] != 0).any())
    # fp32, as a CPU model would run it: the fp32 roundings of ~N additions
    xf = x.clone().requires_grad_(True)
    loss32, _ = der.der_term(xf, level_row, LEVELS, valid, records, 0.1)
    loss32.backward()
    assert abs(float(loss32) - want_loss) <= 1e-5 * want_loss
    assert torch.allclose(xf.grad.double(), want_grad, rtol=1e-5, atol=1e-9)
    # nothing to compare: an exact zero that still backpropagates (zeros)
    zero, N0 = der.der_term(xd, level_row, LEVELS, valid, [None, None, None], 0.1)
    assert float(zero) == 0.0 and N0 == 0 and zero.requires_grad
    assert D.der_term(x, level_row, LEVELS, valid, [None, None, None], 0.1)[:2] == (0.0, 0)


def test_model_branch_on_a_cpu_model_goes_through_the_bank():
    """PtTransformer._cl_terms' 'der' branch on CPU tensors: records looked up by video_id, another length skipped"""
    from vilco_amd.cl_methods import der
    from vilco_amd.modeling.meta_archs import PtTransformer
    C = 5
    x, level_row, records, valid = _case(C)
    bank = der.DERBank()
    bank.record('a', records[0], 13, LEVELS)
    bank.record('c', records[2], 13, LEVELS)
    batch = [_clip('a'), _clip('x'), _clip('c')]
    levels = [x[:, r:r + T] for r, T in zip(level_row, LEVELS)]
    stub = types.SimpleNamespace(der_bank=bank, der_alpha=0.25, n_known=2, cl_name='der', _der_step=(None, batch))
    stub._der_loss = types.MethodType(PtTransformer._der_loss, stub)
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), levels, [], None, cat_logits=(x, level_row),
                                  level_len=torch.tensor(valid, dtype=torch.int32))
    want = D.der_term(x, level_row, LEVELS, valid, records, 0.25)[0]
    assert abs(float(out['der_loss']) - want) <= 1e-5 * want and abs(float(out['final_loss']) - 1.0 - want) <= 1e-5
    batch[2] = _clip('c', 12)
    stub._der_step = (None, batch)
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), levels, [], None, cat_logits=(x, level_row),
                                  level_len=torch.tensor(valid, dtype=torch.int32))
    want = D.der_term(x, level_row, LEVELS, valid, [records[0], None, None], 0.25)[0]
    assert abs(float(out['der_loss']) - want) <= 1e-5 * want and bank.skipped == 1
    # without known classes the method adds nothing
    stub.n_known = 0
    assert 'der_loss' not in PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), levels, [], None)


def test_step_inputs_carry_the_table_slot():
    from vilco_amd.modeling.meta_archs import StepInputs
    assert "der_tab" in StepInputs.__slots__ and "der_tab" not in StepInputs.HOST
    inp = StepInputs()
    for k in StepInputs.__slots__:
        setattr(inp, k, None)
    inp.feats_cf, inp.der_tab = torch.zeros(2, 4, 8), torch.zeros(2, 2, dtype=torch.int64)
    assert [k for k, _ in inp.tensors()] == ["feats_cf", "der_tab"] and ("der_tab", (2, 2)) in inp.signature()


def test_op_refuses_cpu_tensors():
    from vilco_amd import ops
    x, level_row, _, valid = _case(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.der_replay(x, level_row, LEVELS, torch.tensor(valid, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int64), 0.1)


def test_cabi_rows_exist():
    from vilco_amd import _lib
    text = open(os.path.join(ROOT, "include", "vilco_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("vilco_der_workspace", "vilco_der_fwd", "vilco_der_bwd"):
        assert n in _lib.SIGNATURES and n + "(" in text and hasattr(lib, n), n
    assert _lib.DerDesc._cname_ == "vilco_der_desc" and "} vilco_der_desc;" in text
    assert ctypes.sizeof(_lib.DerDesc) == _lib.load().vilco_abi_sizeof(b"vilco_der_desc") == 72


def test_entry_points_validate_on_the_host():
    """null pointers, L <= 0, B <= 0, a level outside R, a short workspace: refused before anything is enqueued"""
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                                             # dummy, suitably aligned addresses
    rows, lens = (ctypes.c_int32 * 2)(0, 9), (ctypes.c_int32 * 2)(8, 4)
    ok = dict(logits=x, level_row=ctypes.addressof(rows), level_T=ctypes.addressof(lens), level_dev=x, level_len=x, der_tab=x,
              B=3, R=13, C=5, L=2, alpha=0.1)
    nws = lib.vilco_der_workspace(3 * 12)
    assert nws >= 256 + 8 * 2 and lib.vilco_der_workspace(-1) == 0

    def fwd(ws=x, out=x, nbytes=nws, **kw):
        return lib.vilco_der_fwd(ctypes.byref(_lib.DerDesc(**dict(ok, **kw))), out, ws, nbytes, None)

    def bwd(ws=x, g=x, dl=x, nbytes=nws, **kw):
        return lib.vilco_der_bwd(ctypes.byref(_lib.DerDesc(**dict(ok, **kw))), g, dl, ws, nbytes, None)
    for call in (fwd, bwd):
        for bad in (dict(logits=None), dict(level_row=None), dict(level_T=None), dict(level_dev=None), dict(level_len=None),
                    dict(der_tab=None), dict(L=0), dict(L=-1), dict(B=0), dict(B=-2), dict(R=12), dict(C=0), dict(ws=None)):
            assert call(**bad) == -1, (call.__name__, bad)
        assert call(nbytes=nws - 1) == -4, call.__name__
    assert lib.vilco_der_fwd(None, x, x, nws, None) == -1 and lib.vilco_der_bwd(None, x, x, x, nws, None) == -1
    assert fwd(out=None) == -1 and bwd(g=None) == -1 and bwd(dl=None) == -1
    neg = (ctypes.c_int32 * 2)(-1, 9)
    assert fwd(level_row=ctypes.addressof(neg)) == -1
    zero = (ctypes.c_int32 * 2)(8, 0)
    assert fwd(level_T=ctypes.addressof(zero)) == -1
