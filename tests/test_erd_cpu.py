"""Elastic Response Distillation without a GPU: the float64 restatement (tests/erd_restatement.py) against the tensor-op body
cl_methods.erd.select_rows / erd_term a CPU model evaluates; the bank; the refusals, by their messages; option validation; the
support row; the model branch; the C entry points' host-side validation; a two-task episode on a CPU model."""
import ctypes
import os
import random
import types
import weakref

import numpy as np
import pytest
import torch

import erd_restatement as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (16, 8, 4)
ROWS = (0, 17, 26)            # a separator row between the levels
R = 30
VALID = [[16, 8, 4], [11, 6, 3], [5, 3, 2]]
C, N_OLD = 5, 3


def _clip(vid, n=13, labels=(1,)):
    return {'video_id': vid, 'feats': torch.zeros(4, n), 'labels': torch.tensor(labels, dtype=torch.long)}


def _teacher(seed, B=3, C_=C):
    """teacher logits [B, P, C] with a few confident positions per clip and offsets [B, P, 2] >= 0"""
    g = torch.Generator().manual_seed(seed)
    P = sum(LEVELS)
    z = torch.randn(B, P, C_, generator=g)
    for b in range(B):
        for i in torch.randperm(P, generator=g)[:6].tolist():
            z[b, i, 0] += 6.0
    o = torch.rand(B, P, 2, generator=g) * 3.0
    return z, o


def _records(z, o, n_old=N_OLD, a_c=2.0, a_r=2.0, valid=VALID):
    sels = [E.select(z[b].numpy(), o[b].numpy(), LEVELS, valid[b], n_old, a_c, a_r) for b in range(z.shape[0])]
    return sels, [E.make_record(z[b].numpy(), o[b].numpy(), s, n_old) for b, s in enumerate(sels)]


def _as_record(rec, length=13):
    from vilco_amd.cl_methods import erd
    kc, kr = rec['val_cls'].shape[0], rec['val_reg'].shape[0]
    vc, vr = torch.zeros(max(kc, 1), rec['n_old']), torch.zeros(max(kr, 1), 2)
    vc[:kc], vr[:kr] = torch.from_numpy(rec['val_cls']), torch.from_numpy(rec['val_reg'])
    return erd.Record(torch.from_numpy(rec['map_cls']), torch.from_numpy(rec['map_reg']), vc, vr, kc, kr, rec['n_old'], length, LEVELS)


def _student(seed, B=3, C_=C, raw=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, R, C_, generator=g)
    o = torch.randn(B, R, 2, generator=g) if raw else torch.rand(B, R, 2, generator=g) * 3.0
    return x, o


# ------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_select_rows_is_the_restatement(seed):
    from vilco_amd.cl_methods import erd
    z, o = _teacher(seed)
    o[0, 3] = 0.0
    sels, recs = _records(z, o, a_r=1.0)
    assert all(E.margin(s) > 1e-6 for s in sels)
    got = erd.select_rows(z, o, LEVELS, torch.tensor(VALID, dtype=torch.int32), N_OLD, 2.0, 1.0)
    assert sum(len(s['S_cls']) for s in sels) > 0 and sum(len(s['S_reg']) for s in sels) > 0
    for (mc, mr, vc, vr, kc, kr), s, r in zip(got, sels, recs):
        assert (kc, kr) == (len(s['S_cls']), len(s['S_reg']))
        assert np.array_equal(mc.numpy(), r['map_cls']) and np.array_equal(mr.numpy(), r['map_reg'])
        assert np.array_equal(vc[:kc].numpy(), r['val_cls']) and np.array_equal(vr[:kr].numpy(), r['val_reg'])
        assert set(s['S_reg']) <= {int(i) for i in s['V']} and all(i in s['V'] for i in s['S_cls'])


def test_constant_responses_select_nothing_and_padding_is_never_selected():
    from vilco_amd.cl_methods import erd
    z, o = _teacher(5)
    z[0, :, :N_OLD] = 0.25                                      # sigma = 0: the comparison is strict
    z[1, 11, 1] = 50.0                                          # the first padded position of level 0 of clip 1
    got = erd.select_rows(z, o, LEVELS, torch.tensor(VALID, dtype=torch.int32), N_OLD, 2.0, 2.0)
    assert got[0][4] == got[0][5] == 0 and int(got[0][0].max()) == -1
    assert int(got[1][0][11]) == -1 and int(got[1][1][11]) == -1
    s = E.select(z[1].numpy(), o[1].numpy(), LEVELS, VALID[1], N_OLD, 2.0, 2.0)
    assert 11 not in s['S_cls'] and np.array_equal(got[1][0].numpy(), E.make_record(z[1].numpy(), o[1].numpy(), s, N_OLD)['map_cls'])


# ------------------------------------------------------------------------------------------------- the term
@pytest.mark.parametrize("raw", [False, True])
def test_erd_term_is_the_restatement(raw):
    from vilco_amd.cl_methods import erd
    z, o_hat = _teacher(7)
    _, recs = _records(z, o_hat)
    recs[1] = None
    x, o = _student(8, raw=raw)
    scale = torch.tensor([1.5, 0.75, 2.0]) if raw else None
    want = E.term(x.numpy(), o.numpy(), None if scale is None else scale.numpy(), ROWS, LEVELS, VALID, recs, 0.7, 1.3)
    assert want['N_c'] > 0 and want['N_r'] > 0
    for dt, tol in ((torch.float64, 1e-6), (torch.float32, 2e-5)):      # (ctr_diou_loss_1d computes in fp32 whatever it is given)
        xa, oa = x.to(dt).requires_grad_(True), o.to(dt).requires_grad_(True)
        sa = None if scale is None else scale.to(dt).requires_grad_(True)
        loss, cls, reg, nc, nr = erd.erd_term(xa, oa, sa, ROWS, LEVELS, torch.tensor(VALID), [None if r is None else _as_record(r) for r in recs],
                                              0.7, 1.3)
        loss.backward()
        assert (nc, nr) == (want['N_c'], want['N_r'])
        for got, ref in ((loss, want['loss']), (cls, want['cls']), (reg, want['reg'])):
            assert abs(float(got.detach()) - ref) <= tol * max(abs(ref), 1e-30)
        pairs = [(xa.grad, want['d_logits']), (oa.grad, want['d_offsets'])] + ([] if sa is None else [(sa.grad, want['d_scale'])])
        for got, ref in pairs:
            assert float((got.double() - ref).abs().max()) <= tol * float(ref.abs().max())
    assert float(want['d_logits'][1].abs().max()) == 0.0 and float(want['d_logits'][:, :, N_OLD:].abs().max()) == 0.0


def test_a_part_without_positions_is_an_exact_zero():
    from vilco_amd.cl_methods import erd
    x, o = _student(3)
    xa, oa = x.requires_grad_(True), o.requires_grad_(True)
    loss, cls, reg, nc, nr = erd.erd_term(xa, oa, None, ROWS, LEVELS, torch.tensor(VALID), [None] * 3, 1.0, 1.0)
    loss.backward()
    assert float(loss) == 0.0 and (nc, nr) == (0, 0) and float(xa.grad.abs().max()) == 0.0 and float(oa.grad.abs().max()) == 0.0
    want = E.term(x.detach().numpy(), o.detach().numpy(), None, ROWS, LEVELS, VALID, [None] * 3, 1.0, 1.0)
    assert want['loss'] == 0.0 and float(want['d_logits'].abs().max()) == 0.0


def test_diou_gradient_at_ties_and_clamps_is_autograds():
    """student == record: each side of min / max gets half; student 0 against a positive record stays finite"""
    from vilco_amd.modeling.losses import ctr_diou_loss_1d
    g = torch.tensor([[1.5, 0.5], [2.0, 3.0]], dtype=torch.float64)
    for p0 in (g.clone(), torch.zeros_like(g)):
        p = p0.clone().requires_grad_(True)
        q = p0.clone().requires_grad_(True)
        ctr_diou_loss_1d(p, g, reduction='sum', check=False).backward()
        E.diou(q, g).sum().backward()
        assert bool(torch.isfinite(p.grad).all()) and torch.allclose(p.grad.double(), q.grad, rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------------------------------------- the bank
def test_bank_records_clears_skips_and_builds_table_rows():
    from vilco_amd.cl_methods import erd
    z, o = _teacher(1)
    _, recs = _records(z, o)
    bank = erd.ERDBank()
    for vid, r in zip('abc', recs):
        rec = _as_record(r)
        bank.record(vid, rec.map_cls, rec.map_reg, rec.val_cls, rec.val_reg, rec.k_cls, rec.k_reg, N_OLD, 13, LEVELS)
    assert len(bank) == 3 and 'a' in bank and bank.get('zz') is None
    P = sum(LEVELS)
    assert bank.nbytes() == sum(8 * P + 4 * N_OLD * r['val_cls'].shape[0] + 8 * r['val_reg'].shape[0] for r in recs)
    batch = [_clip('a'), _clip('x'), _clip('c')]
    tab = bank.table_for(batch, [13, 13, 13], level_T=LEVELS)
    assert tab.dtype == torch.int64 and tuple(tab.shape) == (3, erd.TAB_COLS) and bank.skipped == 0
    ra = bank.get('a')
    assert tab[0].tolist() == [ra.map_cls.data_ptr(), ra.map_reg.data_ptr(), ra.val_cls.data_ptr(), ra.val_reg.data_ptr(), N_OLD]
    assert tab[1].tolist() == [0] * 5 and all(a != 0 for a in tab[2].tolist())
    assert bank.table_for(batch, [13, 13, 12])[2].tolist() == [0] * 5 and bank.skipped == 1      # a re-cropped clip
    assert bank.table_for(batch, [13, 13, 13], level_T=(16, 8, 2, 2)).tolist() == [[0] * 5] * 3 and bank.skipped == 3
    with pytest.raises(ValueError):
        bank.record('d', ra.map_cls[:-1], ra.map_reg, ra.val_cls, ra.val_reg, ra.k_cls, ra.k_reg, N_OLD, 13, LEVELS)
    with pytest.raises(ValueError):
        bank.record('d', ra.map_cls, ra.map_reg, ra.val_cls[:, :2], ra.val_reg, ra.k_cls, ra.k_reg, N_OLD, 13, LEVELS)
    # clear() retires the records: the buffers live until release()
    ref = weakref.ref(ra.map_cls)
    del ra, rec, tab
    bank.clear()
    assert len(bank) == 0 and ref() is not None and len(bank.retired) == 1
    assert bank.table_for(batch, [13, 13, 13]).tolist() == [[0] * 5] * 3
    assert bank.release() == 3 and ref() is None and bank.retired == []
    assert erd.empty_table(2, 'cpu').tolist() == [[0] * 5] * 2


def test_step_table_is_all_zero_without_known_classes_or_bank():
    from vilco_amd.cl_methods import erd
    z, o = _teacher(1)
    rec = _as_record(_records(z, o)[1][0])
    bank = erd.ERDBank()
    bank.record('a', rec.map_cls, rec.map_reg, rec.val_cls, rec.val_reg, rec.k_cls, rec.k_reg, N_OLD, 13, LEVELS)
    batch = [_clip('a'), _clip('u', labels=()), _clip('x')]          # the unlabelled clip is no row of the step
    model = types.SimpleNamespace(erd_bank=bank, n_known=0, device=torch.device('cpu'), _der_levels=lambda: LEVELS)
    assert erd.step_table(model, batch).tolist() == [[0] * 5] * 2
    model.n_known = 3
    assert erd.step_table(model, batch)[0, 4] == N_OLD and erd.step_table(model, batch)[1].tolist() == [0] * 5
    model.erd_bank = None
    assert erd.step_table(model, batch).tolist() == [[0] * 5] * 2


def test_record_bound_is_cantellis():
    from vilco_amd.cl_methods import erd
    P = sum(LEVELS)
    assert erd.record_bound(3, LEVELS, 4, 2.0, 2.0) == 3 * (8 * P + 16 * (P // 5) + 8 * (P // 5))
    assert erd.record_bound(1, LEVELS, 4, 0.0, -1.0) == 8 * P + 16 * P + 8 * P


# ------------------------------------------------------------------------------------------------- hooks, refusals, options
def _cfg(**cl):
    from vilco_amd.core.config import make_config
    cfg = make_config()
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], name='erd', type_sampling='random', **cl)
    return cfg


def test_make_hooks_accepts_erd_under_run_episodes_and_refuses_the_rest():
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import erd, hooks
    from vilco_amd.core import config as c
    for k, v in erd.OPTIONS.items():
        assert c.EXTRA_DEFAULTS['cl_cfg'][k] == v and k not in c.DEFAULTS['cl_cfg']
    assert erd.OPTIONS == {'erd_alpha_cls': 2.0, 'erd_alpha_reg': 2.0, 'erd_lambda_cls': 1.0, 'erd_lambda_reg': 1.0}
    assert hooks.support('erd') == hooks.SUPPORT_MORE['erd'] == ({hooks.MQ: hooks.HOOKS}, False) and hooks.NAMED['erd'] is hooks.ERD
    assert 'erd' not in hooks.SUPPORT
    made = hooks.make_hooks(_cfg(), 'run_episodes')
    assert len(made) == 1 and isinstance(made[0], hooks.ERD)
    for driver in ('run_episodes_bic', 'run_episodes_nlq'):
        with pytest.raises(ValueError, match="cl_cfg.name 'erd' is not supported by %s" % driver):
            hooks.make_hooks(_cfg(), driver)
        assert erd.check_supported('pod', driver=driver) is False, "other methods are not this module's business"
    with pytest.raises(ValueError, match="'erd' is not supported by run_episodes_bic"):
        train_cl.run_episodes_bic(_cfg(), None, None)
    with pytest.raises(ValueError, match="'erd' is not supported by run_episodes_nlq"):
        train_cl.run_episodes_nlq(_cfg(), None, None, None, None)
    model = types.SimpleNamespace(erd_bank=None)
    with pytest.raises(ValueError, match="'erd' does not support data parallelism"):
        train_cl.run_episodes(_cfg(), model, None, reducer=object())
    with pytest.raises(ValueError, match="'erd' with type_sampling 'icarl'"):
        train_cl.run_episodes(dict(_cfg(), cl_cfg=dict(_cfg()['cl_cfg'], type_sampling='icarl')), model, None)
    with pytest.raises(ValueError, match=r"'erd' cannot resume inside a task \(start_epoch = 1\)"):
        train_cl.run_episodes(_cfg(), model, None, start_epoch=1)
    assert model.erd_bank is None, "a refused run leaves the model alone"


@pytest.mark.parametrize("bad", [dict(erd_alpha_cls=float('nan')), dict(erd_alpha_reg=float('inf')), dict(erd_lambda_cls=-0.5),
                                 dict(erd_lambda_reg=float('nan')), dict(erd_lambda_reg=-1e-9), dict(erd_alpha_cls='x')])
def test_options_are_validated_in_begin_run(bad):
    from vilco_amd.cl_methods import hooks
    model = types.SimpleNamespace(erd_bank=None)
    with pytest.raises(ValueError, match=list(bad)[0]):
        hooks.ERD(_cfg(**bad)).begin_run(model, None)
    assert model.erd_bank is None


def test_begin_run_sets_the_options_and_needs_no_state_file():
    from vilco_amd.cl_methods import erd, hooks
    model = types.SimpleNamespace(erd_bank=None)
    hooks.ERD(_cfg(erd_alpha_cls=-1.0, erd_lambda_reg=0.0)).begin_run(model, None, start_task=1)      # a negative alpha is a choice
    assert (model.erd_alpha_cls, model.erd_alpha_reg, model.erd_lambda_cls, model.erd_lambda_reg) == (-1.0, 2.0, 1.0, 0.0)
    assert isinstance(model.erd_bank, erd.ERDBank)


def test_begin_task_records_only_with_known_classes_and_releases_afterwards(monkeypatch):
    from vilco_amd.cl_methods import erd, hooks
    calls = []

    def fake(model, bank, loader, j, opts):
        calls.append((len(bank), len(bank.retired), loader, j, opts['erd_alpha_cls']))
        return 7, 1234
    monkeypatch.setattr(erd, 'record_clips', fake)
    z, o = _teacher(1)
    rec = _as_record(_records(z, o)[1][0])
    bank = erd.ERDBank()
    bank.record('old', rec.map_cls, rec.map_reg, rec.val_cls, rec.val_reg, rec.k_cls, rec.k_reg, N_OLD, 13, LEVELS)
    model = types.SimpleNamespace(erd_bank=bank, n_known=0)
    h = hooks.ERD(_cfg())
    h.begin_run(model, None)
    entry = {}
    assert h.begin_task(0, model, None, 'loader0', entry) is None and entry == {} and calls == [] and len(bank) == 1
    model.n_known = 2
    h.begin_task(1, model, None, 'loader1', entry)
    assert entry == {'erd_recorded': 7, 'erd_bytes': 1234}
    assert calls == [(0, 1, 'loader1', 1, 2.0)], "cleared before the pass, the old buffers kept until it is over"
    assert bank.retired == []


def test_model_branch_on_cpu_tensors_goes_through_the_bank():
    """PtTransformer._cl_terms' 'erd' branch on CPU tensors: records looked up by video_id, another length skipped; equal to
    erd_term, the three entries in the loss dict"""
    from vilco_amd.cl_methods import erd
    from vilco_amd.modeling.meta_archs import PtTransformer
    z, o_hat = _teacher(7)
    _, recs = _records(z, o_hat)
    bank = erd.ERDBank()
    for vid, r in (('a', recs[0]), ('c', recs[2])):
        rec = _as_record(r)
        bank.record(vid, rec.map_cls, rec.map_reg, rec.val_cls, rec.val_reg, rec.k_cls, rec.k_reg, N_OLD, 13, LEVELS)
    batch = [_clip('a'), _clip('x'), _clip('c')]
    x, o = _student(9)
    stub = types.SimpleNamespace(erd_bank=bank, erd_lambda_cls=0.5, erd_lambda_reg=2.0, n_known=N_OLD, cl_name='erd',
                                 _erd_tab_step=(None, batch), _coda_ortho=None)
    stub._erd_loss = types.MethodType(PtTransformer._erd_loss, stub)
    lens = torch.tensor(VALID, dtype=torch.int32)
    levels = [x[:, r:r + T] for r, T in zip(ROWS, LEVELS)]
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), levels, [], None, cat_logits=(x, ROWS), level_len=lens,
                                  cat_offsets=(o, None))
    want = E.term(x.numpy(), o.numpy(), None, ROWS, LEVELS, VALID, [recs[0], None, recs[2]], 0.5, 2.0)
    assert set(out) == {'erd_loss', 'erd_cls_loss', 'erd_reg_loss', 'final_loss'}
    for k, ref in (('erd_loss', want['loss']), ('erd_cls_loss', want['cls']), ('erd_reg_loss', want['reg'])):
        assert abs(float(out[k]) - ref) <= 1e-5 * abs(ref) and ref > 0
    assert abs(float(out['final_loss']) - 1.0 - want['loss']) <= 1e-5 * (1 + want['loss'])
    batch[2] = _clip('c', 12)
    stub._erd_tab_step = (None, batch)
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), levels, [], None, cat_logits=(x, ROWS), level_len=lens,
                                  cat_offsets=(o, None))
    want = E.term(x.numpy(), o.numpy(), None, ROWS, LEVELS, VALID, [recs[0], None, None], 0.5, 2.0)
    assert abs(float(out['erd_loss']) - want['loss']) <= 1e-5 * want['loss'] and bank.skipped == 1
    stub.n_known = 0                                                # without known classes the method adds nothing
    assert 'erd_loss' not in PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), levels, [], None, cat_logits=(x, ROWS),
                                                     level_len=lens, cat_offsets=(o, None))


def test_step_inputs_carry_the_table_slot():
    from vilco_amd.modeling.meta_archs import StepInputs
    assert "erd_tab" in StepInputs.__slots__ and "erd_tab" not in StepInputs.HOST
    inp = StepInputs()
    for k in StepInputs.__slots__:
        setattr(inp, k, None)
    inp.feats_cf, inp.erd_tab = torch.zeros(2, 4, 8), torch.zeros(2, 5, dtype=torch.int64)
    assert [k for k, _ in inp.tensors()] == ["feats_cf", "erd_tab"] and ("erd_tab", (2, 5)) in inp.signature()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from vilco_amd import ops
    x, o = _student(1)
    z, oh = _teacher(1)
    lens = torch.tensor(VALID, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.erd_distill(x, o, None, ROWS, LEVELS, lens, torch.zeros(3, 5, dtype=torch.int64), 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.erd_select(z, oh, LEVELS, lens, N_OLD, 2.0, 2.0)
    assert ops.ERD_TAB_COLS == 5


def test_cabi_rows_exist():
    from vilco_amd import _lib
    text = open(os.path.join(ROOT, "include", "vilco_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("vilco_erd_workspace", "vilco_erd_fwd", "vilco_erd_bwd", "vilco_erd_select", "vilco_erd_select_fill",
              "vilco_erd_pairs_per_round"):
        assert n in _lib.SIGNATURES and n + "(" in text and hasattr(lib, n), n
    for cls, name, size in ((_lib.ErdDesc, "vilco_erd_desc", 96), (_lib.ErdSelectDesc, "vilco_erd_select_desc", 104)):
        assert cls._cname_ == name and "} %s;" % name in text
        assert ctypes.sizeof(cls) == _lib.load().vilco_abi_sizeof(name.encode()) == size
    assert _lib.load().vilco_erd_pairs_per_round() >= 4


def test_entry_points_validate_on_the_host():
    """null pointers, L outside 1..16, B < 1, a level outside R, P != sum T_l, n_old outside 1..C, a short workspace: refused
    before anything is enqueued"""
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                                             # dummy, suitably aligned addresses
    rows = (ctypes.c_int32 * 17)(*([0, 17] + [26] * 15))
    lens = (ctypes.c_int32 * 17)(*([16, 8] + [1] * 15))
    ok = dict(logits=x, offsets=x, scale=None, level_row=ctypes.addressof(rows), level_T=ctypes.addressof(lens), level_dev=x,
              level_len=x, erd_tab=x, B=3, R=30, C=5, L=2, lambda_cls=1.0, lambda_reg=1.0)
    nws = lib.vilco_erd_workspace(3 * 24)
    assert nws >= 512 + 8 * 20 and lib.vilco_erd_workspace(-1) == 0

    def fwd(ws=x, out=x, nbytes=nws, **kw):
        return lib.vilco_erd_fwd(ctypes.byref(_lib.ErdDesc(**dict(ok, **kw))), out, ws, nbytes, None)

    def bwd(ws=x, g=x, dl=x, do=x, ds=None, nbytes=nws, **kw):
        return lib.vilco_erd_bwd(ctypes.byref(_lib.ErdDesc(**dict(ok, **kw))), g, dl, do, ds, ws, nbytes, None)
    for call in (fwd, bwd):
        for bad in (dict(logits=None), dict(offsets=None), dict(level_row=None), dict(level_T=None), dict(level_dev=None),
                    dict(level_len=None), dict(erd_tab=None), dict(L=0), dict(L=17), dict(B=0), dict(R=24), dict(C=0), dict(ws=None)):
            assert call(**bad) == -1, (call.__name__, bad)
        assert call(nbytes=nws - 1) == -4, call.__name__
    assert fwd(out=None) == -1 and bwd(g=None) == -1 and bwd(dl=None) == -1 and bwd(do=None) == -1
    assert bwd(scale=x, ds=None) == -1, "the raw-offset route needs somewhere to put d scale"
    assert lib.vilco_erd_fwd(None, x, x, nws, None) == -1 and lib.vilco_erd_bwd(None, x, x, x, None, x, nws, None) == -1
    sel = dict(logits=x, offsets=x, level_T=ctypes.addressof(lens), level_len=x, conf=x, flags=x, counts=x, out_tab=x, B=3, P=24,
               C=5, n_old=3, L=2, alpha_cls=2.0, alpha_reg=2.0)
    for call in (lib.vilco_erd_select, lib.vilco_erd_select_fill):
        for bad in (dict(logits=None), dict(offsets=None), dict(level_T=None), dict(level_len=None), dict(conf=None),
                    dict(flags=None), dict(counts=None), dict(B=0), dict(P=23), dict(C=0), dict(n_old=0), dict(n_old=6), dict(L=0),
                    dict(L=17), dict(alpha_cls=float('nan'))):
            assert call(ctypes.byref(_lib.ErdSelectDesc(**dict(sel, **bad))), None) == -1, bad
        assert call(None, None) == -1
    assert lib.vilco_erd_select_fill(ctypes.byref(_lib.ErdSelectDesc(**dict(sel, out_tab=None))), None) == -1


# ------------------------------------------------------------------------------------------------- a two-task episode, CPU
class _TinyDetector(torch.nn.Module):
    """the model's contract as the ERD hook and PtTransformer._cl_terms use it, small enough for the CPU: a get_emb pass gives the
    per-level logits, finished offsets and masks of a batch; a training pass gives the loss dict through _cl_terms"""
    cl_name, use_adapt, type_sampling = 'erd', False, 'random'

    def __init__(self, n_classes):
        super().__init__()
        self.cls = torch.nn.Linear(4, n_classes)
        self.reg = torch.nn.Linear(4, 2)
        self.scale = torch.nn.Parameter(torch.tensor([1.0, 0.5, 2.0]))
        self.n_known, self.erd_bank, self._coda_ortho = 0, None, None
        from vilco_amd.modeling.meta_archs import PtTransformer
        self._erd_loss = types.MethodType(PtTransformer._erd_loss, self)
        self._cl_terms = types.MethodType(PtTransformer._cl_terms, self)

    device = property(lambda self: torch.device('cpu'))

    def _der_levels(self):
        return LEVELS

    def grow(self, n_new):
        old = self.cls
        self.cls = torch.nn.Linear(4, old.out_features + n_new)
        with torch.no_grad():
            self.cls.weight[:old.out_features], self.cls.bias[:old.out_features] = old.weight, old.bias

    def forward(self, video_list, task_id=-1, get_emb=False):
        from vilco_amd.cl_methods import erd
        vids = erd.labelled(video_list)
        lens = torch.tensor([[min(T, max(1, erd.clip_len(v) * T // 16)) for T in LEVELS] for v in vids], dtype=torch.int32)
        feats = [torch.stack([v['pyr'][sum(LEVELS[:l]):sum(LEVELS[:l + 1])] for v in vids]) for l in range(3)]
        logits = [self.cls(f) for f in feats]
        raw = [self.reg(f) for f in feats]
        if get_emb:
            masks = [torch.arange(T)[None, :] < lens[:, l:l + 1] for l, T in enumerate(LEVELS)]
            return logits, [torch.relu(r * self.scale[l]) for l, r in enumerate(raw)], masks
        self._erd_tab_step = (None, video_list)
        x, o = torch.cat(logits, dim=1), torch.cat(raw, dim=1)
        rows = [sum(LEVELS[:l]) for l in range(3)]
        return self._cl_terms({}, x.square().mean(), logits, None, None, cat_logits=(x, rows), level_len=lens,
                              cat_offsets=(o, self.scale))


def test_two_task_episode_on_the_cpu():
    """the hook points in the drivers' order over two tasks of a CPU model (the drivers themselves place the model on the device):
    task 0 records nothing and has no erd term; task 1 logs erd_recorded > 0 and erd_bytes, every step has a finite erd_loss made
    of its two parts, the gradient reaches the offsets' Scale, and a third task releases the second's buffers after recording"""
    from vilco_amd.cl_methods import erd, hooks
    g = torch.Generator().manual_seed(0)
    P = sum(LEVELS)

    def clips(names, n):
        out = []
        for k, name in enumerate(names):
            pyr = torch.randn(P, 4, generator=g)
            pyr[torch.randperm(P, generator=g)[:5]] *= 6.0
            out.append(dict(_clip(name, n - k), pyr=pyr))
        return out
    tasks = [[clips('ab', 16), clips('cd', 14)], [clips('ef', 16), clips('gh', 12)], [clips('ij', 16)]]
    torch.manual_seed(0)
    model = _TinyDetector(2)
    (hook,) = hooks.make_hooks(_cfg(erd_lambda_reg=0.5), 'run_episodes')
    hook.begin_run(model, None)
    log = []
    for j, loader in enumerate(tasks):
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        entry = {'task': j, 'history': []}
        hook.begin_task(j, model, opt, loader, entry)
        if j == 2:
            break
        model.train()
        for batch in loader:
            opt.zero_grad()
            out = model(batch, task_id=j)
            out['final_loss'].backward()
            if j == 1:
                assert model.scale.grad is not None and bool(torch.isfinite(model.scale.grad).all())
            opt.step()
            entry['history'].append({k: float(v.detach()) for k, v in out.items()})
        log.append(entry)
        model.n_known = model.cls.out_features
        model.grow(2)
    assert 'erd_recorded' not in log[0] and 'erd_bytes' not in log[0] and all('erd_loss' not in h for h in log[0]['history'])
    assert log[1]['erd_recorded'] == 4 and log[1]['erd_bytes'] >= 4 * 8 * P
    hist = log[1]['history']
    assert len(hist) == 2 and all(np.isfinite(h['erd_loss']) and h['erd_loss'] >= 0 for h in hist)
    assert hist[0]['erd_loss'] == 0.0 and hist[1]['erd_loss'] > 0, "before its first update the student IS the teacher"
    assert all(abs(h['erd_loss'] - h['erd_cls_loss'] - h['erd_reg_loss']) <= 1e-6 * h['erd_loss'] for h in hist)
    assert hist[1]['erd_reg_loss'] > 0 and hist[1]['erd_cls_loss'] > 0
    # the third task: re-recorded from the model as it stands, the second task's records gone, nothing left retired
    assert entry['erd_recorded'] == 2 and set(model.erd_bank.records) == {'i', 'j'} and model.erd_bank.retired == []
    assert model.erd_bank.get('i').n_old == 4 and model.erd_bank.skipped == 0
