"""ER-ACE without a GPU (vilco_amd/cl_methods/ace.py, hooks.ERACE, PtTransformer.losses' window, the C ABI rows): the float64
restatement (tests/ace_restatement.py) is the plain loss when every window is 0 and has the method's invariants otherwise; the
window table, the support checks and a two-task episode of a CPU model through PtTransformer.losses."""
import ctypes
import dataclasses
import os
import types

import pytest
import torch

import ace_restatement as A
import loss_cases as LC
from parity_util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# two levels, three clips, GT on both sides of every window used below; clip 1 is valid for 21 of 40 points
SMALL = LC.Case('ace_small', 5, (40, 20), (LC._spread((0, 3, 4, 1)), LC._spread((1, 4), 1.0), LC._spread((4,), 2.5)), (40, 21, 33), seed=7)


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.name)
def test_all_zero_windows_restate_the_plain_loss(case):
    want, got = LC.expected(case), A.expected(case, None)
    assert abs(got['norm'] - want['norm']) <= 1e-12 * want['norm']
    for k in LC.LOSS_KEYS:
        assert abs(got['losses'][k] - want['losses'][k]) <= 1e-11 * max(abs(want['losses'][k]), 1e-3), k
    for name in ('dlogits', 'doffsets'):
        for l, (a, b) in enumerate(zip(got[name], want[name])):
            assert rel_err(a, b, 1e-9) < 1e-10, (name, l)
    if case.scale:
        assert rel_err(got['dscale'], want['dscale'], 1e-9) < 1e-10
    assert rel_err(got['dgauss'], want['dgauss'], 1e-9) < 1e-10


def test_out_of_range_windows_are_the_full_loss():
    assert A.windows([-1, 5, 12, 4, 0], 5, 5) == [0, 0, 0, 4, 0] and A.windows(None, 2, 5) == [0, 0]
    assert A.expected(SMALL, (-1, 5, 77)) is A.expected(SMALL, None)


@pytest.mark.parametrize("lo", [(2, 2, 2), (0, 2, 4), (4, 0, 3)])
def test_invariants_of_the_window(lo):
    full, win = A.expected(SMALL, None), A.expected(SMALL, lo)
    C = SMALL.ncls
    for l, g in enumerate(win['dlogits']):
        for b, lo_b in enumerate(lo):
            assert bool((g[b, :, :lo_b] == 0).all()), "columns below the window carry exactly no gradient"
            assert bool((g[b, :, lo_b:] != 0).any())
    # a row's regression gradient does not depend on lo (same normaliser: #pos is the assignment's)
    assert win['norm'] == full['norm']
    reg_only = lambda lo_: A._evaluate(dataclasses.replace(SMALL, gw=(None, 1.0, None, None)), A.windows(lo_, 3, C))   # noqa: E731
    a, b_ = reg_only(None), reg_only(lo)
    assert any(bool((t != 0).any()) for t in a['doffsets'])
    for x, y in zip(a['doffsets'], b_['doffsets']):
        assert torch.equal(x, y)
    assert a['losses']['reg_loss'] == b_['losses']['reg_loss']
    # clip 1's GT classes are (1, 4): under lo = 2 class 1 leaves its classification sum, the rows stay positive
    assert win['losses']['cls_loss'] != full['losses']['cls_loss'] or lo == (0, 0, 0)
    # the al score of a masked, non-gap row is 1 / (C - lo_b): push one class of clip 1 below it on every valid row
    pushed = dataclasses.replace(SMALL, name='ace_small_pushed', edits=(('logit_shift', 1, 4, -14.0),))
    sc = A.expected(pushed, lo)['al_score']
    assert abs(float(sc[1, 4]) - 1.0 / (C - lo[1])) < 1e-15
    assert bool((sc[1, :lo[1]] == 0).all())


def test_a_class_below_the_window_keeps_the_row_positive():
    """clip 2's only GT class is 4... under lo = 0; make clip 1's classes (1, 4) and lo = (0, 5 -> 0, 0): nothing changes; with
    clip b's every class below lo_b the regression loss is the full one and the al term counts no involved class there"""
    case = dataclasses.replace(SMALL, name='ace_small_below', gts=(SMALL.gts[0], LC._spread((1, 0), 1.0), SMALL.gts[2]))
    full, win = A.expected(case, None), A.expected(case, (0, 2, 0))
    assert win['losses']['reg_loss'] == full['losses']['reg_loss'] > 0 and win['norm'] == full['norm']
    assert win['losses']['cls_loss'] < full['losses']['cls_loss']
    assert bool((win['al_score'][1, :2] == 0).all()) and bool((win['al_score'][1, 2:] > 0).all())


# ------------------------------------------------------------------------------------------------- the window table
def _clip(vid, labels=(1,), n=13):
    return {'video_id': vid, 'feats': torch.zeros(4, n), 'labels': torch.tensor(labels), 'segments': torch.tensor([[2.0, 6.0]] * len(labels))}


def test_step_table():
    from vilco_amd.cl_methods import ace, der
    assert ace.clip_key is der.clip_key
    model = types.SimpleNamespace(n_known=3, memory={0: [_clip('m0', (0,))], 2: [_clip('m2', (2,)), _clip('m3', (2,))]},
                                  device=torch.device('cpu'))
    batch = [_clip('t0', (3,)), _clip('m2', (2,)), _clip('nolabel', ()), _clip('t1', (4,)), _clip('m0', (0,))]
    tab = ace.step_table(model, batch)
    assert tab.dtype == torch.int32 and tab.tolist() == [3, 0, 3, 0], "one entry per labelled clip, in batch order"
    model.memory = {}
    assert ace.step_table(model, batch).tolist() == [3, 3, 3, 3], "an empty memory: every clip is a task clip"
    model.memory = None
    assert ace.step_table(model, batch).tolist() == [3, 3, 3, 3]
    model.n_known, model.memory = 0, {0: [_clip('t0', (0,))]}
    assert ace.step_table(model, batch).tolist() == [0, 0, 0, 0], "nothing known: the plain loss"
    assert ace.column_mask(torch.tensor([0, 2, 5, -1, 4], dtype=torch.int32), 5).tolist() == \
        [[True] * 5, [False, False, True, True, True], [True] * 5, [True] * 5, [False] * 4 + [True]]


def test_step_inputs_carry_the_window_slot():
    from vilco_amd.modeling.meta_archs import StepInputs
    assert "ace_lo" in StepInputs.__slots__ and "ace_lo" not in StepInputs.HOST
    inp = StepInputs()
    for k in StepInputs.__slots__:
        setattr(inp, k, None)
    inp.feats_cf, inp.ace_lo = torch.zeros(2, 4, 8), torch.zeros(2, dtype=torch.int32)
    assert [k for k, _ in inp.tensors()] == ["feats_cf", "ace_lo"] and ("ace_lo", (2,)) in inp.signature()


# ------------------------------------------------------------------------------------------------- support
def _cfg(name='er_ace', **cl):
    from vilco_amd.core.config import make_config
    cfg = make_config()
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], name=name, type_sampling='random', **cl)
    return cfg


def test_make_hooks_accepts_er_ace_under_run_episodes_and_refuses_the_rest():
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import ace, hooks
    assert hooks.support('er_ace') == hooks.SUPPORT_MORE['er_ace'] == ({hooks.MQ: hooks.HOOKS}, False)
    assert 'er_ace' not in hooks.SUPPORT and hooks.NAMED['er_ace'] is hooks.ERACE
    made = hooks.make_hooks(_cfg(), 'run_episodes')
    assert len(made) == 1 and isinstance(made[0], hooks.ERACE)
    for driver in ('run_episodes_bic', 'run_episodes_nlq'):
        with pytest.raises(ValueError, match="cl_cfg.name 'er_ace' is not supported by %s" % driver):
            hooks.make_hooks(_cfg(), driver)
        with pytest.raises(ValueError, match=driver):
            ace.check_supported('er_ace', driver=driver)
        assert ace.check_supported('der', driver=driver) is False, "other methods are not this module's business"
    assert ace.check_supported('er_ace') is True and ace.check_supported(None) is False
    with pytest.raises(ValueError, match="'er_ace' is not supported by run_episodes_bic"):
        train_cl.run_episodes_bic(_cfg(), None, None)
    with pytest.raises(ValueError, match="'er_ace' is not supported by run_episodes_nlq"):
        train_cl.run_episodes_nlq(_cfg(), None, None, None, None)
    with pytest.raises(ValueError, match=r"'er_ace' does not support data parallelism \(reducer is not None\)"):
        ace.check_supported('er_ace', reducer=object())
    model = types.SimpleNamespace()
    with pytest.raises(ValueError, match="'er_ace' does not support data parallelism"):
        train_cl.run_episodes(_cfg(), model, None, reducer=object())
    assert vars(model) == {}, "a refused run leaves the model alone"
    # no state: begin_run takes any resume point, with or without a replayed stream
    for stream in (types.SimpleNamespace(train_enable=False), types.SimpleNamespace(train_enable=True), None):
        hooks.ERACE(_cfg()).begin_run(model, stream, start_task=3, start_epoch=2, ckpt_folder=None)
    assert vars(model) == {}
    # the other methods' hooks are what they were
    assert [type(h) for h in hooks.make_hooks(_cfg('der'), 'run_episodes')] == [hooks.DER]
    assert hooks.make_hooks(_cfg(None), 'run_episodes_nlq') == []


# ------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_two_entries():
    from vilco_amd import _lib
    text = open(os.path.join(ROOT, "include", "vilco_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("vilco_mq_loss_ace_fwd", "vilco_mq_loss_ace_bwd"):
        assert n in _lib.SIGNATURES and "int %s(const vilco_loss_desc* d, const int32_t* cls_lo," % n in text and hasattr(lib, n), n
    plain_f, ace_f = _lib.SIGNATURES["vilco_mq_loss_fwd"], _lib.SIGNATURES["vilco_mq_loss_ace_fwd"]
    plain_b, ace_b = _lib.SIGNATURES["vilco_mq_loss_bwd"], _lib.SIGNATURES["vilco_mq_loss_ace_bwd"]
    assert len(ace_f[1]) == len(plain_f[1]) + 1 and len(ace_b[1]) == len(plain_b[1]) + 1
    assert ctypes.sizeof(_lib.LossDesc) == _lib.load().vilco_abi_sizeof(b"vilco_loss_desc"), "the descriptor did not change"


def test_entry_points_refuse_before_anything_is_enqueued():
    """null pointers (cls_lo among them), C = 129, a short workspace: the plain entries' returns, in the plain entries' order"""
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                                             # a dummy, suitably aligned address: nothing reads it
    ok = dict(logits=x, offsets=x, level_scale=None, points=x, row_level=x, row_pos=x, level_len=x, gt=x, gauss=x, loss_norm=x,
              B=3, R=61, C=5, L=2, Nmax=4, center_radius=1.5, label_smoothing=0.0, momentum=0.9, loss_weight=1.0, al_weight=0.2,
              use_al=1)
    nws = lib.vilco_mq_loss_workspace(3, 61, 5)

    def fwd(cls_lo=x, out=x, nbytes=nws, **kw):
        return lib.vilco_mq_loss_ace_fwd(ctypes.byref(_lib.LossDesc(**dict(ok, **kw))), cls_lo, out, x, x, x, nbytes, None)

    def bwd(cls_lo=x, dl=x, ds=None, **kw):
        return lib.vilco_mq_loss_ace_bwd(ctypes.byref(_lib.LossDesc(**dict(ok, **kw))), cls_lo, None, None, None, x, x, x, dl, x, ds,
                                         x, None)
    BADARG, UNSUPPORTED, WORKSPACE = -1, lib.vilco_mq_loss_fwd(ctypes.byref(_lib.LossDesc(**dict(ok, C=129))), x, x, x, x, nws, None), -4
    assert UNSUPPORTED not in (0, BADARG, WORKSPACE)
    for call in (fwd, bwd):
        assert call(cls_lo=None) == BADARG, call.__name__
        assert call(logits=None) == BADARG and call(B=0) == BADARG and call(gauss=None) == BADARG
        assert call(C=129) == UNSUPPORTED, "C = 129: refused, nothing launched"
        assert call(C=129, cls_lo=None) == BADARG, "a null table is reported first"
    assert fwd(nbytes=nws - 1) == WORKSPACE and fwd(out=None) == BADARG
    assert bwd(dl=None) == BADARG and bwd(level_scale=x, ds=None) == BADARG


def test_op_validates_the_table_before_the_library_is_called(monkeypatch):
    from vilco_amd import _lib, ops

    def boom():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, 'load', boom)
    z = torch.zeros(2, 4, 3)
    rest = (torch.zeros(2, 4, 2), None, torch.ones(6, 3), (torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32),
            torch.zeros(4, dtype=torch.int32)), torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 4), torch.ones(1), 1.5, 0.0, 0.9)
    for bad, exc in ((torch.zeros(2, dtype=torch.int64), ValueError), (torch.zeros(3, dtype=torch.int32), ValueError),
                     (torch.zeros(2, 1, dtype=torch.int32), ValueError), ([0, 0], ValueError),
                     (torch.zeros(4, dtype=torch.int32)[::2], ValueError), (torch.zeros(2, dtype=torch.int32, device='meta'), RuntimeError)):
        with pytest.raises(exc, match="cls_lo"):
            ops.mq_loss_ace(z, *rest, 1.0, 0.2, True, bad)
    with pytest.raises(ValueError, match="loss_weight must be > 0"):
        ops.mq_loss_ace(z, *rest, 0.0, 0.2, True, torch.zeros(2, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------- a two-task episode, CPU
T0 = 16


class _TinyDetector(torch.nn.Module):
    """the model's contract as the ER-ACE hook and PtTransformer.losses use it, small enough for the CPU: two pyramid levels, a
    k = 3 conv as the last layer of either head, the label assignment and the losses PtTransformer's own"""
    use_adapt, type_sampling, sync_free_loss = False, 'random', True
    train_label_smoothing, train_loss_weight, al_loss_weight, loss_normalizer_momentum = 0.0, 1.0, 0.2, 0.9
    train_center_sample, train_center_sample_radius = 'radius', 1.5

    def __init__(self, cl_name, n_classes):
        super().__init__()
        from vilco_amd.modeling.meta_archs import PtTransformer
        self.cl_name, self.num_classes = cl_name, n_classes
        self.cls = torch.nn.Conv1d(4, n_classes, 3, padding=1)
        self.reg = torch.nn.Conv1d(4, 2, 3, padding=1)
        for k, v in (('mu', 0.0), ('sigma', 1.0), ('mu_reg_left', -0.5), ('sigma_reg_left', 1.0), ('mu_reg_right', 0.5), ('sigma_reg_right', 1.0)):
            setattr(self, k, torch.nn.Parameter(torch.full((n_classes, 1), v)))
        self.n_known, self.memory, self._coda_ortho, self._loss_norm = 0, {}, None, 100.0
        for name in ('losses', 'label_points', 'label_points_single_video', '_loss_norm_tensor', '_cl_terms', '_ace_window'):
            setattr(self, name, types.MethodType(getattr(PtTransformer, name), self))

    device = property(lambda self: torch.device('cpu'))

    def grow(self, n_new):
        old, n = self.cls, self.num_classes
        self.cls = torch.nn.Conv1d(4, n + n_new, 3, padding=1)
        with torch.no_grad():
            self.cls.weight[:n], self.cls.bias[:n] = old.weight, old.bias
        for k in ('mu', 'sigma', 'mu_reg_left', 'sigma_reg_left', 'mu_reg_right', 'sigma_reg_right'):
            v = getattr(self, k).data
            setattr(self, k, torch.nn.Parameter(torch.cat([v, v[:1].expand(n_new, 1)]).clone()))
        self.n_known, self.num_classes = n, n + n_new

    def forward(self, video_list, task_id=-1):
        from vilco_amd.cl_methods import ace
        vids = ace.labelled(video_list)
        x = torch.stack([torch.nn.functional.pad(v['feats'], (0, T0 - v['feats'].shape[-1])) for v in vids])
        lens = torch.tensor([v['feats'].shape[-1] for v in vids])
        levels = [x, torch.nn.functional.avg_pool1d(x, 2)]
        masks = [torch.arange(T0 >> l)[None, :] < ((lens + (1 << l) - 1) >> l)[:, None] for l in range(2)]
        logits = [self.cls(f).transpose(1, 2) * m[..., None] for f, m in zip(levels, masks)]
        offsets = [torch.relu(self.reg(f)).transpose(1, 2) * m[..., None] for f, m in zip(levels, masks)]
        points = [torch.stack([torch.arange(0, T0, 1 << l).float(), torch.full((T0 >> l,), lo), torch.full((T0 >> l,), hi),
                               torch.full((T0 >> l,), float(1 << l))], dim=1) for l, (lo, hi) in enumerate(((0.0, 4.0), (4.0, 1e4)))]
        self._ace_step = (None, video_list)
        segs, labs = [v['segments'] for v in vids], [v['labels'] for v in vids]
        gt_cls, gt_off, np_cls, np_reg = self.label_points(points, segs, labs)
        return self.losses(masks, logits, offsets, gt_cls, gt_off, label_list=labs, normal_probs_cls=np_cls, normal_probs_reg=np_reg)


def _episode(name):
    """two tasks of two classes each, in the drivers' order of hook points; the memory holds two clips of task 0 from its end on.
    Task 1: a batch of task clips only, then one that mixes a memory clip in.  -> log, model, the classification conv's gradients"""
    from vilco_amd.cl_methods import hooks
    g = torch.Generator().manual_seed(1)

    def clip(vid, label, n=T0):
        return {'video_id': vid, 'feats': torch.randn(4, n, generator=g), 'labels': torch.tensor([label]),
                'segments': torch.tensor([[3.0, 9.0 + label]])}
    task0 = [[clip('a', 0), clip('b', 1, 13)], [clip('c', 1), clip('d', 0, 11)]]
    task1 = [[clip('e', 2), clip('f', 3, 14)], [clip('g', 3, 12), task0[0][0]]]
    torch.manual_seed(0)
    model = _TinyDetector(name, 2)
    made = hooks.make_hooks(_cfg(name), 'run_episodes')
    hooks.each(made, 'begin_run', model, types.SimpleNamespace(train_enable=True, memory={}, num_tasks=2, seed=0))
    log, grads = [], []
    for j, loader in enumerate((task0, task1)):
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        entry = {'task': j, 'history': []}
        hooks.each(made, 'begin_task', j, model, opt, loader, entry)
        model.train()
        for batch in loader:
            opt.zero_grad()
            out = model(batch, task_id=j)
            out['final_loss'].backward()
            grads.append((j, model.cls.weight.grad.clone(), model.cls.bias.grad.clone()))
            opt.step()
            entry['history'].append({k: float(v.detach().sum()) for k, v in out.items()})
        hooks.each(made, 'end_training', j, model, opt, j == 0)
        log.append(entry)
        if j == 0:
            model.memory = {0: [task0[0][0]], 1: [task0[1][0]]}
            hooks.each(made, 'after_reload', j, model, entry)
            torch.manual_seed(5)
            model.grow(2)
            hooks.each(made, 'before_next_task', j, model, opt, loader, 0)
    return log, model, grads


def test_two_task_episode_on_the_cpu():
    log_p, model_p, grads_p = _episode(None)
    log_a, model_a, grads_a = _episode('er_ace')
    # task 0: nothing is known, the method is the plain loss -- the same numbers, the same gradients
    assert log_a[0]['history'] == log_p[0]['history'] and len(log_a[0]['history']) == 2
    for (ja, wa, ba), (jp, wp, bp) in zip(grads_a[:2], grads_p[:2]):
        assert ja == jp == 0 and torch.equal(wa, wp) and torch.equal(ba, bp)
    assert model_a.n_known == model_p.n_known == 2 and model_a.cls.out_channels == 4
    # task 1, a batch of task clips only: the old classes' rows of the classification conv get exactly zero gradient
    (_, w_a, b_a), (_, w_p, b_p) = grads_a[2], grads_p[2]
    assert bool((w_a[:2] == 0).all()) and bool((b_a[:2] == 0).all())
    assert bool((w_a[2:] != 0).any()) and bool((b_a[2:] != 0).all())
    assert bool((w_p[:2] != 0).any()) and bool((b_p[:2] != 0).all()), "the plain loss trains them down as background"
    h_a, h_p = log_a[1]['history'][0], log_p[1]['history'][0]
    assert h_a['reg_loss'] == h_p['reg_loss'] > 0, "same incoming model, same assignment: the regression loss does not see the window"
    assert 0 < h_a['cls_loss'] < h_p['cls_loss'] and all(torch.isfinite(torch.tensor(v)) for v in h_a.values())
    # a batch with a memory clip: that clip is scored over all classes, the old rows train again
    (_, w_a, b_a) = grads_a[3]
    assert bool((w_a[:2] != 0).any()) and bool((b_a[:2] != 0).all())
    assert all(bool(torch.isfinite(p).all()) for p in model_a.parameters())
