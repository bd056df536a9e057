"""Synaptic Intelligence without a GPU: the float64 restatement (tests/si_restatement.py) satisfies the properties that define
the method, `regularizers._entries(model, 'si')` keeps MAS's bookkeeping, and the two C entry points that carry SI
(vilco_optim_step with si_ptrs, vilco_si_consolidate) refuse bad arguments before they touch memory."""
import ctypes

import pytest
import torch

import si_restatement as S


# ------------------------------------------------------------------------------------------------------- the restatement
def test_path_integral_is_the_loss_drop_to_first_order():
    """L = 1/2 sum a theta^2, plain SGD (no momentum, decay or clipping): L(theta + d) - L(theta) = g d + 1/2 a d^2 exactly, so
    over a run  sum omega = (L_start - L_end) + sum_steps 1/2 a d^2 : the drop in loss plus a second-order term, which is
    lr a / 2 of each step's first-order term -- here at most 0.1 %."""
    gen = torch.Generator().manual_seed(0)
    a = torch.rand(50, generator=gen, dtype=torch.float64) + 0.5
    theta = torch.randn(50, generator=gen, dtype=torch.float64)
    omega, buf = torch.zeros(50, dtype=torch.float64), None
    lr = S.R.f32(1e-3)

    def loss(t):
        return float(0.5 * (a * t * t).sum())
    start, second = loss(theta), 0.0
    for step in range(1, 201):
        g = a * theta
        new, buf, omega = S.sgd_si_step(theta, g, buf, omega, step, lr, 0.0, 0.0)
        second += float(0.5 * (a * (new - theta) ** 2).sum())
        theta = new
    drop = start - loss(theta)
    assert drop > 0.1 * start
    assert abs(float(omega.sum()) - (drop + second)) <= 1e-12 * drop
    assert 0 < second <= 1e-3 * drop
    assert bool((omega >= 0).all())            # every coordinate descends its own parabola


def test_path_integral_uses_the_clipped_gradient_without_the_decay_and_the_full_displacement():
    p, g = torch.tensor([1.0, -2.0], dtype=torch.float64), torch.tensor([0.5, 0.25], dtype=torch.float64)
    lr, wd, c = S.R.f32(0.1), S.R.f32(0.5), 0.5
    new, buf, omega = S.sgd_si_step(p, g, None, torch.zeros(2, dtype=torch.float64), 1, lr, wd, 0.9, c)
    assert torch.allclose(new, p - lr * (c * g + wd * p), rtol=1e-15)
    assert torch.allclose(omega, -(c * g) * (new - p), rtol=1e-15)          # gr = c g, the displacement contains wd p
    pa, m, v, om = S.adamw_si_step(p, g, torch.zeros(2), torch.zeros(2), torch.ones(2, dtype=torch.float64), 1, lr, wd, 0.9,
                                   0.999, 1e-8, c)
    assert torch.allclose(om, 1.0 - (c * g) * (pa - p), rtol=1e-15)          # accumulates onto what is there


def test_consolidation_clamps_resets_and_anchors():
    f64 = torch.float64
    theta = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=f64)
    start = torch.tensor([[0.5, 2.0], [3.5, 4.0], [5.0, 5.0]], dtype=f64)
    omega = torch.tensor([[0.2, -0.3], [0.0, 0.7], [-1.0, 0.4]], dtype=f64)
    old = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=f64)              # the head had two rows when it was consolidated
    xi = 0.1
    imp, opt, om, ts, _ = S.consolidate(theta, omega, start, old, xi)
    x = S.R.f32(xi)
    want = torch.tensor([[1.0 + 0.2 / (0.25 + x), 2.0], [3.0, 4.0 + 0.7 / x], [0.0, 0.4 / (1.0 + x)]], dtype=torch.float64)
    assert torch.allclose(imp, want, rtol=1e-14, atol=0)
    assert imp[0, 1] == 2.0 and imp[2, 0] == 0.0               # max(omega, 0): a negative path integral adds nothing
    assert torch.equal(om, torch.zeros(3, 2, dtype=torch.float64))
    assert torch.equal(ts, theta.double()) and torch.equal(opt, theta.double())
    first = S.consolidate(theta, omega, start, None, xi)[0]
    assert torch.allclose(first, want - torch.tensor([[1.0, 2.0], [3.0, 4.0], [0.0, 0.0]], dtype=torch.float64), rtol=1e-14, atol=0)
    assert bool((first >= 0).all())


def test_penalty_restatement():
    p = [torch.tensor([1.0, 2.0, 3.0])]
    val = S.penalty(p, [(0, torch.tensor([2.0, 0.5]), torch.tensor([0.0, 4.0]))], 0.25)
    assert abs(val - S.R.f32(0.25) * (2.0 * 1.0 + 0.5 * 4.0)) < 1e-15


# ------------------------------------------------------------------------------------------------------- bookkeeping
class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.body = torch.nn.Linear(3, 2)
        self.head = torch.nn.Linear(3, 5)                     # grown from 4 rows
        self.scale = torch.nn.Parameter(torch.ones(1))
        self.reg_params = {}


def test_entries_bookkeeping_for_si():
    from vilco_amd.cl_methods import regularizers
    m = _Stub()
    assert regularizers._entries(m, 'si') == []
    imp = {'body.weight': torch.rand(2, 3), 'head.weight': torch.rand(4, 3), 'scale': torch.rand(1)}
    opt = {k: torch.randn_like(v) for k, v in imp.items()}
    m.reg_params = {'importance': [imp], 'optpar': [opt]}
    got = regularizers._entries(m, 'si')
    assert [(p is q, i is imp[n], o is opt[n]) for (p, i, o), (n, q) in
            zip(got, [('body.weight', m.body.weight), ('head.weight', m.head.weight)])] == [(True, True, True)] * 2
    assert len(regularizers._entries(m, 'mas')) == 2 and regularizers._entries(m, 'ewc') == []      # MAS's key, not EWC's
    with pytest.raises(ValueError):
        regularizers._entries(m, 'sii')
    # the autograd form of the penalty walks the same entries: prefix of the grown head, 'scale' left out
    loss = regularizers.get_regularized_loss(torch.zeros(()), m, 0.5, kind='si')
    want = S.penalty([m.body.weight, m.head.weight], [(0, imp['body.weight'], opt['body.weight']),
                                                      (1, imp['head.weight'], opt['head.weight'])], 0.5)
    assert abs(float(loss.detach()) - want) <= 1e-5 * want
    assert regularizers.si_xi({}) == 0.1 and regularizers.si_xi({'si_xi': 0.5}) == 0.5


def test_si_is_not_in_the_config_defaults():
    from vilco_amd.core.config import make_config
    assert 'si_xi' not in make_config()['cl_cfg']


def test_resume_inside_a_task_is_refused():
    from vilco_amd.cl_methods import hooks

    def si_check(cfg, start_epoch):
        """the run's hooks through begin_run (no model, no stream) -> does the run use SI's?"""
        made = hooks.make_hooks(cfg, 'run_episodes')
        hooks.each(made, 'begin_run', None, None, 0, start_epoch)
        return any(type(h) is hooks.SI for h in made)
    cfg = {'cl_cfg': {'name': 'si'}}
    assert si_check(cfg, 0) is True and si_check({'cl_cfg': {'name': 'mas'}}, 3) is False
    with pytest.raises(ValueError, match="start_epoch"):
        si_check(cfg, 1)


# ------------------------------------------------------------------------------------------------------- C ABI
FAKE = 4096          # a non-null address: every check below fails before anything is dereferenced or launched


def _table(rows, kw):
    """a vilco_chunk_table of one tensor and one chunk over FAKE addresses; takes its fields out of `kw`"""
    from vilco_amd import _lib
    d = dict(ptrs=FAKE, numel=FAKE, chunk_tensor=FAKE, chunk_off=FAKE, rows=rows, n=1, nchunks=1, chunk=S.R.CHUNK)
    d.update({k: kw.pop(k) for k in list(kw) if k in d})
    return _lib.ChunkTable(**d)


def test_si_consolidate_rejects_bad_arguments_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()

    def desc(**kw):
        return _lib.SiDesc(table=_table(5, kw), numel_old=kw.pop('numel_old', FAKE), xi=kw.pop('xi', 0.1), **kw)
    assert lib.vilco_si_consolidate(None, None) == -1
    for table in ('ptrs', 'numel', 'numel_old', 'chunk_tensor', 'chunk_off'):
        assert lib.vilco_si_consolidate(ctypes.byref(desc(**{table: None})), None) == -1, table
    for xi in (0.0, -0.1, float('nan')):
        assert lib.vilco_si_consolidate(ctypes.byref(desc(xi=xi)), None) == -1, xi
    for n in (0, -1):
        assert lib.vilco_si_consolidate(ctypes.byref(desc(n=n)), None) == -1, n
    assert lib.vilco_si_consolidate(ctypes.byref(desc(chunk=0)), None) == -1
    assert lib.vilco_si_consolidate(ctypes.byref(desc(nchunks=-1)), None) == -1
    assert lib.vilco_si_consolidate(ctypes.byref(desc(rows=4)), None) == -1            # reads five rows
    assert lib.vilco_si_consolidate(ctypes.byref(desc(nchunks=0)), None) == 0          # nothing to do, nothing launched


def test_optim_step_with_si_rejects_bad_arguments_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()
    lr = (ctypes.c_float * 1)(1e-3)

    def desc(**kw):
        d = dict(table=_table(4, kw), kind=0, group=FAKE, lr=ctypes.addressof(lr), wd=ctypes.addressof(lr), ngroups=1, beta1=0.9,
                 beta2=0.999, eps=1e-8, momentum=0.9, tensor_step=FAKE, si_ptrs=FAKE)
        d.update(kw)
        return _lib.OptimDesc(**d)
    assert lib.vilco_optim_step(None, None) == -1
    for bad in (dict(ptrs=None), dict(numel=None), dict(group=None), dict(tensor_step=None), dict(n=-1), dict(chunk=0),
                dict(kind=2), dict(ngroups=0), dict(rows=3), dict(kind=1, rows=2)):       # AdamW reads four rows, SGD three
        assert lib.vilco_optim_step(ctypes.byref(desc(**bad)), None) == -1, bad
    assert lib.vilco_optim_step(ctypes.byref(desc(nchunks=0)), None) == 0
    assert lib.vilco_optim_step(ctypes.byref(desc(kind=1, rows=3, nchunks=0)), None) == 0
    assert ctypes.sizeof(_lib.OptimDesc) == lib.vilco_abi_sizeof(b"vilco_optim_desc")
    assert ctypes.sizeof(_lib.SiDesc) == lib.vilco_abi_sizeof(b"vilco_si_desc") > 0
    assert _lib.OptimDesc._fields_[-1][0] == "si_ptrs"              # appended: older callers' descriptors stay a prefix
