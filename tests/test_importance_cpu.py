"""EWC / MAS importance over the whole task and the online merge, without a GPU: the float64 restatement
(tests/importance_restatement.py) against the reference-recorded consolidation goldens (tests/golden/cl_parts.pt), and the
host-tensor path of `on_task_update` against the restatement; the argument checks of vilco_cl_accumulate."""
import ctypes
import os

import pytest
import torch

from importance_restatement import GrowToy, RecordingSGD, importance, merge, toy_loader
import optim_restatement as R
from parity_util import HERE, cases, rel_err

U = 2.0 ** -24          # one fp32 rounding, relative


def _gold():
    return torch.load(os.path.join(HERE, "golden", "cl_parts.pt"), weights_only=False)


def _key(kind):
    return 'fisher' if kind == 'ewc' else 'importance'


def _batch_grads(model, loader):
    out = []
    for batch in loader:
        model.zero_grad(set_to_none=True)
        model(batch)['final_loss'].backward()
        out.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    return out


def _params(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def _within(got, want, n_roundings):
    """elementwise |got - want| <= n_roundings * 2^-24 * |want|"""
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape
    return bool(((got - want).abs() <= n_roundings * U * want.abs()).all())


@pytest.mark.parametrize("kind", ["ewc", "mas"])
def test_restatement_last_matches_reference(kind):
    """ties the restatement to the reference: its 'last' / 'per_task' result is what EWC.py:24-56 / MAS.py:23-57 recorded"""
    want = _gold()[kind + '_update']
    model = cases.RegToy()
    imp = importance(_batch_grads(model, cases.reg_toy_loader()), kind, 'last')
    imps, opts = merge([imp], [_params(model)], 'per_task')
    assert len(imps) == len(want[_key(kind)]) == 1 and len(opts) == len(want['optpar']) == 1
    for got, ref in ((imps[0], want[_key(kind)][0]), (opts[0], want['optpar'][0])):
        assert sorted(got) == sorted(ref)
        for n, w in ref.items():
            assert rel_err(got[n], w) < 1e-5, n


@pytest.mark.parametrize("kind", ["ewc", "mas"])
def test_host_mean_importance_matches_restatement(kind):
    """N = 3 batches: one rounding for the squares (positive terms, each within one rounding), N - 1 adds, the fp32 value of
    1 / N and the scaling: N + 2 roundings at the most"""
    from vilco_amd.cl_methods import regularizers
    model = cases.RegToy()
    opt = RecordingSGD(model)
    reg = regularizers.on_task_update(cases.reg_toy_loader(), 'cpu', opt, model, kind=kind, importance='mean')
    grads = opt.batches()
    assert len(grads) == 3
    want = importance(grads, kind, 'mean')
    assert len(reg[_key(kind)]) == len(reg['optpar']) == 1
    got = reg[_key(kind)][0]
    assert list(got) == [n for n, _ in model.named_parameters() if n in want] and 'unused' not in got
    for n, w in want.items():
        assert _within(got[n], w, 3 + 2), n
        assert torch.equal(reg['optpar'][0][n], dict(model.named_parameters())[n].data)
    last = importance(grads, kind, 'last')
    assert not torch.allclose(got['body.weight'].double(), last['body.weight'], rtol=1e-3)


def test_host_mean_importance_takes_the_union_over_batches():
    """a parameter that gets a gradient in the second batch only is in the dictionary, with that batch's share of the mean"""
    from vilco_amd.cl_methods import regularizers

    class Late(GrowToy):
        def __init__(self):
            super().__init__()
            self.late = torch.nn.Parameter(torch.tensor([0.5, -2.0]))
            self.calls = 0

        def forward(self, x):
            out = super().forward(x)
            self.calls += 1
            if self.calls == 2:
                out['final_loss'] = out['final_loss'] + (self.late * self.late).sum()
            return out

    torch.manual_seed(4)
    model = Late()
    opt = RecordingSGD(model)
    reg = regularizers.on_task_update(toy_loader(50), 'cpu', opt, model, kind='ewc', importance='mean')
    want = importance(opt.batches(), 'ewc', 'mean')
    assert sorted(reg['fisher'][0]) == sorted(want) and 'late' in want
    for n, w in want.items():
        assert _within(reg['fisher'][0][n], w, 3 + 2), n
    assert _within(reg['fisher'][0]['late'], torch.tensor([1.0, 16.0], dtype=torch.float64) / 3, 2)


class _Toy2(GrowToy):
    """GrowToy with a parameter that is frozen in the second task (carried) and one that leaves the model (dropped)"""
    def __init__(self):
        super().__init__()
        self.frozen = torch.nn.Parameter(torch.randn(5))
        self.gone = torch.nn.Parameter(torch.randn(5))

    def forward(self, x):
        h = torch.tanh(self.body(x) * self.frozen)
        if hasattr(self, 'gone'):
            h = h + self.gone
        return {'final_loss': self.head(h).pow(2).mean()}


@pytest.mark.parametrize("kind", ["ewc", "mas"])
def test_host_online_merge_matches_restatement(kind):
    """two tasks, the head grows from 4 to 7 rows in between, gamma = 0.9.  Against the restatement fed with the gradients the
    passes saw: one rounding for each task's f(g), the fp32 value of gamma, the product, the sum: 4 roundings at the most"""
    from vilco_amd.cl_methods import regularizers
    torch.manual_seed(6)
    model = _Toy2()
    tasks, params = [], []
    opt = RecordingSGD(model)
    regularizers.on_task_update(toy_loader(30), 'cpu', opt, model, kind=kind, merge='online', gamma=0.9)
    tasks.append(importance(opt.batches(), kind, 'last'))
    params.append(_params(model))
    assert len(model.reg_params[_key(kind)]) == len(model.reg_params['optpar']) == 1

    model.grow(7)
    model.frozen.requires_grad_(False)
    del model.gone
    with torch.no_grad():
        model.body.weight.add_(0.05)
    model.zero_grad(set_to_none=True)
    opt = RecordingSGD(model)
    reg = regularizers.on_task_update(toy_loader(40), 'cpu', opt, model, kind=kind, merge='online', gamma=0.9)
    tasks.append(importance(opt.batches(), kind, 'last'))
    params.append(_params(model))

    imps, opts = merge(tasks, params, 'online', gamma=0.9)
    assert len(reg[_key(kind)]) == len(reg['optpar']) == len(imps) == 1
    got = reg[_key(kind)][0]
    assert sorted(got) == sorted(imps[0]) == sorted(reg['optpar'][0])
    assert 'frozen' in got and 'gone' not in got and 'frozen' not in tasks[1]
    for n, w in imps[0].items():
        assert _within(got[n], w, 4), n
        assert torch.equal(reg['optpar'][0][n], dict(model.named_parameters())[n].data), n
        assert rel_err(reg['optpar'][0][n], opts[0][n]) == 0.0
    assert got['head.weight'].shape == (7, 5)
    assert torch.equal(got['head.weight'][4:].double(), tasks[1]['head.weight'][4:].float().double())
    # the merged state is a valid penalty state: one entry per parameter
    assert len(regularizers._entries(model, kind)) == len(got)


@pytest.mark.parametrize("kind", ["ewc", "mas"])
def test_defaults_keep_the_reference_layout(kind):
    """without the new arguments: one more dictionary per task, equal to the explicit 'last' / 'per_task' call bit for bit"""
    from vilco_amd.cl_methods import regularizers
    a, b = cases.RegToy(), cases.RegToy()
    for k in (1, 2, 3):
        ra = regularizers.on_task_update(cases.reg_toy_loader(), 'cpu', torch.optim.SGD(a.parameters(), lr=0.1), a, kind=kind)
        rb = regularizers.on_task_update(cases.reg_toy_loader(), 'cpu', torch.optim.SGD(b.parameters(), lr=0.1), b, kind=kind,
                                         importance='last', merge='per_task', gamma=1.0)
        assert len(ra[_key(kind)]) == len(ra['optpar']) == len(rb[_key(kind)]) == k
    want = _gold()[kind + '_update']
    for key in (_key(kind), 'optpar'):
        for da, db in zip(ra[key], rb[key]):
            assert list(da) == list(db) == list(want[key][0])
            for n in da:
                assert torch.equal(da[n], db[n])
                assert rel_err(da[n], want[key][0][n]) < 1e-5


def test_unknown_modes_raise():
    from vilco_amd.cl_methods import regularizers
    model = cases.RegToy()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="'last', 'mean'"):
        regularizers.on_task_update(cases.reg_toy_loader(), 'cpu', opt, model, importance='sum')
    with pytest.raises(ValueError, match="'per_task', 'online'"):
        regularizers.on_task_update(cases.reg_toy_loader(), 'cpu', opt, model, merge='ema')
    assert model.reg_params == {}
    with pytest.raises(ValueError, match="'last', 'mean'"):
        regularizers.importance_options({'importance': 'fisher'})
    with pytest.raises(ValueError, match="'per_task', 'online'"):
        regularizers.importance_options({'importance_merge': True})
    assert regularizers.importance_options({}) == dict(importance='last', merge='per_task', gamma=1.0)
    assert regularizers.importance_options({'importance': 'mean', 'importance_merge': 'online', 'importance_gamma': 0.9}) == \
        dict(importance='mean', merge='online', gamma=0.9)
    from vilco_amd.core.config import make_config
    cfg = make_config(dataset=dict(input_dim=96), cl_cfg=dict(name='ewc', importance='mean'))
    assert cfg['cl_cfg']['importance'] == 'mean' and 'importance_merge' not in cfg['cl_cfg']
    assert regularizers.importance_options(cfg['cl_cfg'])['importance'] == 'mean'


def test_cl_accumulate_host_path_and_its_checks():
    from vilco_amd import ops
    x = torch.tensor([1.0, -2.0, 3.0, -4.0])
    acc = torch.full((6,), float('nan'))
    ops.cl_accumulate([x], [acc], ops.CL_OP_ABS, 0.5, 0.0, numels=[3])           # beta == 0: acc is not read
    assert torch.equal(acc[:3], torch.tensor([0.5, 1.0, 1.5])) and bool(acc[3:].isnan().all())
    ops.cl_accumulate([x], [acc], ops.CL_OP_SQUARE, 2.0, -1.0, numels=[2])
    assert torch.equal(acc[:3], torch.tensor([1.5, 7.0, 1.5]))
    ops.cl_accumulate([torch.full((6,), float('inf'))], [acc], ops.CL_OP_COPY, 0.0, 2.0, numels=[3])   # alpha == 0: src is not read
    assert torch.equal(acc[:3], torch.tensor([3.0, 14.0, 3.0]))
    ops.cl_accumulate([], [], ops.CL_OP_COPY, 1.0, 1.0)
    with pytest.raises(ValueError, match="op must be"):
        ops.cl_accumulate([x], [acc], 3, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="prefix"):
        ops.cl_accumulate([x], [acc], ops.CL_OP_COPY, 1.0, 1.0, numels=[5])
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        ops.cl_accumulate([x.double()], [acc], ops.CL_OP_COPY, 1.0, 1.0, numels=[2])


def test_cl_accumulate_rejects_bad_arguments_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                                            # dummy addresses: every check precedes the launch
    ok = dict(ptrs=x, numel=x, chunk_tensor=x, chunk_off=x, rows=2, n=1, nchunks=1, chunk=R.CHUNK)

    def call(op=1, **kw):
        return lib.vilco_cl_accumulate(ctypes.byref(_lib.ChunkTable(**dict(ok, **kw))), op, 1.0, 0.0, None)
    for bad in (dict(ptrs=None), dict(numel=None), dict(chunk_tensor=None), dict(chunk_off=None), dict(n=-1), dict(nchunks=-1),
                dict(chunk=0), dict(chunk=-4), dict(op=-1), dict(op=3), dict(rows=1)):
        assert call(**bad) == -1, bad
    assert lib.vilco_cl_accumulate(None, 1, 1.0, 0.0, None) == -1
    assert call(nchunks=0) == 0 and call(n=0, nchunks=0) == 0          # nothing to do: no launch, OK
