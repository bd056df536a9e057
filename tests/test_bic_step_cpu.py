"""CPU: the contract of the BiC stage-1 step without a GPU.  The restatement (tests/bic_correct_restatement.py) equals the
oracle's bias layers on the recorded splits and values, the split table is validated on the host -- in ops and again in
the C launcher, before any device work --, the driver takes `use_graph`, and a CPU model keeps the reference's loop."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import bic_correct_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("vilco_bic_correct_fwd", "vilco_bic_correct_bwd_workspace", "vilco_bic_correct_bwd")


def test_restatement_equals_the_oracle_on_the_recorded_layers():
    from oracle import mq_oracle as O
    g = torch.load(os.path.join(HERE, "golden", "distill.pt"), weights_only=False)['bic']
    splits, alphas, betas = g['splits'], g['alphas'], g['betas']
    C = splits[-1]
    r = np.random.RandomState(5)
    x = r.uniform(-30, 30, (2, 9, C))
    dy = r.uniform(-1, 1, (2, 9, C))
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(alphas, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(betas, dtype=torch.float64, requires_grad=True)
    y = O.bic_correct(xt, splits, a, b)
    y.backward(torch.tensor(dy))
    np.testing.assert_allclose(R.forward(x, splits, alphas, betas), y.detach().numpy(), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(R.dx(dy, splits, alphas), xt.grad.numpy(), rtol=1e-14, atol=1e-14)
    da, db, _, _ = R.dparams(dy, x, splits)
    np.testing.assert_allclose(da, a.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(db, b.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_abi_symbols_declared_and_bound():
    from vilco_amd import _lib, ops
    with open(os.path.join(os.path.dirname(HERE), "include", "vilco_hip.h")) as h:
        header = h.read()
    for name in NEW:
        assert name + "(" in header and name in _lib.SIGNATURES, name
    assert "meta_archs.py:26-35" in header and ":821-836" in header
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)
    assert ctypes.sizeof(_lib.BicCorrectDesc) == lib.vilco_abi_sizeof(b"vilco_bic_correct_desc") > 0
    assert callable(ops.bic_correct)


def _desc(splits, C, n_layers=None, rows=8):
    from vilco_amd import _lib
    arr = (ctypes.c_int32 * max(len(splits), 1))(*splits)
    d = _lib.BicCorrectDesc()
    d.x = d.y = d.table = 4096                       # dummy aligned addresses: every check precedes the launch
    d.splits = ctypes.addressof(arr) if splits else None
    d.rows, d.C, d.S, d.ldx, d.ldy = rows, C, len(splits), C, C
    d.n_layers = len(splits) if n_layers is None else n_layers
    return d, arr


BAD_TABLES = [
    ("an empty table", (), 12, None, -1),
    ("a non-increasing table", (3, 3, 12), 12, None, -1),
    ("a decreasing table", (7, 3, 12), 12, None, -1),
    ("last != C", (3, 7), 12, None, -1),
    ("last past C", (3, 13), 12, None, -1),
    ("C > 128", (3, 129), 129, None, -2),
    ("more layers than splits", (3, 7, 12), 12, 4, -1),
]


@pytest.mark.parametrize("what,splits,C,n_layers,status", BAD_TABLES, ids=[b[0] for b in BAD_TABLES])
def test_split_table_is_validated_on_the_host(what, splits, C, n_layers, status):
    from vilco_amd import _lib, ops
    lib = _lib.load()
    d, keep = _desc(splits, C, n_layers)
    assert lib.vilco_bic_correct_fwd(ctypes.byref(d), None) == status, what
    assert lib.vilco_bic_correct_bwd(ctypes.byref(d), None, C, None, None, 0, None) == status, what
    with pytest.raises(ValueError, match="bic_correct"):
        ops.bic_split_table(splits, C, len(splits) if n_layers is None else n_layers)


def test_other_arguments_are_validated_on_the_host():
    from vilco_amd import _lib, ops
    from vilco_amd.modeling.meta_archs import BiasLayer
    lib = _lib.load()
    assert ops.bic_split_table([3, 7, 12], 12, 3) == (3, 7, 12)
    d, keep = _desc((3, 7, 12), 12)
    d.ldx = 11
    assert lib.vilco_bic_correct_fwd(ctypes.byref(d), None) == -1            # a row stride below C
    d, keep = _desc((3, 7, 12), 12)
    d.table = None
    assert lib.vilco_bic_correct_fwd(ctypes.byref(d), None) == -1
    d, keep = _desc((3, 7, 12), 12, rows=1 << 24)
    assert lib.vilco_bic_correct_fwd(ctypes.byref(d), None) == -2            # rows * C would pass 2^31
    d, keep = _desc((3, 7, 12), 12, rows=0)
    assert lib.vilco_bic_correct_fwd(ctypes.byref(d), None) == 0             # nothing to launch
    d, keep = _desc((3, 7, 12), 12)
    assert lib.vilco_bic_correct_bwd(ctypes.byref(d), 4096, 12, 4096, 4096, 16, None) == -4     # parameter gradients: workspace
    assert lib.vilco_bic_correct_bwd(ctypes.byref(d), None, 12, 4096, 4096, 1 << 20, None) == -1
    assert lib.vilco_bic_correct_bwd_workspace(-1) == 0 and lib.vilco_bic_correct_bwd_workspace(100) > 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bic_correct(torch.zeros(2, 5, 12), [3, 7, 12], [BiasLayer() for _ in range(3)])


def test_driver_takes_use_graph():
    from vilco_amd.train_cl import run_episodes, run_episodes_bic
    p = inspect.signature(run_episodes_bic).parameters
    assert 'use_graph' in p and p['use_graph'].default is False
    assert inspect.signature(run_episodes).parameters['use_graph'].default is False


def test_cpu_model_walks_the_python_loop(monkeypatch):
    """on a CPU model `_bic_correct` never reaches the device op, and its result is the oracle's"""
    from oracle import mq_oracle as O
    from vilco_amd import ops
    from vilco_amd.modeling.meta_archs import BiasLayer, PtTransformer

    def boom(*a, **k):
        raise AssertionError("the device op was called for a CPU tensor")
    monkeypatch.setattr(ops, "bic_correct", boom)

    class Head:
        class cls_head:
            class conv:
                out_channels = 12
    m = PtTransformer.__new__(PtTransformer)
    torch.nn.Module.__init__(m)
    object.__setattr__(m, "cls_head", Head)
    m.list_splits, m.list_bias_layers, m._cat = [3, 7, 12], [BiasLayer() for _ in range(3)], None
    with torch.no_grad():
        for l, (a, b) in zip(m.list_bias_layers, [(-1.5, 0.5), (0.0, -2.0), (37.0, 0.25)]):
            l.alpha.fill_(a)
            l.beta.fill_(b)
    assert m._bic_op_ready()
    x = torch.randn(2, 6, 12)
    want = O.bic_correct(x, m.list_splits, [l.alpha.item() for l in m.list_bias_layers], [l.beta.item() for l in m.list_bias_layers])
    assert torch.equal(m._bic_correct(x), want)
    levels = m._bic_correct_levels([x[:, :4], x[:, 4:]])
    assert torch.equal(torch.cat(levels, dim=1), want)
