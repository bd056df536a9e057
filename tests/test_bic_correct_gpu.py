"""GPU: ops.bic_correct (csrc/bic.hip: vilco_bic_correct_fwd / _bwd) against the float64 restatement
(tests/bic_correct_restatement.py).

Shapes: B = 2 clips of pyramid levels 16, 8, 4, 2 (and 3, 1) laid out as LevelCat does, one separator row between levels --
R = 33 (and 5) rows; dense rows and rows at a stride above C; C = 12 / splits (3, 7, 12), C = 5 / one split, C = 128 / splits
(1, 2, 65, 128): a split of width 1 and one across the 64-lane boundary; at C = 128 the forward runs 9 workgroups and the
parameter-gradient reduction 3.  alpha = -1.5, 0, 37 (, 0.75), beta of both signs, logits in +-30.

What the forward defines for the rows nobody labels: EVERY row of [B, R] gets alpha x + beta -- separator rows and rows past a
clip's valid length are not special (the ATen module does the same to a level's padded rows, which the distillation term reads).

Bounds, from fp32 rounding alone (u = 2^-24 per rounding; alpha, beta, x, dy are fp32 values, the restatement is exact in them):
  forward   two roundings, fl(fl(a x) + b):   |err| <= 2^-23 (|a x| + |b|)
  dx        one rounding:                      |err| <= 2^-23 |a dy|
  dalpha_i, dbeta_i   exact products and fp64 sums, one rounding of the total:   |err| <= 2^-23 sum |terms|
Every case prints its worst error / bound ratio (run with -s); they are expected far below 1."""
import numpy as np
import pytest
import torch

import bic_correct_restatement as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
ALPHAS, BETAS = (-1.5, 0.0, 37.0, 0.75), (0.5, -2.0, 0.25, -0.125)
SENTINEL = -12345.678
CASES = [
    ("C12", (16, 8, 4, 2), 12, (3, 7, 12), 0),
    ("C12-stride", (16, 8, 4, 2), 12, (3, 7, 12), 5),
    ("C5", (3, 1), 5, (5,), 0),
    ("C5-stride", (3, 1), 5, (5,), 3),
    ("C128", (16, 8, 4, 2), 128, (1, 2, 65, 128), 0),
    ("C128-stride", (16, 8, 4, 2), 128, (1, 2, 65, 128), 1),
]


def _layers(dev, n, requires_grad=True):
    from vilco_amd.modeling.meta_archs import BiasLayer
    layers = [BiasLayer().to(dev) for _ in range(n)]
    with torch.no_grad():
        for l, a, b in zip(layers, ALPHAS, BETAS):
            l.alpha.fill_(a)
            l.beta.fill_(b)
    for l in layers:
        for p in l.parameters():
            p.requires_grad = requires_grad
    return layers


def _data(levels, C, seed):
    """x, dy [2, R, C] float32 in the LevelCat row layout: zero separator rows between levels, as the head leaves them"""
    R_ = sum(levels) + len(levels) - 1
    r = np.random.RandomState(seed)
    x = r.uniform(-30, 30, (2, R_, C)).astype(np.float32)
    dy = r.uniform(-1, 1, (2, R_, C)).astype(np.float32)
    row = 0
    for T in levels[:-1]:
        row += T
        x[:, row] = 0.0
        row += 1
    return x, dy


def _in_buffer(x, pad, dev, guard=8):
    """x as a view of rows at stride C + pad inside a sentinel-filled buffer with `guard` floats in front and behind"""
    B, R_, C = x.shape
    ld = C + pad
    buf = torch.full((guard + B * R_ * ld + guard,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf.as_strided((B, R_, C), (R_ * ld, ld, 1), guard)
    view.copy_(torch.from_numpy(x))
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside.as_strided((B, R_, C), (R_ * ld, ld, 1), guard).fill_(True)
    return buf, view, inside


def _ratio(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ok = bound > 0
    assert np.all(err[~ok] == 0.0)                                 # a zero bound (alpha = 0 = beta) admits no error
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("name,levels,C,splits,pad", CASES, ids=[c[0] for c in CASES])
def test_forward_and_gradients_against_the_restatement(dev, name, levels, C, splits, pad):
    from vilco_amd import ops
    S = len(splits)
    layers = _layers(dev, S)
    al, be = ALPHAS[:S], BETAS[:S]
    x, dy = _data(levels, C, 11 + C + pad)
    buf, xv, _ = _in_buffer(x, pad, dev)
    xv.requires_grad_(True)
    y = ops.bic_correct(xv, splits, layers)
    assert y.shape == xv.shape and y.is_contiguous()
    want = R.forward(x, splits, al, be)
    r_f = _ratio(y.detach().cpu().numpy(), want, U * R.forward_terms(x, splits, al, be))
    dyt = torch.from_numpy(dy).to(dev)
    gx, = torch.autograd.grad(y, xv, dyt, retain_graph=True)
    r_x = _ratio(gx.cpu().numpy(), R.dx(dy, splits, al), U * np.abs(R.dx(dy, splits, al)))
    runs = []
    for _ in range(2):                                              # two launches of the backward: the same bits
        for l in layers:
            l.alpha.grad = l.beta.grad = None
        y.backward(dyt, retain_graph=True)
        runs.append((torch.cat([l.alpha.grad for l in layers]).clone(), torch.cat([l.beta.grad for l in layers]).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    da, db, ta, tb = R.dparams(dy, x, splits)
    r_a = _ratio(runs[0][0].cpu().numpy(), da, U * ta)
    r_b = _ratio(runs[0][1].cpu().numpy(), db, U * tb)
    print("bic_correct %-12s worst error / bound: forward %.3f  dx %.3f  dalpha %.3f  dbeta %.3f" % (name, r_f, r_x, r_a, r_b))
    assert r_f <= 1.0 and r_x <= 1.0 and r_a <= 1.0 and r_b <= 1.0, (name, r_f, r_x, r_a, r_b)
    # separator rows (x = 0) and every other row alike: beta of the column's split
    sep = levels[0]
    assert torch.equal(y[:, sep], torch.tensor(np.repeat(be, np.diff((0,) + splits)), dtype=torch.float32, device=dev).expand(2, C))


@pytest.mark.parametrize("name,levels,C,splits,pad", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("guard", [8, 7], ids=["aligned", "unaligned"])
def test_in_place_equals_out_of_place_and_writes_nothing_else(dev, name, levels, C, splits, pad, guard):
    """frozen layers; the buffer around and between the rows keeps its sentinel: nothing outside [B, R, C] is written"""
    from vilco_amd import ops
    layers = _layers(dev, len(splits), requires_grad=False)
    x, _ = _data(levels, C, 3 + C)
    buf, xv, inside = _in_buffer(x, pad, dev, guard)
    with torch.no_grad():
        out = ops.bic_correct(xv, splits, layers)
        dense = ops.bic_correct(torch.from_numpy(x).to(dev), splits, layers)
        assert torch.equal(buf[~inside], torch.full_like(buf[~inside], SENTINEL))          # out of place: the input untouched
        assert torch.equal(xv, torch.from_numpy(x).to(dev))
        ret = ops.bic_correct(xv, splits, layers, inplace=True)
    assert ret.data_ptr() == xv.data_ptr()
    assert torch.equal(xv, out) and torch.equal(dense, out)                                # bit-equal, whatever the path
    assert torch.equal(buf[~inside], torch.full_like(buf[~inside], SENTINEL))
    assert (~inside).sum().item() == 2 * guard + pad * xv.shape[0] * xv.shape[1]


def test_frozen_layers_get_no_gradient_and_no_reduction(dev):
    from vilco_amd import ops
    splits = (3, 7, 12)
    layers = _layers(dev, 3, requires_grad=False)
    layers[1].alpha.requires_grad = True                            # one parameter of one layer only
    x, dy = _data((3, 1), 12, 2)
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    ops.bic_correct(xt, splits, layers).backward(torch.from_numpy(dy).to(dev))
    assert [l.alpha.grad is None for l in layers] == [True, False, True] and all(l.beta.grad is None for l in layers)
    da, _, ta, _ = R.dparams(dy, x, splits)
    assert abs(float(layers[1].alpha.grad) - da[1]) <= U * ta[1]
    np.testing.assert_array_equal(xt.grad.cpu().numpy(), R.dx(dy, splits, ALPHAS[:3]).astype(np.float32))
    # all frozen: backward is the dx launch alone, no gradient tensor anywhere
    layers[1].alpha.requires_grad = False
    layers[1].alpha.grad = None
    xt.grad = None
    ops.bic_correct(xt, splits, layers).backward(torch.from_numpy(dy).to(dev))
    assert all(p.grad is None for l in layers for p in l.parameters()) and xt.grad is not None
    with pytest.raises(RuntimeError, match="in place"):
        layers[0].beta.requires_grad = True
        ops.bic_correct(torch.from_numpy(x).to(dev), splits, layers, inplace=True)


def test_values_written_after_the_first_call_are_seen(dev):
    """alpha / beta are read from the layers' memory by the kernel: no table is rebuilt when they change -- what a replayed
    graph relies on after stage 2"""
    from vilco_amd import ops
    splits = (3, 7, 12)
    layers = _layers(dev, 3, requires_grad=False)
    x, _ = _data((3, 1), 12, 4)
    xt = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        first = ops.bic_correct(xt, splits, layers)
        n_tabs = len(ops._bic_tabs)
        layers[2].alpha.data.fill_(0.625)
        layers[2].beta.data.fill_(-3.0)
        second = ops.bic_correct(xt, splits, layers)
    assert len(ops._bic_tabs) == n_tabs
    al, be = ALPHAS[:2] + (0.625,), BETAS[:2] + (-3.0,)
    assert _ratio(second.cpu().numpy(), R.forward(x, splits, al, be), U * R.forward_terms(x, splits, al, be)) <= 1.0
    assert torch.equal(first[..., :7], second[..., :7]) and not torch.equal(first[..., 7:], second[..., 7:])


def test_bad_tables_and_foreign_tensors_raise(dev):
    from vilco_amd import ops
    from vilco_amd.modeling.meta_archs import BiasLayer
    x = torch.zeros(2, 5, 12, device=dev)
    layers = _layers(dev, 3, requires_grad=False)
    for splits, ls in [((), []), ((3, 3, 12), layers), ((3, 7), layers[:2]), ((3, 7, 12), layers + layers[:1])]:
        with pytest.raises(ValueError, match="bic_correct"):
            ops.bic_correct(x, splits, ls)
    with pytest.raises(ValueError, match="at most 128"):
        ops.bic_correct(torch.zeros(2, 5, 129, device=dev), (3, 129), layers[:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bic_correct(x.cpu(), (3, 7, 12), layers)
    with pytest.raises(RuntimeError, match="lives on"):
        ops.bic_correct(x, (3, 7, 12), layers[:2] + [BiasLayer()])
