"""ops.cl_distill (csrc/distill.hip: the iCaRL / BiC distillation term of MQ/libs/modeling/meta_archs.py:1482-1519 and its
gradient) against the fp64 restatement (tests/distill_restatement.py, tied to the oracle in test_distill_op_cpu.py).

Bounds (derived, not measured): the kernel works in fp32 from the same fp32 inputs the restatement reads.  A row's sum is a
lane-strided partial of <= 3 terms here followed by a 6-step wave tree, the rows are added in fp64: a few eps = 6e-8 each;
the device expf / log1pf / logf carry a few ulp per term.  Both stay far inside 1e-5 of the loss and 1e-5 of the largest
gradient element."""
import ctypes

import pytest
import torch

from parity_util import GRAD_FLOOR, rel_err
from distill_restatement import distill_grad, distill_loss

pytestmark = pytest.mark.gpu

LEVEL_T = (5, 2, 1)                     # a one-row level; rows that are no multiple of the four waves of a block
LEVEL_ROW = (0, 6, 9)                   # one separator row between the levels
R = 10
SHAPES = [(1, 1, 1), (7, 7, 3), (130, 130, 65), (130, 200, 130)]       # (C, ldt, n_known)
LOSS_TOL = GRAD_TOL = 1e-5


def _inputs(dev, C, ldt, kind="normal", seed=0):
    g = torch.Generator().manual_seed(1000 * C + ldt + seed)
    logits = 3 * torch.randn(2, R, C, generator=g)
    targets = torch.rand(sum(LEVEL_T), ldt, generator=g)            # rows do not sum to 1
    if kind == "extreme":
        logits = 80.0 * (2 * torch.randint(0, 2, (2, R, C), generator=g) - 1).float()
        targets = torch.randint(0, 2, (sum(LEVEL_T), ldt), generator=g).float()
    elif kind == "softmax":
        targets = torch.softmax(torch.randn(sum(LEVEL_T), ldt, generator=g), dim=1)
    return logits.to(dev), targets.to(dev)


def _run(logits, targets, n_known, mode, scale, clip, g=1.0):
    from vilco_amd import ops
    x = logits.clone().requires_grad_(True)
    loss = ops.cl_distill(x, LEVEL_ROW, LEVEL_T, targets, n_known, mode, scale, clip=clip)
    (g * loss).backward()
    return loss.detach(), x.grad


def _check(dev, C, ldt, n_known, mode, clip, kind="normal"):
    logits, targets = _inputs(dev, C, ldt, kind)
    scale = 0.01 * n_known / C
    loss, grad = _run(logits, targets, n_known, mode, scale, clip, g=1.7)
    want = distill_loss(logits.cpu(), LEVEL_ROW, LEVEL_T, targets.cpu(), n_known, mode, scale, clip)
    wgrad = distill_grad(logits.cpu(), LEVEL_ROW, LEVEL_T, targets.cpu(), n_known, mode, scale, clip, g=1.7)
    el, eg = rel_err(loss, want), rel_err(grad, wgrad, GRAD_FLOOR)
    print("C %d ldt %d n_known %d mode %d clip %d %s: loss %.9g want %.9g rel %.2e, grad rel %.2e" %
          (C, ldt, n_known, mode, clip, kind, float(loss), float(want), el, eg))
    assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
    assert el < LOSS_TOL, (el, float(loss), float(want))
    assert eg < GRAD_TOL, eg
    return logits, targets, loss, grad


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C,ldt,n_known", SHAPES)
def test_loss_and_gradient_match_the_restatement(dev, C, ldt, n_known, mode):
    _check(dev, C, ldt, n_known, mode, clip=0)


@pytest.mark.parametrize("mode", [0, 1])
def test_the_second_clip_of_the_batch(dev, mode):
    _check(dev, 130, 200, 130, mode, clip=1)
    _check(dev, 7, 7, 3, mode, clip=1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C,ldt,n_known", SHAPES)
def test_saturated_logits_and_hard_targets_stay_finite(dev, C, ldt, n_known, mode):
    """logits of +-80 against targets of exactly 0 and 1: bce and the half-temperature softmax must not overflow"""
    _check(dev, C, ldt, n_known, mode, clip=0, kind="extreme")


def test_bic_targets_that_are_a_distribution(dev):
    """the ordinary BiC case next to the unnormalised one above: sum_y p = 1 must not be assumed either way"""
    _check(dev, 130, 130, 65, 1, clip=0, kind="softmax")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("C,ldt,n_known", SHAPES)
def test_gradient_is_written_inside_the_footprint_only(dev, C, ldt, n_known, mode, clip):
    """vilco_cl_distill_bwd over a d_logits pre-filled with a sentinel: the other clip, the separator rows and the columns
    at or beyond n_known keep the sentinel's bits; the footprint holds the gradient"""
    from vilco_amd import _lib, ops
    lib = _lib.load()
    logits, targets = _inputs(dev, C, ldt)
    scale = 0.01 * n_known / C
    tab = ops._distill_levels(LEVEL_ROW, LEVEL_T, logits.device)
    d = ops._distill_desc(logits, targets, tab, n_known, mode, scale, clip)
    sentinel = -1234.5
    dl = torch.full_like(logits, sentinel)
    g = torch.full((1,), 1.7, device=dev)
    _lib.check(lib.vilco_cl_distill_bwd(ctypes.byref(d), g.data_ptr(), dl.data_ptr(), None))
    torch.cuda.synchronize()
    inside = torch.zeros(2, R, C, dtype=torch.bool, device=dev)
    for r, T in zip(LEVEL_ROW, LEVEL_T):
        inside[clip, r:r + T, :n_known] = True
    assert inside.sum().item() == sum(LEVEL_T) * n_known
    assert torch.equal(dl[~inside], torch.full_like(dl[~inside], sentinel))
    wgrad = distill_grad(logits.cpu(), LEVEL_ROW, LEVEL_T, targets.cpu(), n_known, mode, scale, clip, g=1.7)
    assert rel_err(dl[inside], wgrad.to(dev)[inside], GRAD_FLOOR) < GRAD_TOL
    _, grad = _run(logits, targets, n_known, mode, scale, clip, g=1.7)           # the autograd path: zeros outside
    assert torch.equal(grad[inside], dl[inside]) and torch.count_nonzero(grad[~inside]).item() == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_two_calls_return_the_same_bits(dev, mode):
    for C, ldt, n_known in SHAPES:
        logits, targets = _inputs(dev, C, ldt)
        a = _run(logits, targets, n_known, mode, 0.004, 0)
        b = _run(logits, targets, n_known, mode, 0.004, 0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_level_list_and_numpy_targets_take_the_same_kernel(dev):
    """the per-level list of logits (no separator rows) and NumPy targets: concatenated once, same numbers"""
    from vilco_amd import ops
    logits, targets = _inputs(dev, 7, 7)
    levels = [logits[:, r:r + T].contiguous() for r, T in zip(LEVEL_ROW, LEVEL_T)]
    want = ops.cl_distill(logits, LEVEL_ROW, LEVEL_T, targets, 3, 0, 0.0)
    views = list(targets.split(LEVEL_T))
    buf, lens = ops.distill_targets(views, logits.device)
    assert lens == LEVEL_T and buf.data_ptr() == targets.data_ptr()           # views of one buffer are taken as they are
    assert torch.equal(ops.cl_distill(levels, None, None, views, 3, 0, 0.0), want)
    assert torch.equal(ops.cl_distill(levels, None, None, [v.cpu().numpy() for v in views], 3, 0, 0.0), want)
    with pytest.raises(ValueError, match="level lengths"):
        ops.cl_distill(levels, None, None, views[:2] + [torch.zeros(2, 7, device=dev)], 3, 0, 0.0)


def test_many_rows_take_more_than_one_block_and_more_than_one_round(dev):
    """4100 + 3 rows: past the 1024-block cap of the grid, so waves own several rows each (the row-strided loop) -- the other
    cases run one block or two.  Same bounds: <= 2e3 fp64 row adds per wave do not show at 1e-5."""
    from vilco_amd import ops
    g = torch.Generator().manual_seed(5)
    lt, C, n_known = (4100, 3), 67, 66
    rows = (0, 4101)
    logits = (3 * torch.randn(1, 4104, C, generator=g)).to(dev)
    targets = torch.rand(sum(lt), 70, generator=g).to(dev)
    for mode in (0, 1):
        x = logits.clone().requires_grad_(True)
        loss = ops.cl_distill(x, rows, lt, targets, n_known, mode, 0.003)
        loss.backward()
        want = distill_loss(logits.cpu(), rows, lt, targets.cpu(), n_known, mode, 0.003)
        wgrad = distill_grad(logits.cpu(), rows, lt, targets.cpu(), n_known, mode, 0.003)
        assert rel_err(loss, want) < LOSS_TOL and rel_err(x.grad, wgrad, GRAD_FLOOR) < GRAD_TOL
