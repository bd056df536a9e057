"""vilco_cl_accumulate on the device, and the consolidation pass built on it (importance='mean', merge='online') against the
float64 restatement (tests/importance_restatement.py).  Bounds are counted roundings of 2^-24, not measurements."""
import pytest
import torch

from importance_restatement import GrowToy, RecordingSGD, importance, toy_loader
from parity_util import cases, rel_err

U = 2.0 ** -24
pytestmark = pytest.mark.gpu


def _f64(x, op):
    x = x.double().cpu()
    return x if op == 0 else x * x if op == 1 else x.abs()


def _pairs(dev, seed=0):
    """(src, acc) pairs of every size class of the kernel: below one 16-byte access, around the wave, around one chunk, several
    chunks; src alone, acc alone and both starting one element into their allocation (not 16-byte aligned)"""
    from vilco_amd.ops import CL_CHUNK
    g = torch.Generator().manual_seed(seed)
    sizes = [1, 3, 63, 64, 65, CL_CHUNK - 1, CL_CHUNK, CL_CHUNK + 1, 2 * CL_CHUNK + 5, 2 * CL_CHUNK + 5]
    shift = {4: (1, 0), 7: (0, 1), 9: (1, 1)}                  # pair -> (src, acc) start offsets in elements
    srcs, accs = [], []
    for i, n in enumerate(sizes):
        so, ao = shift.get(i, (0, 0))
        srcs.append(torch.randn(n + so, generator=g).to(dev)[so:])
        accs.append(torch.randn(n + ao, generator=g).to(dev)[ao:])
        assert srcs[-1].data_ptr() % 16 == 4 * so and accs[-1].data_ptr() % 16 == 4 * ao
    return srcs, accs


@pytest.mark.parametrize("op", [0, 1, 2])
def test_kernel_matches_float64(dev, op):
    """|got - want| <= 4 * 2^-24 * (|beta acc| + |alpha f(x)|): f(x), alpha f(x) and the fused multiply-add round once each, and
    alpha / beta are rounded to fp32 on the way in"""
    from vilco_amd import ops
    alpha, beta = 0.7, -1.3
    srcs, accs = _pairs(dev, seed=op)
    before = [a.clone() for a in accs]
    ops.cl_accumulate(srcs, accs, op, alpha, beta)
    for s, a0, a in zip(srcs, before, accs):
        t1, t2 = beta * a0.double().cpu(), alpha * _f64(s, op)
        err = (a.double().cpu() - (t1 + t2)).abs()
        bound = 4 * U * (t1.abs() + t2.abs())
        print("op %d numel %d: max err / bound = %.3f" % (op, s.numel(), float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), (op, s.numel())


@pytest.mark.parametrize("op", [0, 1, 2])
def test_beta_zero_does_not_read_the_accumulator(dev, op):
    from vilco_amd import ops
    srcs, accs = _pairs(dev, seed=10 + op)
    for a in accs:
        a.fill_(float('nan'))
    ops.cl_accumulate(srcs, accs, op, 0.7, 0.0)
    for s, a in zip(srcs, accs):
        want = 0.7 * _f64(s, op)
        assert bool(torch.isfinite(a).all()), s.numel()
        assert bool(((a.double().cpu() - want).abs() <= 4 * U * want.abs()).all()), s.numel()


def test_prefix_leaves_the_rest_alone(dev):
    """numel shorter than the allocation: what lies past it, and the element in front of a view, keep their bits"""
    from vilco_amd import ops
    from vilco_amd.ops import CL_CHUNK
    g = torch.Generator().manual_seed(3)
    bufs = [torch.randn(n, generator=g).to(dev) for n in (100, 2 * CL_CHUNK + 1, 2 * CL_CHUNK + 1)]
    accs = [b[1:] for b in bufs]                             # element 0 of each buffer is the sentinel
    srcs = [torch.randn(a.numel() + 1, generator=g).to(dev)[so:so + a.numel()] for a, so in zip(accs, (0, 0, 1))]
    numels = [37, CL_CHUNK + 7, 2 * CL_CHUNK - 29]           # the last pair shares its misalignment: head, wide body, tail
    before = [b.clone() for b in bufs]
    ops.cl_accumulate(srcs, accs, 1, 0.7, -1.3, numels=numels)
    for b, b0, s, n in zip(bufs, before, srcs, numels):
        assert torch.equal(b[:1], b0[:1]) and torch.equal(b[1 + n:], b0[1 + n:])
        t1, t2 = -1.3 * b0[1:1 + n].double().cpu(), 0.7 * _f64(s[:n], 1)
        assert bool(((b[1:1 + n].double().cpu() - (t1 + t2)).abs() <= 4 * U * (t1.abs() + t2.abs())).all())
        assert not torch.equal(b[1:1 + n], b0[1:1 + n])


def test_repeated_calls_give_the_same_bits(dev):
    from vilco_amd import ops
    srcs, accs = _pairs(dev, seed=20)
    again = [a.clone() for a in accs]
    ops.cl_accumulate(srcs, accs, 1, 0.7, -1.3)
    ops.cl_accumulate(srcs, again, 1, 0.7, -1.3)
    assert all(torch.equal(a, b) for a, b in zip(accs, again))


def test_device_tensors_never_take_the_host_path(dev):
    from vilco_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cl_accumulate([torch.zeros(4)], [torch.zeros(4, device=dev)], 0, 1.0, 1.0)


@pytest.mark.parametrize("kind", ["ewc", "mas"])
def test_mean_importance_matches_restatement(dev, kind):
    """against the restatement fed with exactly the gradients the pass saw, N = 3 batches: (N + 2) * 2^-24 relative, elementwise
    (N adds, one square, one scale)"""
    from vilco_amd.cl_methods import regularizers
    key = 'fisher' if kind == 'ewc' else 'importance'
    model = cases.RegToy().to(dev)
    opt = RecordingSGD(model)
    reg = regularizers.on_task_update(cases.reg_toy_loader(dev), dev, opt, model, kind=kind, importance='mean')
    grads = opt.batches()
    assert len(grads) == 3 and len(reg[key]) == len(reg['optpar']) == 1
    want = importance(grads, kind, 'mean')
    got = reg[key][0]
    assert sorted(got) == sorted(want)
    for n, w in want.items():
        assert got[n].is_cuda and got[n].shape == w.shape
        err = (got[n].double().cpu() - w).abs()
        print("%s %s: max err / bound = %.3f" % (kind, n, float((err / (5 * U * w.abs()).clamp_min(1e-300)).max())))
        assert bool((err <= (3 + 2) * U * w.abs()).all()), n
        assert torch.equal(reg['optpar'][0][n], dict(model.named_parameters())[n].data)
    other = cases.RegToy().to(dev)
    last = regularizers.on_task_update(cases.reg_toy_loader(dev), dev, torch.optim.SGD(other.parameters(), lr=0.1), other, kind=kind)
    assert rel_err(got['body.weight'], last[key][0]['body.weight']) > 1e-2


@pytest.mark.parametrize("kind", ["ewc", "mas"])
def test_online_merge_with_a_growing_head(dev, kind):
    """Linear(5, 4) consolidated, grown to Linear(5, 7), consolidated again with gamma = 0.9: rows 0..3 are 0.9 F1 + F2 within
    3 * 2^-24 (the fp32 value of gamma, the product, the sum), rows 4..6 are F2's bits; one dictionary; the penalty kernel
    takes it as it is"""
    from vilco_amd.cl_methods import regularizers
    key = 'fisher' if kind == 'ewc' else 'importance'
    f = (lambda g: g.pow(2)) if kind == 'ewc' else (lambda g: g.abs())
    torch.manual_seed(7)
    model = GrowToy(4).to(dev)
    regularizers.on_task_update(toy_loader(30, dev), dev, torch.optim.SGD(model.parameters(), lr=0.1), model, kind=kind,
                                merge='online', gamma=0.9)
    F1 = {n: v.clone() for n, v in model.reg_params[key][0].items()}
    model.grow(7)
    with torch.no_grad():
        model.body.weight.add_(0.05)
    reg = regularizers.on_task_update(toy_loader(40, dev), dev, torch.optim.SGD(model.parameters(), lr=0.1), model, kind=kind,
                                      merge='online', gamma=0.9)
    F2 = {n: f(p.grad.detach()) for n, p in model.named_parameters()}          # 'last': the last batch's gradients are in p.grad
    assert len(reg[key]) == len(reg['optpar']) == 1
    got, params = reg[key][0], dict(model.named_parameters())
    assert sorted(got) == sorted(params) == sorted(reg['optpar'][0])
    for n, p in params.items():
        assert torch.equal(reg['optpar'][0][n], p.data), n
        k = F1[n].shape[0]
        want = 0.9 * F1[n].double().cpu() + F2[n][:k].double().cpu()
        assert bool(((got[n][:k].double().cpu() - want).abs() <= 3 * U * want.abs()).all()), n
        assert torch.equal(got[n][k:], F2[n][k:]), n
    assert got['head.weight'].shape == (7, 5) and F1['head.weight'].shape == (4, 5)

    # the merged state under the penalty: one entry per parameter (the kernel without atomics), value and gradient as autograd's
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(dev))
    items = regularizers._entries(model, kind)
    assert len({id(p) for p, _, _ in items}) == len(items) == len(params)
    zero = torch.zeros((), device=dev)
    want_pen = regularizers.get_regularized_loss(zero, model, 0.37, kind=kind)
    model.zero_grad(set_to_none=True)
    want_pen.backward()
    want_grad = {n: p.grad.clone() for n, p in params.items()}
    model.zero_grad(set_to_none=True)
    pen = regularizers.apply_penalty(model, 0.37, kind=kind)
    assert float(want_pen) > 0 and abs(float(pen) - float(want_pen)) <= 1e-5 * abs(float(want_pen))
    for n, p in params.items():
        assert rel_err(p.grad, want_grad[n]) < 1e-5, n
