"""Pins the float64 restatement of the step kernels (tests/optim_restatement.py) to what it restates, without a GPU:
torch.optim.AdamW, torch.optim.SGD(momentum=0.9) and clip_grad_norm_ in float64, and the reference's penalty expression
(oracle.mq_oracle.cl_penalty) under autograd.  Everything is float64 on the CPU; the bar is 1e-13 relative."""
import warnings

import pytest
import torch

from optim_restatement import Stepper, clip, f32, penalty

TOL = 1e-13
SHAPES = [(30, 7), (5,), (400,), (1, 16, 1), (11, 3, 3), (64,)]
LRS, WDS = (1e-2, 3e-3, 2e-2), (0.05, 0.0, 0.01)


def _close(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max()) <= TOL * max(float(want.abs().max()), 1e-300)


def _groups(ps):
    """three groups with their own lr and weight decay; ps[2] is listed twice in group 1"""
    return [{"params": [ps[0], ps[1]], "lr": f32(LRS[0]), "weight_decay": f32(WDS[0])},
            {"params": [ps[2], ps[3], ps[2]], "lr": f32(LRS[1]), "weight_decay": f32(WDS[1])},
            {"params": [ps[4], ps[5]], "lr": f32(LRS[2]), "weight_decay": f32(WDS[2])}]


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
@pytest.mark.parametrize("max_norm", [-1.0, 0.5])
def test_stepper_matches_torch_optim(kind, max_norm):
    """6 steps; ps[1] has no gradient on step 3, ps[2] is stepped twice per iteration; parameters, state tensors and step
    counts agree with torch.optim, norm and coefficient with clip_grad_norm_"""
    gen = torch.Generator().manual_seed(0)
    ref_p = [torch.randn(s, dtype=torch.float64, generator=gen).requires_grad_(True) for s in SHAPES]
    my_p = [p.detach().clone() for p in ref_p]
    for p in my_p:
        p.grad = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # the duplicated parameter
        if kind == "AdamW":
            ref = torch.optim.AdamW(_groups(ref_p), lr=1e-2, betas=(f32(0.9), f32(0.999)), eps=f32(1e-8))
        else:
            ref = torch.optim.SGD(_groups(ref_p), lr=1e-2, momentum=f32(0.9))
    mine = Stepper(_groups(my_p), kind)
    want_steps = [0] * len(SHAPES)
    for it in range(6):
        for i, (a, b) in enumerate(zip(ref_p, my_p)):
            g = 3.0 * torch.randn(a.shape, dtype=torch.float64, generator=gen)
            a.grad, b.grad = (None, None) if (i == 1 and it == 3) else (g.clone(), g.clone())
            want_steps[i] += 0 if a.grad is None else (2 if i == 2 else 1)
        want_norm = None
        if max_norm > 0:
            live = [p for p in ref_p if p.grad is not None]
            want_norm = float(torch.nn.utils.clip_grad_norm_(live, f32(max_norm)))
            scaled = live[0].grad.clone()
        ref.step()
        norm, coef = mine.step(max_norm)
        if max_norm > 0:
            assert abs(norm - want_norm) <= TOL * want_norm and coef < 1.0
            assert _close(my_p[0].grad * coef, scaled)
        else:
            assert coef == 1.0
        for i, (a, b) in enumerate(zip(ref_p, my_p)):
            assert _close(b, a), (it, i)
            st, rs = mine.state.get(id(b)), ref.state[a]
            if kind == "AdamW":
                assert float(rs['step']) == st['step'] == want_steps[i], (it, i)
                assert _close(st['exp_avg'], rs['exp_avg']) and _close(st['exp_avg_sq'], rs['exp_avg_sq']), (it, i)
            else:
                assert st['step'] == want_steps[i] and 'step' not in rs            # torch.optim.SGD keeps no count
                assert _close(st['momentum_buffer'], rs['momentum_buffer']), (it, i)
    assert want_steps == [6, 5, 12, 6, 6, 6]


def test_clip_edges():
    g = [torch.tensor([3.0, 0.0]), torch.tensor([[4.0]])]
    assert clip(g, -1.0) == (5.0, 1.0) and clip(g, 0.0) == (5.0, 1.0)
    assert clip(g, 7.0) == (5.0, 1.0)
    norm, coef = clip(g, 0.5)
    assert norm == 5.0 and coef == 0.5 / (5.0 + 1e-6)
    assert clip([torch.zeros(4)], 0.5) == (0.0, 1.0) and clip([], 0.5) == (0.0, 1.0)


def test_penalty_matches_reference_expression():
    """two tasks; the class head had 4 rows when task 0 was consolidated and 7 at task 1, so task 0's entries cover a prefix of
    head.weight / head.bias; 'scale' is skipped by name as in EWC.py:15.  Value and gradient against the oracle + autograd."""
    from oracle.mq_oracle import cl_penalty
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)
    named = [("body.weight", rnd(5, 6)), ("head.weight", rnd(7, 5)), ("head.bias", rnd(7)), ("head.scale", rnd(1))]
    named = [(n, p.requires_grad_(True)) for n, p in named]
    rows = ({"body.weight": 5, "head.weight": 4, "head.bias": 4, "head.scale": 1},
            {"body.weight": 5, "head.weight": 7, "head.bias": 7})
    imps = [{n: rnd(r, *dict(named)[n].shape[1:]).abs() for n, r in d.items()} for d in rows]
    opts = [{n: rnd(r, *dict(named)[n].shape[1:]) for n, r in d.items()} for d in rows]
    lam = f32(0.37)
    base = [rnd(*p.shape) for _, p in named]                          # gradients that are already there
    want = cl_penalty(named, imps, opts, lam)
    want.backward()
    want = want.detach()
    entries = [(i, imp_d[n], opt_d[n]) for imp_d, opt_d in zip(imps, opts) for i, (n, _) in enumerate(named)
               if 'scale' not in n and n in imp_d]
    assert len(entries) == 6
    value, grads, mags = penalty([p for _, p in named], base, entries, lam)
    assert abs(value - float(want)) <= TOL * float(want) and mags['value_abs'] == value > 0
    for (n, p), b, g, k, s in zip(named, base, grads, mags['touched'], mags['abs_sum']):
        auto = torch.zeros_like(p) if p.grad is None else p.grad
        assert _close(g, b + auto), n
        assert bool((s >= g.abs() - 1e-12).all())
    assert mags['touched'][1][:4].eq(2).all() and mags['touched'][1][4:].eq(1).all() and mags['touched'][3].eq(0).all()
    assert torch.equal(grads[1][4:], base[1][4:] + named[1][1].grad[4:]) and torch.equal(grads[3], base[3])
