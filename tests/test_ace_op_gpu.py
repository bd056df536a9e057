"""ops.mq_loss_ace (vilco_mq_loss_ace_fwd / _bwd, csrc/loss.hip with WIN = true) against the float64 restatement of
tests/ace_restatement.py, at the tolerances of loss_cases.check: three clips, two pyramid levels with a separator row, R = 257
(one workgroup and one row) and R = 61 (less than one), C and the windows on both sides of the kernel's 32-bit bitset words."""
import dataclasses

import pytest
import torch

import ace_restatement as A
import loss_cases as LC

pytestmark = pytest.mark.gpu

BIG, SMALL = (170, 86), (40, 20)                  # + 1 separator row: R = 257 = LT + 1 and R = 61 < LT
LENS = {BIG: (170, 150, 101), SMALL: (40, 33, 25)}
GTS5 = (LC._spread((0, 3, 4, 1)), LC._spread((2, 4), 1.0), LC._spread((4, 1, 3), 2.5))
# (every clip holds the last class: under a window of that class alone its score is 1 and -log(1 - score) is for nobody)
GTS65 = (LC._spread((0, 31, 32, 64)), LC._spread((33, 64, 5), 1.0), LC._spread((64, 31), 2.5))
# a row of C = 5 logits whose class-3 score over any window that holds class 3 stays below 1 - 1e-2
TOP3 = (-2.0, -2.0, -2.0, 3.0, -2.0)


def _case(name, C, Ts, seed, **kw):
    kw.setdefault('gts', GTS5 if C == 5 else GTS65)
    if C == 5:       # windows of two or three classes: a logit spread of 2 would push the best softmax score past 1 - 1e-2
        kw.setdefault('logit_std', 0.5)
        kw.setdefault('logit_mean', 0.0)
    return LC.Case(name, C, Ts, kw.pop('gts'), LENS[Ts], seed=seed, **kw)


GRID = [(_case('c5_%s' % ('big' if Ts == BIG else 'small'), 5, Ts, 201 + i), lo)
        for i, Ts in enumerate((BIG, SMALL)) for lo in ((0, 0, 0), (2, 2, 2), (4, 4, 4), (0, 2, 4))]
GRID += [(_case('c65_%s' % ('big' if Ts == BIG else 'small'), 65, Ts, 211 + i), lo)
         for i, Ts in enumerate((BIG, SMALL)) for lo in ((31, 31, 31), (32, 32, 32), (33, 33, 33), (64, 64, 64), (0, 32, 64))]

NAMED = [
    # an al tie between two rows inside the window: level 0 q 10 and q 30 of clip 0 hold the same logits and the best class-3
    # score of the clip; the first row wins and takes the gradient (torch.max does the same)
    (_case('al_tie_in_window', 5, BIG, 221, edits=(('logits', 0, 0, 10, TOP3), ('logits', 0, 0, 30, TOP3))), (2, 2, 0)),
    # ... and across the two workgroups of R = 257: device rows 10 and 171 + 85 = 256
    (_case('al_tie_two_workgroups', 5, BIG, 222, edits=(('logits', 0, 0, 10, TOP3), ('logits', 0, 1, 85, TOP3))), (2, 0, 4)),
    # class 4 of clip 1 is pushed below the uniform 1 / (C - lo) on every valid row: a masked row holds the maximum
    (_case('masked_winner', 5, SMALL, 223, edits=(('logit_shift', 1, 4, -14.0),)), (2, 2, 2)),
    (_case('masked_winner_lo0', 5, SMALL, 223, edits=(('logit_shift', 1, 4, -14.0),)), (0, 0, 0)),
    # clip 1's only GT class (1) lies below its window: its rows stay positive for regression, no classification bit is visited
    (_case('gt_below_window', 5, SMALL, 224, gts=(GTS5[0], LC._spread((1,), 1.0), GTS5[2])), (0, 2, 4)),
    (_case('gt_below_window_65', 65, BIG, 225, gts=(GTS65[0], LC._spread((31, 5), 1.0), GTS65[2])), (0, 32, 64)),
    (_case('gt_below_single_class_window', 5, SMALL, 233, gts=(GTS5[0], LC._spread((1, 3), 1.0), GTS5[2]), use_al=False), (0, 4, 4)),
    # a clip without GT, the table padded to 5 slots
    (_case('clip_without_gt', 5, SMALL, 226, gts=(GTS5[0], ([], []), GTS5[2]), nmax=5), (2, 2, 0)),
    (_case('use_al_0', 5, SMALL, 227, use_al=False), (0, 2, 4)),
    (_case('no_level_scale', 5, BIG, 228, scale=False), (0, 2, 4)),
    (_case('grad_final_only', 5, SMALL, 229, gw=(None, None, None, 1.0)), (0, 2, 4)),
    (_case('grad_cls_al_only', 65, SMALL, 230, gw=(0.7, None, -0.4, None)), (0, 32, 64)),
    (_case('grad_reg_only', 5, SMALL, 231, gw=(None, 1.0, None, None)), (4, 2, 0)),
    (_case('smoothing', 65, SMALL, 232, smoothing=0.1), (33, 0, 64)),
]


def _id(v):
    return v.name if isinstance(v, LC.Case) else "lo_" + "_".join(str(x) for x in v)


@pytest.mark.parametrize("case,lo", GRID + NAMED, ids=_id)
def test_windowed_loss_is_the_restatement(dev, case, lo):
    want, got = A.expected(case, lo), A.run_device(case, dev, lo)
    print("%s lo=%s: losses %s" % (case.name, lo, {k: (got['losses'][k], want['losses'][k]) for k in LC.LOSS_KEYS}))
    LC.check(case, want, got)
    # below the window: exactly zero, every element assigned
    for l, g in enumerate(got['dlogits']):
        assert bool(torch.isfinite(g).all())
        for b, lo_b in enumerate(lo):
            assert bool((g[b, :, :lo_b] == 0).all()), (l, b)


def test_named_cases_decide_what_they_say():
    """on the restatement (CPU numbers): the tie, the masked winner, the GT below the window and the empty clip are in the data"""
    by = {c.name: (c, lo) for c, lo in NAMED}
    c, lo = by['al_tie_in_window']
    d = A.build(c)
    x = torch.cat(d['logits'], 1)[0, :, lo[0]:].softmax(-1)[:, 3 - lo[0]]
    assert x[10] == x[30] == x.max() and int((x == x.max()).sum()) == 2
    assert float(x.max()) < 1 - 1e-2
    only_al = A.expected(dataclasses.replace(c, name='al_tie_al_only', gw=(None, None, 1.0, None)), lo)['dlogits'][0]
    assert bool((only_al[0, 10, lo[0]:] != 0).all()) and bool((only_al[0, 30] == 0).all()), "the first of the tied rows takes the gradient"
    c, lo = by['al_tie_two_workgroups']
    assert LC.device_row(c, 0, 10) == 10 and 170 + 1 + 85 == 256 == A.device_inputs(c, torch.device('cpu'))['lg'].shape[1] - 1
    c, lo = by['masked_winner']
    assert abs(float(A.expected(c, lo)['al_score'][1, 4]) - 1.0 / 3) < 1e-15
    assert abs(float(A.expected(by['masked_winner_lo0'][0], (0, 0, 0))['al_score'][1, 4]) - 1.0 / 5) < 1e-15
    c, lo = by['gt_below_window']
    full, win = A.expected(c, (0, 0, 4)), A.expected(c, lo)
    assert win['losses']['reg_loss'] == full['losses']['reg_loss'] > 0 and win['norm'] == full['norm']
    assert any(bool((t[1] != 0).any()) for t in win['doffsets']), "clip 1's rows are positive for regression"
    c, lo = by['clip_without_gt']
    assert all(bool((t[1] == 0).all()) for t in A.expected(c, lo)['doffsets'])


BITS = [GRID[0][0], GRID[4][0], GRID[8][0], GRID[13][0], NAMED[5][0], NAMED[6][0], NAMED[7][0], NAMED[8][0], NAMED[10][0]]


@pytest.mark.parametrize("case", BITS, ids=_id)
def test_all_zero_table_is_the_plain_op_bit_for_bit(dev, case):
    """outputs, saved normaliser = loss_norm after the call, all four gradients; almax_state left zero by both"""
    plain = A.run_device(case, dev, plain=True)
    ace = A.run_device(case, dev, [0] * len(case.gts))
    assert A.raw_equal(plain['raw'], ace['raw'])
    assert plain['almax_clean'] and ace['almax_clean'] and ace['final_again'] == plain['final_again']
    assert ace['losses'] == plain['losses'] and ace['norm'] == plain['norm']


@pytest.mark.parametrize("case", [GRID[3][0], GRID[13][0]], ids=_id)
def test_out_of_range_windows_are_zero(dev, case):
    C = case.ncls
    full = A.run_device(case, dev, [0, 0, 0])
    assert A.raw_equal(full['raw'], A.run_device(case, dev, [-1, C, C + 1000])['raw'])
    assert A.raw_equal(full['raw'], A.run_device(case, dev, [-2 ** 31, 2 ** 31 - 1, -1])['raw'])
    one = A.run_device(case, dev, [C - 1, -1, C])
    assert A.raw_equal(one['raw'], A.run_device(case, dev, [C - 1, 0, 0])['raw']) and not torch.equal(one['raw']['out'], full['raw']['out'])


def test_two_calls_give_the_same_bits(dev):
    case, lo = GRID[-1]
    assert A.raw_equal(A.run_device(case, dev, lo)['raw'], A.run_device(case, dev, lo)['raw'])


def test_table_rewritten_in_place_changes_the_next_call(dev):
    """the kernels read the caller's table when they run: no copy is kept from an earlier call"""
    case, lo = GRID[3]
    x = A.device_inputs(case, dev)
    x = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in x.items()}
    tab = torch.zeros(3, dtype=torch.int32, device=dev)
    first = torch.stack(A.call(case, x, torch.full((1,), A.INIT_NORM, device=dev), tab))
    tab.copy_(torch.tensor(lo, dtype=torch.int32))
    second = torch.stack(A.call(case, x, torch.full((1,), A.INIT_NORM, device=dev), tab))
    tab.zero_()
    third = torch.stack(A.call(case, x, torch.full((1,), A.INIT_NORM, device=dev), tab))
    want0, want1 = A.expected(case, None)['losses'], A.expected(case, lo)['losses']
    assert torch.equal(first, third) and not torch.equal(first, second)
    for got, want in ((first, want0), (second, want1)):
        for i, k in enumerate(LC.LOSS_KEYS):
            assert abs(float(got[i]) - want[k]) <= case.loss_tol * max(abs(want[k]), 1e-3), k
    assert second[1] == first[1] and second[0] < first[0], "same regression loss, a smaller classification sum"


def test_refusals(dev):
    from vilco_amd import ops
    case = GRID[4][0]
    x = A.device_inputs(case, dev)
    norm = torch.full((1,), A.INIT_NORM, device=dev)
    args = (x['lg'], x['of'], x['sc'], x['gauss'], x['tables'], x['lvl_len'], x['gt'], norm, 1.5, 0.0, 0.9, 1.0, 0.2, True)
    for bad, exc in ((torch.zeros(3, dtype=torch.int64, device=dev), ValueError), (torch.zeros(4, dtype=torch.int32, device=dev), ValueError),
                     (torch.zeros(3, 1, dtype=torch.int32, device=dev), ValueError), (torch.zeros(3, dtype=torch.int32), RuntimeError),
                     (torch.zeros(6, dtype=torch.int32, device=dev)[::2], ValueError), (None, ValueError)):
        with pytest.raises(exc, match="cls_lo"):
            ops.mq_loss_ace(*args, bad)
    # C = 129: refused by the library, nothing launched -- the normaliser and the packed-maximum state are untouched
    wide = torch.zeros(3, x['lg'].shape[1], 129, device=dev)
    with pytest.raises(RuntimeError):
        ops.mq_loss_ace(wide, x['of'], x['sc'], torch.ones(6, 129, device=dev), *args[4:], torch.zeros(3, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert float(norm) == A.INIT_NORM
    state = ops._almax_state.get((dev.index, 3 * 129))
    assert state is None or bool((state == 0).all())
    # and the op still works afterwards
    got = ops.mq_loss_ace(*args, torch.tensor([0, 2, 4], dtype=torch.int32, device=dev))
    assert bool(torch.isfinite(torch.stack(got)).all())
