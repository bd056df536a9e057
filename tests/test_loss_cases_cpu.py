"""The table of tests/loss_cases.py, checked without a GPU: every case takes its decisions either exactly on a threshold (where
the case says so) or far enough from it that float32 decides as float64 does; the float64 reference itself behaves as the
kernel is held to at the one point where the two could differ by convention (a DIoU prediction equal to its target)."""
import dataclasses
import math

import pytest
import torch

import loss_cases as lc

KINDS = ('inside', 'far_lo', 'far_hi')
_audits = {}


def _audit(case):
    if case.name not in _audits:
        _audits[case.name] = lc.audit(case)
    return _audits[case.name]


def _entries(au, kind):
    for b, tab in enumerate(au[kind]):
        for pi, row in enumerate(tab or ()):
            for j, v in enumerate(row):
                yield b, pi, j, v


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_assignment_decisions_sit_on_a_threshold_or_well_away(case):
    au = _audit(case)
    for kind in KINDS:
        zeros = {(b, pi, j) for b, pi, j, v in _entries(au, kind) if v == 0.0}
        assert len(zeros) == lc.ON_EDGE[case.name][KINDS.index(kind)], (kind, len(zeros))
        for b, pi, j, v in _entries(au, kind):
            assert v == 0.0 or abs(v) >= (1e-4 if (b, j) in case.off_grid else 1e-2), (kind, b, pi, j, v)
        for k, b, level, q, j in case.named:
            if k != kind:
                continue
            pi = lc.point_index(case, level, q)
            assert (b, pi, j) in zeros, (k, b, level, q, j, au[kind][b][pi][j])
            # ... and that comparison alone decides the label there: a valid row, the other conditions hold with room
            assert au['valid'][b][pi] == 1
            others = {'inside': au['inside'][b][pi][j] > 0, 'far_lo': au['far_lo'][b][pi][j] >= 0, 'far_hi': au['far_hi'][b][pi][j] >= 0}
            assert all(ok for o, ok in others.items() if o != kind), (k, b, level, q, j)
    for b, pi, j, v in _entries(au, 'len'):
        assert math.isnan(v) or abs(v) >= 1e-4, ('len', b, pi, j, v)


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_al_scores_tie_bit_equal_or_not_at_all(case):
    au = _audit(case)
    for b in range(len(case.gts)):
        for c in range(case.ncls):
            best, second, gap = au['al_best'][b][c], au['al_second'][b][c], au['al_gap'][b][c]
            assert best == second or gap >= 1e-5, (b, c, best, second)
            if case.al_on:                  # 1 - score keeps five digits in float32, log(score) stays finite
                assert 1e-6 <= best <= 1 - 1e-2, (b, c, best)


def test_every_named_case_is_in_the_table():
    names = {c.name for c in lc.CASES}
    assert names == set(lc.ON_EDGE)
    for n in ('finish_BC_330', 'finish_nparts_260', 'rows_256', 'rows_257', 'rows_131', 'classes_1', 'classes_2', 'classes_32',
              'classes_33', 'classes_64', 'classes_65', 'classes_128', 'thresholds_radius', 'thresholds_none', 'near_ties',
              'al_tie_one_workgroup', 'al_tie_two_workgroups', 'masked_winner', 'no_level_scale', 'grad_final_only', 'grad_reg_only',
              'saturation_smooth_0', 'saturation_smooth_0.1', 'diou_zero_and_huge', 'diou_tie', 'empty_clip'):
        assert n in names, n


def test_shapes_reach_the_code_they_are_meant_for():
    def rows(c):
        return sum(c.Ts) + (lc.L - 1 if c.gaps else 0)
    c = lc.BY_NAME['finish_BC_330']
    assert len(c.gts) * c.ncls == 330 > 256
    c = lc.BY_NAME['finish_nparts_260']
    assert len(c.gts) * -(-rows(c) // 256) == 260 > 256 and all(1 <= len(g[1]) <= 2 for g in c.gts)
    assert [rows(lc.BY_NAME[n]) for n in ('rows_256', 'rows_257', 'rows_131')] == [256, 257, 131]
    for name, (a, b_) in (('al_tie_one_workgroup', ((0, 10), (0, 200))), ('al_tie_two_workgroups', ((0, 10), (1, 9)))):
        c = lc.BY_NAME[name]
        ra, rb = lc.device_row(c, *a), lc.device_row(c, *b_)
        assert (ra // 256 == rb // 256) == (name == 'al_tie_one_workgroup') and rb - ra == (190 if ra // 256 == rb // 256 else 256)
    c = lc.BY_NAME['thresholds_radius']          # t == ctr -+ 1.5 stride is outside while the neighbouring points are inside
    au = _audit(c)
    assert [au['inside'][1][lc.point_index(c, 1, q)][0] for q in (5, 6, 7, 8)] == [0.0, 2.0, 2.0, 0.0]
    c = lc.BY_NAME['empty_clip']
    assert [len(g[1]) for g in c.gts] == [2, 0, 3] and c.nmax == 4 and not c.al_on and c.gw[2:] == (None, None)


@pytest.mark.parametrize("name,pairs", [('al_tie_one_workgroup', ((0, 10), (0, 200))), ('al_tie_two_workgroups', ((0, 10), (1, 9)))])
def test_al_tie_rows_hold_the_class_maximum_and_the_first_gets_the_gradient(name, pairs):
    case = lc.BY_NAME[name]
    au, want = _audit(case), lc.expected(case)
    (l0, q0), (l1, q1) = pairs
    for b, c in ((0, 6), (1, 2)):
        assert au['al_row'][b][c] == lc.point_index(case, l0, q0) and au['al_best'][b][c] == au['al_second'][b][c]
        assert au['valid'][b][lc.point_index(case, l1, q1)] == 1
        # bit-identical logits, different gradient rows: torch.max sent the al gradient to the first
        first, later = want['dlogits'][l0][b, q0], want['dlogits'][l1][b, q1]
        assert float((first - later).abs().max()) > 1e-3 * float(first.abs().max())


def test_masked_row_wins_the_shifted_class():
    case = lc.BY_NAME['masked_winner']
    au = _audit(case)
    assert au['al_row_valid'][1][4] == 0 and au['al_best'][1][4] == 1.0 / case.ncls
    assert all(au['al_row_valid'][1][c] == 1 for c in range(case.ncls) if c != 4)


def test_reference_splits_the_diou_gradient_evenly_at_a_tie():
    """autograd through torch.min / torch.max at lp == lg: half of each side.  The reference gradient at the tie is the mean of
    the gradients just above and just below it, and those two differ: the kernel has one value to match."""
    case = lc.BY_NAME['diou_tie']
    h = 2.0 ** -20

    def moved(sign):
        edits = tuple((k, b, l, q, tuple(v + sign * h * (v == t) for v, t in zip(vals, tgt)))
                      for (k, b, l, q, vals), tgt in zip(case.edits, ((2.0, 2.0), (1.0, 3.0), (3.0, 1.0), (4.0, 4.0))))
        return lc.expected(dataclasses.replace(case, name='%s/%+d' % (case.name, sign), edits=edits))
    tie, up, down = lc.expected(case), moved(+1), moved(-1)
    for l, q, sides in ((1, 6, (0, 1)), (1, 5, (0,)), (1, 7, (1,)), (0, 12, (0, 1))):
        for s in sides:
            g, gu, gd = (float(w['doffsets'][l][0, q, s]) for w in (tie, up, down))
            assert abs(gu - gd) > 1e-2 * max(abs(gu), abs(gd)), (l, q, s, gu, gd)
            assert abs(g - 0.5 * (gu + gd)) < 1e-5 * abs(gu - gd), (l, q, s, g, gu, gd)


def test_non_positive_loss_weight_is_refused():
    """loss_weight <= 0 asks for cls / max(reg, 0.01) as the weight: the model routes that to the tensor expressions, the fused op
    must not multiply by the negative number"""
    from vilco_amd import ops
    z = torch.zeros(1, 4, 3)
    for w in (0.0, -1.0):
        with pytest.raises(ValueError, match="loss_weight"):
            ops.mq_loss(z, torch.zeros(1, 4, 2), None, torch.ones(6, 3), (torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32),
                        torch.zeros(4, dtype=torch.int32)), torch.ones(1, 1, dtype=torch.int32), torch.zeros(1, 4), torch.ones(1),
                        1.5, 0.0, 0.9, w, 0.2, True)
