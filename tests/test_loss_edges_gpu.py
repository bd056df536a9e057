"""ops.mq_loss (csrc/loss.hip) against the float64 oracle at the edges of its decisions: the table of tests/loss_cases.py --
strided loops of the finish kernel, row and class counts at the workgroup / bitset-word boundaries, points exactly on the
assignment thresholds, near-ties of the GT length, ties of the packed "al" maximum, a masked winner, level_scale=None, partial
upstream gradients, saturated logits, DIoU corners, a clip without GT.  tests/test_loss_cases_cpu.py shows that every case
takes its decisions away from float32 rounding (or exactly on a threshold)."""
import pytest
import torch

import loss_cases as lc
from parity_util import rel_err

pytestmark = pytest.mark.gpu

_got = {}


def _run(name, dev):
    """one device run per case, shared by the parametrised test and the named ones"""
    case = lc.BY_NAME[name]
    if name not in _got:
        _got[name] = lc.run_device(case, dev)
    return case, lc.expected(case), _got[name]


@pytest.mark.parametrize("name", [c.name for c in lc.CASES])
def test_loss_edge_case(dev, name):
    case, want, got = _run(name, dev)
    lc.check(case, want, got)


def test_too_many_classes_are_refused(dev):
    """C = 129 > MAXC: the library's unsupported status, nothing launched, nothing written"""
    from vilco_amd import ops
    case = lc.Case('classes_129', 129, lc._pow2(64), (lc._spread((128, 0)),), (64,), seed=47)
    x = lc.device_inputs(case, dev)
    norm = torch.full((1,), lc.INIT_NORM, device=dev)
    with pytest.raises(RuntimeError, match="not supported"):
        lc.call(case, x, norm)
    assert float(norm) == lc.INIT_NORM
    assert bool((ops._almax_state[(dev.index, 129)] == 0).all())


@pytest.mark.parametrize("name", ["thresholds_radius", "thresholds_none"])
def test_points_on_a_threshold_are_labelled_as_the_oracle_labels_them(dev, name):
    """far == range bound is inside the range (both ends), left == 0 / right == 0 / t == ctr -+ 1.5 stride is outside: the named
    rows' own gradients, row by row (a row wrongly positive or negative changes its focal target and its offsets' gradient)"""
    case, want, got = _run(name, dev)
    for kind, b, level, q, _ in case.named:
        for key in ('dlogits', 'doffsets'):
            w, g = want[key][level][b, q], got[key][level][b, q]
            assert rel_err(g, w, 1e-9) < 1e-4, (kind, b, level, q, key, g, w)
        positive = kind != 'inside'
        assert bool(want['doffsets'][level][b, q].abs().max() > 0) == positive, (kind, b, level, q)
        assert bool(got['doffsets'][level][b, q].abs().max() > 0) == positive, (kind, b, level, q)


def test_best_gt_of_a_near_tie_is_the_shortest_not_the_first(dev):
    """clip 0 of near_ties: class 3's GT (second, shorter by 5e-4) weights the row with its mu/sigma; class 7's bit is set too"""
    case, want, got = _run('near_ties', dev)
    g, w = got['dgauss'], want['dgauss']
    assert float(w[:, 3].abs().max()) > 0 and float(w[:, 7].abs().max()) == 0      # the oracle: only class 3's parameters
    assert float(g[:, 7].abs().max()) == 0
    assert rel_err(g[:, 3], w[:, 3], 1e-9) < 1e-4
    assert float(w[:, 5].abs().max()) == 0 and float(g[:, 5].abs().max()) == 0      # clip 1: the first of three equal lengths wins
    assert rel_err(g[:, 2], w[:, 2], 1e-9) < 1e-4


@pytest.mark.parametrize("name,first,later", [('al_tie_one_workgroup', (0, 10), (0, 200)), ('al_tie_two_workgroups', (0, 10), (1, 9))])
def test_al_tie_sends_the_gradient_to_the_first_row(dev, name, first, later):
    """two rows with bit-identical logits hold a class maximum: the earlier carries the al gradient, the later its focal part only"""
    case, want, got = _run(name, dev)
    for b in (0, 1):
        for l, q in (first, later):
            w, g = want['dlogits'][l][b, q], got['dlogits'][l][b, q]
            assert rel_err(g, w, 1e-9) < 1e-4, (b, l, q, g, w)


def test_masked_winner_contributes_its_value_and_no_gradient(dev):
    case, want, got = _run('masked_winner', dev)
    row = lc.audit(case)['al_row'][1][4]
    level = next(l for l in range(lc.L) if row < sum(case.Ts[:l + 1]))
    q = row - sum(case.Ts[:level])
    assert float(got['dlogits'][level][1, q].abs().max()) == 0.0
    assert abs(got['losses']['al_loss'] - want['losses']['al_loss']) <= 2e-5 * want['losses']['al_loss']


def test_diou_gradient_at_prediction_equal_to_target(dev):
    """the four tied rows of diou_tie, row by row: half the gradient of min and of max on each tied side"""
    case, want, got = _run('diou_tie', dev)
    for l, q in ((1, 6), (1, 5), (1, 7), (0, 12)):
        w, g = want['doffsets'][l][0, q], got['doffsets'][l][0, q]
        assert rel_err(g, w, 1e-9) < 1e-4, (l, q, g, w)
