"""CPU: guards of the MQ evaluator edge cases (metrics_edge_cases.py), run on the fp64 restatement alone: every case really
contains what the device test of the same name relies on, so a device test cannot pass because its case went stale."""
import numpy as np
import pytest

import metrics_edge_cases as E
import metrics_restatement as R


@pytest.mark.parametrize("n_gt", E.MANY_GT)
def test_many_gt_threshold_zero_locks_every_gt(n_gt):
    c = E.det_many_gt(n_gt)
    assert c.thr[0] == 0.0 and c.n_pred == E.MANY_GT_PRED
    _, tp = c.expected()
    assert int(tp[0].sum()) == min(c.n_pred, n_gt)
    # in rank order the TPs at threshold 0.0 are exactly the first n_gt predictions
    rank = np.argsort(c.score, kind='stable')[::-1]
    assert tp[0][rank][:min(c.n_pred, n_gt)].all()
    # the integer grid really ties tIoU values, and the exact-match threshold is met by some but not all
    assert 0 < tp[3].sum() < tp[1].sum() or n_gt == 1


def test_special_values_case_has_tp_and_fp_among_nan_rows():
    c = E.det_special()
    _, tp = c.expected()
    nan_rows = np.isnan(c.ts) | np.isnan(c.te)
    assert nan_rows.sum() > 50
    for t in range(len(c.thr)):
        assert tp[t][nan_rows].any() and not tp[t][nan_rows].all()
    for v in (np.inf, -np.inf, 0.5):
        assert (c.score == v).sum() > 50
    assert np.isnan(c.score).sum() > 50
    assert ((c.score == 0) & np.signbit(c.score)).sum() > 50 and ((c.score == 0) & ~np.signbit(c.score)).sum() > 50
    assert (c.te < c.ts).sum() > 50 and (c.te == c.ts).sum() > 50 and (c.ge == c.gs).sum() >= 6
    assert np.isinf(c.ts).sum() > 50 and np.isinf(c.te).sum() > 50
    # threshold 0.0 is not "everything": a negative tIoU fails it
    assert tp[0].sum() < c.n_pred


def test_threshold_above_one_matches_only_nan_rows():
    c = E.det_thresholds("above_one")
    _, tp = c.expected()
    assert c.thr[2] == 1.5
    assert tp[2].any() and not (tp[2] & ~np.isnan(c.ts)).any()
    assert len(E.det_thresholds("sixteen").thr) == 16 and len(E.det_thresholds("one").thr) == 1


def test_class_without_gt_is_zero_not_nan():
    c = E.det_class_without_gt()
    assert not (c.gcls == 2).any() and (c.cls == 2).sum() > 100
    ap, tp = c.expected()
    assert np.isfinite(ap).all()
    assert np.all(ap[:, 2] == 0.0) and not tp[:, c.cls == 2].any()
    assert np.all(ap[:, :2].max(axis=0) > 0)


@pytest.mark.parametrize("n_vid", E.N_VID)
def test_key_vid_case_reaches_the_last_video_and_outside(n_vid):
    c = E.det_key_vid(n_vid)
    _, tp = c.expected()
    assert (c.vidx == n_vid - 1).sum() >= 40
    out = (c.vidx < 0) | (c.vidx >= n_vid)
    assert out.sum() >= 36 and not tp[:, out].any()
    assert tp[0].any()


@pytest.mark.parametrize("n_cls", E.N_CLS)
def test_key_cls_case_has_ignored_labels(n_cls):
    c = E.det_key_cls(n_cls)
    ap, tp = c.expected()
    for lab in (-1, n_cls, n_cls + 1):
        assert (c.cls == lab).sum() >= 3
    assert not tp[:, (c.cls < 0) | (c.cls >= n_cls)].any()
    assert ap.shape == (5, n_cls) and (ap[0] > 0).sum() > n_cls // 2


def test_empty_predictions_shape():
    c = E.det_n_pred(0)
    ap, tp = c.expected()
    assert tp.shape == (5, 0) and np.all(ap == 0)


@pytest.mark.parametrize("n_gt", E.CUT_GT)
def test_cutoff_changes_the_count_and_both_sides_hit(n_gt):
    groups = E.ret_cutoffs(n_gt)
    for r_idx, r in enumerate(E.CUT_RANKS):
        inside, _ = R.retrieval_hits([groups[(r, r * n_gt)]], E.CUT_TIOUS, E.CUT_RANKS)        # target at the last admitted row
        outside, _ = R.retrieval_hits([groups[(r, r * n_gt + 1)]], E.CUT_TIOUS, E.CUT_RANKS)   # at the first excluded row
        assert inside.sum() > 0 and outside.sum() > 0
        assert inside[4, r_idx] == outside[4, r_idx] + 1
        if r * n_gt - 1 > 0:
            before, _ = R.retrieval_hits([groups[(r, r * n_gt - 1)]], E.CUT_TIOUS, E.CUT_RANKS)
            assert np.array_equal(before[:, r_idx], inside[:, r_idx])
    empty, total = R.retrieval_hits([groups[(1, 0)]], E.CUT_TIOUS, E.CUT_RANKS)
    assert empty.sum() == 0 and total == n_gt


def test_rank_limits_case():
    groups = list(E.ret_limits())
    hits, total = R.retrieval_hits(groups, E.LIMIT_TIOUS, E.LIMIT_RANKS)
    every, _ = R.retrieval_hits(groups, E.LIMIT_TIOUS, (10 ** 6,))
    assert hits.shape == (16, 8) and total == sum(len(g) for _, g in groups)
    assert np.all(hits[:, 0] == 0)                                     # rank 0 counts nothing
    assert np.array_equal(hits[:, 7], every[:, 0])                     # rank 100 is "all predictions"
    assert np.all(np.diff(hits, axis=1) >= 0) and np.any(hits[:, 6] < hits[:, 7]) and hits[0, 1] > 0


def test_degenerate_overlaps_are_no_hits():
    for name, (pred, gt) in E.RET_DEGENERATE.items():
        hits, total = R.retrieval_hits([(pred, gt)], E.CUT_TIOUS, E.CUT_RANKS)
        assert total == len(gt)
        want = {"nan_then_exact": [0, 1], "exact_then_nan": [1, 1], "nan_among_gt": [1, 1]}.get(name, [0, 0])
        assert hits.tolist() == [want] * 5, name
