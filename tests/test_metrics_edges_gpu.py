"""GPU: the MQ device evaluators (csrc/evaluate.hip: vilco_det_ap, vilco_retrieval_hits) against the fp64 restatement on the
edge cases of metrics_edge_cases.py -- more than 64 GT in a group, prediction counts around the radix tile, class and video
keys of two and three radix digits, 1 and 16 thresholds and thresholds of 0.0 and above 1, NaN / inf / signed-zero scores,
NaN / inf / reversed / zero-length boundaries, a class without GT, the Recall@K cut-off at r * n_gt rows, 8 ranks, NaN and
0/0 overlaps.  Bars: TP flags equal, hit counts equal, AP within 1e-12 absolute, repeated calls bitwise equal.
test_metrics_edges_cpu.py guards that each case contains what it is meant to exercise.

Seen on the MI355X: with the ternary max / min that ev_hits_kernel had before (a NaN prediction boundary fell to the GT side),
test_retrieval_nan_prediction_boundary_is_no_hit, test_retrieval_degenerate_overlaps (pred_nan_start, pred_nan_end,
pred_nan_both, nan_then_exact, nan_among_gt) and test_wrappers_pass_nan_rows_through failed -- the device counted hits where
the overlap is NaN -- and so did the "edges" golden of test_metrics_gpu.py; every detection case passed as it was, seg_tiou's
ternaries included."""
import json

import numpy as np
import pytest

import metrics_edge_cases as E
import metrics_restatement as R

pytestmark = pytest.mark.gpu


def _check_det(c):
    ap_r, tp_r = c.expected()
    ap_d, tp_d = c.run_device()
    assert tp_d.shape == tp_r.shape and ap_d.shape == ap_r.shape
    np.testing.assert_array_equal(tp_d, tp_r)
    assert np.isfinite(ap_r).all()                       # the restatement yields no NaN AP, so none is allowed
    np.testing.assert_allclose(ap_d, ap_r, rtol=0, atol=1e-12)
    return ap_d, tp_d


@pytest.mark.parametrize("n_gt", E.MANY_GT)
def test_det_many_gt_in_one_group(n_gt):
    c = E.det_many_gt(n_gt)
    ap_d, tp_d = _check_det(c)
    assert int(tp_d[0].sum()) == min(c.n_pred, n_gt)     # threshold 0.0: every prediction locks a GT until all are locked
    if n_gt == E.MANY_GT[-1]:
        ap_2, tp_2 = c.run_device()
        assert ap_2.tobytes() == ap_d.tobytes() and np.array_equal(tp_2, tp_d)


@pytest.mark.parametrize("n_pred", E.N_PRED)
def test_det_prediction_counts(n_pred):
    c = E.det_n_pred(n_pred)
    ap_d, tp_d = _check_det(c)
    if n_pred == 0:
        assert tp_d.shape == (len(c.thr), 0) and np.all(ap_d == 0)


@pytest.mark.parametrize("n_cls", E.N_CLS)
def test_det_class_key_width(n_cls):
    _check_det(E.det_key_cls(n_cls))


@pytest.mark.parametrize("n_vid", E.N_VID)
def test_det_video_key_width(n_vid):
    c = E.det_key_vid(n_vid)
    _, tp_d = _check_det(c)
    assert not tp_d[:, (c.vidx < 0) | (c.vidx >= n_vid)].any()


@pytest.mark.parametrize("name", sorted(E.THR_SETS))
def test_det_threshold_counts(name):
    _check_det(E.det_thresholds(name))


def test_det_special_values():
    c = E.det_special()
    ap_d, tp_d = _check_det(c)
    ap_2, tp_2 = c.run_device()
    assert ap_2.tobytes() == ap_d.tobytes() and np.array_equal(tp_2, tp_d)


def test_det_class_without_gt():
    c = E.det_class_without_gt()
    ap_d, tp_d = _check_det(c)
    assert np.all(ap_d[:, 2] == 0.0) and not tp_d[:, c.cls == 2].any()


@pytest.mark.parametrize("n_gt", E.CUT_GT)
def test_retrieval_cutoffs(n_gt):
    groups = E.ret_cutoffs(n_gt)
    keys = sorted(groups)
    # every group on its own (an off-by-one in the cut-off changes its count), then all of them in one call
    for k in keys:
        h_r, t_r = R.retrieval_hits([groups[k]], E.CUT_TIOUS, E.CUT_RANKS)
        h_d, t_d = E.run_device_hits([groups[k]], E.CUT_TIOUS, E.CUT_RANKS)
        assert t_d == t_r == n_gt
        np.testing.assert_array_equal(h_d, h_r, err_msg="rank %d, %d predictions" % k)
    h_r, t_r = R.retrieval_hits([groups[k] for k in keys], E.CUT_TIOUS, E.CUT_RANKS)
    h_d, t_d = E.run_device_hits([groups[k] for k in keys], E.CUT_TIOUS, E.CUT_RANKS)
    assert t_d == t_r
    np.testing.assert_array_equal(h_d, h_r)


def test_retrieval_argument_limits():
    groups = list(E.ret_limits())
    h_r, t_r = R.retrieval_hits(groups, E.LIMIT_TIOUS, E.LIMIT_RANKS)
    h_d, t_d = E.run_device_hits(groups, E.LIMIT_TIOUS, E.LIMIT_RANKS)
    assert t_d == t_r and h_d.shape == (16, 8)
    np.testing.assert_array_equal(h_d, h_r)
    assert np.all(h_d[:, 0] == 0)                                      # rank 0 counts nothing
    every, _ = E.run_device_hits(groups, E.LIMIT_TIOUS, (10 ** 6,))
    np.testing.assert_array_equal(h_d[:, 7], every[:, 0])              # rank 100 is "all predictions" here


def test_retrieval_nan_prediction_boundary_is_no_hit():
    """prediction (NaN, 10) against GT (0, 10): the reference's iou() gives NaN, and NaN > t is false"""
    hits, total = E.run_device_hits([E.RET_DEGENERATE["pred_nan_start"]], E.CUT_TIOUS, E.CUT_RANKS)
    assert total == 1
    np.testing.assert_array_equal(hits, np.zeros((5, 2), np.int64))


def test_retrieval_degenerate_overlaps():
    bad = []
    for name, (pred, gt) in E.RET_DEGENERATE.items():
        h_r, t_r = R.retrieval_hits([(pred, gt)], E.CUT_TIOUS, E.CUT_RANKS)
        h_d, t_d = E.run_device_hits([(pred, gt)], E.CUT_TIOUS, E.CUT_RANKS)
        print(name, "restatement", h_r[:, 0].tolist(), h_r[:, 1].tolist(), "device", h_d[:, 0].tolist(), h_d[:, 1].tolist())
        if t_d != t_r or not np.array_equal(h_d, h_r):
            bad.append(name)
    assert not bad
    allg = list(E.RET_DEGENERATE.values())
    h_r, t_r = R.retrieval_hits(allg, E.CUT_TIOUS, E.CUT_RANKS)
    h_d, t_d = E.run_device_hits(allg, E.CUT_TIOUS, E.CUT_RANKS)
    assert t_d == t_r
    np.testing.assert_array_equal(h_d, h_r)


def test_wrappers_pass_nan_rows_through(tmp_path):
    """Moment_Retrieval.hits() and ANETdetection.evaluate() on a tiny annotation file and results with NaN segments: nothing
    between the loaders and the kernels drops or reorders a NaN row"""
    from vilco_amd.utils import metrics as M
    nan = float('nan')

    def ants(lab, segs):
        return [{"segment": list(s), "label_id": lab, "label": "c%d" % lab} for s in segs]

    gt = {"a": ants(0, [(0.0, 10.0), (20.0, 30.0)]), "b": ants(1, [(0.0, 10.0)]) + ants(0, [(5.0, 9.0)])}
    path = tmp_path / "ann.json"
    path.write_text(json.dumps({v: {"subset": "val", "clip_id": v, "annotations": a} for v, a in gt.items()}))
    rows = [("a", nan, 10.0, 0, 0.9), ("a", 0.0, 10.0, 0, 0.8), ("a", 20.0, nan, 0, 0.7), ("a", 21.0, 30.0, 0, 0.6),
            ("b", nan, 10.0, 1, 0.5), ("b", 0.0, 10.0, 1, 0.4), ("b", nan, nan, 0, 0.95), ("a", 20.0, 30.0, 0, nan)]
    results = {}
    for v, s, e, lab, sc in rows:
        results.setdefault(v, []).append({"segment": [s, e], "score": sc, "label": "c%d" % lab})
    obj = json.loads(json.dumps({"version": "1.0", "external_data": "", "results": results}))     # NaN survives the JSON text
    hits, total = M.Moment_Retrieval(ground_truth_filename=str(path), prediction_filename=obj, subset='val').hits()
    groups = [([(nan, 10.0), (0.0, 10.0), (20.0, nan), (21.0, 30.0), (20.0, 30.0)], [(0.0, 10.0), (20.0, 30.0)]),   # a, c0
              ([(nan, 10.0), (0.0, 10.0)], [(0.0, 10.0)]),                                                            # b, c1
              ([(nan, nan)], [(5.0, 9.0)])]                                                                           # b, c0
    h_r, t_r = R.retrieval_hits(groups)
    assert total == t_r == 4
    np.testing.assert_array_equal(hits, h_r)
    assert h_r[0].tolist() == [1, 3]                      # rank 1: only a/c0's GT 0 inside the first r * n_gt rows

    thr = np.linspace(0.1, 0.5, 5)
    ev = M.ANETdetection(str(path), split='val', tiou_thresholds=thr)
    preds = {'video-id': [r[0] for r in rows], 't-start': np.array([r[1] for r in rows]),
             't-end': np.array([r[2] for r in rows]), 'label': np.array([r[3] for r in rows]),
             'score': np.array([r[4] for r in rows])}
    mAP, avg, _ = ev.evaluate(preds, verbose=False)
    vid = {"a": 0, "b": 1}
    ap_r, tp_r = R.det_ap(np.array([vid[r[0]] for r in rows]), preds['label'], preds['t-start'], preds['t-end'], preds['score'],
                          np.array([0, 0, 1, 1]), np.array([0, 0, 1, 0]), np.array([0.0, 20.0, 0.0, 5.0]),
                          np.array([10.0, 30.0, 10.0, 9.0]), 2, thr)
    np.testing.assert_allclose(ev.ap, ap_r, rtol=0, atol=1e-12)
    np.testing.assert_allclose(mAP, ap_r.mean(axis=1), rtol=0, atol=1e-12)
    gtd, cols = ev.prepare(preds)
    _, tp_d = M.det_ap_device(gtd, *cols, thr, want_flags=True)
    np.testing.assert_array_equal(tp_d, tp_r)
    assert tp_r[:, [0, 6, 7]].all()                       # the NaN rows are in the result: NaN tIoU / NaN score rank first
