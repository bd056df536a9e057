"""CPU: the NumPy restatement of the MQ evaluators against the imported reference's goldens (tests/golden/metrics_*.npz),
the ground-truth loaders and the label remap, and argument checking of the evaluator C-ABI entries."""
import ctypes
import json

import numpy as np
import pytest

import metrics_restatement as R
from vilco_amd.utils import metrics as M


@pytest.mark.parametrize("name", R.GOLDENS)
def test_restatement_matches_reference_goldens(name, tmp_path):
    g = R.golden(name)
    path = R.ann_file(g, tmp_path)
    for e in range(int(g['n_eval'])):
        ap, _ = R.restated_det(path, g, e)
        assert ap.shape == g['ap%d' % e].shape
        np.testing.assert_allclose(ap, g['ap%d' % e], rtol=0, atol=1e-12)
        np.testing.assert_allclose(ap.mean(axis=1), g['mAP%d' % e], rtol=0, atol=1e-12)
        if 'recall%d' % e in g:
            hits, total = R.restated_recall(path, g, e)
            np.testing.assert_array_equal(hits / float(total), g['recall%d' % e])


def test_golden_cases_are_not_trivial():
    g = R.golden("json")
    assert np.all(g['ap1'] == 0)                                    # empty predictions
    assert np.all(g['ap0'][:, 3] == 0) and np.all(g['ap0'][:, :3].max(axis=1) > 0)   # class 3 has no predictions
    assert (R.golden("large")['pred0_label'] == 0).sum() > 18000
    assert int(R.golden("cl")['n_eval']) == 3


def test_remap_is_simultaneous():
    np.testing.assert_array_equal(M._remap([3, 0, 1, 5], {3: 0, 0: 1}), [0, 1, 1, 5])
    np.testing.assert_array_equal(M._remap([], {1: 0}), [])


def test_remove_duplicates_and_json_loader(tmp_path):
    g = R.golden("json")
    path = R.ann_file(g, tmp_path)
    gt, ai = M.load_gt_seg_from_json(path, split="val")
    db = json.loads(str(g['ann']))
    vids, labels = [], []
    for k, v in db.items():
        if v['subset'] != 'val':
            continue
        ants = M.remove_duplicate_annotations(v['annotations'])
        assert len(ants) <= len(v['annotations'])
        vids += [k] * len(ants)
        labels += [a['label_id'] for a in ants]
    assert gt['video-id'] == vids
    assert ai == {1: 0, 3: 1, 4: 2, 6: 3}
    np.testing.assert_array_equal(gt['label'], [ai[x] for x in labels])
    assert len(M.remove_duplicate_annotations(db['v01']['annotations'])) == len(db['v01']['annotations']) - 2


def test_cl_loader_accumulates_tasks(tmp_path):
    g = R.golden("cl")
    gt, ai = M.load_gt_seg_from_json(R.ann_file(g, tmp_path), use_cl=True)
    assert len(gt) == 3 and len(ai) == 3
    assert len(gt[0]['label']) < len(gt[1]['label']) < len(gt[2]['label'])
    assert gt[2]['video-id'][:len(gt[0]['video-id'])] == gt[0]['video-id']


def test_pred_json_loader(tmp_path):
    p = tmp_path / "pred.json"
    p.write_text(json.dumps({"database": {"a": [{"segment": [1, 2], "label_id": 3, "scores": 0.5}],
                                          "b": [{"segment": [0.5, 4], "label_id": 1, "scores": 0.25}]}}))
    d = M.load_pred_seg_from_json(str(p))
    assert d['video-id'] == ['a', 'b']
    np.testing.assert_array_equal(d['t-start'], [1.0, 0.5])
    np.testing.assert_array_equal(d['label'], [3, 1])
    np.testing.assert_array_equal(d['score'], [0.5, 0.25])


def test_restatement_nan_and_ties():
    # 0/0 tIoU is matched; equal scores rank the later row first
    ap, tp = R.det_ap(np.array([0, 0]), np.array([0, 0]), np.array([5.0, 5.0]), np.array([5.0, 5.0]), np.array([0.5, 0.5]),
                      np.array([0]), np.array([0]), np.array([5.0]), np.array([5.0]), 1, [0.5])
    assert tp.tolist() == [[False, True]]
    assert ap[0, 0] == 1.0


def test_evaluator_abi_rejects_bad_arguments():
    from vilco_amd import _lib
    lib = _lib.load()
    thr = (ctypes.c_double * 17)(*([0.5] * 17))
    rk = (ctypes.c_int32 * 9)(*([1] * 9))
    dummy = 256
    assert lib.vilco_det_ap(None, None, None, None, None, -1, None, None, None, None, None, 0, 0, None, 1, 1, thr, 1, None,
                            None, None, 0, None) == -1
    args = [dummy] * 5 + [10, dummy, dummy, dummy, dummy, dummy, 1, 1, dummy, 1, 1, thr]
    assert lib.vilco_det_ap(*args, 17, dummy, None, dummy, 1 << 30, None) == -2          # > 16 thresholds
    a2 = list(args); a2[14] = 1 << 16
    assert lib.vilco_det_ap(*a2, 1, dummy, None, dummy, 1 << 30, None) == -2             # class count beyond the key
    a3 = list(args); a3[15] = (1 << 24) - 1
    assert lib.vilco_det_ap(*a3, 1, dummy, None, dummy, 1 << 30, None) == -2             # video count beyond the key
    need = lib.vilco_det_ap_workspace(10, 1, 1)
    assert need > 0
    assert lib.vilco_det_ap(*args, 1, dummy, None, dummy, need - 1, None) == -4
    assert lib.vilco_retrieval_hits(None, None, None, None, None, None, None, -1, thr, 1, rk, 1, None, None, None, 0,
                                    None) == -1
    r = [dummy] * 7 + [1, thr]
    assert lib.vilco_retrieval_hits(*r, 17, rk, 1, dummy, dummy, None, 0, None) == -2
    assert lib.vilco_retrieval_hits(*r, 1, rk, 9, dummy, dummy, None, 0, None) == -2
    neg = (ctypes.c_int32 * 2)(1, -1)
    assert lib.vilco_retrieval_hits(*r, 1, neg, 2, dummy, dummy, None, 0, None) == -1    # a negative rank
