"""CPU: the NumPy restatement of the NLQ evaluators against the imported reference's goldens (tests/golden/nlq_metrics.npz),
both ground-truth loaders, the submission-file helper, and argument checking of the `vilco_nlq_recall` C-ABI entry."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import nlq_metrics_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("case", R.EGO_CASES)
def test_restatement_matches_reference_goldens(case):
    g = R.golden()
    gt = R.text(g, 'gt')
    recs = R.text(g, case + '_pred')
    flags, top1 = R.evaluate(recs, R.gt_windows(gt))
    np.testing.assert_array_equal(flags.transpose(1, 2, 0), g[case + '_flags'])
    np.testing.assert_array_equal(_bits(top1), _bits(g[case + '_avg']))          # bit-equal, NaN positions included
    np.testing.assert_array_equal(R.recall(flags), g[case + '_frac'])
    np.testing.assert_array_equal(R.recall(flags) * 100, g[case + '_pct'])
    np.testing.assert_array_equal(R.recall(flags), g[case + '_mean'])
    n = len(recs)
    miou = float(g[case + '_miou'])
    if np.isnan(miou):
        assert np.isnan(top1).any()
    else:
        assert abs(top1.sum() / n - miou) <= (n - 1) * 2.0 ** -53
    # evaluate_anet: fp32 arithmetic, float32 counts over n
    f32, _ = R.evaluate(recs, R.gt_windows(gt), mode=1)
    want = (f32.sum(axis=0).T.astype(np.float32) / np.float32(n))
    np.testing.assert_array_equal(want, g[case + '_anet_frac'])
    np.testing.assert_array_equal(want * np.float32(100), g[case + '_anet_pct'])


def test_packed_restatement_equals_record_restatement():
    g = R.golden()
    from vilco_amd.utils import metrics_nlq as M
    win = R.gt_windows(R.text(g, 'gt'))
    for case in R.EGO_CASES:
        recs = R.text(g, case + '_pred')
        pred, cnt = M._pack_records([r['predicted_times'] for r in recs], 10)
        gt = np.array([win[(r['clip_uid'], r['annotation_uid'])][r['query_idx']] for r in recs])
        for mode in (0, 1):
            f0, t0 = R.evaluate(recs, win, mode=mode)
            f1, t1 = R.flags_and_top1(pred, cnt, gt, mode=mode)
            np.testing.assert_array_equal(f0, f1)
            np.testing.assert_array_equal(_bits(t0), _bits(t1))


def test_golden_cases_are_not_trivial():
    g = R.golden()
    rows = R.text(g, 'rows_pred')
    assert {len(r['predicted_times']) for r in rows} >= {1, 4, 5, 9, 10, 11, 300}
    flags = g['rows_flags']                                          # [thr, rank, n]
    n_base = 39
    for j, k in enumerate(R.TOPK):                                   # the hit at row K + 1 is not counted, the one at row K is
        miss, hit = n_base + 2 * j, n_base + 2 * j + 1
        assert len(rows[miss]['predicted_times']) > k
        assert not flags[:, j, miss].any() and flags[:, j, hit].all()
        if j + 1 < len(R.TOPK):
            assert flags[:, j + 1, miss].all()
    e = g['edges_flags']
    assert e[0, 0, 0] and not e[1, 0, 0]                             # IoU == 0.5: over 0.3, not over 0.5
    assert g['edges_avg'][1] == 0.3 and not e[0, 0, 1]               # IoU == 0.3 in fp64 is not a hit ...
    assert g['edges_anet_frac'][0, 0] > g['edges_frac'][0, 0]        # ... float32(0.3) is
    assert e[0, 0, 6]                                                # one ulp above
    assert np.isnan(g['nan_miou']) and np.isnan(g['nan_avg'][0]) and not np.isnan(g['nan_avg'][1:]).any()
    assert all(np.isfinite(g[c + '_miou']) for c in ('rows', 'edges'))
    assert g['seg_pct'].shape == (13, 2, 3) and int(g['seg_id'].max()) == 12
    assert str(g['unknown_raises']) == "Instance not present!"
    assert g['edges_pct'][0, 0] == g['edges_frac'][0, 0] * 100       # verbose: percent


def test_segment_prefixes_follow_from_integer_counts():
    g = R.golden()
    recs, seg = R.text(g, 'seg_pred'), g['seg_id']
    flags, _ = R.evaluate(recs, R.gt_windows(R.text(g, 'gt')))
    hits = np.stack([flags[seg == s].sum(axis=0) for s in range(13)]).cumsum(axis=0)
    n = np.cumsum(np.bincount(seg, minlength=13))
    for s in range(13):
        np.testing.assert_array_equal(hits[s].astype(np.float64) / np.float64(n[s]) * 100, g['seg_pct'][s])


def test_unknown_key_raises():
    g = R.golden()
    with pytest.raises(AssertionError, match="Instance not present!"):
        R.evaluate(R.text(g, 'unknown_pred'), R.gt_windows(R.text(g, 'gt')))


def test_loaders_both_formats(tmp_path):
    from vilco_amd.utils import ReferringRecall, make_nlq_evaluator
    g = R.golden()
    gt = R.text(g, 'gt')
    ev = make_nlq_evaluator(R.write_ego4d(gt, tmp_path))
    assert ev.dataset == "ego4d_cl" and list(ev.thresholds) == [0.3, 0.5] and list(ev.topK) == [1, 5, 10]
    assert ev.num_gt_queries == int(g['num_gt_queries'][0]) == 360
    assert set(ev.gt_dict) == set(R.gt_windows(gt))
    assert ev.gt_dict[("c0", "a0_0")]["language_queries"][1]["clip_end_sec"] == 7.0
    # the flat table the device reads, and the key -> row lookup
    win = R.gt_windows(gt)
    for key in (("c0", "a0_0", 1), ("c17", "a17_1", 2), ("c59", "a59_1", -1)):
        assert ev._gt.table[ev._gt.index(key)].tolist() == win[key[:2]][key[2]]
    with pytest.raises(AssertionError, match="Instance not present!"):
        ev._gt.index(("nope", "a0_0", 0))
    with pytest.raises(IndexError):
        ev._gt.index(("c0", "a0_0", 3))
    rows = R.to_jsonl_gt(gt)
    an = ReferringRecall(dataset="tacos", gt_file=R.write_jsonl(rows, tmp_path))
    assert an.num_gt_queries == int(g['num_gt_queries'][1]) == len(rows)
    assert an.gt_dict["c0_a0_0_0"] == [0.0, 10.0]
    assert an._gt.table[an._gt.index("c3_a3_1_2")].tolist() == win[("c3", "a3_1")][2]
    with pytest.raises(KeyError):
        an._gt.index("nope")
    cfg = {"dataset_name": "ego4d", "dataset": {"json_file": R.write_ego4d(gt, tmp_path)}}
    assert make_nlq_evaluator(cfg).dataset == "ego4d"


def test_submission_helper_equals_recorded_file():
    from vilco_amd.utils import metrics_nlq as M
    g = R.golden()
    records = R.text(g, 'sub_records')
    want = R.text(g, 'sub_json')
    assert max(len(r['predicted_times']) for r in records) == 300
    assert M.submission(records) == want
    assert max(len(r['predicted_times']) for r in want['results']) == 10
    assert len(records[6]['predicted_times']) == 300                 # the input list is left as it was


def test_abi_entries_declared_and_in_table():
    from vilco_amd import _lib
    with open(os.path.join(ROOT, "include", "vilco_hip.h")) as f:
        header = f.read()
    for name in ("vilco_nlq_recall", "vilco_nlq_recall_workspace"):
        assert re.search(r"\b%s\(" % name, header)
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vilco_nlq_recall"][1]) == 21


def test_nlq_recall_abi_rejects_bad_arguments():
    from vilco_amd import _lib
    lib = _lib.load()
    thr = (ctypes.c_double * 17)(*([0.5] * 17))
    rk = (ctypes.c_int32 * 9)(*([1] * 9))
    d = 256
    need = lib.vilco_nlq_recall_workspace(100, 3)
    assert need >= 100 * 3 * 2
    assert lib.vilco_nlq_recall_workspace(-1, 3) == 0 and lib.vilco_nlq_recall_workspace(100, 9) == 0

    def call(pred=d, fp32=0, cnt=d, k_cap=5, gt=d, seg=None, n=100, n_seg=1, thr_=thr, n_thr=2, rk_=rk, n_rank=3, mode=0,
             hits=d, nq=d, top1=d, top1_sum=d, flags=None, ws=d, ws_bytes=need):
        return lib.vilco_nlq_recall(pred, fp32, cnt, k_cap, gt, seg, n, n_seg, thr_, n_thr, rk_, n_rank, mode, hits, nq, top1,
                                    top1_sum, flags, ws, ws_bytes, None)
    for kw in (dict(pred=None), dict(cnt=None), dict(gt=None), dict(hits=None), dict(nq=None), dict(top1=None),
               dict(top1_sum=None), dict(ws=None), dict(thr_=None), dict(rk_=None), dict(n=-1), dict(n_seg=0), dict(k_cap=0),
               dict(gt=d + 8), dict(pred=d + 8), dict(pred=d + 4, fp32=1)):
        assert call(**kw) == -1, kw
    bad_rank = (ctypes.c_int32 * 3)(1, 0, 10)
    assert call(rk_=bad_rank) == -1
    for kw in (dict(n_thr=17), dict(n_thr=0), dict(n_rank=9), dict(n_rank=0), dict(mode=2), dict(mode=-1)):
        assert call(**kw) == -2, kw
    assert call(ws_bytes=need - 1) == -4
    assert call(n=1000) == -4                                        # the workspace grows with the query count
