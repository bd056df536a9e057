"""CPU: the NumPy restatement of the external-score fusion against the imported reference's goldens
(tests/golden/ext_scores.npz), the result / score-file loaders and `results_to_dict` / `results_to_array` against golden
content, and the C-ABI surface of `vilco_score_fuse` (declared, exported, bound, argument checking on the host)."""
import ctypes
import json
import pickle

import numpy as np
import pytest

import postprocessing_restatement as P
from vilco_amd.utils import postprocessing as PP


def _cases():
    return range(int(P.golden()['n_case']))


@pytest.mark.parametrize("c", [0, 1, 2])
def test_restatement_matches_reference_goldens(c):
    g = P.golden()
    got = P.fuse(P.case_results(g, c), P.case_cls(g, c), num_pred=int(g['num_pred%d' % c]), topk=int(g['topk%d' % c]))
    P.assert_columns_equal(got, g, c)


def test_golden_cases_cover_the_edges():
    g = P.golden()
    assert list(_cases()) == [0, 1, 2]
    cnt = np.unique(g['res0_vid'], return_counts=True)[1].tolist()
    assert all(n in cnt for n in (1, 7, 16, 17, 200, 201, 260)) and int(g['num_pred0']) == 200
    assert int(g['num_pred1']) == 50 and max(np.unique(g['res1_vid'], return_counts=True)[1]) > 50
    assert sorted(int(g['topk%d' % c]) for c in _cases()) == [1, 2, 3]
    assert sorted(int(g['task%d' % c]) for c in _cases()) == [0, 1, 2]
    assert sorted(str(g['fmt%d' % c]) for c in _cases()) == ['json', 'json_wrapped', 'pkl']
    assert g['res0_score'].dtype == np.float32 and g['res1_score'].dtype == np.float64
    assert (g['out0_score'] == 0).any()                                  # a zero class score among the chosen classes
    for c in _cases():
        assert float(g['avg%d' % c]) > 0
        # tie-free, so the reference's unspecified tie order is not in the goldens
        for v in np.unique(g['res%d_vid' % c]):
            s = g['res%d_score' % c][g['res%d_vid' % c] == v]
            assert len(np.unique(s)) == len(s)
        for vec in P.case_cls(g, c).values():
            top = np.sort(vec)[::-1][:int(g['topk%d' % c]) + 1]
            assert len(np.unique(top)) == len(top)


def test_loaders(tmp_path):
    g = P.golden()
    cls = P.case_cls(g, 1)
    for fmt in ('pkl', 'json', 'json_wrapped'):
        assert PP.load_cls_scores(P.write_score_file(cls, fmt, tmp_path, name=fmt)) == cls
    p = tmp_path / "plain.json"
    p.write_text(json.dumps({"results": cls, "version": "1.0"}))
    assert PP.load_results_from_json(str(p)) == cls                      # the 'results' wrapper is removed
    p.write_text(json.dumps(cls))
    assert PP.load_results_from_json(str(p)) == cls
    q = tmp_path / "res.pkl"
    res = P.case_results(g, 2)
    q.write_bytes(pickle.dumps(res))
    back = PP.load_results_from_pkl(str(q))
    assert back['video-id'] == res['video-id']
    np.testing.assert_array_equal(back['score'], res['score'])
    with pytest.raises(AssertionError):
        PP.load_results_from_pkl(str(tmp_path / "missing.pkl"))


def test_results_to_dict_and_array_match_reference():
    g = P.golden()
    res = P.case_results(g, 2)
    assert PP.results_to_dict(res) == json.loads(str(g['rdict2']))
    arr = PP.results_to_array(res, int(g['num_pred2']))
    assert list(arr) == sorted(set(res['video-id']))
    assert [len(arr[v]['score']) for v in arr] == g['rarr2_cnt'].tolist()
    np.testing.assert_array_equal(np.concatenate([arr[v]['label'] for v in arr]), g['rarr2_label'])
    assert np.concatenate([arr[v]['score'] for v in arr]).tobytes() == g['rarr2_score'].tobytes()
    np.testing.assert_array_equal(np.concatenate([arr[v]['segment'] for v in arr]), g['rarr2_segment'])
    # num_pred cuts every video
    arr = PP.results_to_array(res, 3)
    assert all(len(a['score']) == 3 and a['segment'].shape == (3, 2) for a in arr.values())
    assert all(np.all(np.diff(a['score']) < 0) for a in arr.values())


def test_results_to_array_tie_rule():
    res = {'video-id': ['a'] * 4, 't-start': np.arange(4.0), 't-end': np.arange(4.0) + 1, 'label': np.arange(4),
           'score': np.array([0.5, 0.7, 0.5, 0.5])}
    assert PP.results_to_array(res, 3)['a']['label'].tolist() == [1, 3, 2]      # equal scores: the later row first


def test_symbols_declared_exported_and_bound():
    import os
    import re
    from vilco_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vilco_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vilco_score_fuse", "vilco_score_fuse_workspace"):
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    mk = open(os.path.join(root, "vilco_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bfuse\.hip\b", mk, flags=re.M)


def _args(**over):
    """a call that passes every check: 2 videos of 3 and 1 rows, 4 classes, num_pred 2, topk 2"""
    i32 = ctypes.c_int32
    a = dict(score=256, ts=256, te=256, pred_off=(i32 * 3)(0, 3, 4), n_pred=4, n_vid=2, cls=256, n_cls=4, num_pred=2, topk=2,
             out_off=(i32 * 3)(0, 4, 6), n_out=6, ovid=256, olab=256, ots=256, ote=256, osc=256, ws=256, ws_bytes=1 << 20,
             stream=None)
    a.update(over)
    return list(a.values())


def test_launcher_rejects_bad_arguments_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()
    i32 = ctypes.c_int32
    BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
    need = lib.vilco_score_fuse_workspace(4, 2)
    assert need > 0
    assert lib.vilco_score_fuse_workspace(-1, 2) == 0 and lib.vilco_score_fuse_workspace(4, -1) == 0
    # the last check a good call meets on the host is the workspace size
    assert lib.vilco_score_fuse(*_args(ws_bytes=need - 1)) == WORKSPACE
    for k in ('score', 'ts', 'te', 'pred_off', 'cls', 'out_off', 'ovid', 'olab', 'ots', 'ote', 'osc', 'ws'):
        assert lib.vilco_score_fuse(*_args(**{k: None})) == BADARG, k                # null pointers
    for k in ('n_pred', 'n_vid', 'n_cls', 'n_out'):
        assert lib.vilco_score_fuse(*_args(**{k: -1})) == BADARG, k                  # negative counts
    assert lib.vilco_score_fuse(*_args(topk=5)) == BADARG                            # topk > n_cls
    assert lib.vilco_score_fuse(*_args(topk=0)) == BADARG
    assert lib.vilco_score_fuse(*_args(num_pred=0)) == BADARG
    assert lib.vilco_score_fuse(*_args(pred_off=(i32 * 3)(0, 5, 4))) == BADARG       # non-monotone offsets
    assert lib.vilco_score_fuse(*_args(pred_off=(i32 * 3)(1, 3, 4))) == BADARG       # do not start at 0
    assert lib.vilco_score_fuse(*_args(pred_off=(i32 * 3)(0, 3, 5))) == BADARG       # do not end at n_pred
    assert lib.vilco_score_fuse(*_args(out_off=(i32 * 3)(0, 6, 4), n_out=4)) == BADARG
    assert lib.vilco_score_fuse(*_args(out_off=(i32 * 3)(0, 4, 8), n_out=8)) == BADARG   # not topk * min(num_pred, rows)
    assert lib.vilco_score_fuse(*_args(n_out=7)) == BADARG
    assert lib.vilco_score_fuse(*_args(topk=65, n_cls=100, out_off=(i32 * 3)(0, 130, 195), n_out=195)) == UNSUPPORTED
    # no videos: nothing to launch
    assert lib.vilco_score_fuse(*_args(pred_off=(i32 * 1)(0), out_off=(i32 * 1)(0), n_pred=0, n_vid=0, n_out=0)) == 0


def test_missing_video_raises_keyerror(tmp_path):
    g = P.golden()
    cls = P.case_cls(g, 2)
    cls.pop(sorted(cls)[0])
    with pytest.raises(KeyError):
        PP.postprocess_results(P.case_results(g, 2), P.write_score_file(cls, 'pkl', tmp_path))
    with pytest.raises(KeyError):
        PP.fuse_external_scores(P.case_results(g, 2), cls)


def test_exported_from_utils():
    from vilco_amd import utils
    for name in ("load_results_from_pkl", "load_results_from_json", "results_to_dict", "results_to_array",
                 "postprocess_results", "fuse_external_scores"):
        assert callable(getattr(utils, name))
