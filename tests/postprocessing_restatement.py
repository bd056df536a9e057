"""NumPy restatement of the external-score fusion (MQ/libs/utils/postprocessing.py:97-155), written from the definition
with the project's tie rule: both rankings are the reverse of a stable ascending sort (descending value, equal values
and NaN with the later index first).  Test infrastructure only: the product fuses on the device
(vilco_amd.utils.postprocessing)."""
import json
import os
import pickle

import numpy as np


def _desc(x):
    return np.argsort(x, kind='stable')[::-1]


def fuse(results, cls_scores, num_pred=200, topk=2):
    """result columns + {video: class-score vector} -> the fused host columns, in the reference's row order"""
    vids = np.asarray(results['video-id'], dtype=object)
    score = np.asarray(results['score']).astype(np.float64)
    ts = np.asarray(results['t-start']).astype(np.float64)
    te = np.asarray(results['t-end']).astype(np.float64)
    out = {'video-id': [], 't-start': [], 't-end': [], 'label': [], 'score': []}
    for v in sorted(set(vids.tolist())):
        rows = np.flatnonzero(vids == v)
        rows = rows[_desc(score[rows])[:num_pred]]
        cs = np.asarray(cls_scores[v], dtype=np.float64)
        top = _desc(cs)[:topk]
        with np.errstate(invalid='ignore'):
            out['score'].append(np.sqrt(cs[top][:, None] * score[rows][None, :]).reshape(-1))
        out['t-start'].append(np.tile(ts[rows], len(top)))
        out['t-end'].append(np.tile(te[rows], len(top)))
        out['label'].append(np.repeat(top, len(rows)).astype(np.int64))
        out['video-id'] += [v] * (len(rows) * len(top))
    for k, dt in (('t-start', np.float64), ('t-end', np.float64), ('label', np.int64), ('score', np.float64)):
        out[k] = np.concatenate(out[k]) if out[k] else np.zeros(0, dtype=dt)
    return out


# ----------------------------------------------------------------------------------------------- golden-case plumbing
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ext_scores.npz"))


def case_results(g, c):
    return {'video-id': [str(x) for x in g['res%d_vid' % c]], 't-start': g['res%d_ts' % c], 't-end': g['res%d_te' % c],
            'label': g['res%d_label' % c], 'score': g['res%d_score' % c]}


def case_cls(g, c):
    return json.loads(str(g['cls%d' % c]))


def write_score_file(cls, fmt, tmp_path, name="scores"):
    """the score table in one of the formats the goldens name: 'pkl', 'json', 'json_wrapped'"""
    if fmt == 'pkl':
        p = tmp_path / (name + ".pkl")
        p.write_bytes(pickle.dumps(cls))
    else:
        p = tmp_path / (name + ".json")
        p.write_text(json.dumps({"version": "1.0", "results": cls} if fmt == 'json_wrapped' else cls))
    return str(p)


def ann_file(g, tmp_path):
    p = tmp_path / "ann.pkl"
    p.write_bytes(pickle.dumps(json.loads(str(g['ann']))))
    return str(p)


def assert_columns_equal(got, g, c):
    """byte-equal scores, equal labels / segments / row order against the golden columns of case c"""
    assert [str(v) for v in got['video-id']] == [str(v) for v in g['out%d_vid' % c]]
    np.testing.assert_array_equal(np.asarray(got['label'], np.int64), g['out%d_label' % c])
    np.testing.assert_array_equal(np.asarray(got['t-start'], np.float64), g['out%d_ts' % c])
    np.testing.assert_array_equal(np.asarray(got['t-end'], np.float64), g['out%d_te' % c])
    assert np.asarray(got['score'], np.float64).tobytes() == g['out%d_score' % c].tobytes()
