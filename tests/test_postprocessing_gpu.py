"""GPU: external classification scores fused on the device (csrc/fuse.hip via vilco_amd.utils.postprocessing) against the
imported reference's goldens (tests/golden/ext_scores.npz) -- fused scores byte-equal, labels / segments / row order equal,
AP within 1e-12 -- against the NumPy restatement on NaN and tie-heavy inputs, and through the validation loop."""
import os

import numpy as np
import pytest
import torch

import metrics_restatement as R
import postprocessing_restatement as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _case(g, c, tmp_path):
    return (P.case_results(g, c), P.write_score_file(P.case_cls(g, c), str(g['fmt%d' % c]), tmp_path),
            int(g['num_pred%d' % c]), int(g['topk%d' % c]))


@pytest.mark.parametrize("c", [0, 1, 2])
def test_device_columns_match_reference_goldens(c, tmp_path):
    from vilco_amd.utils import postprocessing as PP
    g = P.golden()
    res, path, num_pred, topk = _case(g, c, tmp_path)
    got = PP.postprocess_results(res, path, num_pred=num_pred, topk=topk)
    assert got['label'].dtype == np.int64 and got['score'].dtype == np.float64
    P.assert_columns_equal(got, g, c)
    # the device form: same rows, one video id per video, offsets that delimit them
    fused = PP.fuse_external_scores(res, P.case_cls(g, c), num_pred=num_pred, topk=topk)
    assert all(fused[k].is_cuda for k in ('video-index', 'label', 't-start', 't-end', 'score'))
    assert fused['video-id'] == sorted(set(res['video-id']))
    assert fused['score'].cpu().numpy().tobytes() == g['out%d_score' % c].tobytes()
    vid_rows = [fused['video-id'][i] for i in fused['video-index'].cpu().numpy()]
    assert vid_rows == [str(v) for v in g['out%d_vid' % c]]
    cnt = np.unique(np.asarray(res['video-id']), return_counts=True)[1]
    np.testing.assert_array_equal(np.diff(fused['offsets']), topk * np.minimum(cnt, num_pred))
    # a pickled result dict is read from its path
    import pickle
    p = tmp_path / "res.pkl"
    p.write_bytes(pickle.dumps(res))
    P.assert_columns_equal(PP.postprocess_results(str(p), path, num_pred=num_pred, topk=topk), g, c)


def _assert_same(got, want, equal_nan=False):
    assert got['video-id'] == want['video-id']
    np.testing.assert_array_equal(got['label'], want['label'])
    np.testing.assert_array_equal(got['t-start'], want['t-start'])
    np.testing.assert_array_equal(got['t-end'], want['t-end'])
    if equal_nan:
        assert np.array_equal(got['score'], want['score'], equal_nan=True)
        keep = ~np.isnan(want['score'])
        assert got['score'][keep].tobytes() == want['score'][keep].tobytes()
    else:
        assert got['score'].tobytes() == want['score'].tobytes()


def test_negative_class_score_gives_nan():
    from vilco_amd.utils import postprocessing as PP
    rng = np.random.default_rng(3)
    n = 40
    res = {'video-id': ['a'] * 25 + ['b'] * 15, 't-start': rng.uniform(0, 50, n), 't-end': rng.uniform(50, 90, n),
           'label': np.zeros(n, np.int64), 'score': rng.uniform(0.05, 1, n)}
    cls = {'a': [-0.5, -0.25, -0.75, -1.0], 'b': [0.5, -0.125, -0.25, -0.5]}
    want = P.fuse(res, cls, num_pred=20, topk=2)
    assert np.isnan(want['score']).sum() == 2 * 20 + 15 and (~np.isnan(want['score'])).sum() == 15
    got = PP.fused_to_host(PP.fuse_external_scores(res, cls, num_pred=20, topk=2))
    _assert_same(got, want, equal_nan=True)
    assert got['label'][:40].tolist() == [1] * 20 + [0] * 20          # ranked by value, NaN or not


def _tie_case(rng, n_vid=37, num_pred=50, n_cls=12):
    vids, score = [], []
    for v in range(n_vid):
        n = int(rng.integers(1, 140))
        s = np.round(rng.uniform(0, 1, n), 1)                            # ~11 distinct values: large tie groups
        if v % 3 == 0 and n > num_pred + 10:
            s[np.argsort(s, kind='stable')[::-1][num_pred - 6:num_pred + 6]] = 0.35   # a tie group that straddles num_pred
        vids += ["v%03d" % v] * n
        score.append(s)
    score = np.concatenate(score)
    n = len(vids)
    order = rng.permutation(n)
    res = {'video-id': [vids[i] for i in order], 't-start': rng.uniform(0, 50, n).astype(np.float32),
           't-end': rng.uniform(50, 90, n).astype(np.float32), 'label': np.zeros(n, np.int64), 'score': score[order]}
    cls = {}
    for v in sorted(set(vids)):
        c = np.round(rng.uniform(0, 1, n_cls), 1)
        c[rng.choice(n_cls, 4, replace=False)] = c.max()                 # equal class scores at the topk cut
        cls[v] = c.tolist()
    return res, cls


def test_ties_match_restatement_and_runs_are_bytewise_equal():
    from vilco_amd.utils import postprocessing as PP
    rng = np.random.default_rng(5)
    res, cls = _tie_case(rng)
    # the case is what it claims to be
    vids = np.asarray(res['video-id'])
    straddle = 0
    for v in np.unique(vids):
        s = np.sort(res['score'][vids == v])[::-1]
        straddle += len(s) > 50 and s[49] == s[50]
        top = np.sort(cls[v])[::-1]
        assert top[1] == top[2] == top[3]
    assert straddle >= 3
    want = P.fuse(res, cls, num_pred=50, topk=3)
    a = PP.fuse_external_scores(res, cls, num_pred=50, topk=3)
    b = PP.fuse_external_scores(res, cls, num_pred=50, topk=3)
    _assert_same(PP.fused_to_host(a), want)
    for k in ('video-index', 'label', 't-start', 't-end', 'score'):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes()


def test_video_larger_than_the_lds_table():
    """a video of more rows than the kernel ranks out of LDS takes the workspace path: same rows"""
    from vilco_amd.utils import postprocessing as PP
    rng = np.random.default_rng(9)
    n_big, n_small = 5000, 30
    n = n_big + n_small
    res = {'video-id': ['big'] * n_big + ['small'] * n_small, 't-start': rng.uniform(0, 50, n), 't-end': rng.uniform(50, 90, n),
           'label': np.zeros(n, np.int64), 'score': np.round(rng.uniform(0, 1, n), 3)}
    cls = {'big': rng.uniform(0, 1, 20).tolist(), 'small': rng.uniform(0, 1, 20).tolist()}
    want = P.fuse(res, cls, num_pred=4500, topk=2)
    _assert_same(PP.fused_to_host(PP.fuse_external_scores(res, cls, num_pred=4500, topk=2)), want)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_evaluator_on_device_columns(c, tmp_path):
    from vilco_amd.utils import metrics as M
    from vilco_amd.utils import postprocessing as PP
    g = P.golden()
    res, path, num_pred, topk = _case(g, c, tmp_path)
    ev = M.ANETdetection(P.ann_file(g, tmp_path), 'val', tiou_thresholds=g['thr'], use_cl=True)
    task = int(g['task%d' % c])
    fused = PP.fuse_external_scores(res, P.case_cls(g, c), num_pred=num_pred, topk=topk)
    gt, cols = ev.prepare(fused, task)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in cols)
    assert cols[4].data_ptr() == fused['score'].data_ptr()              # passed on as it is
    mAP, avg, _ = ev.evaluate(fused, current_task_id=task, verbose=False)
    np.testing.assert_allclose(ev.ap, g['ap%d' % c], rtol=0, atol=1e-12)
    np.testing.assert_allclose(mAP, g['mAP%d' % c], rtol=0, atol=1e-12)
    assert abs(avg - float(g['avg%d' % c])) <= 1e-12
    ap_dev = ev.ap.copy()
    # the host-format output gives the same values
    host = PP.postprocess_results(res, path, num_pred=num_pred, topk=topk)
    mAP_h, avg_h, _ = ev.evaluate(host, current_task_id=task, verbose=False)
    np.testing.assert_allclose(ev.ap, g['ap%d' % c], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(ev.ap, ap_dev)
    assert avg_h == avg


def test_evaluator_remaps_device_labels_without_cl(tmp_path):
    """a JSON annotation set (labels remapped through the activity index): device columns score as the host columns do"""
    from vilco_amd.utils import metrics as M
    from vilco_amd.utils import postprocessing as PP
    g = R.golden("json")
    ev = M.ANETdetection(R.ann_file(g, tmp_path), 'val', tiou_thresholds=g['thr'])
    res = R.preds(g, 0)
    rng = np.random.default_rng(13)
    cls = {v: rng.uniform(0, 1, 8).tolist() for v in set(res['video-id'])}
    fused = PP.fuse_external_scores(res, cls, num_pred=30, topk=3)
    ev.evaluate(fused, verbose=False)
    ap_dev = ev.ap.copy()
    ev.evaluate(PP.fused_to_host(fused), verbose=False)
    assert ap_dev.max() > 0
    np.testing.assert_array_equal(ap_dev, ev.ap)


class _ValTasks:
    def get_valSet_by_taskNum(self, n):
        from parity_util import cases
        return [([[c] for c in cases.eval_clips(k)], 3 + k) for k in range(n)]


class _Replay(torch.nn.Module):
    """returns, clip by clip, the outputs the reference model produced (the recorded result dicts of eval_formats.pt)"""
    list_bias_layers = ()

    def __init__(self, calls):
        super().__init__()
        self.by_vid = {}
        for c in calls:
            vids = c['video-id']
            for vid in dict.fromkeys(vids):
                rows = [i for i, v in enumerate(vids) if v == vid]
                self.by_vid[vid] = {'video_id': vid, 'segments': torch.tensor(np.stack([c['t-start'][rows], c['t-end'][rows]], 1)),
                                    'scores': torch.tensor(c['score'][rows]), 'labels': torch.tensor(c['label'][rows])}

    def forward(self, video_list, task_id=0, is_training=False):
        return [self.by_vid[v['video_id']] for v in video_list]


def _validation_setup(tmp_path):
    from vilco_amd.utils.metrics import make_mq_evaluators
    rec = torch.load(os.path.join(HERE, "golden", "eval_formats.pt"), weights_only=False)
    gf = R.golden("formats")
    ev, rv = make_mq_evaluators(R.ann_file(gf, tmp_path), split='val', use_cl=True)
    return rec, gf, ev, rv


def test_validation_loop_with_external_scores(tmp_path):
    """valid_one_epoch_cl_single_gpu / final_validate with ext_score_file return what the reference's loop gives with it.
    Without the fused path this fails with NotImplementedError."""
    import json
    from vilco_amd.utils import train_utils as tu
    g = P.golden()
    rec, gf, ev, rv = _validation_setup(tmp_path)
    path = P.write_score_file(json.loads(str(g['valid_cls'])), 'pkl', tmp_path)
    model = _Replay(rec['valid']['results'])
    ret = tu.valid_one_epoch_cl_single_gpu(_ValTasks(), model, 0, 1, ext_score_file=path, evaluator=ev, output_file='g',
                                           retrieval_eval=rv, idx_classes=rec['idx_classes'])
    assert len(ret) == 5
    np.testing.assert_allclose(np.array(ret, dtype=np.float64), g['valid_ret'], rtol=0, atol=1e-12)
    assert abs(ret[4] - gf['valid_ret'][4]) > 1e-6                      # the fused rows score differently from the plain ones
    fin = tu.final_validate(_ValTasks(), model, 0, 1, ext_score_file=path, evaluator=ev, output_file='g',
                            list_val_recall_ii={'val': [0.5]}, list_val_mAP_ii={'val': [0.5]}, retrieval_eval=rv,
                            idx_classes=rec['idx_classes'])
    assert len(fin) == 7
    np.testing.assert_allclose(np.array(fin[:5], dtype=np.float64), g['valid_ret'], rtol=0, atol=1e-12)
    assert np.isfinite(fin[5]) and np.isfinite(fin[6])


def test_validation_loop_without_external_scores_is_unchanged(tmp_path):
    from vilco_amd.utils import train_utils as tu
    rec, gf, ev, rv = _validation_setup(tmp_path)
    ret = tu.valid_one_epoch_cl_single_gpu(_ValTasks(), _Replay(rec['valid']['results']), 0, 1, ext_score_file=None,
                                           evaluator=ev, output_file='g', retrieval_eval=rv, idx_classes=rec['idx_classes'])
    np.testing.assert_allclose(np.array(ret, dtype=np.float64), gf['valid_ret'], rtol=0, atol=1e-12)


def test_driver_callback_passes_the_config_key_through(tmp_path):
    """train_cl.make_mq_validate hands cfg['test_cfg']['ext_score_file'] to the validation loop"""
    import json
    from vilco_amd import train_cl
    g = P.golden()
    rec, gf, ev, rv = _validation_setup(tmp_path)
    path = P.write_score_file(json.loads(str(g['valid_cls'])), 'json_wrapped', tmp_path)
    model = _Replay(rec['valid']['results'])
    cfg = {'dataset_name': 'ego4d_cl', 'test_cfg': {'ext_score_file': path}}
    validate = train_cl.make_mq_validate(cfg, _ValTasks(), ev, retrieval_eval=rv, idx_classes=rec['idx_classes'])
    assert abs(validate(model, 0, 1) - g['valid_ret'][4]) <= 1e-12
    cfg['test_cfg']['ext_score_file'] = None
    validate = train_cl.make_mq_validate(cfg, _ValTasks(), ev, retrieval_eval=rv, idx_classes=rec['idx_classes'])
    assert abs(validate(model, 0, 1) - gf['valid_ret'][4]) <= 1e-12
