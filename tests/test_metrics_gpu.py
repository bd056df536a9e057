"""GPU: the HIP evaluators (csrc/evaluate.hip via vilco_amd.utils.metrics) against the imported reference's goldens and
against the NumPy restatement on seeded large and tie-heavy inputs: every TP flag equal, AP within 1e-12, recall counts
equal; repeated calls bitwise equal."""
import numpy as np
import pytest
import torch

import metrics_restatement as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", R.GOLDENS)
def test_device_matches_reference_goldens(name, tmp_path):
    from vilco_amd.utils import metrics as M
    g = R.golden(name)
    path = R.ann_file(g, tmp_path)
    use_cl = bool(g['use_cl'])
    ev, ret = M.make_mq_evaluators(path, split=str(g['split']), tiou_thresholds=tuple(g['thr']), use_cl=use_cl)
    for e in range(int(g['n_eval'])):
        mAP, avg, _ = ev.evaluate(R.preds(g, e), current_task_id=R.task(g, e), verbose=False)
        np.testing.assert_allclose(ev.ap, g['ap%d' % e], rtol=0, atol=1e-12)
        np.testing.assert_allclose(mAP, g['mAP%d' % e], rtol=0, atol=1e-12)
        assert abs(avg - float(g['avg%d' % e])) <= 1e-12
        # TP flags equal the restatement's
        gt, cols = ev.prepare(R.preds(g, e), R.task(g, e))
        ap_d, tp_d = M.det_ap_device(gt, *cols, g['thr'], want_flags=True)
        ap_r, tp_r = R.restated_det(path, g, e)
        np.testing.assert_array_equal(tp_d, tp_r)
        if 'recall%d' % e in g:
            import json
            r = ret(json.loads(str(g['rjson%d' % e])), current_task_id=R.task(g, e))
            np.testing.assert_array_equal(r, g['recall%d' % e])


_random_case, _device_gt = R.random_case, R.device_gt


@pytest.mark.parametrize("ties", [False, True])
def test_device_matches_restatement_large(ties):
    from vilco_amd.utils import metrics as M
    rng = np.random.default_rng(7 + ties)
    n_pred, n_cls, n_vid = (200_000, 110, 2000) if not ties else (60_000, 20, 300)
    (vidx, cls, ts, te, score), (gvid, gcls, gs, ge) = _random_case(rng, n_pred, n_cls, n_vid, ties)
    gt = _device_gt(gvid, gcls, gs, ge, n_cls, n_vid)
    # the device GT indexes videos by sorted string id; map the prediction videos the same way
    vmap = M._video_index(np.array(["%d" % v for v in vidx], dtype=object), gt.video_index)
    gv = M._video_index(np.array(["%d" % v for v in gvid], dtype=object), gt.video_index)
    c = np.where((cls >= 0) & (cls < n_cls), cls, -1).astype(np.int32)
    thr = np.linspace(0.1, 0.5, 5)
    ap_d, tp_d = M.det_ap_device(gt, vmap, c, ts, te, score, thr, want_flags=True)
    ap_r, tp_r = R.det_ap(vmap, c, ts, te, score, gv, gcls, gs, ge, n_cls, thr)
    np.testing.assert_array_equal(tp_d, tp_r)
    np.testing.assert_allclose(ap_d, ap_r, rtol=0, atol=1e-12)
    ap_2, tp_2 = M.det_ap_device(gt, vmap, c, ts, te, score, thr, want_flags=True)
    assert ap_2.tobytes() == ap_d.tobytes() and np.array_equal(tp_2, tp_d)


def test_retrieval_device_matches_restatement():
    from vilco_amd.utils import metrics as M
    rng = np.random.default_rng(11)
    groups = []
    for k in range(3000):
        m = int(rng.integers(1, 90 if k % 500 == 0 else 4))     # some groups of > 64 GT
        gs = np.round(rng.uniform(0, 100, m), 1 if k % 2 else 6)
        g = np.stack([gs, gs + np.round(rng.uniform(0, 10, m), 1)], 1)
        n = int(rng.integers(0, 12))
        ps = np.round(rng.uniform(0, 100, n), 1)
        p = np.stack([ps, ps + np.round(rng.uniform(0, 10, n), 1)], 1)
        groups.append((p, g))
    ps = np.concatenate([p[:, 0] for p, _ in groups]); pe = np.concatenate([p[:, 1] for p, _ in groups])
    pcnt = np.array([len(p) for p, _ in groups]); poff = np.r_[0, np.cumsum(pcnt)[:-1]]
    gs = np.concatenate([g[:, 0] for _, g in groups]); ge = np.concatenate([g[:, 1] for _, g in groups])
    goff = np.r_[0, np.cumsum([len(g) for _, g in groups])]
    hits, total = M.retrieval_hits_device(ps, pe, poff, pcnt, gs, ge, goff, M.RETRIEVAL_TIOUS, M.RETRIEVAL_RANKS)
    h_r, t_r = R.retrieval_hits(groups)
    assert total == t_r
    np.testing.assert_array_equal(hits, h_r)
    hits2, _ = M.retrieval_hits_device(ps, pe, poff, pcnt, gs, ge, goff, M.RETRIEVAL_TIOUS, M.RETRIEVAL_RANKS)
    np.testing.assert_array_equal(hits2, hits)


def test_missing_prediction_video_raises(tmp_path):
    import json
    from vilco_amd.utils import metrics as M
    g = R.golden("cl")
    _, ret = M.make_mq_evaluators(R.ann_file(g, tmp_path), use_cl=True)
    obj = json.loads(str(g['rjson0']))
    obj['results'].pop(sorted(obj['results'])[0])
    with pytest.raises(KeyError):
        ret(obj, current_task_id=0)


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


def test_validation_loop_with_device_evaluators(tmp_path):
    """valid_one_epoch_cl_single_gpu with make_mq_evaluators returns the five-tuple the reference's evaluators give"""
    import os
    from vilco_amd.utils import train_utils as tu
    from vilco_amd.utils.metrics import make_mq_evaluators
    rec = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_formats.pt"),
                     weights_only=False)
    g = R.golden("formats")
    ev, rv = make_mq_evaluators(R.ann_file(g, tmp_path), split='val', use_cl=True)
    ret = tu.valid_one_epoch_cl_single_gpu(_ValTasks(), _Replay(rec['valid']['results']), 0, 1, evaluator=ev, output_file='g',
                                           retrieval_eval=rv, idx_classes=rec['idx_classes'])
    assert len(ret) == 5
    np.testing.assert_allclose(np.array(ret, dtype=np.float64), g['valid_ret'], rtol=0, atol=1e-12)
