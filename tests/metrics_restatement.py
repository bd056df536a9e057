"""NumPy restatement of the MQ evaluators (MQ/libs/utils/metrics.py:274-393, get_retrieval_performance.py:116-184), written
from the definitions, with the project's tie rule (the later row first on equal scores / equal tIoU) and the TP flags of every
prediction.  Test infrastructure only: the product scores on the device (vilco_amd.utils.metrics)."""
import numpy as np


def _desc(x):
    """the reverse of a stable ascending sort: NaN first, equal keys with the later row first"""
    return np.argsort(x, kind='stable')[::-1]


def det_ap(vidx, cls, ts, te, score, gt_vidx, gt_cls, gt_s, gt_e, n_cls, thresholds):
    """ap[n_thr, n_cls], tp flags [n_thr, n_pred] (input order).  Predictions with cls outside [0, n_cls) are ignored,
    those of a video without GT of their class are FPs.  GT rows in the reference's order.  A class without GT rows has AP 0
    whatever its predictions: the reference builds its class index from the GT labels and cannot reach that state (its
    recall would be 0/0), so 0 is the value this library documents (include/vilco_hip.h, vilco_det_ap)."""
    thr = np.asarray(thresholds, dtype=np.float64)
    n_thr, n = len(thr), len(cls)
    ap = np.zeros((n_thr, n_cls))
    tp_all = np.zeros((n_thr, n), dtype=bool)
    for c in range(n_cls):
        gsel = np.flatnonzero(gt_cls == c)
        npos = float(len(gsel))
        rows = np.flatnonzero(cls == c)
        if len(rows) == 0 or len(gsel) == 0:
            continue
        rows = rows[_desc(score[rows])]
        by_video = {}
        for j in gsel:
            by_video.setdefault(int(gt_vidx[j]), []).append(j)
        locked = {v: np.zeros((n_thr, len(js)), dtype=bool) for v, js in by_video.items()}
        tp = np.zeros((n_thr, len(rows)))
        for k, r in enumerate(rows):
            js = by_video.get(int(vidx[r]))
            if js is None:
                continue
            gs, ge = gt_s[js], gt_e[js]
            inter = (np.minimum(te[r], ge) - np.maximum(ts[r], gs)).clip(0)
            with np.errstate(invalid='ignore', divide='ignore'):
                tiou = inter / ((ge - gs) + (te[r] - ts[r]) - inter)
            order = _desc(tiou)
            lk = locked[int(vidx[r])]
            for t in range(n_thr):
                for j in order:
                    if tiou[j] < thr[t]:
                        break
                    if lk[t, j]:
                        continue
                    lk[t, j] = True
                    tp[t, k] = 1
                    tp_all[t, r] = True
                    break
        fp = 1 - tp
        tpc, fpc = np.cumsum(tp, axis=1), np.cumsum(fp, axis=1)
        rec, prec = tpc / npos, tpc / (tpc + fpc)
        for t in range(n_thr):
            mprec = np.hstack([[0], prec[t], [0]])
            mrec = np.hstack([[0], rec[t], [1]])
            mprec = np.maximum.accumulate(mprec[::-1])[::-1]
            idx = np.flatnonzero(mrec[1:] != mrec[:-1]) + 1
            ap[t, c] = np.sum((mrec[idx] - mrec[idx - 1]) * mprec[idx])
    return ap, tp_all


def overlap(ps, pe, gs, ge):
    """iou(), get_retrieval_performance.py:166-184: intersection over the hull, [n_pred, n_gt]; np.maximum / np.minimum
    propagate NaN, so a NaN boundary on either side gives a NaN overlap, which is no hit"""
    inter = np.maximum(0.0, np.minimum(pe[:, None], ge[None, :]) - np.maximum(ps[:, None], gs[None, :]))
    union = np.maximum(0.0, np.maximum(pe[:, None], ge[None, :]) - np.minimum(ps[:, None], gs[None, :]))
    with np.errstate(invalid='ignore', divide='ignore'):
        return 1.0 * inter / union


def retrieval_hits(groups, tious=(0.1, 0.2, 0.3, 0.4, 0.5), ranks=(1, 5)):
    """groups: [(pred [n, 2], gt [m, 2])] -> (hits[n_thr, n_rank], total)"""
    hits = np.zeros((len(tious), len(ranks)), dtype=np.int64)
    total = 0
    for pred, gt in groups:
        pred, gt = np.asarray(pred, np.float64).reshape(-1, 2), np.asarray(gt, np.float64).reshape(-1, 2)
        m = len(gt)
        total += m
        if len(pred) == 0:
            continue
        ov = overlap(pred[:, 0], pred[:, 1], gt[:, 0], gt[:, 1])
        for i, t in enumerate(tious):
            for j, r in enumerate(ranks):
                hits[i, j] += int((ov[:r * m] > t).any(axis=0).sum())
    return hits, total


# ----------------------------------------------------------------------------------------------- golden-case plumbing
GOLDENS = ("json", "large", "cl", "formats", "edges")


def golden(name):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_%s.npz" % name))


def ann_file(g, tmp_path):
    """the case's annotation file (CL: the pickle) under tmp_path"""
    import json
    import pickle
    ann = json.loads(str(g['ann']))
    if bool(g['use_cl']):
        p = tmp_path / "ann.pkl"
        p.write_bytes(pickle.dumps(ann))
    else:
        p = tmp_path / "ann.json"
        p.write_text(json.dumps(ann))
    return str(p)


def preds(g, e):
    return {'video-id': [str(x) for x in g['pred%d_vid' % e]], 't-start': g['pred%d_ts' % e], 't-end': g['pred%d_te' % e],
            'label': g['pred%d_label' % e], 'score': g['pred%d_score' % e]}


def task(g, e):
    t = int(g['task%d' % e])
    return None if t < 0 else t


def restated_det(path, g, e):
    """the restatement on the host columns the product packs (vilco_amd.utils.metrics' loaders / remap, no GPU)"""
    from vilco_amd.utils import metrics as M
    use_cl = bool(g['use_cl'])
    gt, ai = M.load_gt_seg_from_json(path, split=str(g['split']) or None, use_cl=use_cl)
    t = task(g, e)
    if use_cl:
        gt, ai = gt[t], ai[t]
    vindex = {v: i for i, v in enumerate(sorted(set(gt['video-id'])))}
    gvid = np.array([vindex[v] for v in gt['video-id']], dtype=np.int64)
    p = preds(g, e)
    cls = p['label'] if use_cl else M._remap(p['label'], ai)
    vidx = M._video_index(np.asarray(p['video-id'], dtype=object), vindex)
    return det_ap(vidx, cls, p['t-start'], p['t-end'], p['score'], gvid, gt['label'], gt['t-start'], gt['t-end'], len(ai),
                  g['thr'])


def restated_recall(path, g, e):
    import json
    from vilco_amd.utils import metrics as M
    mr = M.Moment_Retrieval.__new__(M.Moment_Retrieval)
    mr.use_cl = bool(g['use_cl'])
    mr.ground_truth = M._load_retrieval_gt(path, str(g['split']), mr.use_cl)
    mr.prediction = M._load_retrieval_pred(json.loads(str(g['rjson%d' % e])))
    ps, pe, poff, pcnt, gs, ge, goff = mr.pack(task(g, e))
    groups = [(np.stack([ps[o:o + c], pe[o:o + c]], 1), np.stack([gs[goff[k]:goff[k + 1]], ge[goff[k]:goff[k + 1]]], 1))
              for k, (o, c) in enumerate(zip(poff, pcnt))]
    return retrieval_hits(groups)


# ------------------------------------------------------------------------------------------------- seeded random cases
def random_case(rng, n_pred, n_cls, n_vid, ties):
    n_gt = n_vid * 5
    gvid = rng.integers(0, n_vid, n_gt)
    gcls = rng.integers(0, n_cls, n_gt)
    gs = np.round(rng.uniform(0, 100, n_gt), 0 if ties else 6)
    ge = gs + np.round(rng.uniform(0, 20, n_gt), 0 if ties else 6)
    src = rng.integers(0, n_gt, n_pred)
    vidx = np.where(rng.uniform(size=n_pred) < 0.97, gvid[src], n_vid + 1).astype(np.int64)
    cls = np.where(rng.uniform(size=n_pred) < 0.9, gcls[src], rng.integers(-1, n_cls + 2, n_pred))
    jit = 0 if ties else 3.0
    ts = np.round(gs[src] + rng.normal(0, 3, n_pred), 0) if ties else gs[src] + rng.normal(0, jit, n_pred)
    te = np.maximum(ts, np.round(ge[src] + rng.normal(0, 3, n_pred), 0) if ties else ge[src] + rng.normal(0, jit, n_pred))
    score = np.round(rng.uniform(size=n_pred), 1) if ties else rng.uniform(size=n_pred)
    return (vidx, cls, ts, te, score), (gvid, gcls, gs, ge)


def device_gt(gvid, gcls, gs, ge, n_cls, n_vid):
    from vilco_amd.utils import metrics as M
    gt = M._DetGT({'video-id': ["%d" % v for v in gvid], 't-start': gs, 't-end': ge, 'label': gcls},
                  {i: i for i in range(n_cls)})
    return gt
