"""NumPy restatement of the NLQ evaluators (NLQ/libs/utils/metrics.py:47-68, 107-177; NLQ/evaluate_ego4d_nlq.py:61-116), written
from the definitions, plus the helpers the NLQ metric tests share: the golden file, the ground-truth files in both formats and
the synthetic ground truth of the three-task NLQ episode case.  Test infrastructure only: the product scores on the device
(vilco_amd.utils.metrics_nlq)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS = (0.3, 0.5)
TOPK = (1, 5, 10)
EGO_CASES = ("rows", "edges", "nan")


def golden():
    return np.load(os.path.join(HERE, "golden", "nlq_metrics.npz"))


def text(g, key):
    return json.loads(str(g[key]))


def write_ego4d(gt, tmp_path, name="gt.json"):
    p = os.path.join(str(tmp_path), name)
    with open(p, "w") as f:
        json.dump(gt, f)
    return p


def write_jsonl(rows, tmp_path, name="gt.jsonl"):
    p = os.path.join(str(tmp_path), name)
    with open(p, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows))
    return p


def to_jsonl_gt(gt):
    """the jsonl ground truth ({query_id, timestamps}) of every query of an Ego4D ground truth"""
    out = []
    for video in gt["videos"]:
        for clip in video["clips"]:
            for ann in clip["annotations"]:
                for i, q in enumerate(ann["language_queries"]):
                    out.append({"query_id": "%s_%s_%d" % (clip["clip_uid"], ann["annotation_uid"], i),
                                "timestamps": [q["clip_start_sec"], q["clip_end_sec"]]})
    return out


def to_submission(records):
    """Ego4D records -> the jsonl datasets' record format"""
    return [{"query_id": "%s_%s_%d" % (r["clip_uid"], r["annotation_uid"], r["query_idx"]),
             "predicted_times": r["predicted_times"], "video_id": r["clip_uid"]} for r in records]


def gt_windows(gt):
    """{(clip_uid, annotation_uid): [[start, end], ...]}"""
    out = {}
    for video in gt["videos"]:
        for clip in video["clips"]:
            for ann in clip["annotations"]:
                out[(clip["clip_uid"], ann["annotation_uid"])] = [[q["clip_start_sec"], q["clip_end_sec"]]
                                                                  for q in ann["language_queries"]]
    return out


def iou64(rows, gt):
    """intersection over hull in fp64, both clamped at 0; 0/0 is NaN"""
    p = np.asarray(rows, dtype=np.float64).reshape(-1, np.shape(rows)[-1])
    inter = np.maximum(0.0, np.minimum(p[:, 1], gt[1]) - np.maximum(p[:, 0], gt[0]))
    hull = np.maximum(0.0, np.maximum(p[:, 1], gt[1]) - np.minimum(p[:, 0], gt[0]))
    with np.errstate(invalid='ignore', divide='ignore'):
        return 1.0 * inter / hull


def iou32(rows, gt):
    """fp32 operands, intersection clamped at 0, hull not, fp32 quotient"""
    p = np.asarray(rows, dtype=np.float64).reshape(-1, np.shape(rows)[-1]).astype(np.float32)
    g = np.asarray(gt, dtype=np.float64).astype(np.float32)
    inter = np.minimum(p[:, 1], g[1]) - np.maximum(p[:, 0], g[0])
    hull = np.maximum(p[:, 1], g[1]) - np.minimum(p[:, 0], g[0])
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.where(inter < 0, np.float32(0), inter) / hull
    assert q.dtype == np.float32
    return q.astype(np.float64)


def flags_and_top1(pred, cnt, gt, thresholds=THRESHOLDS, ranks=TOPK, mode=0):
    """flags [n, n_thr, n_rank] and the first-row IoU [n] of packed predictions pred [n, k_cap, 2], cnt [n], gt [n, 2]"""
    pred, gt = np.asarray(pred), np.asarray(gt, dtype=np.float64)
    n, k_cap = pred.shape[:2]
    p = pred.astype(np.float64)
    g = gt[:, None, :]
    with np.errstate(invalid='ignore', divide='ignore'):
        if mode == 0:
            inter = np.maximum(0.0, np.minimum(p[..., 1], g[..., 1]) - np.maximum(p[..., 0], g[..., 0]))
            hull = np.maximum(0.0, np.maximum(p[..., 1], g[..., 1]) - np.minimum(p[..., 0], g[..., 0]))
            ov = 1.0 * inter / hull
        else:
            p32, g32 = p.astype(np.float32), g.astype(np.float32)
            inter = np.minimum(p32[..., 1], g32[..., 1]) - np.maximum(p32[..., 0], g32[..., 0])
            hull = np.maximum(p32[..., 1], g32[..., 1]) - np.minimum(p32[..., 0], g32[..., 0])
            ov = (np.where(inter < 0, np.float32(0), inter) / hull).astype(np.float64)
    valid = np.arange(k_cap)[None, :] < np.asarray(cnt)[:, None]
    flags = np.zeros((n, len(thresholds), len(ranks)), dtype=bool)
    for t, thr in enumerate(thresholds):
        over = (ov > thr) & valid
        for r, k in enumerate(ranks):
            flags[:, t, r] = over[:, :k].any(axis=1)
    top1 = np.where(np.asarray(cnt) > 0, ov[:, 0], np.nan)
    return flags, top1


def evaluate(records, windows, thresholds=THRESHOLDS, ranks=TOPK, mode=0):
    """(flags [n, n_thr, n_rank], first-row IoU [n]) of Ego4D records against gt_windows()"""
    flags = np.zeros((len(records), len(thresholds), len(ranks)), dtype=bool)
    top1 = np.zeros(len(records))
    for i, rec in enumerate(records):
        key = (rec["clip_uid"], rec["annotation_uid"])
        assert key in windows, "Instance not present!"
        ov = (iou64 if mode == 0 else iou32)(rec["predicted_times"], windows[key][rec["query_idx"]])
        top1[i] = ov[0]
        for t, thr in enumerate(thresholds):
            for r, k in enumerate(ranks):
                flags[i, t, r] = (ov > thr)[:k].any()
    return flags, top1


def recall(flags):
    """the mean of the booleans: an exact integer sum over n"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return flags.sum(axis=0).astype(np.float64) / np.float64(len(flags))


def episode_gt():
    """synthetic Ego4D ground truth for the query ids of cases.nlq_episode_query: clip 'clipXX' holds annotation 'annXX' whose
    language query k is the query's first moment (earlier indices are fillers no record refers to)"""
    from parity_util import cases
    clips = []
    for task in range(cases.NLQ_EP_TASKS):
        for k in range(cases.NLQ_EP_PER_TASK):
            q = cases.nlq_episode_query(task, k)
            uid, idx = q['query_id'].split("_")[:2]
            s, e = [float(x) for x in q['segments'][0]]
            queries = [{"clip_start_sec": 0.0, "clip_end_sec": 1.0 + j} for j in range(int(idx))]
            queries.append({"clip_start_sec": s, "clip_end_sec": e})
            clips.append({"clip_uid": q['video_id'], "annotations": [{"annotation_uid": uid, "language_queries": queries}]})
    return {"videos": [{"clips": clips}]}
