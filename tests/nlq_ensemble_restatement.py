"""Plain-Python restatement of the NLQ ensembling recipe (NLQ/ensemble.py:7-101, 123-143 with NLQ/temporal_nms.py:6-74), written
from the rules (include/vilco_hip.h, `vilco_nlq_ensemble`), plus the helpers the ensemble tests share: the golden file
(tests/golden/nlq_ensemble.npz) and its cases as Python lists.  Test infrastructure only: the product runs on the device
(vilco_amd.utils.ensemble_nlq).  Rows are [start, end, score]; all arithmetic is Python float (fp64)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(max_input=4, top1_max_input=1, distance=2, nms_thd=0.5, max_after_nms=5, pad=True)
PARAM_ORDER = ("max_input", "top1_max_input", "distance", "nms_thd", "max_after_nms", "pad")


def top1_generator(rows, distance=2):
    """proposals [start, end, score, total] of the rows' centres, by total descending (equal totals in centre order)"""
    by_centre = {}
    for r in rows:
        by_centre[(r[1] + r[0]) / 2] = [r[0], r[1], r[2]]              # equal centres: the later row stays
    centres = sorted(by_centre)
    clusters = [[centres[0]]]
    for prev, cur in zip(centres, centres[1:]):
        if cur - prev < distance:
            clusters[-1].append(cur)
        else:
            clusters.append([cur])
    out = []
    for cl in clusters:
        members = [by_centre[c] for c in cl]
        total = 0
        for m in members:
            total = total + m[2]
        best = members[0]
        for m in members[1:]:
            if m[2] > best[2]:
                best = m
        c = len(members)
        if c % 2:
            mid = members[(c - 1) // 2]
        else:
            mid = members[c // 2] if members[c // 2][2] > members[c // 2 - 1][2] else members[c // 2 - 1]
        out.append([(a + b) / 2 for a, b in zip(mid, best)] + [total])
    order = sorted(range(len(out)), key=lambda i: (-out[i][3], i))
    return [out[i] for i in order]


def overlap(a, b):
    """intersection over the span; 0 for an empty span"""
    inter = min(a[1], b[1]) - max(a[0], b[0])
    inter = inter if inter > 0 else 0.0
    span = max(a[1], b[1]) - min(a[0], b[0])
    return 0.0 if span == 0 else inter / span


def temporal_nms(rows, nms_thd, max_after_nms=100):
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][2], i))
    left = [rows[i] for i in order]
    kept = []
    while left and len(kept) < max_after_nms:
        head = left[0]
        kept.append(head)
        left = [r for r in left[1:] if not overlap(head, r) > nms_thd]
    return kept


def ensemble_query(models, max_input=4, top1_max_input=1, distance=2, nms_thd=0.5, max_after_nms=5, pad=True):
    """models: per model the query's rows.  Returns (rows [start, end, score] after NMS and padding, rows kept before padding,
    proposals)"""
    top1 = [r for rows in models for r in rows[:top1_max_input]]
    props = top1_generator(top1, distance) if top1_max_input > 0 else []
    fusion = [list(r[:3]) for rows in models for r in rows[:max_input]] + [p[:3] for p in props]
    kept = temporal_nms(fusion, nms_thd, max_after_nms)
    out = [list(r) for r in kept]
    if pad:
        out += [list(kept[-1])] * (max_after_nms - len(kept))
    return out, len(kept), props


# ------------------------------------------------------------------------------------------------------------ the golden file
def golden():
    return np.load(os.path.join(HERE, "golden", "nlq_ensemble.npz"))


def case_names(g):
    return json.loads(str(g["cases"]))


def case_params(g, name):
    v = g[name + "__params"]
    return dict(max_input=int(v[0]), top1_max_input=int(v[1]), distance=float(v[2]), nms_thd=float(v[3]),
                max_after_nms=int(v[4]), pad=bool(v[5]))


def case_rows(g, name):
    """the case's inputs as lists: [query][model] -> rows"""
    pred, cnt = g[name + "__pred"], g[name + "__cnt"]
    n_model, n_query = cnt.shape
    return [[pred[m, q, :cnt[m, q]].astype(np.float64).tolist() for m in range(n_model)] for q in range(n_query)]


def ensemble_case(g, name):
    """the restatement on a whole case, in the golden's array layout: out [n, max_after_nms, 3], out_cnt, prop, prop_cnt"""
    p = case_params(g, name)
    rows = case_rows(g, name)
    n, n_model = len(rows), g[name + "__cnt"].shape[0]
    out = np.zeros((n, p["max_after_nms"], 3))
    out_cnt = np.zeros(n, dtype=np.int32)
    prop = np.zeros((n, max(n_model * p["top1_max_input"], 1), 4))
    prop_cnt = np.zeros(n, dtype=np.int32)
    for q, models in enumerate(rows):
        o, k, pr = ensemble_query(models, **p)
        out[q, :len(o)] = o
        out_cnt[q] = k
        prop_cnt[q] = len(pr)
        if pr:
            prop[q, :len(pr)] = pr
    return out, out_cnt, prop, prop_cnt


def ego4d_gt(windows):
    """an Ego4D ground truth with one clip, annotation and query per window: keys ('c<i>', 'a<i>', 0)"""
    clips = [{"clip_uid": "c%d" % i, "annotations": [{"annotation_uid": "a%d" % i, "language_queries": [
        {"clip_start_sec": float(s), "clip_end_sec": float(e)}]}]} for i, (s, e) in enumerate(windows)]
    return {"videos": [{"clips": clips}]}


def records(models_rows, q):
    """the record dicts of one model for queries 0..n: models_rows[q] = rows"""
    return {"query_idx": 0, "annotation_uid": "a%d" % q, "predicted_times": models_rows, "clip_uid": "c%d" % q}
