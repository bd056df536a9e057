"""Golden vectors of the MQ EVALUATORS from the IMPORTED REFERENCE (this container only).
Run:  python tests/golden/make_golden_metrics.py   ->  tests/golden/metrics_*.npz

Synthetic ground truth in both formats the reference reads -- the CL pickle ({'val': [{'dict_db', 'label_dict'}]}, stored here
as its JSON-able content) and a JSON annotation file with duplicate events and two subsets -- scored by the reference's
`ANETdetection` (MQ/libs/utils/metrics.py; `np.float` patched, num_workers=1: joblib's workers would not see the patch) and
`evaluation_retrieval` (get_retrieval_performance.py).  Per npz: 'ann' (annotation content as JSON text), 'use_cl', 'split',
'thr', and per evaluation e: the prediction columns pred{e}_*, the task id, ap{e}[thr, cls], mAP{e}, avg{e}, and for the
retrieval metric the prediction object rjson{e} (JSON text) and recall{e}[5, 2]; metrics_formats.npz also holds
'valid_ret', the five-tuple valid_one_epoch_cl_single_gpu returns with these evaluators at current task 1.
Cases: empty predictions, a class without predictions, predictions in videos without GT, the label-remap quirks (simultaneous
map; a label missing from the GT stays raw), the 0/0 tIoU, a (class, video) group of more than 64 GT, a class of ~20 000
predictions, three CL tasks (current_task_id 0/1/2), and the recorded result dicts of eval_formats.pt against a synthetic
annotation set for those clips.  metrics_edges.npz: the edge set of `case_edges` (NaN / reversed / zero-length boundaries, special
score values, equal scores, tied tIoU, the Recall@K cut-off at r * n_gt - 1 / r * n_gt / r * n_gt + 1 predictions)."""
import importlib.util
import json
import os
import pickle
import sys
import tempfile

# The reference ranks with NumPy's default argsort()[::-1].  NumPy's AVX-512 / AVX2 sort kernels order equal keys their own
# way at every size; its portable introsort is an insertion sort, hence stable, up to 16 elements.  The tied cases of
# case_edges are recorded with the portable sort (and assert that it was stable); the tie-free cases do not depend on this.
os.environ.setdefault("NPY_DISABLE_CPU_FEATURES", "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX2")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/MQ/libs/utils"
THR = np.linspace(0.1, 0.5, 5)


def _load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


np.float = float          # removed alias the reference still uses (metrics.py:345-346)
ref_metrics = _load("metrics")
ref_retrieval = _load("get_retrieval_performance")


def score_det(ann_path, use_cl, split, preds, task):
    ev = ref_metrics.ANETdetection(ann_path, split=split, tiou_thresholds=THR, num_workers=1, use_cl=use_cl)
    p = {k: (list(v) if k == 'video-id' else np.asarray(v)) for k, v in preds.items()}
    mAP, avg, _ = ev.evaluate(p, current_task_id=task, verbose=False)
    return ev.ap, mAP, avg


def score_ret(ann_path, use_cl, split, rjson, task):
    with tempfile.NamedTemporaryFile('w', suffix='.json', delete=False) as f:
        json.dump(rjson, f)
    try:
        return ref_retrieval.evaluation_retrieval(ann_path, f.name, split, THR, use_cl=use_cl, current_task_id=task)
    finally:
        os.unlink(f.name)


def anet_obj(preds, name=lambda l: "c%d" % l):
    out = {}
    for v, s, e, l, sc in zip(preds['video-id'], preds['t-start'], preds['t-end'], preds['label'], preds['score']):
        out.setdefault(v, []).append({"segment": [float(s), float(e)], "score": float(sc), "label": name(int(l))})
    return {"version": "1.0", "external_data": "", "results": out}


def write_case(name, ann, use_cl, split, evals, extra=None):
    """evals: [(preds, task, rjson or None)]"""
    suffix = '.pkl' if use_cl else '.json'
    with tempfile.NamedTemporaryFile('wb' if use_cl else 'w', suffix=suffix, delete=False) as f:
        if use_cl:
            pickle.dump(ann, f)
        else:
            json.dump(ann, f)
    out = {'ann': np.array(json.dumps(ann)), 'use_cl': np.array(use_cl), 'split': np.array(split or ''), 'thr': THR,
           'n_eval': np.array(len(evals))}
    out.update(extra or {})
    try:
        for e, (preds, task, rjson) in enumerate(evals):
            ap, mAP, avg = score_det(f.name, use_cl, split, preds, task)
            out.update({'pred%d_vid' % e: np.array(preds['video-id'], dtype=str).reshape(-1),
                        'pred%d_ts' % e: np.asarray(preds['t-start'], np.float64),
                        'pred%d_te' % e: np.asarray(preds['t-end'], np.float64),
                        'pred%d_label' % e: np.asarray(preds['label'], np.int64),
                        'pred%d_score' % e: np.asarray(preds['score'], np.float64),
                        'task%d' % e: np.array(-1 if task is None else task),
                        'ap%d' % e: np.asarray(ap, np.float64), 'mAP%d' % e: np.asarray(mAP, np.float64),
                        'avg%d' % e: np.array(avg, np.float64)})
            if rjson is not None:
                out['rjson%d' % e] = np.array(json.dumps(rjson))
                out['recall%d' % e] = np.asarray(score_ret(f.name, use_cl, split, rjson, task), np.float64)
    finally:
        os.unlink(f.name)
    path = os.path.join(HERE, "metrics_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes")


def near(rng, s, e, jitter):
    return s + rng.normal(0, jitter), e + rng.normal(0, jitter)


def make_preds(rng, gt_rows, n_extra_per_gt, vids_extra, labels_extra, jitter=2.0):
    """predictions near the GT rows (label kept) plus random ones; scores continuous (tie-free)"""
    V, S, E, L = [], [], [], []
    for v, s, e, l in gt_rows:
        for _ in range(n_extra_per_gt):
            a, b = near(rng, s, e, jitter)
            V.append(v); S.append(min(a, b)); E.append(max(a, b)); L.append(l)
    for v in vids_extra:
        for l in labels_extra:
            s = rng.uniform(0, 100)
            V.append(v); S.append(s); E.append(s + rng.uniform(0.5, 20)); L.append(l)
    return {'video-id': V, 't-start': np.array(S), 't-end': np.array(E), 'label': np.array(L, np.int64),
            'score': rng.permutation(len(V)) / max(len(V), 1) + rng.uniform(0, 1e-4, len(V))}


def case_json(rng):
    # GT labels {1, 3, 4, 6}: activity_index {1: 0, 3: 1, 4: 2, 6: 3}
    db, rows = {}, []
    for k in range(12):
        vid = "v%02d" % k
        subset = "val" if k < 9 else "train"
        ants = []
        n = 70 if k == 0 else rng.integers(2, 8)      # video 0: one (class, video) group of > 64 GT
        for j in range(n):
            lab = 1 if k == 0 else int(rng.choice([1, 3, 4, 6]))
            s = rng.uniform(0, 200)
            ants.append({"segment": [s, s + rng.uniform(1, 15)], "label_id": lab, "label": "c%d" % lab})
        if k == 1:
            ants.append(dict(ants[0]))                                     # exact duplicate
            ants.append({"segment": [ants[1]["segment"][0] + 5e-4, ants[1]["segment"][1]], "label_id": ants[1]["label_id"],
                         "label": ants[1]["label"]})                      # duplicate within tol
        if k == 2:
            ants.append({"segment": [50.0, 50.0], "label_id": 4, "label": "c4"})   # zero-length GT
        db[vid] = {"subset": subset, "clip_id": vid, "annotations": ants}
        if subset == "val":
            rows += [(vid, a["segment"][0], a["segment"][1], a["label_id"]) for a in ref_metrics.remove_duplicate_annotations(ants)]
    # no raw 6 predictions -> class 3 has none; raw 3 -> 1 and raw 1 -> 0 (simultaneous); raw 0 / 2 missing -> stay raw and
    # collide with classes 0 / 2; raw 9 -> ignored; videos x0/x1 have no GT; v09 is train-only
    rows6 = [r for r in rows if r[3] != 6]
    p = make_preds(rng, rows6, 3, ["x0", "x1", "v09", "v03"], [0, 2, 9, 3])
    # the 0/0 case: a zero-length prediction on the zero-length GT
    for k, val in (('video-id', "v02"), ('t-start', 50.0), ('t-end', 50.0), ('label', 4), ('score', 0.77777)):
        p[k] = p[k] + [val] if k == 'video-id' else np.append(p[k], val)
    empty = {'video-id': [], 't-start': np.zeros(0), 't-end': np.zeros(0), 'label': np.zeros(0, np.int64),
             'score': np.zeros(0)}
    write_case("json", db, False, "val", [(p, None, anet_obj(p)), (empty, None, None)])


def case_large(rng):
    db, rows = {}, []
    for k in range(200):
        vid = "L%03d" % k
        ants = []
        for j in range(int(rng.integers(1, 6))):
            lab = int(rng.choice([0, 1, 2], p=[0.8, 0.1, 0.1]))
            s = rng.uniform(0, 300)
            ants.append({"segment": [s, s + rng.uniform(1, 30)], "label_id": lab, "label": "c%d" % lab})
        db[vid] = {"subset": "val", "clip_id": vid, "annotations": ants}
        rows += [(vid, a["segment"][0], a["segment"][1], a["label_id"]) for a in ants]
    p = make_preds(rng, rows, 0, [], [])
    V, S, E, L = [], [], [], []
    for i in range(21000):                                  # ~20 000 predictions of class 0
        v, s, e, l = rows[int(rng.integers(len(rows)))]
        if rng.uniform() < 0.9:
            l = 0
        a, b = near(rng, s, e, 8.0)
        V.append(v); S.append(min(a, b)); E.append(max(a, b)); L.append(l)
    p = {'video-id': V, 't-start': np.array(S), 't-end': np.array(E), 'label': np.array(L, np.int64),
         'score': (rng.permutation(len(V)) + rng.uniform(0, 0.5, len(V))) / len(V)}
    write_case("large", db, False, "val", [(p, None, None)])


def cl_ann(rng, tasks):
    """tasks: [(videos, labels)] -> the CL pickle's content"""
    val = []
    for vids, labels in tasks:
        label_dict = {"name_%d" % l: int(l) for l in labels}
        dict_db = []
        for v in vids:
            n = int(rng.integers(1, 6))
            segs, labs = [], []
            for _ in range(n):
                s = rng.uniform(0, 100)
                segs.append([s, s + rng.uniform(1, 20)]); labs.append(int(rng.choice(labels)))
            dict_db.append({"id": v, "segments": segs, "labels": labs})
        val.append({"dict_db": dict_db, "label_dict": label_dict})
    return {"val": val}


def case_cl(rng):
    tasks = [(["t0_%d" % i for i in range(6)], [0, 1, 2]), (["t1_%d" % i for i in range(6)], [3, 4]),
             (["t2_%d" % i for i in range(6)], [5, 6, 7])]
    ann = cl_ann(rng, tasks)
    evals = []
    acc = []
    for t, sub in enumerate(ann["val"]):
        acc += [(d["id"], s[0], s[1], l) for d in sub["dict_db"] for s, l in zip(d["segments"], d["labels"])]
        # labels as the model emits them (class indices of the task's activity index, plus raw ids)
        ai = {j: i for i, j in enumerate(sorted(set(r[3] for r in acc)))}
        rows = [(v, s, e, ai[l]) for v, s, e, l in acc]
        p = make_preds(rng, rows, 3, [d["id"] for d in sub["dict_db"][:2]], [0, 1])
        names = {v: k for k, v in sub["label_dict"].items()}
        vids_t = [d["id"] for d in sub["dict_db"]]
        keep = [i for i, v in enumerate(p['video-id']) if v in vids_t]
        pr = {k: ([p[k][i] for i in keep] if k == 'video-id' else p[k][keep]) for k in p}
        pr['label'] = np.array([sorted(names)[int(l) % len(names)] for l in pr['label']], np.int64)
        evals.append((p, t, anet_obj(pr, name=lambda l, n=names: n[l])))
    write_case("cl", ann, True, "val", evals)


def case_formats(rng):
    import torch
    rec = torch.load(os.path.join(HERE, "eval_formats.pt"), weights_only=False)
    names = rec["idx_classes"]
    results = rec["valid"]["results"]
    val = []
    for res in results:
        vids = sorted(set(res["video-id"]))
        labels = sorted(set(int(l) for l in res["label"]))
        dict_db = []
        for v in vids:
            idx = [i for i, x in enumerate(res["video-id"]) if x == v]
            pick = rng.choice(idx, size=min(6, len(idx)), replace=False)
            segs = [[float(res["t-start"][i]) + rng.normal(0, 1), float(res["t-end"][i]) + rng.normal(0, 1)] for i in pick]
            dict_db.append({"id": v, "segments": segs, "labels": [int(res["label"][i]) for i in pick]})
        val.append({"dict_db": dict_db, "label_dict": {names[l]: l for l in labels}})
    ann = {"val": val}
    evals = [(res, t, rec["valid"]["json"][t]) for t, res in enumerate(results)]
    # what valid_one_epoch_cl_single_gpu (train_utils.py:1016-1173) returns with these evaluators at current task 1: every task's
    # records scored by the evaluator at current_task_id=1, by the retrieval metric at its own task; query-weighted means
    # (3 + task queries, the recording's loaders)
    with tempfile.NamedTemporaryFile('wb', suffix='.pkl', delete=False) as f:
        pickle.dump(ann, f)
    try:
        acc = np.zeros(5)
        wsum = 0
        for t, res in enumerate(results):
            _, _, avg = score_det(f.name, True, "val", res, 1)
            r = score_ret(f.name, True, "val", rec["valid"]["json"][t], t)
            nq = 3 + t
            acc += nq * np.array([r[2, 0], r[2, 1], r[4, 0], r[4, 1], avg])
            wsum += nq
    finally:
        os.unlink(f.name)
    write_case("formats", ann, True, "val", evals, extra={'valid_ret': acc / wsum})


def assert_order_defined(ann, p):
    """The reference ranks with argsort()[::-1] (metrics.py:305, 329), whose order of equal keys is whatever NumPy's default
    sort does.  The edge set keeps every class at 16 predictions or fewer and every (class, video) group at 16 GT or fewer,
    where the portable sort is an insertion sort, i.e. stable; this asserts it on the very arrays the reference will sort."""
    lab = np.asarray(p['label'])
    for c in np.unique(lab):
        rows = np.flatnonzero(lab == c)
        assert len(rows) <= 16
        sc = np.asarray(p['score'])[rows]
        assert np.array_equal(sc.argsort(), sc.argsort(kind='stable')), c
        for r in rows:
            cand = np.array([a["segment"] for a in ann[p['video-id'][r]]["annotations"] if a["label_id"] == c], np.float64)
            if len(cand) == 0:
                continue
            assert len(cand) <= 16
            with np.errstate(invalid='ignore', divide='ignore'):
                t = ref_metrics.segment_iou(np.array([p['t-start'][r], p['t-end'][r]]), cand)
            assert np.array_equal(t.argsort(), t.argsort(kind='stable')), (c, r)


def case_edges():
    """Left out: NaN in a GROUND-TRUTH boundary (remove_duplicate_annotations and the JSON annotation file are not meant to
    carry it; the device tests cover it against the restatement), groups of more than 16 GT or classes of more than 16
    predictions with tied keys (the reference's order of ties is NumPy's introsort there, not a rule), and a class of the
    activity index without GT (the reference builds the index from the GT labels and cannot reach it)."""
    nan, inf = float('nan'), float('inf')

    def ants(lab, segs):
        return [{"segment": [float(a), float(b)], "label_id": lab, "label": "c%d" % lab} for a, b in segs]

    gt = {"e0": ants(0, [(0, 10), (20, 30), (40, 50)]),
          "e1": ants(1, [(50, 50), (10, 20), (60, 70)]),                       # a zero-length GT
          "e2": ants(2, [(0, 10), (20, 30), (40, 50), (60, 70)]),
          "e3": ants(3, [(0, 10), (20, 30)]),
          "e4": ants(4, [(20 * k, 20 * k + 10) for k in range(8)])}           # integer grid: tied tIoU
    rows = [
        # class 0: NaN start / end / both, more of them than GT (NaN tIoU is the best overlap until every GT is locked)
        ("e0", nan, 10, 0, .9), ("e0", 5, nan, 0, .8), ("e0", nan, nan, 0, .7), ("e0", 60, 70, 0, .95), ("e0", 21, 29, 0, .6),
        ("e0", nan, 50, 0, .5), ("e0", 41, nan, 0, .4), ("e0", 40, 50, 0, .3),
        # class 1: zero length on the zero-length GT (0/0), end < start (union 0 or negative), again zero length
        ("e1", 50, 50, 1, .9), ("e1", 20, 10, 1, .8), ("e1", 18, 12, 1, .7), ("e1", 65, 61, 1, .6), ("e1", 12, 18, 1, .5),
        ("e1", 50, 50, 1, .45), ("e1", 70, 60, 1, .4),
        # class 2: scores NaN, +inf, -inf, 0.0, -0.0; the 0.0 / -0.0 rows are one tie group whose order decides the flags
        ("e2", 0, 10, 2, nan), ("e2", 1, 10, 2, inf), ("e2", 0, 9, 2, -inf), ("e2", 20, 30, 2, 0.0), ("e2", 26, 30, 2, -0.0),
        ("e2", 20, 29, 2, 0.0), ("e2", 27, 30, 2, -0.0), ("e2", 40, 50, 2, .5), ("e2", 41, 50, 2, nan), ("e2", 60, 70, 2, -inf),
        ("e2", 61, 70, 2, inf), ("e2", 62, 70, 2, .5), ("e2", 2, 10, 2, nan),
        # class 3: equal scores, the weaker overlap sometimes ranked first
        ("e3", 0, 4, 3, .5), ("e3", 0, 10, 3, .5), ("e3", 0, 3, 3, .5), ("e3", 20, 30, 3, .7), ("e3", 20, 23, 3, .7),
        ("e3", 20, 24, 3, .5), ("e3", 1, 10, 3, .5), ("e3", 20, 29, 3, .5),
        # class 4: predictions that overlap two or all GT equally
        ("e4", 5, 25, 4, .9), ("e4", 10, 20, 4, .8), ("e4", 25, 45, 4, .7), ("e4", 5, 25, 4, .6), ("e4", 45, 65, 4, .5),
        ("e4", 0, 150, 4, .4), ("e4", 65, 85, 4, .3), ("e4", 5, 25, 4, .2), ("e4", 0, 150, 4, .1), ("e4", 30, 40, 4, .05)]
    # Recall@K cut-off: groups of 2 GT with r * 2 - 1, r * 2, r * 2 + 1 predictions for r = 1 and r = 5; the only prediction
    # that overlaps GT 0 is the last one, the first overlaps GT 1
    cut = {}
    for k, n in enumerate((1, 2, 3, 9, 10, 11)):
        vid = "q%d" % k
        gt[vid] = ants(5, [(10, 20), (40, 50)])
        segs = [[100.0 + i, 101.0 + i] for i in range(n)]
        segs[0] = [40.0, 49.0]
        segs[-1] = [10.0, 19.0]
        cut[vid] = [{"segment": s, "score": 1.0 - 0.01 * i, "label": "c5"} for i, s in enumerate(segs)]
    ann = {v: {"subset": "val", "clip_id": v, "annotations": a} for v, a in gt.items()}

    def preds(rs):
        return {'video-id': [r[0] for r in rs], 't-start': np.array([r[1] for r in rs], np.float64),
                't-end': np.array([r[2] for r in rs], np.float64), 'label': np.array([r[3] for r in rs], np.int64),
                'score': np.array([r[4] for r in rs], np.float64)}

    evals = []
    for rs in (rows, rows[::-1]):                      # reversed input: "the later row first" names other rows
        p = preds(rs)
        assert_order_defined(ann, p)
        obj = anet_obj(p)
        obj["results"].update(cut)
        evals.append((p, None, obj))
    write_case("edges", ann, False, "val", evals)


if __name__ == "__main__":
    rng = np.random.default_rng(20261016)
    case_json(rng)
    case_large(rng)
    case_cl(rng)
    case_formats(rng)
    case_edges()
