"""Golden vectors of validation with EXTERNAL CLASSIFICATION SCORES from the IMPORTED REFERENCE (this container only).
Run:  python tests/golden/make_golden_ext_scores.py   ->  tests/golden/ext_scores.npz  (data only)

The reference's `postprocess_results` (MQ/libs/utils/postprocessing.py:97-155) followed by its `ANETdetection`
(`np.float` patched, num_workers=1 as in make_golden_metrics.py) on synthetic result dicts over the annotation content of
metrics_cl.npz (three CL tasks).  Per case c: the inputs res{c}_* (result columns in the dtype the model emits them),
cls{c} (the score file's content as JSON text), fmt{c} ('pkl', 'json' or 'json_wrapped' = under a top-level 'results'
key), num_pred{c}, topk{c}, task{c}; the fused columns out{c}_*; ap{c}, mAP{c}, avg{c}.  Also the reference's
`results_to_dict` (rdict2, JSON text) and `results_to_array` (rarr2_*) of case 2, and 'valid_ret': the five-tuple of the
reference's valid_one_epoch_cl_single_gpu logic (train_utils.py:1016-1173) at current task 1 with ext_score_file set
(valid_cls), built as metrics_formats.npz's valid_ret was -- the retrieval metric sees the un-fused rows.

Cases: videos of 1, 7, 16, 17, 200, 201 and 260 rows at num_pred = 200; num_pred = 50; topk 1, 2 and 3; scores that came
from fp32; a pickle score file and JSON ones with and without the wrapper; a zero class score among the chosen classes.
The reference ranks with an unstable argsort, so ties have no defined order there: the script asserts that no two scores
inside a video are equal and that each video's topk + 1 largest class scores are distinct."""
import importlib.util
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/MQ/libs/utils"
THR = np.linspace(0.1, 0.5, 5)

np.float = float          # removed alias the reference still uses (metrics.py:345-346)


def _load_pkg():
    """the reference's metrics / postprocessing / get_retrieval_performance as submodules of a stand-in package, so that
    postprocessing.py's `from .metrics import ...` resolves without running libs/utils/__init__.py"""
    pkg = types.ModuleType("ref_mq_utils")
    pkg.__path__ = [REF]
    sys.modules["ref_mq_utils"] = pkg
    mods = {}
    for name in ("metrics", "postprocessing", "get_retrieval_performance"):
        spec = importlib.util.spec_from_file_location("ref_mq_utils." + name, os.path.join(REF, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


REFM = _load_pkg()
ref_metrics, ref_post, ref_retrieval = REFM["metrics"], REFM["postprocessing"], REFM["get_retrieval_performance"]


def write_scores(cls, fmt):
    suffix = '.pkl' if fmt == 'pkl' else '.json'
    with tempfile.NamedTemporaryFile('wb' if fmt == 'pkl' else 'w', suffix=suffix, delete=False) as f:
        if fmt == 'pkl':
            pickle.dump(cls, f)
        elif fmt == 'json_wrapped':
            json.dump({"version": "1.0", "results": cls}, f)
        else:
            json.dump(cls, f)
    return f.name


def check_tie_free(res, cls, topk):
    vids = np.asarray(res['video-id'])
    for v in sorted(set(vids.tolist())):
        s = np.asarray(res['score'])[vids == v].astype(np.float64)
        assert len(np.unique(s)) == len(s), "equal scores inside video %s" % v
        top = np.sort(np.asarray(cls[v], np.float64))[::-1][:topk + 1]
        assert len(np.unique(top)) == len(top), "equal class scores at the cut of video %s" % v


def score_det(ann_path, preds, task):
    ev = ref_metrics.ANETdetection(ann_path, split="val", tiou_thresholds=THR, num_workers=1, use_cl=True)
    p = {k: (list(v) if k == 'video-id' else np.asarray(v)) for k, v in preds.items()}
    mAP, avg, _ = ev.evaluate(p, current_task_id=task, verbose=False)
    return ev.ap, mAP, avg


def fused(res, cls, fmt, num_pred, topk):
    check_tie_free(res, cls, topk)
    path = write_scores(cls, fmt)
    try:
        return ref_post.postprocess_results({k: (list(v) if k == 'video-id' else np.asarray(v)) for k, v in res.items()},
                                            path, num_pred=num_pred, topk=topk)
    finally:
        os.unlink(path)


def make_results(rng, ann, task, counts, fp32):
    """rows near the ground truth of the videos of tasks 0..task plus random ones; counts: rows per video, in video order"""
    V, S, E, L = [], [], [], []
    vids = [d for sub in ann["val"][:task + 1] for d in sub["dict_db"]]
    for d, n in zip(vids, counts):
        for i in range(n):
            if i % 3 != 2:
                seg = d["segments"][i % len(d["segments"])]
                a, b = seg[0] + rng.normal(0, 2.0), seg[1] + rng.normal(0, 2.0)
            else:
                a = rng.uniform(0, 100)
                b = a + rng.uniform(0.5, 20)
            V.append(d["id"]); S.append(min(a, b)); E.append(max(a, b)); L.append(int(rng.integers(0, 8)))
    n = len(V)
    score = rng.permutation(n) / n + rng.uniform(0, 0.5 / n, n)
    order = rng.permutation(n)            # the rows of a video are not contiguous and not sorted
    ft = np.float32 if fp32 else np.float64
    return {'video-id': [V[i] for i in order], 't-start': np.array(S)[order].astype(np.float32),
            't-end': np.array(E)[order].astype(np.float32), 'label': np.array(L, np.int64)[order], 'score': score[order].astype(ft)}


def make_cls(rng, ann, task, n_cls=8, zero_in=None):
    """per video a class-score vector: the video's ground-truth classes score high"""
    cls = {}
    for sub in ann["val"][:task + 1]:
        for d in sub["dict_db"]:
            s = rng.uniform(0.01, 0.4, n_cls)
            for l in set(d["labels"]):
                s[l] += rng.uniform(0.4, 0.6)
            cls[d["id"]] = [float(x) for x in s]
    if zero_in is not None:               # the second-best class of this video has score exactly 0, the rest lie below
        s = -rng.uniform(0.01, 0.4, n_cls)
        d = [d for sub in ann["val"] for d in sub["dict_db"] if d["id"] == zero_in][0]
        best = d["labels"][0]
        s[best] = 0.8
        s[(best + 1) % n_cls] = 0.0
        cls[zero_in] = [float(x) for x in s]
    return cls


def main():
    rng = np.random.default_rng(20261017)
    gcl = np.load(os.path.join(HERE, "metrics_cl.npz"))
    ann = json.loads(str(gcl['ann']))
    out = {'ann': np.array(json.dumps(ann)), 'thr': THR}
    with tempfile.NamedTemporaryFile('wb', suffix='.pkl', delete=False) as f:
        pickle.dump(ann, f)
    ann_path = f.name
    edge = [1, 7, 16, 17, 200, 201, 260]
    cases = [
        # (task, rows per video, fp32, fmt, num_pred, topk, zero_in)
        (2, edge + [int(x) for x in rng.integers(3, 13, 11)], True, 'pkl', 200, 2, 't0_1'),
        (0, [int(x) for x in rng.integers(30, 71, 6)], False, 'json_wrapped', 50, 3, None),
        (1, [int(x) for x in rng.integers(5, 30, 12)], True, 'json', 200, 1, None),
    ]
    try:
        for c, (task, counts, fp32, fmt, num_pred, topk, zero_in) in enumerate(cases):
            res = make_results(rng, ann, task, counts, fp32)
            cls = make_cls(rng, ann, task, zero_in=zero_in)
            new = fused(res, cls, fmt, num_pred, topk)
            if zero_in is not None:
                assert (np.asarray(new['score'])[np.asarray(new['video-id']) == zero_in] == 0).any()
            assert not np.isnan(new['score']).any()
            ap, mAP, avg = score_det(ann_path, new, task)
            assert avg > 0
            out.update({'res%d_vid' % c: np.array(res['video-id'], dtype=str), 'res%d_ts' % c: res['t-start'],
                        'res%d_te' % c: res['t-end'], 'res%d_label' % c: res['label'], 'res%d_score' % c: res['score'],
                        'cls%d' % c: np.array(json.dumps(cls)), 'fmt%d' % c: np.array(fmt),
                        'num_pred%d' % c: np.array(num_pred), 'topk%d' % c: np.array(topk), 'task%d' % c: np.array(task),
                        'out%d_vid' % c: np.array(new['video-id'], dtype=str),
                        'out%d_ts' % c: np.asarray(new['t-start'], np.float64),
                        'out%d_te' % c: np.asarray(new['t-end'], np.float64),
                        'out%d_label' % c: np.asarray(new['label'], np.int64),
                        'out%d_score' % c: np.asarray(new['score'], np.float64),
                        'ap%d' % c: np.asarray(ap, np.float64), 'mAP%d' % c: np.asarray(mAP, np.float64),
                        'avg%d' % c: np.array(avg, np.float64)})
            if c == 2:
                out['rdict2'] = np.array(json.dumps(ref_post.results_to_dict(res)))
                arr = ref_post.results_to_array(res, num_pred)
                out['rarr2_cnt'] = np.array([len(arr[v]['score']) for v in sorted(arr)])
                out['rarr2_label'] = np.concatenate([arr[v]['label'] for v in sorted(arr)]).astype(np.int64)
                out['rarr2_score'] = np.concatenate([arr[v]['score'] for v in sorted(arr)]).astype(np.float64)
                out['rarr2_segment'] = np.concatenate([arr[v]['segment'] for v in sorted(arr)]).astype(np.float64)
        out['n_case'] = np.array(len(cases))
    finally:
        os.unlink(ann_path)

    # valid_one_epoch_cl_single_gpu with ext_score_file at current task 1 over the recorded result dicts of
    # eval_formats.pt and metrics_formats.npz's annotations: per task the retrieval metric on the rows as recorded (its own
    # task), the evaluator on the fused rows (current task); query-weighted means (3 + task queries)
    import torch
    rec = torch.load(os.path.join(HERE, "eval_formats.pt"), weights_only=False)
    gf = np.load(os.path.join(HERE, "metrics_formats.npz"))
    fann = json.loads(str(gf['ann']))
    results = rec["valid"]["results"]
    vcls = {}
    for sub in fann["val"]:
        for d in sub["dict_db"]:
            s = rng.uniform(0.01, 0.4, 22)
            for l in set(d["labels"]):
                s[l] += rng.uniform(0.4, 0.6)
            vcls[d["id"]] = [float(x) for x in s]
    with tempfile.NamedTemporaryFile('wb', suffix='.pkl', delete=False) as f:
        pickle.dump(fann, f)
    try:
        acc, wsum = np.zeros(5), 0
        for t, res in enumerate(results):
            new = fused(res, vcls, 'pkl', 200, 2)
            _, _, avg = score_det(f.name, new, 1)
            with tempfile.NamedTemporaryFile('w', suffix='.json', delete=False) as jf:
                json.dump(rec["valid"]["json"][t], jf)
            try:
                r = ref_retrieval.evaluation_retrieval(f.name, jf.name, "val", THR, use_cl=True, current_task_id=t)
            finally:
                os.unlink(jf.name)
            nq = 3 + t
            acc += nq * np.array([r[2, 0], r[2, 1], r[4, 0], r[4, 1], avg])
            wsum += nq
    finally:
        os.unlink(f.name)
    out['valid_cls'] = np.array(json.dumps(vcls))
    out['valid_ret'] = acc / wsum
    assert out['valid_ret'][4] > 0
    path = os.path.join(HERE, "ext_scores.npz")
    np.savez_compressed(path, **out)
    print("ext_scores.npz", os.path.getsize(path), "bytes; valid_ret", out['valid_ret'])


if __name__ == "__main__":
    main()
