"""Golden vectors of the NLQ EVALUATORS from the IMPORTED REFERENCE (build machine only).
Run:  python tests/golden/make_golden_nlq_metrics.py   ->  tests/golden/nlq_metrics.npz   (data only)

`ReferringRecall` (NLQ/libs/utils/metrics.py; `terminaltables` comes from tests/golden/_shims) and `evaluate_nlq_performance`
(NLQ/evaluate_ego4d_nlq.py) score synthetic records against a synthetic ground truth in both formats the reference reads.
Inputs are kept as JSON text ('gt': the Ego4D ground truth; '<case>_pred': the record list), outputs as arrays:
  <case>_frac / _pct      evaluate(verbose=False) / (verbose=True): the latter is in percent (display_results works in place)
  <case>_mean, _miou      evaluate_nlq_performance: mean_results and mIoU
  <case>_avg, _flags      per_instance: average_IoU [n] and results [n_thr][n_rank][n]
  <case>_anet_frac / _pct evaluate_anet on the same records in the jsonl format (float32 [n_rank][n_thr])
Cases: 'rows' (1, 4, 5, 9, 10, 11 and 300 rows; a hit exactly at row K + 1 for each K), 'edges' (IoU equal to a threshold:
0.5 and 0.3 in fp64 do not count, float32(0.3) counts in evaluate_anet; disjoint, nested, negative starts; one key twice),
'nan' (a zero-length prediction on a zero-length ground truth as first and as later row), 'seg' (13 segments, 'seg_id' per
record, 'seg_pct' [13]: evaluate on the prefixes 1..13, as final_validate calls it), 'unknown' (a key that is not in the ground
truth: 'unknown_raises'), 'episode_pct' (the reference's recorded final-validation records of nlq_episode.pt against
nlq_metrics_restatement.episode_gt()), 'sub_records' / 'sub_json' (the record list and the challenge submission file the
reference's valid_one_epoch_nlq_singlegpu produces for the 'rows' case returned by a stand-in model as fp32 tensors;
annotation uids there carry '-' for '_', the query id being split at '_').  'ref_seconds_once' / 'ref_seconds_prefixes': the reference evaluator's time on 5 000
queries x 5 rows, once and on the 13 prefixes."""
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference/NLQ")
sys.path.insert(0, "/root/reference/NLQ/libs/utils")

import metrics as ref_metrics                 # noqa: E402  (the reference's module)
import evaluate_ego4d_nlq as ref_eval         # noqa: E402
import nlq_metrics_restatement as R           # noqa: E402

THR, TOPK = list(R.THRESHOLDS), list(R.TOPK)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(invalid='ignore', divide='ignore'):
        return fn(*a, **k)


def make_gt(rng, n_clip=60):
    clips = []
    for c in range(n_clip):
        anns = []
        for a in range(2):
            qs = []
            for _ in range(3):
                s = round(float(rng.uniform(0, 400)), 3)
                qs.append({"clip_start_sec": s, "clip_end_sec": round(s + float(rng.uniform(1, 60)), 3), "query": "q"})
            anns.append({"annotation_uid": "a%d_%d" % (c, a), "language_queries": qs})
        clips.append({"clip_uid": "c%d" % c, "annotations": anns})
    q = clips[0]["annotations"][0]["language_queries"]
    q[0].update(clip_start_sec=0.0, clip_end_sec=10.0)
    q[1].update(clip_start_sec=7.0, clip_end_sec=7.0)          # zero length
    return {"version": "1", "videos": [{"video_uid": "v0", "clips": clips[:30]}, {"video_uid": "v1", "clips": clips[30:]}]}


def window(gt, c, a, i):
    q = R.gt_windows(gt)[("c%d" % c, "a%d_%d" % (c, a))][i]
    return q[0], q[1]


def rec(c, a, i, rows):
    return {"query_idx": i, "annotation_uid": "a%d_%d" % (c, a), "predicted_times": [[float(x) for x in r] for r in rows],
            "clip_uid": "c%d" % c}


def near_rows(rng, gt, c, a, i, n):
    s, e = window(gt, c, a, i)
    rows = []
    for _ in range(n):
        a0, b0 = s + rng.normal(0, 0.6 * (e - s)), e + rng.normal(0, 0.6 * (e - s))
        rows.append([min(a0, b0), max(a0, b0), float(rng.uniform())])
    return rows


def case_rows(rng, gt):
    out = [rec(c, c % 2, c % 3, near_rows(rng, gt, c, c % 2, c % 3, n))
           for c, n in zip(range(1, 40), [1, 4, 5, 9, 10, 11, 300] * 6)]
    for j, k in enumerate(TOPK):                                # misses in rows 0..K-1, the window itself at row K
        c = 40 + j
        s, e = window(gt, c, 0, 0)
        out.append(rec(c, 0, 0, [[e + 10 + r, e + 20 + r, 0.5] for r in range(k)] + [[s, e, 0.1]] + [[s, e, 0.05]] * 2))
        out.append(rec(c, 1, 1, [[e + 10 + r, e + 20 + r, 0.5] for r in range(k - 1)] + [list(window(gt, c, 1, 1)) + [0.1]]))
    return out


def case_edges(rng, gt):
    # ground truth (c0, a0_0, 0) is [0, 10]
    e = [rec(0, 0, 0, [[0.0, 5.0, 0.9]]),                       # 5 / 10 == 0.5: not > 0.5
         rec(0, 0, 0, [[0.0, 3.0, 0.9]]),                       # 3 / 10 == 0.3 in fp64: not > 0.3; float32(0.3) > 0.3
         rec(0, 0, 0, [[20.0, 30.0, 0.9], [10.0, 12.0, 0.8]]),  # disjoint, touching
         rec(0, 0, 0, [[2.0, 4.0, 0.9], [1.0, 9.5, 0.8]]),      # nested in the ground truth
         rec(0, 0, 0, [[-30.0, 40.0, 0.9], [-1.0, 11.0, 0.8]]),  # the ground truth nested in the prediction
         rec(0, 0, 0, [[-2.0, 4.0, 0.9], [-5.0, -1.0, 0.8], [-0.5, 10.0, 0.7]]),
         rec(0, 0, 0, [[0.0, 3.0000000000000004, 0.9]]),        # one ulp above 0.3
         rec(0, 0, 0, [[4.0, 2.0, 0.9], [0.0, 10.0, 0.5]])]     # end before start
    for c in (3, 4):                                            # one key twice in one list
        rows = near_rows(rng, gt, c, 1, 2, 6)
        e += [rec(c, 1, 2, rows), rec(c, 1, 2, rows[::-1])]
    return e


def case_nan(rng, gt):
    # ground truth (c0, a0_0, 1) is [7, 7]
    return [rec(0, 0, 1, [[7.0, 7.0, 0.9], [6.0, 8.0, 0.5]]),   # NaN first: the mean IoU is NaN
            rec(0, 0, 1, [[6.0, 8.0, 0.9], [7.0, 7.0, 0.5]]),   # NaN later: no effect
            rec(0, 0, 0, [[1.0, 9.0, 0.9]]),
            rec(5, 0, 0, near_rows(rng, gt, 5, 0, 0, 7))]


def case_seg(rng, gt, n_seg=13):
    recs, seg = [], []
    for s in range(n_seg):
        for _ in range(int(rng.integers(3, 12))):
            c, a, i = int(rng.integers(1, 60)), int(rng.integers(0, 2)), int(rng.integers(0, 3))
            recs.append(rec(c, a, i, near_rows(rng, gt, c, a, i, int(rng.integers(1, 13)))))
            seg.append(s)
    return recs, np.array(seg, dtype=np.int32)


def main():
    rng = np.random.default_rng(20261016)
    gt = make_gt(rng)
    out = {'gt': np.array(json.dumps(gt)), 'thresholds': np.array(THR), 'topK': np.array(TOPK)}
    with tempfile.TemporaryDirectory() as tmp:
        ego = ref_metrics.ReferringRecall("ego4d_cl", R.write_ego4d(gt, tmp))
        anet = ref_metrics.ReferringRecall("other", R.write_jsonl(R.to_jsonl_gt(gt), tmp))
        out['num_gt_queries'] = np.array([ego.num_gt_queries, anet.num_gt_queries])
        for name, fn in (("rows", case_rows), ("edges", case_edges), ("nan", case_nan)):
            recs = fn(rng, gt)
            out[name + '_pred'] = np.array(json.dumps(recs))
            out[name + '_frac'] = quiet(ego.evaluate, recs, verbose=False)[0]
            out[name + '_pct'] = quiet(ego.evaluate, recs, verbose=True)[0]
            mean, miou, per = quiet(ref_eval.evaluate_nlq_performance, recs, gt, THR, TOPK, per_instance=True)
            out[name + '_mean'], out[name + '_miou'] = mean, np.array(miou)
            out[name + '_avg'] = np.array(per['average_IoU'], dtype=np.float64).reshape(-1)   # (each entry is a [1] array)
            out[name + '_flags'] = np.array(per['results'], dtype=bool)
            out[name + '_overlap'] = np.asarray(per['overlap'], dtype=np.float64)
            sub = R.to_submission(recs)
            out[name + '_anet_frac'] = quiet(anet.evaluate_anet, sub, verbose=False).numpy()
            out[name + '_anet_pct'] = quiet(anet.evaluate_anet, sub, verbose=True).numpy()
        recs, seg = case_seg(rng, gt)
        out['seg_pred'], out['seg_id'] = np.array(json.dumps(recs)), seg
        out['seg_pct'] = np.stack([quiet(ego.evaluate, [r for r, s in zip(recs, seg) if s <= k], verbose=True)[0]
                                   for k in range(13)])
        unknown = [rec(1, 0, 0, [[1.0, 2.0, 0.5]]), dict(rec(1, 0, 0, [[1.0, 2.0, 0.5]]), clip_uid="nope")]
        out['unknown_pred'] = np.array(json.dumps(unknown))
        try:
            quiet(ego.evaluate, unknown, verbose=False)
            out['unknown_raises'] = np.array("")
        except AssertionError as e:
            out['unknown_raises'] = np.array(str(e))
        # the reference's own recorded final-validation records of the three-task episode
        import torch
        final = torch.load(os.path.join(HERE, "nlq_episode.pt"), weights_only=False)['tasks'][-1]['results']
        ep = ref_metrics.ReferringRecall("ego4d_cl", R.write_ego4d(R.episode_gt(), tmp, "ep.json"))
        out['episode_pct'] = quiet(ep.evaluate, final, verbose=True)[0]
        out['episode_frac'] = quiet(ep.evaluate, final, verbose=False)[0]
        # the challenge submission file, written by the reference's own valid_one_epoch_nlq_singlegpu (train_utils.py:610-700)
        # from a stand-in model that returns the 'rows' case as fp32 tensors; the recording evaluator keeps its record list
        sys.path.insert(0, HERE)
        import make_golden_nlq_episode as mge
        import make_golden_nlq_model as mgm
        TU = mge.ref_train_utils(mgm.ref_modules())
        rows = json.loads(str(out['rows_pred']))

        class Model:
            def eval(self):
                return self

            def __call__(self, video_list, is_training=False):
                r = rows[video_list[0]['i']]['predicted_times']
                t = torch.tensor(r, dtype=torch.float32)
                return [{'segments': t[:, :2].contiguous(), 'scores': t[:, 2].contiguous()}]

        class Keep:
            dataset = "ego4d"

            def evaluate(self, results, verbose=True):
                self.results = json.loads(json.dumps(results))
                return np.zeros((2, 3)), ""
        loader = [[{'i': i, 'query_id': '%s_%d' % (r['annotation_uid'].replace('_', '-'), r['query_idx']),
                    'video_id': r['clip_uid']}] for i, r in enumerate(rows)]
        keep, sub_path = Keep(), os.path.join(tmp, "sub.json")
        quiet(TU.valid_one_epoch_nlq_singlegpu, loader, Model(), 0, evaluator=keep, output_file=sub_path, print_freq=10 ** 9)
        out['sub_records'] = np.array(json.dumps(keep.results))
        with open(sub_path) as f:
            out['sub_json'] = np.array(f.read())
        # timing of the reference evaluator: 5 000 queries x 5 rows in 13 segments
        big, bseg = [], []
        for q in range(5000):
            c, a, i = int(rng.integers(1, 60)), int(rng.integers(0, 2)), int(rng.integers(0, 3))
            big.append(rec(c, a, i, near_rows(rng, gt, c, a, i, 5)))
            bseg.append(q * 13 // 5000)
        t0 = time.perf_counter()
        quiet(ego.evaluate, big, verbose=True)
        t1 = time.perf_counter()
        for k in range(13):
            quiet(ego.evaluate, [r for r, s in zip(big, bseg) if s <= k], verbose=True)
        t2 = time.perf_counter()
        out['ref_seconds_once'], out['ref_seconds_prefixes'] = np.array(t1 - t0), np.array(t2 - t1)
        print("reference evaluator, 5000 x 5: once %.3f s, 13 prefixes %.3f s" % (t1 - t0, t2 - t1))
    path = os.path.join(HERE, "nlq_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
