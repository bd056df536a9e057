"""Golden vectors of the NLQ ENSEMBLE from the IMPORTED REFERENCE (build machine only).
Run:  python tests/golden/make_golden_nlq_ensemble.py   ->  tests/golden/nlq_ensemble.npz   (data only)

The reference's own `top1_generator`, `post_processing_mr_nms` (NLQ/ensemble.py) and `temporal_nms` (NLQ/temporal_nms.py) are
imported and run per query inside a line-for-line restatement of the twelve-line loop of the reference's `__main__`
(NLQ/ensemble.py:123-143), generalised from three models to M.  With the reference's constants the loop ends in
`post_processing_mr_nms` itself; its [start, end] rows are recorded ('<case>__mr') and must equal the rows of the route below.
For every case, the reference's constants included, the scores and the number of rows kept before padding come from
`temporal_nms` called directly on the same fusion list, padded as `post_processing_mr_nms` pads.  `top1_generator` has its
distance of 2 in its body: a case with distance d (a power of two) calls it on rows whose starts and ends are scaled by
2 / d, which is exact, and scales the proposals back.

Per case '<name>': '__pred' [M, n, k_cap, 3] (rows past '__cnt' [M, n] are zero), '__params' (max_input, top1_max_input,
distance, nms_thd, max_after_nms, pad), '__out' [n, max_after_nms, 3] (start, end, score; zero rows past the kept ones
without padding), '__out_cnt' [n], '__prop' [n, M * top1_max_input, 4] (start, end, score, total) with '__prop_cnt' [n],
'__gt' [n, 2] (a ground-truth window per query, for the evaluator).  'cases': the names; 'fp32_cases': those whose values are
all fp32-representable.  'tnms_*' / 'top1_*': single lists through `temporal_nms` (max_after_nms = 100) and
`top1_generator`.  'ref_seconds': the reference loop on 5 000 queries x 3 models on this host."""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/NLQ")

import ensemble as ref_ens                    # noqa: E402  (the reference's modules)
import temporal_nms as ref_nms                # noqa: E402
import nlq_ensemble_restatement as R          # noqa: E402

F32 = lambda x: float(np.float32(x))          # noqa: E731


def reference_query(items, max_input=4, top1_max_input=1, distance=2, nms_thd=0.5, max_after_nms=5, pad=True):
    """the loop body of NLQ/ensemble.py:123-143 for one query; items = the M records.  Returns (rows [start, end, score],
    kept, proposals, the rows of post_processing_mr_nms or None)"""
    default = (nms_thd, max_after_nms, pad, distance) == (0.5, 5, True, 2)
    top1_generator_output = []
    if top1_max_input > 0:
        top1_generator_list = []
        for item in items:
            top1_generator_list.extend(item["predicted_times"][:top1_max_input])
        k = 2 / distance
        scaled = [[r[0] * k, r[1] * k, r[2]] for r in top1_generator_list]
        assert all(a[0] / k == b[0] and a[1] / k == b[1] for a, b in zip(scaled, top1_generator_list))
        top1_generator_output = [[p[0] / k, p[1] / k] + p[2:] for p in ref_ens.top1_generator(scaled)]
    fusion_output = items[0].copy()
    fusion_output["predicted_times"] = fusion_output["predicted_times"][:max_input]
    for item in items[1:]:
        fusion_output["predicted_times"].extend(item["predicted_times"][:max_input])
    fusion_output["predicted_times"].extend(top1_generator_output)
    fusion = fusion_output["predicted_times"]
    mr = None
    if default:
        with contextlib.redirect_stdout(io.StringIO()):
            mr = ref_ens.post_processing_mr_nms(fusion, idx=2)
    moments = [[item[0], item[1], item[2]] for item in fusion]
    moments = sorted(moments, key=lambda x: x[2], reverse=True)
    after = ref_nms.temporal_nms(moments, nms_thd=nms_thd, max_after_nms=max_after_nms)
    kept = len(after)
    if pad and kept < max_after_nms:
        after = after + [after[-1]] * (max_after_nms - kept)
    if mr is not None:
        assert mr == [[r[0], r[1]] for r in after]
    return after, kept, top1_generator_output, mr


CASES, OUT = [], {}


def add_case(name, queries, fp32=True, gt=None, **params):
    """queries: [query][model] -> rows"""
    p = dict(R.DEFAULTS, **params)
    n, n_model = len(queries), len(queries[0])
    if fp32:
        queries = [[[[F32(x) for x in r] for r in rows] for rows in models] for models in queries]
    k_cap = max(max(len(rows) for models in queries for rows in models), p["max_input"])
    pred = np.zeros((n_model, n, k_cap, 3))
    cnt = np.zeros((n_model, n), dtype=np.int32)
    out = np.zeros((n, p["max_after_nms"], 3))
    out_cnt = np.zeros(n, dtype=np.int32)
    prop = np.zeros((n, max(n_model * p["top1_max_input"], 1), 4))
    prop_cnt = np.zeros(n, dtype=np.int32)
    mrs = []
    for q, models in enumerate(queries):
        for m, rows in enumerate(models):
            assert len(rows) >= 1
            pred[m, q, :len(rows)] = rows
            cnt[m, q] = len(rows)
        items = [{"query_idx": 0, "predicted_times": [list(r) for r in rows]} for rows in models]
        after, kept, props, mr = reference_query(items, **p)
        out[q, :len(after)] = after
        out_cnt[q] = kept
        prop_cnt[q] = len(props)
        for i, pr in enumerate(props):
            assert pr[3] == 0
            prop[q, i] = [pr[0], pr[1], pr[2], pr[4]]
        mrs.append(mr)
    if fp32:
        assert np.array_equal(pred.astype(np.float32).astype(np.float64), pred)
    OUT.update({name + "__pred": pred, name + "__cnt": cnt, name + "__out": out, name + "__out_cnt": out_cnt,
                name + "__prop": prop, name + "__prop_cnt": prop_cnt,
                name + "__params": np.array([float(p[k]) for k in R.PARAM_ORDER]),
                name + "__gt": np.zeros((n, 2)) if gt is None else np.asarray(gt, dtype=np.float64)})
    if mrs[0] is not None:
        OUT[name + "__mr"] = np.array(mrs, dtype=np.float64)
    CASES.append((name, fp32))
    return out, out_cnt, prop, prop_cnt


def rows_of(*r):
    return [list(x) for x in r]


def far(k, score, base=1000.0):
    """rows far from everything else and from each other"""
    return [base + 10.0 * k, base + 10.0 * k + 1.0, score]


def bulk(rng, n, fp32=True):
    """three models, five rows each, starts jittered around a common base, occasional far outliers"""
    queries, gts = [], []
    for _ in range(n):
        base = rng.uniform(0, 400)
        length = rng.uniform(2, 30)
        tight = rng.uniform() < 0.08                    # the models agree closely: few survivors
        models = []
        for m in range(3):
            rows = []
            for r in range(5):
                sd = (0.4 if tight else 3.0) * (1 + (0 if tight else r))
                s = base + rng.normal(0, sd)
                ln = length * (rng.uniform(0.9, 1.1) if tight else rng.uniform(0.5, 1.5))
                if rng.uniform() < 0.08:
                    s = rng.uniform(0, 400)              # a far outlier
                rows.append([round(s, 3), round(s + ln, 3), rng.uniform(0.05, 1.0)])
            rows.sort(key=lambda x: -x[2])
            models.append(rows)
        queries.append(models)
        gts.append([round(base, 3), round(base + length, 3)])
    return queries, gts


def main():
    up = float(np.nextafter(np.float32(3), np.float32(4)))      # just above 3 in fp32
    up53 = float(np.nextafter(np.float32(53), np.float32(54)))
    under4 = float(np.nextafter(np.float32(4), np.float32(0)))  # just under 4 in fp32

    # ---- M = 1: the proposal duplicates the top-1 row and the span overlap of 1 suppresses it; 1..4 survivors are padded
    o, k, p, pc = add_case("m1", [
        [rows_of([0, 4, .9], [10, 12, .8], [20, 25, .7], [30, 31, .6])],          # 4 survivors
        [rows_of([5, 6, .5])],                                                    # exactly one row: 1 survivor
        [rows_of([0, 4, .9], [0.5, 4, .8], [20, 25, .7])],                        # 2 survivors
        [rows_of([0, 4, .9], [10, 12, .8], [20, 25, .7], [10, 12.5, .6])],        # 3 survivors
    ])
    assert k.tolist() == [4, 1, 2, 3] and pc.tolist() == [1, 1, 1, 1]
    assert p[0, 0].tolist() == [0, 4, F32(.9), F32(.9)] and (o[0, 4] == o[0, 3]).all() and (o[1] == o[1, 0]).all()

    # ---- M = 2: an even cluster, the middle by strict comparison, a tie; a model with one row
    o, k, p, pc = add_case("m2", [
        [rows_of([0, 4, .9], far(0, .3)), rows_of([1, 4, .6], far(1, .2))],       # middle = max = A
        [rows_of([0, 4, .6], far(0, .3)), rows_of([1, 4, .9], far(1, .2))],       # the upper middle is greater: B
        [rows_of([0, 4, .75], far(0, .3)), rows_of([1, 4, .75])],                 # a tie: the lower middle, A
        [rows_of([0, 4, .75]), rows_of([100, 104, .75], far(1, .2), far(2, .1), far(3, .05), far(4, .01))],
    ])
    assert p[0, 0, :2].tolist() == [0, 4] and p[1, 0, :2].tolist() == [1, 4] and p[2, 0, :2].tolist() == [0, 4]
    assert pc.tolist() == [1, 1, 1, 2] and p[3, 0, 3] == p[3, 1, 3] and p[3, 0, 0] == 0       # equal totals: centre order

    # ---- M = 3: the centre rules, ties and overlaps under the reference's constants
    tie_models = [rows_of([0, 2, .75], [100, 101, .5]), rows_of([1.5, 3.5, .25], [200, 201, .5]),
                  rows_of([3, 5, .5], [300, 301, .125])]
    o, k, p, pc = add_case("m3", [
        [rows_of([0, 4, .9]), rows_of([1, 3, .8]), rows_of([-1, 5, .7])],                      # 0 all centres equal
        [rows_of([0, 2, .9], far(0, .1)), rows_of([2, 4, .8]), rows_of([9, 11, .7])],          # 1 a gap of exactly 2.0
        [rows_of([0, 2, .9], far(0, .1)), rows_of([2, under4, .8]), rows_of([9, 11, .7])],     # 2 a gap just under 2.0
        [rows_of([-1, 1, .5]), rows_of([0.5, 2.5, .9]), rows_of([2, 4, .7])],                  # 3 the chain 0 / 1.5 / 3.0
        [rows_of([0, 2, .5]), rows_of([10, 12, .5]), rows_of([20, 22, .75])],                  # 4 equal cluster totals
        tie_models,                                                                            # 5 ties: models, then proposals
        [rows_of([0, 1, .5], [10, 11, .5]), rows_of([20, 21, .5], [30, 31, .5]),
         rows_of([40, 41, .5], [50, 51, .5])],                                                 # 6 ties: model, then row order
        [rows_of([0, 4, .9], [1, 3, .85]), rows_of([50, 54, .8], [51, up53, .75]),
         rows_of([-9, -5, .7], [-8, -6, .65])],                                                # 7 overlap 0.5 / just above
        [rows_of([2, 2, .9], [2, 2, .8]), rows_of([7, 7, .7]), rows_of([7, 7, .6], [30, 40, .5])],   # 8 zero-length rows
        [rows_of([0, 10, .9], [20, 30, .5], [40, 50, .4], [60, 70, .3], [80, 90, .95]),
         rows_of([100, 110, .8], [120, 130, .2]), rows_of([140, 150, .7], [160, 170, .1])],    # 9 more than 5; row 5 unread
        [rows_of([0, 10, .9], [20, 30, .5]), rows_of([0.5, 10, .8], [40, 50, .2]), rows_of([0, 10.5, .7], [60, 70, .3], [80, 90, .1])],   # 10 exactly 5
    ])
    assert pc[0] == 1 and p[0, 0].tolist() == [-1, 5, F32(.7), F32(.7)]                        # the last model wins
    assert pc[1] == 3 and pc[2] == 2 and pc[3] == 1 and p[3, 0, :2].tolist() == [0.5, 2.5]
    assert pc[4] == 3 and p[4, :, 0].tolist() == [20, 0, 10]
    assert o[5, :, :2].tolist() == [[0, 2], [100, 101], [200, 201], [3, 5], [0.75, 2.75]] and k[5] == 5
    assert (o[5, 1:, 2] == 0.5).all()
    assert o[6, :, 0].tolist() == [0, 10, 20, 30, 40]
    assert [0.0, 4.0] in o[7, :, :2].tolist() and [1.0, 3.0] in o[7, :, :2].tolist()          # exactly 0.5: both kept
    assert [50.0, 54.0] in o[7, :, :2].tolist() and [51.0, up53] not in o[7, :, :2].tolist()    # just above: dropped
    assert [-8.0, -6.0] in o[7, :, :2].tolist() and k[7] == 5                                 # negative starts, nested
    assert o[8, :, :2].tolist() == [[2, 2], [2, 2], [2, 2], [7, 7], [7, 7]]                 # span 0: the duplicates stay
    assert k[9] == 5 and o[9, :, 0].tolist() == [0, 100, 140, 20, 40]                         # the 5th row of model 0 is cut
    assert k[10] == 5 and k.min() <= 2

    # ---- top1_max_input = 2: a cluster of four whose middle is not its maximum; a model with fewer rows than that
    o, k, p, pc = add_case("top2", [
        [rows_of([0, 2, .9], [1, 3, .2]), rows_of([2, 4, .6], [3, 5, .3])],       # centres 1 2 3 4: max row 0, middle row 2
        [rows_of([0, 2, .9]), rows_of([1, 4, .6], [30, 50, .3])],
    ], top1_max_input=2)
    assert pc.tolist() == [1, 2] and p[0, 0, :2].tolist() == [1, 3] and p[0, 0, 3] == sum([F32(.9), F32(.2), F32(.6), F32(.3)])

    # ---- top1_max_input = 0: no generator; M = 1 is a plain temporal_nms.  Other thresholds, no padding.
    nms_rows = rows_of([0, 4, .9], [1, 3, .8], [1, up, .75], [2, 2, .7], [2, 2, .6], [-5, -1, .5], [-4.5, -1, .4],
                       [100, 200, .3], [120, 130, .2], [300, 301, .1])
    o, k, p, pc = add_case("nms_only", [[nms_rows], [nms_rows[:1]], [nms_rows[:3]]], top1_max_input=0, max_input=10,
                           max_after_nms=9)
    assert pc.tolist() == [0, 0, 0] and k.tolist() == [8, 1, 2]
    o, k, p, pc = add_case("nms_thd03", [[nms_rows], [nms_rows[5:]]], top1_max_input=0, max_input=10, nms_thd=0.3,
                           max_after_nms=8, pad=False)
    assert k.tolist() == [7, 4] and (o[0, 7:] == 0).all()
    o, k, p, pc = add_case("nopad", [tie_models, [rows_of([0, 4, .9]), rows_of([0, 4, .8]), rows_of([0, 4.5, .7])]], pad=False)
    assert k.tolist() == [5, 1] and (o[1, 1:] == 0).all()
    o, k, p, pc = add_case("thd07_m3", [[rows_of([0, 4, .9], [1, 4, .5]), rows_of([0, 6, .8]), rows_of([20, 25, .7])]],
                           nms_thd=0.7, max_after_nms=3)
    assert k[0] == 3

    # ---- another distance: 4 joins what 2 splits, 1 splits what 2 joins
    dq = [[rows_of([0, 2, .9]), rows_of([2, 4, .8]), rows_of([5.5, 6.5, .7])],
          [rows_of([0, 2, .9]), rows_of([1, 3, .8]), rows_of([1.5, 3, .7])]]
    _, _, _, pc4 = add_case("dist4", dq, distance=4)
    _, _, _, pc1 = add_case("dist1", dq, distance=1)
    _, _, _, pc2 = add_case("dist2", dq)
    assert pc4.tolist() == [1, 1] and pc2.tolist() == [3, 1] and pc1.tolist() == [3, 2]

    # ---- M = 8, max_input = 10: 80 rows and 8 proposals, more than one candidate per lane; one query
    rng = np.random.default_rng(8)
    big = []
    for m in range(8):
        s = np.round(rng.uniform(0, 300, 10), 2) + 400.0 * m
        s[0] = 400.0 * m + 50.0
        rows = [[float(a), float(a + b), float(c)] for a, b, c in zip(s, np.round(rng.uniform(1, 40, 10), 2),
                                                                       np.sort(rng.uniform(0.05, 1, 10))[::-1])]
        big.append(rows)
    o, k, p, pc = add_case("m8", [big], max_input=10)
    assert pc[0] == 8 and OUT["m8__cnt"].sum() + pc[0] == 88
    shared = [[[r[0] % 400.0, r[0] % 400.0 + r[1] - r[0], r[2]] for r in rows] for rows in big]   # the models overlap
    o, k, p, pc = add_case("m8_nms", [shared, big], max_input=10, top1_max_input=2, max_after_nms=100, pad=False, nms_thd=0.2)
    assert 5 < k[0] < 60 and pc.max() >= 8

    # ---- 300 seeded queries
    queries, gts = bulk(np.random.default_rng(2024), 300)
    o, k, p, pc = add_case("bulk", queries, gt=gts)
    kinds = {"one": int((pc == 1).sum()), "two": int((pc == 2).sum()), "three": int((pc == 3).sum()),
             "padded": int((k < 5).sum())}
    print("bulk:", kinds, "of", len(queries))
    assert min(kinds.values()) >= 20
    queries, gts = bulk(np.random.default_rng(257), 257)
    add_case("tail257", queries, gt=gts)
    queries, gts = bulk(np.random.default_rng(64), 40)
    queries = [[[[x + 1e-9 * (i + 1) / 3 for i, x in enumerate(r)] for r in rows] for rows in models] for models in queries]
    add_case("fp64", queries, fp32=False, gt=gts)
    assert not np.array_equal(OUT["fp64__pred"].astype(np.float32).astype(np.float64), OUT["fp64__pred"])

    # ---- single lists through temporal_nms (max_after_nms = 100, the default) and top1_generator
    rng = np.random.default_rng(100)
    s = np.round(rng.uniform(0, 200, 60), 2)
    lst = [[F32(a), F32(a + b), F32(c)] for a, b, c in zip(s, np.round(rng.uniform(1, 30, 60), 2), rng.uniform(0, 1, 60))]
    OUT["tnms_in"] = np.array(lst)
    OUT["tnms_out"] = np.array(ref_nms.temporal_nms([list(r) for r in lst], 0.5))
    assert 5 < len(OUT["tnms_out"]) < 60
    OUT["tnms_out_thd09_max7"] = np.array(ref_nms.temporal_nms([list(r) for r in lst], 0.9, 7))
    OUT["tnms_one_in"] = np.array([[3.0, 4.0, 0.5]])
    OUT["tnms_one_out"] = np.array(ref_nms.temporal_nms([[3.0, 4.0, 0.5]], 0.5))
    gen = [[F32(a), F32(a + b), F32(c)] for a, b, c in zip(np.round(rng.uniform(0, 40, 13), 1),
                                                          np.round(rng.uniform(1, 9, 13), 1), rng.uniform(0, 1, 13))]
    OUT["top1_in"] = np.array(gen)
    OUT["top1_out"] = np.array(ref_ens.top1_generator([list(r) for r in gen]), dtype=np.float64)
    assert 2 <= len(OUT["top1_out"]) < 13 and (OUT["top1_out"][:, 3] == 0).all()

    # ---- the restatement agrees with everything recorded
    class G(dict):
        pass
    g = G(OUT)
    g["cases"] = json.dumps([c for c, _ in CASES])
    for name, _ in CASES:
        for a, b in zip(R.ensemble_case(g, name), (OUT[name + "__out"], OUT[name + "__out_cnt"], OUT[name + "__prop"],
                                                   OUT[name + "__prop_cnt"])):
            assert a.tobytes() == np.asarray(b, dtype=a.dtype).tobytes(), name

    # ---- the reference's time on the Ego4D-sized job
    queries, _ = bulk(np.random.default_rng(5), 5000)
    files = [[{"query_idx": 0, "predicted_times": models[m]} for models in queries] for m in range(3)]
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        for items in zip(*files):
            reference_query(list(items))
        ref_seconds = time.perf_counter() - t0
    print("ref_seconds (both routes per query, 5000 x 3): %.3f" % ref_seconds)
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        for first_item, second_item, third_item in zip(*files):
            lst = []
            lst.extend(first_item["predicted_times"][:1])
            lst.extend(second_item["predicted_times"][:1])
            lst.extend(third_item["predicted_times"][:1])
            gen_out = ref_ens.top1_generator(lst)
            fusion_output = first_item.copy()
            fusion_output["predicted_times"] = fusion_output["predicted_times"][:4]
            fusion_output["predicted_times"].extend(second_item["predicted_times"][:4])
            fusion_output["predicted_times"].extend(third_item["predicted_times"][:4])
            fusion_output["predicted_times"].extend(gen_out)
            fusion_output["predicted_times"] = ref_ens.post_processing_mr_nms(fusion_output["predicted_times"], idx=2)
        ref_seconds = time.perf_counter() - t0
    print("ref_seconds (the reference loop alone, 5000 x 3): %.3f" % ref_seconds)
    OUT["ref_seconds"] = np.array(ref_seconds)
    OUT["cases"] = np.array(json.dumps([c for c, _ in CASES]))
    OUT["fp32_cases"] = np.array(json.dumps([c for c, f in CASES if f]))
    path = os.path.join(HERE, "nlq_ensemble.npz")
    np.savez_compressed(path, **OUT)
    print("wrote", path, os.path.getsize(path), "bytes;", len(CASES), "cases,",
          sum(OUT[c + "__cnt"].shape[1] for c, _ in CASES), "queries")


if __name__ == "__main__":
    main()
