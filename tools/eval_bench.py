"""Timing of the device MQ evaluator (csrc/evaluate.hip) on seeded inputs: ~400 000 predictions, 110 classes, 5 tIoU
thresholds, 4 000 videos.  Prints one JSON line: the device time of vilco_det_ap (HIP events, after warm-up), the host
preparation time of ANETdetection.evaluate (id / label mapping and column packing), the whole evaluate(), and the NumPy
restatement's CPU time on the same inputs for scale (--no-cpu skips it).
Run:  python tools/eval_bench.py [--preds 400000] [--no-cpu]

--nlq times the NLQ scorer instead (vilco_nlq_recall): 5 000 queries x 5 rows in 13 segments, about the Ego4D NLQ validation
set under the shipped config.  One JSON line: the device time of one launch over the whole stream, the host preparation of
record dicts (key lookup and row packing), `evaluate()` end to end for dicts and for the device-resident stream,
`evaluate_segments` (all 13 cumulative tables), the 13 prefix evaluations of the dict path, and the NumPy restatement on the
CPU for the same input.
Run:  python tools/eval_bench.py --nlq [--queries 5000] [--rows 5] [--segments 13]

--herding times the herding exemplar selection (csrc/herding.hip) for one class of --clips candidates whose descriptors have
config P's level sizes (2304 .. 72 tokens x 1024 channels): device times of vilco_frob_scale, vilco_gram and
vilco_herd_select, the level-0 Gram product alone with its fraction of the HBM peak in bytes of X read, and the same selection
done as the literal greedy loop in torch ops on the device.
Run:  python tools/eval_bench.py --herding [--clips 96] [--keep 10]

--ext-scores times the fusion of external classification scores (csrc/fuse.hip): --videos videos of --rows-per-video rows
(fp32, as the model emits them), --classes classes, num_pred 200, topk 2.  One JSON line: the device time of
vilco_score_fuse alone (HIP events), `fuse_external_scores` end to end (host grouping, upload of the un-fused rows, kernel;
ends in a synchronise), and the route without the kernel re-stated here -- the expansion in NumPy on the host followed by
the upload of the five fused columns -- with a check that both give the same bytes.
Run:  python tools/eval_bench.py --ext-scores [--videos 400] [--rows-per-video 1000] [--classes 110]

--nlq-ensemble times the NLQ ensemble (csrc/ensemble.hip): --queries queries x --models models x 5 rows (fp32, as a record
stream holds them), the reference's parameters.  One JSON line: the device time of vilco_nlq_ensemble alone (HIP events,
after warm-up, median and spread over --repeats groups of --iters launches), `ensemble_streams` end to end (pairing by key,
packing the streams' buffers, the launch; ends in a synchronise), and the fixture's `ref_seconds` (the reference's Python loop
on the same job size, recorded on the host that made tests/golden/nlq_ensemble.npz) for scale.
Run:  python tools/eval_bench.py --nlq-ensemble [--queries 5000] [--models 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preds", type=int, default=400_000)
    ap.add_argument("--classes", type=int, default=110)
    ap.add_argument("--videos", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--nlq", action="store_true")
    ap.add_argument("--queries", type=int, default=5000)
    ap.add_argument("--rows", type=int, default=5)
    ap.add_argument("--segments", type=int, default=13)
    ap.add_argument("--herding", action="store_true")
    ap.add_argument("--clips", type=int, default=96)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--ext-scores", action="store_true")
    ap.add_argument("--rows-per-video", type=int, default=1000)
    ap.add_argument("--nlq-ensemble", action="store_true")
    ap.add_argument("--models", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if a.ext_scores:
        return ext_scores(a)
    if a.nlq_ensemble:
        return nlq_ensemble(a)
    if a.nlq:
        return nlq(a)
    if a.herding:
        return herding(a)
    from vilco_amd import _lib
    from vilco_amd.utils import metrics as M
    rng = np.random.default_rng(0)
    n_gt = a.videos * 4
    db = {}
    gvid = rng.integers(0, a.videos, n_gt); gcls = rng.integers(0, a.classes, n_gt)
    gs = rng.uniform(0, 300, n_gt); ge = gs + rng.uniform(1, 30, n_gt)
    for v in range(a.videos):
        db["vid%05d" % v] = {"subset": "val", "clip_id": "vid%05d" % v, "annotations": []}
    for j in range(n_gt):
        db["vid%05d" % gvid[j]]["annotations"].append({"segment": [gs[j], ge[j]], "label_id": int(gcls[j]),
                                                        "label": str(gcls[j])})
    src = rng.integers(0, n_gt, a.preds)
    preds = {'video-id': ["vid%05d" % v for v in gvid[src]], 't-start': gs[src] + rng.normal(0, 4, a.preds),
             't-end': ge[src] + rng.normal(0, 4, a.preds), 'label': np.where(rng.uniform(size=a.preds) < 0.8, gcls[src],
                                                                             rng.integers(0, a.classes, a.preds)),
             'score': rng.uniform(size=a.preds)}
    with tempfile.NamedTemporaryFile('w', suffix='.json', delete=False) as f:
        json.dump(db, f)
    try:
        ev = M.ANETdetection(f.name, split="val", tiou_thresholds=np.linspace(0.1, 0.5, 5))
    finally:
        os.unlink(f.name)
    for _ in range(2):
        ev.evaluate(preds, verbose=False)
    t0 = time.perf_counter()
    for _ in range(3):
        ev.evaluate(preds, verbose=False)
    t_eval = (time.perf_counter() - t0) / 3
    t0 = time.perf_counter()
    gt, cols = ev.prepare(preds)
    t_host = time.perf_counter() - t0
    # device part alone: the kernels on device-resident columns, HIP events
    lib = _lib.load()
    vidx, cls, ts, te, score = cols
    d = [M._dev(vidx, torch.int32), M._dev(cls, torch.int32), M._dev(ts, torch.float64), M._dev(te, torch.float64),
         M._dev(score, torch.float64)]
    thr = np.linspace(0.1, 0.5, 5)
    out = torch.empty((5, gt.n_cls), dtype=torch.float64, device='cuda')
    nws = lib.vilco_det_ap_workspace(len(cls), gt.n_gt, 5)
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    thr_c = (C.c_double * 5)(*thr.tolist())

    def run():
        _lib.check(lib.vilco_det_ap(*[t.data_ptr() for t in d], len(cls), gt.gs.data_ptr(), gt.ge.data_ptr(),
                                    gt.grp_off.data_ptr(), gt.grp_cls.data_ptr(), gt.grp_vid.data_ptr(), gt.n_grp, gt.n_gt,
                                    gt.cls_npos.data_ptr(), gt.n_cls, gt.n_vid, thr_c, 5, out.data_ptr(), None,
                                    ws.data_ptr(), nws, M._stream()))
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    t_dev = e0.elapsed_time(e1) / a.iters / 1e3
    res = {"preds": a.preds, "classes": gt.n_cls, "videos": gt.n_vid, "thresholds": 5, "device_ms": round(t_dev * 1e3, 3),
           "host_prep_ms": round(t_host * 1e3, 1), "evaluate_ms": round(t_eval * 1e3, 1),
           "mAP": [round(float(x), 6) for x in ev.ap.mean(axis=1)]}
    if not a.no_cpu:
        import metrics_restatement as R
        gv = M._video_index(np.array(gt_vids(ev), dtype=object), gt.video_index)
        t0 = time.perf_counter()
        ap_r, _ = R.det_ap(vidx, cls, ts, te, score, gv, np.asarray(ev.ground_truth['label']), ev.ground_truth['t-start'],
                           ev.ground_truth['t-end'], gt.n_cls, thr)
        res["restatement_cpu_s"] = round(time.perf_counter() - t0, 2)
        res["max_abs_ap_diff_vs_restatement"] = float(np.abs(ap_r - ev.ap).max())
    print(json.dumps(res))


def nlq(a):
    import contextlib
    import io
    import nlq_metrics_restatement as R
    from vilco_amd.utils import make_nlq_evaluator, metrics_nlq as M
    rng = np.random.default_rng(5)
    n_clip = max(a.queries // 6, 1)
    clips = []
    for c in range(n_clip):
        qs = []
        for _ in range(6):
            s = round(float(rng.uniform(0, 400)), 3)
            qs.append({"clip_start_sec": s, "clip_end_sec": round(s + float(rng.uniform(1, 60)), 3)})
        clips.append({"clip_uid": "c%d" % c, "annotations": [{"annotation_uid": "a%d" % c, "language_queries": qs}]})
    gt = {"videos": [{"clips": clips}]}
    win = R.gt_windows(gt)
    recs, seg = [], []
    for q in range(a.queries):
        c, i = int(rng.integers(0, n_clip)), int(rng.integers(0, 6))
        s, e = win[("c%d" % c, "a%d" % c)][i]
        x = s + rng.normal(0, 0.6 * (e - s), a.rows)
        y = e + rng.normal(0, 0.6 * (e - s), a.rows)
        rows = np.stack([np.minimum(x, y), np.maximum(x, y), rng.uniform(size=a.rows)], axis=1).astype(np.float32)
        recs.append({"query_idx": i, "annotation_uid": "a%d" % c, "predicted_times": rows.tolist(), "clip_uid": "c%d" % c})
        seg.append(q * a.segments // a.queries)
    with tempfile.TemporaryDirectory() as tmp:
        ev = make_nlq_evaluator(R.write_ego4d(gt, tmp))
    st = ev.new_stream()
    for r, s in zip(recs, seg):
        t = torch.tensor(r['predicted_times'])                     # host rows, as the model's postprocessing leaves them
        st.append((r['clip_uid'], r['annotation_uid'], r['query_idx']), t[:, :2], t[:, 2], s)

    def timed(fn, reps=5):
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                out = fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, out

    def prep():
        gi = [ev._gt.index((p["clip_uid"], p["annotation_uid"], p["query_idx"])) for p in recs]
        return gi, M._pack_records([p["predicted_times"] for p in recs], 10)
    t_prep, _ = timed(prep)
    t_dict, (tab_d, _) = timed(lambda: ev.evaluate(recs, verbose=True))
    t_stream, (tab_s, _) = timed(lambda: ev.evaluate(st, verbose=True))
    t_segs, tabs = timed(lambda: ev.evaluate_segments(st, verbose=True))
    t_prefix, _ = timed(lambda: [ev.evaluate([r for r, s in zip(recs, seg) if s <= k], verbose=True) for k in range(a.segments)],
                        reps=2)
    assert tab_d.tobytes() == tab_s.tobytes() == tabs[-1][0].tobytes()
    pred, cnt, gi, sg = st.device_columns()
    gtd = ev._gt.device()[gi]
    run = lambda: M.nlq_recall_device(pred, cnt, gtd, ev.thresholds, ev.topK, 0, seg_id=sg, n_seg=a.segments)   # noqa: E731
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    res = {"queries": a.queries, "rows": a.rows, "segments": a.segments,
           "device_ms": round(e0.elapsed_time(e1) / a.iters, 4), "host_prep_dicts_ms": round(t_prep * 1e3, 2),
           "evaluate_dicts_ms": round(t_dict * 1e3, 2), "evaluate_stream_ms": round(t_stream * 1e3, 2),
           "evaluate_segments_ms": round(t_segs * 1e3, 2), "prefix_evaluations_dicts_ms": round(t_prefix * 1e3, 2),
           "R": [[round(float(x), 4) for x in row] for row in tab_s]}
    if not a.no_cpu:
        t0 = time.perf_counter()
        flags, _ = R.evaluate(recs, win)
        res["restatement_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert np.array_equal(R.recall(flags) * 100, tab_s)
    print(json.dumps(res))


HBM_PEAK = 8.0e12          # bytes / s, MI355X


def herding(a):
    from vilco_amd import ops
    dev = torch.device("cuda:0")
    N, m, C_ = a.clips, a.keep, 1024
    dims = [t * C_ for t in (2304, 1152, 576, 288, 144, 72)]
    g = torch.Generator(device=dev).manual_seed(0)
    base = [torch.randn(d, device=dev, generator=g) for d in dims]
    bufs = [b[None, :] + 0.6 * torch.randn(N, d, device=dev, generator=g) for b, d in zip(base, dims)]

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, out

    t_frob, invs = timed(lambda: [ops.frob_scale(b) for b in bufs], a.iters)
    t_gram, grams = timed(lambda: torch.stack([ops.gram(b, i, torch.float64) for b, i in zip(bufs, invs)]), a.iters)
    t_gram0, _ = timed(lambda: ops.gram(bufs[0], invs[0], torch.float64), a.iters)
    t_sel, sel = timed(lambda: ops.herd_select(grams, m), a.iters)

    def literal():
        phis = [b * i[:, None] for b, i in zip(bufs, invs)]
        mus = [p.mean(0) for p in phis]
        mus = [u / u.norm() for u in mus]
        S = [torch.zeros_like(u) for u in mus]
        taken = torch.zeros(N, dtype=torch.bool, device=dev)
        out = []
        for _ in range(min(m, N)):
            cost = torch.zeros(N, device=dev)
            for p, u, s_ in zip(phis, mus, S):
                v = p + s_[None, :]
                v = v / v.norm(dim=1, keepdim=True)
                cost = cost + (u[None, :] - v).pow(2).sum(1)
            k = torch.argmin(cost.masked_fill(taken, float("inf")))
            taken[k] = True
            S = [s_ + p[k] for s_, p in zip(S, phis)]
            out.append(k)
        return torch.stack(out)
    t_lit, sel_lit = timed(literal, 2)
    x0 = 4.0 * N * dims[0]
    print(json.dumps({"clips": N, "keep": m, "levels": len(dims), "floats_per_clip": sum(dims),
                      "frob_scale_ms": round(t_frob, 3), "gram_all_levels_ms": round(t_gram, 3),
                      "gram_level0_ms": round(t_gram0, 3), "gram_level0_bytes_x": int(x0),
                      "gram_level0_fraction_of_hbm_peak": round(x0 / (t_gram0 * 1e-3) / HBM_PEAK, 3),
                      "herd_select_ms": round(t_sel, 3), "herding_device_ms": round(t_frob + t_gram + t_sel, 3),
                      "literal_torch_loop_ms": round(t_lit, 1), "same_selection": sel.tolist() == sel_lit.tolist(),
                      "selection": sel.tolist()}))


def ext_scores(a):
    from vilco_amd import _lib
    from vilco_amd.utils import postprocessing as PP
    n_vid = a.videos if a.videos != 4000 else 400           # 4000 is the detection benchmark's default
    num_pred, topk = 200, 2
    rng = np.random.default_rng(1)
    cnt = rng.integers(max(a.rows_per_video // 2, 1), a.rows_per_video + 1, n_vid)
    n = int(cnt.sum())
    vids = np.repeat(np.array(["vid%05d" % v for v in range(n_vid)], dtype=object), cnt)
    order = rng.permutation(n)
    res = {'video-id': vids[order].tolist(), 't-start': rng.uniform(0, 300, n).astype(np.float32),
           't-end': rng.uniform(300, 400, n).astype(np.float32), 'label': np.zeros(n, np.int64),
           'score': rng.uniform(size=n).astype(np.float32)}
    cls = {"vid%05d" % v: rng.uniform(size=a.classes).tolist() for v in range(n_vid)}

    def numpy_route():
        """the expansion on the host, then the fused columns go up (what the validation loop did before the kernel)"""
        v = np.asarray(res['video-id'], dtype=object)
        uniq, inv = np.unique(v.astype(str), return_inverse=True)
        perm = np.argsort(inv, kind='stable')
        off = np.r_[0, np.cumsum(np.bincount(inv))]
        sc, ts, te = (res[k].astype(np.float64)[perm] for k in ('score', 't-start', 't-end'))
        V, L, S, E, W = [], [], [], [], []
        for i, u in enumerate(uniq):
            lo, hi = off[i], off[i + 1]
            keep = lo + np.argsort(sc[lo:hi], kind='stable')[::-1][:num_pred]
            c = np.asarray(cls[u], np.float64)
            top = np.argsort(c, kind='stable')[::-1][:topk]
            W.append(np.sqrt(c[top][:, None] * sc[keep][None, :]).reshape(-1))
            S.append(np.tile(ts[keep], topk)); E.append(np.tile(te[keep], topk))
            L.append(np.repeat(top, len(keep))); V.append(np.full(topk * len(keep), i))
        cols = [torch.as_tensor(np.concatenate(x).astype(dt)).cuda()
                for x, dt in ((V, np.int32), (L, np.int32), (S, np.float64), (E, np.float64), (W, np.float64))]
        torch.cuda.synchronize()
        return cols

    def device_route():
        f = PP.fuse_external_scores(res, cls, num_pred=num_pred, topk=topk)
        torch.cuda.synchronize()
        return f

    def timed(fn, reps):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            t.append(time.perf_counter() - t0)
        return t, out
    # alternate the two routes so that drift of the box hits both
    t_np, t_dev = [], []
    for _ in range(3):
        t, cols = timed(numpy_route, 3); t_np += t
        t, f = timed(device_route, 3); t_dev += t
    same = all(c.cpu().numpy().tobytes() == f[k].cpu().numpy().tobytes()
               for c, k in zip(cols, ('video-index', 'label', 't-start', 't-end', 'score')))
    # the kernel alone, on device-resident inputs
    lib = _lib.load()
    uniq, vidx, perm = PP._by_video(res)
    c_ = np.bincount(vidx, minlength=n_vid)
    pred_off = np.r_[0, np.cumsum(c_)].astype(np.int32)
    out_off = np.r_[0, np.cumsum(topk * np.minimum(c_, num_pred))].astype(np.int32)
    n_out = int(out_off[-1])
    d = [torch.as_tensor(res[k].astype(np.float64)[perm]).cuda() for k in ('score', 't-start', 't-end')]
    tab = torch.as_tensor(np.stack([np.asarray(cls[u], np.float64) for u in uniq])).cuda()
    o = [torch.empty(n_out, dtype=dt, device='cuda') for dt in (torch.int32, torch.int32, torch.float64, torch.float64,
                                                                 torch.float64)]
    nws = lib.vilco_score_fuse_workspace(n, n_vid)
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    i32p = C.POINTER(C.c_int32)

    def run():
        _lib.check(lib.vilco_score_fuse(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), pred_off.ctypes.data_as(i32p), n,
                                        n_vid, tab.data_ptr(), a.classes, num_pred, topk, out_off.ctypes.data_as(i32p), n_out,
                                        *[t.data_ptr() for t in o], ws.data_ptr(), nws,
                                        torch.cuda.current_stream().cuda_stream))
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = lambda t: [round(x * 1e3, 2) for x in sorted(t)]          # noqa: E731
    print(json.dumps({"videos": n_vid, "rows": n, "fused_rows": n_out, "classes": a.classes, "num_pred": num_pred, "topk": topk,
                      "device_ms": round(e0.elapsed_time(e1) / a.iters, 4), "fuse_external_scores_ms": ms(t_dev),
                      "numpy_expansion_and_upload_ms": ms(t_np), "runs_per_route": len(t_dev), "same_bytes": bool(same)}))


def nlq_ensemble(a):
    import nlq_ensemble_restatement as R
    from vilco_amd.utils import ensemble_nlq as E
    from vilco_amd.utils.metrics_nlq import NLQRecordStream
    rng = np.random.default_rng(5)
    n, M, rows = a.queries, a.models, 5
    base = rng.uniform(0, 400, (1, n, 1))
    start = base + rng.normal(0, 3.0, (M, n, rows)) * (1 + np.arange(rows))
    far = rng.uniform(size=start.shape) < 0.08
    start[far] = rng.uniform(0, 400, int(far.sum()))
    end = start + rng.uniform(2, 30, (1, n, 1)) * rng.uniform(0.5, 1.5, (M, n, rows))
    score = -np.sort(-rng.uniform(0.05, 1.0, (M, n, rows)), axis=2)
    pred = torch.as_tensor(np.stack([start, end, score], axis=3).astype(np.float32)).cuda().contiguous()
    cnt = torch.full((M, n), rows, dtype=torch.int32, device='cuda')
    run = lambda: E.nlq_ensemble_device(pred, cnt)                                   # noqa: E731
    for _ in range(5):
        out, kept = run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / a.iters)
    # the same rows as record streams, scored end to end
    streams = []
    host = pred.cpu()
    for m in range(M):
        st = NLQRecordStream(lambda key: 0, k_cap=10, capacity=n)
        for q in range(n):
            st.append(("c", "a", q), host[m, q, :, :2], host[m, q, :, 2])
        streams.append(st)
    t_e2e = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ens = E.ensemble_streams(streams)
        torch.cuda.synchronize()
        t_e2e.append(time.perf_counter() - t0)
    assert torch.equal(ens.table, out)
    # a sample against the plain-Python restatement
    hp = host.double().numpy()
    for q in range(0, n, max(n // 50, 1)):
        want, k, _ = R.ensemble_query([hp[m, q].tolist() for m in range(M)])
        assert out[q].cpu().tolist() == want and int(kept[q]) == k
    times.sort()
    print(json.dumps({"queries": n, "models": M, "rows": rows, "launches_per_group": a.iters, "groups": a.repeats,
                      "device_ms_median": round(times[len(times) // 2], 4), "device_ms_min": round(times[0], 4),
                      "device_ms_max": round(times[-1], 4),
                      "ensemble_streams_ms": [round(x * 1e3, 2) for x in sorted(t_e2e[1:])],
                      "padded_fraction": round(float((kept < 5).float().mean()), 3),
                      "fixture_ref_seconds": round(float(R.golden()["ref_seconds"]), 3)}))


def gt_vids(ev):
    return list(ev.ground_truth['video-id'])


if __name__ == "__main__":
    main()
