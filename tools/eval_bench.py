"""Timing of the device MQ evaluator (csrc/evaluate.hip) on seeded inputs: ~400 000 predictions, 110 classes, 5 tIoU
thresholds, 4 000 videos.  Prints one JSON line: the device time of vilco_det_ap (HIP events, after warm-up), the host
preparation time of ANETdetection.evaluate (id / label mapping and column packing), the whole evaluate(), and the NumPy
restatement's CPU time on the same inputs for scale (--no-cpu skips it).
Run:  python tools/eval_bench.py [--preds 400000] [--no-cpu]"""
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
    a = ap.parse_args()
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


def gt_vids(ev):
    return list(ev.ground_truth['video-id'])


if __name__ == "__main__":
    main()
