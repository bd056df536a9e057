"""Importance accumulation timing: one `ops.cl_accumulate` launch (acc += g * g) over a synthetic parameter
set with config P's tensor and element counts -- 358 tensors, 210.7 M fp32 elements: 200 matrices of 1024 x 1024 and 158
vectors of 6400 -- against the per-tensor `acc.addcmul_(g, g)` loop on the same tensors.  The two are alternated inside
one process, device events around each, warmed up; prints one JSON line.  Algorithmic bytes: 12 per element (g and acc
read, acc written)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vilco_amd import ops  # noqa: E402


def main(reps=20):
    dev = torch.device('cuda', 0)
    shapes = [(1024, 1024)] * 200 + [(6400,)] * 158
    grads = [torch.randn(s, device=dev) for s in shapes]
    accs = [torch.zeros(s, device=dev) for s in shapes]
    numel = sum(g.numel() for g in grads)

    def fused():
        ops.cl_accumulate(grads, accs, ops.CL_OP_SQUARE, 1.0, 1.0)

    def loop():
        for g, a in zip(grads, accs):
            a.addcmul_(g, g)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        fused()
        loop()
    torch.cuda.synchronize()
    ts = {'fused': [], 'loop': []}
    for _ in range(reps):
        ts['fused'].append(once(fused))
        ts['loop'].append(once(loop))
    out = {"tensors": len(shapes), "elements": numel, "bytes": 12 * numel, "reps": reps}
    for k, v in ts.items():
        v.sort()
        out[k + "_ms_median_min_max"] = (v[len(v) // 2], v[0], v[-1])
        out[k + "_gbps_incl_launches"] = 12 * numel / (1e-3 * v[len(v) // 2]) / 1e9
    out["launches"] = {"fused": 1, "loop": len(shapes)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
