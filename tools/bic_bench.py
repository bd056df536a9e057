"""BiC stage 2 timing: `ops.bic_fit` on a synthetic cache of config P's shape -- 64 held-out clips of
4536 points, C = 110, the 10 newest classes, 2 clips per step, one epoch = 32 steps -- and `ops.bic_eval` over the
whole cache.  Device events around the calls, warmed up, repeated; prints one JSON line.
Algorithmic bytes of a step: rows * ((hi - lo) * 4 + 4 + 16 + 1) (the window of the logits, weight, label words, pos)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vilco_amd import ops  # noqa: E402
from vilco_amd.cl_methods.bic import BiCCache, epoch_orders  # noqa: E402


def main(n_clips=64, pts=4536, C=110, lo=100, hi=110, batch=2, reps=20):
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    N = n_clips * pts
    logits = (3 * torch.randn(N, C, generator=g)).to(dev)
    on = torch.rand(N, C, generator=g) < 0.05
    weight = torch.rand(N, generator=g)
    weight[torch.rand(N, generator=g) < 0.2] = 0
    pos = (on.any(-1) & (weight > 0)).to(torch.uint8).to(dev)
    bits = BiCCache.pack_bits(on.float()).to(dev)
    weight = weight.to(dev)
    ptr = (torch.arange(n_clips + 1) * pts).to(torch.int32).to(dev)
    order = torch.tensor(epoch_orders(n_clips, 1, batch), dtype=torch.int32, device=dev)
    n_steps = order.numel() // batch

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    ab = torch.tensor([1.0, 0.0], device=dev)
    fit = timed(lambda: ops.bic_fit(logits, bits, weight, pos, ptr, order, batch, lo, hi, 0.1, 0.001, ab.clone()))
    ev = timed(lambda: ops.bic_eval(logits, bits, weight, pos, ptr, lo, hi, 0.1, ab))
    step_bytes = batch * pts * ((hi - lo) * 4 + 4 + 16 + 1)
    print(json.dumps({"shape": dict(n_clips=n_clips, pts=pts, C=C, lo=lo, hi=hi, batch=batch, n_steps=n_steps),
                      "fit_ms_median_min_max": fit, "fit_us_per_step": 1e3 * fit[0] / n_steps,
                      "eval_ms_median_min_max": ev, "step_bytes": step_bytes,
                      "fit_gbps_per_step_incl_launches": step_bytes / (1e-3 * fit[0] / n_steps) / 1e9,
                      "eval_bytes": step_bytes // batch * n_clips,
                      "eval_gbps_incl_launches": step_bytes // batch * n_clips / (1e-3 * ev[0]) / 1e9}))


if __name__ == "__main__":
    main()
