"""RWalk update timing: the AdamW update over a chunk table with config P's parameter census -- the gradient-bearing
tensors of the benchmark model after one step -- in four forms in the same process: vilco_optim_step plain (7 fp32 streams per
element: p, m, v read and written, g read), with SI's omega table (9), vilco_optim_step_rwalk on a plain iteration (11: omega and
fisher read and written) and on a checkpoint iteration (15: score and theta_ck read and written as well; 14 if omega's
store of zero is not counted); and
vilco_rwalk_consolidate (flush 5 reads + 2 writes, apply 3 reads + 4 writes: 14).

The forms are alternated, device events around each C call (tables built once: no host -> device copy in the timed window), warmed
up, median of `reps`.  Every regularised tensor is tracked (no address-0 entry), the worst case.  Prints one JSON line with the times,
the ratios to the plain update and the stream ratios they are to be compared with."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vilco_amd import _lib, ops  # noqa: E402
from agem_bench import census  # noqa: E402

STREAMS = {'plain': 7, 'si': 9, 'rwalk_plain': 11, 'rwalk_checkpoint': 15, 'consolidate': 14}


def main(reps=50):
    dev = torch.device('cuda', 0)
    numels = census(dev)
    n = sum(numels)
    gen = torch.Generator(device=dev).manual_seed(0)

    def rows(scale=1.0, positive=False):
        out = [torch.randn(k, device=dev, generator=gen) * scale for k in numels]
        return [t.abs_() for t in out] if positive else out
    p, g, m, v = rows(0.02), rows(1e-3), rows(1e-3), rows(1e-6, True)
    om, fi, sc, ck = rows(1e-6), rows(1e-6, True), rows(1.0, True), rows(0.02)
    imp, opt = rows(), rows()
    plan = ops.ChunkPlan(numels, dev)

    def addrs(*lists):
        return torch.tensor([[t.data_ptr() for t in lst] for lst in lists], dtype=torch.int64).to(dev)
    ptrs, si, rw = addrs(p, g, m, v), addrs(om)[0].contiguous(), addrs(fi, sc, ck)
    cons_ptrs, out_ptrs = addrs(p, fi, sc, om, ck), addrs(imp, opt)
    group = torch.zeros(len(numels), dtype=torch.int32, device=dev)
    tstep = torch.full((len(numels),), 10.0, device=dev)
    amax = torch.empty(max(plan.nchunks, 1), device=dev)
    coef = torch.tensor([2.0, 0.5], device=dev)
    tick = torch.zeros(1, dtype=torch.int32, device=dev)
    partial = torch.empty(2 * max(plan.nchunks, 1), device=dev)
    maxes = torch.empty(2, device=dev)
    lr, wd = (C.c_float * 1)(1e-4), (C.c_float * 1)(0.05)
    lib, stream = _lib.load(), ops._stream()

    def desc(with_si):
        return _lib.OptimDesc(table=plan.table(ptrs, 4), kind=0, group=group.data_ptr(), lr=C.addressof(lr), wd=C.addressof(wd),
                              ngroups=1, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.9, tensor_step=tstep.data_ptr(),
                              norm_coef=coef.data_ptr(), chunk_amax=amax.data_ptr(), lr_dev=None,
                              si_ptrs=si.data_ptr() if with_si else None)
    d_plain, d_si = desc(False), desc(True)
    d_rw = _lib.RwalkStepDesc(optim=desc(True), rw_ptrs=rw.data_ptr(), tick=tick.data_ptr(), alpha=0.9, eps=1e-8, delta_t=10)
    d_cons = _lib.RwalkDesc(table=plan.table(cons_ptrs, 5), out_ptrs=out_ptrs.data_ptr(), partial=partial.data_ptr(),
                            out=maxes.data_ptr(), eps=1e-8)

    def rwalk(t):
        tick.fill_(t)          # (outside the timed window)
        return lambda: _lib.check(lib.vilco_optim_step_rwalk(C.byref(d_rw), stream))
    forms = {'plain': lambda: _lib.check(lib.vilco_optim_step(C.byref(d_plain), stream)),
             'si': lambda: _lib.check(lib.vilco_optim_step(C.byref(d_si), stream)),
             'rwalk_plain': None, 'rwalk_checkpoint': None,
             'consolidate': lambda: _lib.check(lib.vilco_rwalk_consolidate(C.byref(d_cons), stream))}

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b)

    ts = {k: [] for k in forms}
    for it in range(3 + reps):
        for k in forms:
            fn = rwalk(7) if k == 'rwalk_plain' else rwalk(10) if k == 'rwalk_checkpoint' else forms[k]
            t = once(fn)
            if it >= 3:
                ts[k].append(t)
    assert bool(torch.isfinite(maxes).all())
    res = {"tensors": len(numels), "elements": n, "chunks": plan.nchunks, "reps": reps}
    med = {}
    for k, v_ in ts.items():
        v_.sort()
        med[k] = v_[len(v_) // 2]
        res[k + "_us_median_min_max"] = (round(med[k], 1), round(v_[0], 1), round(v_[-1], 1))
    res["gbps_incl_launches"] = {k: round(4 * STREAMS[k] * n / med[k] / 1e3, 1) for k in med}
    res["ratio_to_plain"] = {k: round(med[k] / med['plain'], 3) for k in med}
    res["stream_ratio_to_plain"] = {k: round(STREAMS[k] / STREAMS['plain'], 3) for k in med}
    res["ratio_over_stream_ratio"] = {k: round(med[k] / med['plain'] / (STREAMS[k] / STREAMS['plain']), 3) for k in med}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
