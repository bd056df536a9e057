"""A-GEM projection timing: vilco_agem_project over a chunk table with config P's parameter census -- the
gradient-bearing tensors of the benchmark model after one step (376 tensors, 210.7 M fp32 elements) -- in both branches, against
vilco_grad_norm over the same table in the same process as the yardstick (the dot launch reads twice its bytes).

The three are alternated, device events around each C call (table and pointer tensor built once: no host -> device copy in the
timed window), warmed up, median of `reps`.  The conflicting branch rewrites the gradient, so it is restored (untimed) before
every repetition.  Algorithmic bytes per element: grad_norm 4, dot 8, apply 12 (0 when it does not fire).  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vilco_amd import _lib, ops  # noqa: E402

PEAK_GBPS = 8000.0


def census(dev):
    import bench
    import vilco_amd.modeling as vm
    torch.manual_seed(0)
    model = vm.make_meta_arch('LocPointTransformer', **dict(bench.p_config(), xlnet_config=bench.p_xlnet())).to(dev).train()
    # what the optimizer's plan walks: the parameters one training step leaves a gradient in
    model(bench.synth_batch(2, dev), is_training=True)['final_loss'].backward()
    torch.cuda.synchronize()
    numels = [p.numel() for p in model.parameters() if p.grad is not None]
    del model
    torch.cuda.empty_cache()
    return numels


def main(reps=50):
    dev = torch.device('cuda', 0)
    numels = census(dev)
    n = sum(numels)
    gen = torch.Generator(device=dev).manual_seed(0)
    refs = [torch.randn(k, device=dev, generator=gen) for k in numels]
    conflict = [torch.randn(k, device=dev, generator=gen) - 0.5 * r for k, r in zip(numels, refs)]
    agree = [g + r for g, r in zip(conflict, refs)]
    work = [g.clone() for g in conflict]
    plan = ops.ChunkPlan(numels, dev)
    partial = torch.empty(2 * max(plan.nchunks, 1), device=dev)
    out, coef = torch.empty(3, device=dev), torch.empty(2, device=dev)
    lib = _lib.load()

    def table(grads):
        ptrs = torch.tensor([[g.data_ptr() for g in grads], [r.data_ptr() for r in refs]], dtype=torch.int64).to(dev)
        return ptrs, plan.table(ptrs, 2)
    p_work, t_work = table(work)
    p_agree, t_agree = table(agree)
    stream = ops._stream()

    def project(tb):
        _lib.check(lib.vilco_agem_project(C.byref(tb), partial.data_ptr(), out.data_ptr(), stream))

    def norm():      # reads row 1 of the table: the reference gradients, the same bytes as one of the dot's two streams
        _lib.check(lib.vilco_grad_norm(C.byref(t_work), 1.0, partial.data_ptr(), coef.data_ptr(), stream))

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b)

    ts = {'grad_norm': [], 'agem_agree': [], 'agem_conflict': []}
    alphas = {}
    for it in range(3 + reps):
        torch._foreach_copy_(work, conflict)
        torch.cuda.synchronize()
        t = {'grad_norm': once(norm), 'agem_conflict': once(lambda: project(t_work))}
        alphas['conflict'] = float(out[2])
        t['agem_agree'] = once(lambda: project(t_agree))
        alphas['agree'] = float(out[2])
        if it >= 3:
            for k, v in t.items():
                ts[k].append(v)
    assert alphas['conflict'] < 0 and alphas['agree'] == 0.0, alphas
    res = {"tensors": len(numels), "elements": n, "chunks": plan.nchunks, "reps": reps, "alpha": alphas}
    med = {}
    for k, v in ts.items():
        v.sort()
        med[k] = v[len(v) // 2]
        res[k + "_us_median_min_max"] = (round(v[len(v) // 2], 1), round(v[0], 1), round(v[-1], 1))
    apply_us = med['agem_conflict'] - med['agem_agree']
    res["apply_us_by_difference"] = round(apply_us, 1)
    res["gbps_incl_launches"] = {"grad_norm_4B": round(4 * n / med['grad_norm'] / 1e3, 1),
                                 "dot_finish_idle_apply_8B": round(8 * n / med['agem_agree'] / 1e3, 1),
                                 "apply_12B": round(12 * n / apply_us / 1e3, 1),
                                 "conflict_call_20B": round(20 * n / med['agem_conflict'] / 1e3, 1)}
    res["share_of_8TBps_peak"] = {k: round(v / PEAK_GBPS, 3) for k, v in res["gbps_incl_launches"].items()}
    res["agree_over_grad_norm"] = round(med['agem_agree'] / med['grad_norm'], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
