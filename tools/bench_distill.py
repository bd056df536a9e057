"""Step time of an iCaRL training step WITH its distillation term (n_known > 0): config P, B = 2, cl_name 'icarl', n_known =
half of the classes, device-resident targets -- the step every task of a continual-learning run but the first takes, which
bench.py (n_known == 0) does not measure.

The step is bench.py's (zero grads, forward, backward of final_loss), run eagerly and, where the library can capture it, replayed
through vilco_amd.graph.GraphedStep.  Timing: HIP events around blocks of --steps steps after a warm-up, --repeats blocks per
mode with the two modes alternating; reported per mode: the median block (ms per step), min, max and spread = max - min.

  python tools/bench_distill.py [--root TREE] [--label NAME] [--out FILE]

--root: the source tree to measure (default: the one this file is in) -- the same script measures an older checkout, whose
library must have been built; on a tree that cannot capture the step only the eager number exists ("replayed": null).
One JSON line on stdout; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch
    assert torch.cuda.is_available(), "bench_distill.py measures on the GPU: there is no CPU fallback"
    import bench
    import vilco_amd
    import vilco_amd.modeling as vm
    from vilco_amd import ops
    from vilco_amd.graph import GraphedStep
    assert os.path.abspath(vilco_amd.__file__).startswith(os.path.abspath(args.root)), vilco_amd.__file__
    vilco_amd._lib.load()
    ops.set_precision("f16x2")
    dev = torch.device("cuda", 0)
    cfg = bench.p_config()
    torch.manual_seed(0)
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg, xlnet_config=bench.P_XLNET)).to(dev).train()
    model.cl_name, model.n_known = 'icarl', cfg['num_classes'] // 2
    torch.manual_seed(1000)
    batch = bench.synth_batch(2, dev)
    level_T = [model.max_seq_len // s for s in model.fpn_strides]
    g = torch.Generator().manual_seed(11)
    # every clip's cached outputs: the levels are views of one buffer, the form train_cl.cache_prev_logits hands out
    prev = [list(torch.rand(sum(level_T), cfg['num_classes'], generator=g).to(dev).split(level_T)) for _ in batch]
    params = list(model.parameters())

    def eager():
        for p in params:
            p.grad = None
        losses = model(batch, is_training=True, prev_out_cls_logits=prev)
        losses['final_loss'].backward()
        return losses['dist_loss'].detach()

    graphed = GraphedStep(model, None, eager_steps=2)

    def replayed():
        return graphed(batch, prev_out_cls_logits=prev)['dist_loss']

    for _ in range(4):
        replayed()
    torch.cuda.synchronize()
    modes = {"eager": eager}
    if graphed.stats['replayed'] > 0:
        modes["replayed"] = replayed
    for fn in modes.values():
        for _ in range(args.warmup):
            last = fn()
        torch.cuda.synchronize()
    assert torch.isfinite(last).item() and float(last) > 0.0

    times = {k: [] for k in modes}
    for _ in range(args.repeats):
        for name, fn in modes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)

    def summary(v):
        return None if not v else {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                                   "max_ms": round(max(v), 4), "spread_ms": round(max(v) - min(v), 4),
                                   "blocks_ms": [round(x, 4) for x in v]}
    out = {"label": args.label, "config": "P", "batch": 2, "cl_name": "icarl", "n_known": int(model.n_known),
           "num_classes": int(cfg['num_classes']), "levels": level_T, "steps_per_block": args.steps, "blocks": args.repeats,
           "step": "zero grads + forward + backward, targets resident on the device", "timer": "HIP events per block",
           "eager": summary(times["eager"]), "replayed": summary(times.get("replayed")),
           "graph_stats": dict(graphed.stats), "dist_loss": float(last), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
