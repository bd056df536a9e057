"""Step time of a BiC stage-1 training step from the second task on: config P, B = 2, cl_name 'bic', n_known = 11 of 22
classes, eleven tasks' worth of frozen bias layers (splits 2, 4, ..., 22; alpha / beta away from 1 / 0), device-resident
softmax(. / 2) targets of one cached clip -- the step bench.py (n_known == 0) does not measure.  --cl icarl measures the iCaRL
step of tools/bench_distill.py on the same box instead, for comparison (the replayed BiC step should cost that step plus the
bias correction's two launches, csrc/bic.hip).

The step is bench.py's (zero grads, forward, backward of final_loss), run eagerly and, where the library can capture it, replayed
through vilco_amd.graph.GraphedStep.  Timing: HIP events around blocks of --steps steps after a warm-up, --repeats blocks per
mode with the two modes alternating; reported per mode: the median block (ms per step), min, max and spread = max - min.

  python tools/bench_bic_step.py [--cl bic|icarl] [--root TREE] [--label NAME] [--out FILE]

--root: the source tree to measure (default: the one this file is in) -- the same script measures an older checkout, whose
library must have been built; on a tree that cannot capture the step only the eager number exists ("replayed": null).
One JSON line on stdout; --out also writes it to a file.  profiles/bic_step.json collects the runs: two per case, the noise
stated as the spread between them."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--cl", default="bic", choices=("bic", "icarl"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch
    assert torch.cuda.is_available(), "bench_bic_step.py measures on the GPU: there is no CPU fallback"
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
    model.cl_name, model.n_known = args.cl, cfg['num_classes'] // 2
    n_cls = int(cfg['num_classes'])
    if args.cl == 'bic':
        from vilco_amd.train_cl import _bias_layer
        model.list_splits = list(range(2, n_cls + 1, 2))
        model.list_bias_layers = [_bias_layer(dev) for _ in model.list_splits]
        for i, l in enumerate(model.list_bias_layers):
            l.alpha.data.fill_(1.0 - 0.01 * i)
            l.beta.data.fill_(0.02 * i - 0.1)
        assert model.list_splits[-1] == n_cls and len(model.list_splits) == 11
    torch.manual_seed(1000)
    batch = bench.synth_batch(2, dev)
    level_T = [model.max_seq_len // s for s in model.fpn_strides]
    g = torch.Generator().manual_seed(11)
    # every clip's cached outputs: the levels are views of one buffer, the form train_cl.cache_prev_logits hands out
    if args.cl == 'bic':          # ONE clip's per-level list, as train_one_epoch hands it to a BiC step
        prev = list(torch.softmax(torch.rand(sum(level_T), model.n_known, generator=g), dim=1).to(dev).split(level_T))
    else:
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
    out = {"label": args.label, "config": "P", "batch": 2, "cl_name": args.cl, "bias_layers": len(model.list_bias_layers), "n_known": int(model.n_known),
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
