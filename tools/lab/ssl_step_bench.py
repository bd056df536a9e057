"""ms per training step of the ViLCo recipe's model (config P as bench.py builds it, narration_ssl on, memory_size 1010, narration
tokens 512-d as mq_vilco.yaml) three ways, alternated inside one process:

  unfused   eager, VILCO_FUSED_SSL=0's code: the tensor-expression SSL branch with its host reads (the step before csrc/ssl.hip)
  fused     eager, ops.ssl_pool / ops.ssl_nce
  replayed  GraphedStep over the fused path (forward + backward graph; no optimizer, as bench.py's step)

Every mode is warmed up, then timed in `--rounds` alternating windows of `--steps` steps each with a host clock around work that
ends in a device synchronise; one JSON line: per mode the median window and the min / max over windows (the spread).
With --launches N the script instead runs N steps of ONE mode (--mode) and nothing else, for a kernel-trace run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/lab/ssl_step_bench.py --mode fused --launches 3
(the SSL branch's kernels carry `ssl_` in their names; the unfused branch's are ATen's).  Two such runs with different N give the
launches per step as a difference.  --nce times ops.ssl_nce alone (forward, then forward + backward; device events over 200 calls)
at the recipe's sizes, B = --batch, D = 1024, M = 1010: what the fp64 logits loop and the saved [2B, M] fp64 logits cost."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def build(dev, fused):
    import vilco_amd.modeling as vm
    from vilco_amd.core.config import make_config
    over = dict(dataset=dict(input_dim=2304, num_classes=22, max_seq_len=2304),
                model=dict(embd_dim=1024, fpn_dim=1024, head_dim=1024, n_head=16, backbone_arch=(2, 2, 5), use_abs_pe=True,
                           use_cross_modal=True, n_txt_in=768, max_buffer_len_factor=1.0, use_xl=True),
                train_cfg=dict(init_loss_norm=100, dropout=0.1, droppath=0.1),
                cl_cfg=dict(narration_ssl=True, ssl_factor=0.03, memory_size=1010, narration_dim=512))
    torch.manual_seed(0)
    model = vm.make_meta_arch('LocPointTransformer', **dict(make_config(**over)['model'], xlnet_config=bench.P_XLNET))
    model = model.to(dev).train()
    model.fused_ssl = fused
    return model


def batches(dev, B, n=4):
    out = []
    for s in range(n):
        g = torch.Generator().manual_seed(500 + s)
        out.append([dict(x, narration_feats=torch.randn(512, 12 + (3 * s + i) % 9, generator=g).to(dev),
                         narration_mask=float((s + i) % 3 != 0)) for i, x in enumerate(bench.synth_batch(B, dev, seed=s))])
    return out


def nce_only(dev, B, D=1024, M=1010, n=200):
    from vilco_amd import ops
    g = torch.Generator().manual_seed(1)
    text = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    video = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    bank = torch.randn(M, D, generator=g).to(dev)
    ring = torch.zeros(1, dtype=torch.int32, device=dev)
    mask = torch.ones(B, device=dev)
    out = {"B": B, "D": D, "M": M, "calls": n}
    for name, bwd in (("fwd_us", False), ("fwd_bwd_us", True)):
        ts = []
        for rnd in range(4):                     # the first round warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                loss = ops.ssl_nce(text, video, mask, bank, ring)[0]
                if bwd:
                    text.grad = video.grad = None
                    loss.backward()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                ts.append(e0.elapsed_time(e1) * 1e3 / n)
        out[name] = [round(t, 2) for t in sorted(ts)]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mode", default="all", choices=["all", "unfused", "fused", "replayed"])
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--nce", action="store_true")
    args = ap.parse_args()
    from vilco_amd import ops
    from vilco_amd.graph import GraphedStep
    dev = torch.device("cuda", 0)
    ops.set_precision("f16x2")
    if args.nce:
        return nce_only(dev, args.batch)
    data = batches(dev, args.batch)
    modes = {}
    for name in (("unfused", "fused", "replayed") if args.mode == "all" else (args.mode,)):
        model = build(dev, name != "unfused")
        gs = GraphedStep(model, None, eager_steps=2, enabled=(name == "replayed"))
        modes[name] = (model, gs)

    def run(name, n, k0=0):
        _, gs = modes[name]
        for k in range(n):
            gs(data[(k0 + k) % len(data)])

    if args.launches:
        run(args.mode, 4)
        torch.cuda.synchronize()
        run(args.mode, args.launches)
        torch.cuda.synchronize()
        return
    for name in modes:
        run(name, args.warmup)
    torch.cuda.synchronize()
    times = {name: [] for name in modes}
    for r in range(args.rounds):
        for name in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.steps, r)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    out = {"batch": args.batch, "steps": args.steps, "rounds": args.rounds}
    for name, ts in times.items():
        ts = sorted(ts)
        out[name] = {"ms_median": round(ts[len(ts) // 2], 3), "ms_min": round(ts[0], 3), "ms_max": round(ts[-1], 3),
                     "stats": dict(modes[name][1].stats)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
