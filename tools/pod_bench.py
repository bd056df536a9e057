"""Pooled feature distillation timing: ops.pod_distill forward + backward over the pyramid of the benchmark
configuration (config P: 2 clips, fpn_dim 1024, levels 2304 .. 72) against cl_methods.pod.pod_term -- the same term in tensor
ops under autograd -- on the same device, in the same process, alternated, device events around each form, warmed up, median of
`reps`; an eager call of the op is bound by the host (three + one launches behind Python), so the op is also timed as ten
calls captured in one graph, and the bandwidth figures come from that.  Every row has a record and V = T (clip 1: T - 17 at the
first level, scaled down the pyramid): the worst case.

The op moves three passes over the features (forward reads h; backward reads h and writes d_h): 12 bytes per element; the
fraction of the HBM peak (8 TB/s) that is, launches included, is printed with the times.

--step: also the captured training step of config P with the term (cl_cfg.name 'pod', n_known > 0, a record for every clip
of the batch) next to the plain captured step of the same model class, both timed here (`steps` replays each, after warm-up).
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vilco_amd import ops  # noqa: E402
from vilco_amd.cl_methods import pod  # noqa: E402

PEAK_GBPS = 8000.0


def pyramid(dev, B=2):
    import bench
    cfg = bench.p_config()
    T0, C = cfg['max_seq_len'], cfg['fpn_dim']
    n_levels = cfg['backbone_arch'][-1] + 1
    levels = [T0 // (cfg['scale_factor'] ** l) for l in range(n_levels)]
    g = torch.Generator(device=dev).manual_seed(0)
    feats = [torch.randn(B, T, C, device=dev, generator=g) for T in levels]
    lens = [[max(1, (T0 - (17 if b % 2 else 0)) // (cfg['scale_factor'] ** l)) for l in range(n_levels)] for b in range(B)]
    level_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    recs = []
    for b in range(B):
        parts = [torch.randn(C + T, device=dev, generator=g) for T in levels]
        recs.append(torch.cat([p / p.norm() for p in parts]))
    tab = torch.tensor([r.data_ptr() for r in recs], dtype=torch.int64, device=dev)
    return feats, level_len, lens, recs, tab


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def graphed_us(fn, n=10, reps=20):
    """`n` calls of `fn` captured as one graph; median microseconds per call over `reps` replays: the kernels and the
    boundaries between them, without the host's share of an eager call"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    ts = sorted(once(g.replay) / n for _ in range(reps))
    return round(ts[len(ts) // 2], 1)


def op_times(dev, reps):
    feats, level_len, lens, recs, tab = pyramid(dev)
    xs = [f.requires_grad_(True) for f in feats]
    scale = 1.5

    def run_op():
        loss = ops.pod_distill(xs, level_len, tab, scale)
        torch.autograd.grad(loss, xs)

    def run_body():
        loss, _ = pod.pod_term(xs, lens, recs, scale)
        torch.autograd.grad(loss, xs)

    def run_fwd():
        with torch.no_grad():
            ops.pod_distill(xs, level_len, tab, scale)
    forms = {'op_fwd_bwd': run_op, 'op_fwd': run_fwd, 'tensor_ops_fwd_bwd': run_body}
    ts = {k: [] for k in forms}
    for it in range(3 + reps):
        for k, fn in forms.items():
            t = once(fn)
            if it >= 3:
                ts[k].append(t)
    elems = sum(f.numel() for f in feats)
    res = {"levels": [int(f.shape[1]) for f in feats], "B": int(feats[0].shape[0]), "C": int(feats[0].shape[2]),
           "elements": elems, "reps": reps}
    for k, v in ts.items():
        v.sort()
        res[k + "_us_median_min_max"] = (round(v[len(v) // 2], 1), round(v[0], 1), round(v[-1], 1))
    res["op_fwd_bwd_graphed_us"] = graphed_us(run_op)
    res["op_fwd_graphed_us"] = graphed_us(run_fwd)
    med = res["op_fwd_bwd_graphed_us"]
    res["bytes_three_passes"] = 12 * elems
    res["gbps_incl_launches"] = round(12 * elems / med / 1e3, 1)
    res["fraction_of_hbm_peak"] = round(12 * elems / med / 1e3 / PEAK_GBPS, 3)
    res["fwd_fraction_of_hbm_peak"] = round(4 * elems / res["op_fwd_graphed_us"] / 1e3 / PEAK_GBPS, 3)
    res["eager_speedup_over_tensor_ops"] = round(res["tensor_ops_fwd_bwd_us_median_min_max"][0] /
                                                 res["op_fwd_bwd_us_median_min_max"][0], 2)
    return res


def step_times(dev, steps, warmup):
    """config P's captured step: plain (cl_cfg.name None) and with the term; ms per replay, median"""
    import bench
    import vilco_amd.modeling as vm
    from vilco_amd.graph import GraphedStep
    batch = bench.synth_batch(2, dev)
    out = {}
    for name in (None, 'pod'):
        cfg = bench.p_config()
        cfg['cl_cfg'] = dict(cfg['cl_cfg'], name=name)
        torch.manual_seed(0)
        model = vm.make_meta_arch('LocPointTransformer', **dict(cfg, xlnet_config=bench.p_xlnet())).to(dev).train()
        if name == 'pod':
            model.n_known = 11
            model.pod_bank = pod.PODBank()
            assert pod.record_clips(model, model.pod_bank, [batch], 0) == len(batch)
        gs = GraphedStep(model, None, eager_steps=1)
        ts = []
        for it in range(2 + warmup + steps):
            t = once(lambda: gs(batch, task_id=0))
            if it >= 2 + warmup:
                ts.append(t / 1e3)
        ts.sort()
        key = 'step_with_pod_ms' if name else 'step_plain_ms'
        out[key + "_median_min_max"] = (round(ts[len(ts) // 2], 3), round(ts[0], 3), round(ts[-1], 3))
        out[key.replace('_ms', '_stats')] = dict(gs.stats)
        del gs, model
        torch.cuda.empty_cache()
    out["step_delta_ms"] = round(out["step_with_pod_ms_median_min_max"][0] - out["step_plain_ms_median_min_max"][0], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    res = op_times(dev, args.reps)
    if args.step:
        res.update(step_times(dev, args.steps, args.warmup))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
