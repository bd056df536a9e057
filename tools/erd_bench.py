"""Elastic Response Distillation timing: ops.erd_distill forward and forward + backward over the concatenated head
output of the benchmark configuration (config P: 2 clips, levels 2304 .. 72, the configuration's class count) on the raw-offset
route, with a record for every clip whose sets hold one position in ten (above what mean + 2 std can select: at most one in
five), next to cl_methods.erd.erd_term -- the same term in tensor ops under autograd -- on the same device, in the same process,
alternated, device events around each form, warmed up, median of `reps`.  An eager call of the op is bound by the host (two + one
launches behind Python), so the op is also timed as ten calls captured in one graph, and the bandwidth figures come from that.

Bytes: the forward reads the two maps of every row (8 per position) and the selected rows; the backward reads the maps again and
ASSIGNS every element of d_logits and d_offsets (4 (C + 2) per row of [B, R]); the fraction of the HBM peak (8 TB/s) that is,
launches included, is printed with the times.

--step: also the captured training step of config P with the term (cl_cfg.name 'erd', n_known > 0, every clip of the batch
recorded from the model itself) next to the plain captured step of the same model class, both timed here.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vilco_amd import ops  # noqa: E402
from vilco_amd.cl_methods import erd  # noqa: E402

PEAK_GBPS = 8000.0


def head_output(dev, B=2, n_old=None):
    import bench
    cfg = bench.p_config()
    T0, C = cfg['max_seq_len'], int(cfg['num_classes'])
    n_levels = cfg['backbone_arch'][-1] + 1
    levels = [T0 // (cfg['scale_factor'] ** l) for l in range(n_levels)]
    rows = [sum(levels[:l]) + l for l in range(n_levels)]          # one separator row between levels, as LevelCat lays them out
    R = sum(levels) + n_levels - 1
    n_old = max(1, C // 2) if n_old is None else n_old
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, R, C, device=dev, generator=g)
    o = torch.randn(B, R, 2, device=dev, generator=g)
    scale = torch.ones(n_levels, device=dev)
    lens = [[max(1, (T0 - (17 if b % 2 else 0)) // (cfg['scale_factor'] ** l)) for l in range(n_levels)] for b in range(B)]
    level_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    P = sum(levels)
    recs = []
    for b in range(B):
        sel = erd.valid_mask(levels, lens[b], dev) & (torch.rand(P, device=dev, generator=g) < 0.1)
        maps = []
        for _ in range(2):
            m = torch.full((P,), -1, dtype=torch.int32, device=dev)
            m[sel] = torch.arange(int(sel.sum()), dtype=torch.int32, device=dev)
            maps.append(m)
        k = int(sel.sum())
        recs.append(erd.Record(maps[0], maps[1], torch.randn(max(k, 1), n_old, device=dev, generator=g),
                               torch.rand(max(k, 1), 2, device=dev, generator=g) * 3.0, k, k, n_old, 0, tuple(levels)))
    tab = torch.tensor([r.row() for r in recs], dtype=torch.int64, device=dev)
    return x, o, scale, rows, levels, lens, level_len, recs, tab


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
    x, o, scale, rows, levels, lens, level_len, recs, tab = head_output(dev)
    xs = [t.requires_grad_(True) for t in (x, o, scale)]

    def run_op():
        loss = ops.erd_distill(x, o, scale, rows, levels, level_len, tab, 1.0, 1.0)[0]
        torch.autograd.grad(loss, xs)

    def run_body():
        loss = erd.erd_term(x, o, scale, rows, levels, lens, recs, 1.0, 1.0)[0]
        torch.autograd.grad(loss, xs)

    def run_fwd():
        with torch.no_grad():
            ops.erd_distill(x, o, scale, rows, levels, level_len, tab, 1.0, 1.0)
    forms = {'op_fwd_bwd': run_op, 'op_fwd': run_fwd, 'tensor_ops_fwd_bwd': run_body}
    ts = {k: [] for k in forms}
    for it in range(3 + reps):
        for k, fn in forms.items():
            t = once(fn)
            if it >= 3:
                ts[k].append(t)
    B, R, C = x.shape
    P = sum(levels)
    sel = sum(r.k_cls * r.n_old * 2 + r.k_reg * 4 for r in recs)          # the selected rows, student and record
    res = {"levels": list(levels), "B": int(B), "R": int(R), "C": int(C), "selected_rows": [r.k_cls for r in recs], "reps": reps}
    for k, v in ts.items():
        v.sort()
        res[k + "_us_median_min_max"] = (round(v[len(v) // 2], 1), round(v[0], 1), round(v[-1], 1))
    res["op_fwd_bwd_graphed_us"] = graphed_us(run_op)
    res["op_fwd_graphed_us"] = graphed_us(run_fwd)
    fwd_bytes = 8 * B * P + 4 * sel
    all_bytes = 2 * fwd_bytes + 4 * B * R * (C + 2)
    res["bytes_fwd"], res["bytes_fwd_bwd"] = fwd_bytes, all_bytes
    res["fraction_of_hbm_peak"] = round(all_bytes / res["op_fwd_bwd_graphed_us"] / 1e3 / PEAK_GBPS, 4)
    res["fwd_fraction_of_hbm_peak"] = round(fwd_bytes / res["op_fwd_graphed_us"] / 1e3 / PEAK_GBPS, 4)
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
    for name in (None, 'erd'):
        cfg = bench.p_config()
        cfg['cl_cfg'] = dict(cfg['cl_cfg'], name=name)
        torch.manual_seed(0)
        model = vm.make_meta_arch('LocPointTransformer', **dict(cfg, xlnet_config=bench.p_xlnet())).to(dev).train()
        if name == 'erd':
            model.n_known = 11
            model.erd_bank = erd.ERDBank()
            n, nbytes = erd.record_clips(model, model.erd_bank, [batch], 0)
            assert n == len(batch)
            out["record_bytes_per_clip"] = nbytes // n
        gs = GraphedStep(model, None, eager_steps=1)
        ts = []
        for it in range(2 + warmup + steps):
            t = once(lambda: gs(batch, task_id=0))
            if it >= 2 + warmup:
                ts.append(t / 1e3)
        ts.sort()
        key = 'step_with_erd_ms' if name else 'step_plain_ms'
        out[key + "_median_min_max"] = (round(ts[len(ts) // 2], 3), round(ts[0], 3), round(ts[-1], 3))
        out[key.replace('_ms', '_stats')] = dict(gs.stats)
        del gs, model
        torch.cuda.empty_cache()
    out["step_delta_ms"] = round(out["step_with_erd_ms_median_min_max"][0] - out["step_plain_ms_median_min_max"][0], 3)
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
