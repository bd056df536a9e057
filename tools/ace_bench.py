"""ER-ACE loss timing: ops.mq_loss_ace forward + backward against ops.mq_loss -- the plain entries -- on
identical inputs at the headline loss shape (config P: 2 clips, the six levels 2304 .. 72 in the LevelCat layout with separator
rows, the configuration's class count), in the same process, alternated, device events around each form, warmed up.  An eager
call is bound by the host (two + two launches behind Python), so every form is timed as ten forward + backward calls captured
in one graph and replayed `reps` times: microseconds per call, median (min, max).

Forms: `plain` twice (a, b: their difference is the run-to-run spread a comparison has to beat), `ace_zero` (every window 0:
the same arithmetic through the windowed kernels), `ace_task` (clip 0 a task clip with --known classes masked (default: half of them),
clip 1 a memory clip), `ace_all_task` (both clips task clips).

--plain-only: only the plain forms, for a library built from another commit (VILCO_HIP_LIB names it) that has no ACE entries.
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(dev, B=2, n_gt=8):
    import bench
    cfg = bench.p_config()
    T0, C, sf = cfg['max_seq_len'], cfg['num_classes'], cfg['scale_factor']
    rr = cfg['regression_range']
    L = len(rr)
    g = torch.Generator().manual_seed(0)
    pts, lvl, pos = [], [], []
    for l in range(L):
        T, s = T0 // sf ** l, float(sf ** l)
        if l:
            pts.append(torch.zeros(1, 4)); lvl.append(l); pos.append(1 << 30)
        t = torch.arange(0, T0, sf ** l, dtype=torch.float32)[:, None]
        pts.append(torch.cat([t, torch.tensor([rr[l]], dtype=torch.float32).repeat(T, 1), torch.full((T, 1), s)], dim=1))
        lvl += [l] * T
        pos += list(range(T))
    points = torch.cat(pts).contiguous()
    R = points.shape[0]
    logits = 2.0 * torch.randn(B, R, C, generator=g) - 2.0
    offsets = 3.0 * torch.randn(B, R, 2, generator=g)
    scale = torch.rand(L, generator=g) + 0.5
    gauss = torch.cat([0.2 * torch.randn(1, C, generator=g), 1 + 0.2 * torch.rand(1, C, generator=g),
                       -0.5 + 0.1 * torch.randn(1, C, generator=g), 1 + 0.2 * torch.rand(1, C, generator=g),
                       0.5 + 0.1 * torch.randn(1, C, generator=g), 1 + 0.2 * torch.rand(1, C, generator=g)]).contiguous()
    level_len = torch.tensor([[max(1, (T0 - (17 if b % 2 else 0)) // sf ** l) for l in range(L)] for b in range(B)], dtype=torch.int32)
    gt = torch.zeros(B, 3 * n_gt + 1)
    for b in range(B):
        s0 = torch.randint(0, 4 * (T0 - 600), (n_gt,), generator=g).float() / 4
        ln = torch.tensor([3.0, 7.0, 14.0, 30.0, 60.0, 120.0, 250.0, 500.0])[torch.arange(n_gt) % 8]
        gt[b, :2 * n_gt] = torch.stack([s0, s0 + ln], dim=1).reshape(-1)
        gt[b, 2 * n_gt:3 * n_gt] = torch.randint(0, C, (n_gt,), generator=g).float()
        gt[b, 3 * n_gt] = n_gt
    x = dict(lg=logits.to(dev).requires_grad_(True), of=offsets.to(dev).requires_grad_(True), sc=scale.to(dev).requires_grad_(True),
             gauss=gauss.to(dev).requires_grad_(True),
             tables=(points.to(dev), torch.tensor(lvl, dtype=torch.int32, device=dev), torch.tensor(pos, dtype=torch.int32, device=dev)),
             lvl_len=level_len.to(dev), gt=gt.to(dev), norm=torch.full((1,), 100.0, device=dev))
    return x, dict(B=B, R=R, C=C, L=L, n_gt=n_gt)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def captured(fn, n=10):
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
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--known", type=int, default=None, help="classes masked for a task clip (default: half of them)")
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    from vilco_amd import _lib, ops
    if args.plain_only:
        for name in ("vilco_mq_loss_ace_fwd", "vilco_mq_loss_ace_bwd"):      # a library from before the entries existed
            _lib.SIGNATURES.pop(name, None)
    dev = torch.device('cuda', 0)
    x, shape = inputs(dev)
    if args.known is None:
        args.known = shape['C'] // 2
    leaves = [x['lg'], x['of'], x['sc'], x['gauss']]
    cfg = (1.5, 0.0, 0.9, 1.0, 0.2, True)

    def run(tab):
        a = (x['lg'], x['of'], x['sc'], x['gauss'], x['tables'], x['lvl_len'], x['gt'], x['norm'], *cfg)
        out = ops.mq_loss(*a) if tab is None else ops.mq_loss_ace(*a, tab)
        grads = torch.autograd.grad(out[3], leaves)
        # detached: an output kept alive keeps its autograd graph and the leaves' AccumulateGrad nodes alive, bound to the stream
        # they were made on -- a later capture on another stream would then be made to synchronise with that stream
        return [t.detach() for t in out] + [t.detach() for t in grads]

    def table(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)
    forms = {'plain_a': None, 'plain_b': None}
    if not args.plain_only:
        forms.update(ace_zero=table([0, 0]), ace_task=table([args.known, 0]), ace_all_task=table([args.known, args.known]))
    n = 10

    def call(t):
        run(t)
        return None
    graphs = {k: captured(lambda t=t: call(t), n) for k, t in forms.items()}
    ts = {k: [] for k in forms}
    for it in range(3 + args.reps):
        for k, g in graphs.items():
            t = once(g.replay) / n
            if it >= 3:
                ts[k].append(t)
    res = dict(shape, reps=args.reps, calls_per_replay=n, known=args.known, lib=os.path.basename(_lib.LIB_PATH))
    for k, v in ts.items():
        v.sort()
        res[k + "_us_median_min_max"] = (round(v[len(v) // 2], 2), round(v[0], 2), round(v[-1], 2))
    res["plain_spread_us"] = round(abs(res["plain_a_us_median_min_max"][0] - res["plain_b_us_median_min_max"][0]), 2)
    if not args.plain_only:
        # the same numbers: every window 0 is the plain op bit for bit (eager calls, after the timing)
        x['norm'].fill_(100.0)
        plain_out = run(None)
        x['norm'].fill_(100.0)
        zero_out = run(forms['ace_zero'])
        res["ace_zero_equals_plain_bits"] = all(torch.equal(a, b) for a, b in zip(plain_out, zero_out))
        plain = min(res["plain_a_us_median_min_max"][0], res["plain_b_us_median_min_max"][0])
        for k in ('ace_zero', 'ace_task', 'ace_all_task'):
            res[k + "_minus_plain_us"] = round(res[k + "_us_median_min_max"][0] - plain, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
