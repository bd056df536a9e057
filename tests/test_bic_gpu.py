"""GPU: vilco_bic_eval / vilco_bic_fit (csrc/bic.hip) against the float64 restatement (tests/bic_restatement.py) on
synthetic caches, and the BiC driver end to end on the episode fixture model.

Tolerance: the distance of the SAME restatement run in float32 on the CPU from its float64 run on the same inputs is the
yardstick; the kernels (fp32 per element, fp64 sums) must be within 4 x that distance, with an absolute floor of 1e-6.
Every case prints both distances before it asserts (run with -s to see them)."""
import os
import random

import pytest
import torch

import bic_restatement as R
from parity_util import cases, episode_full_state, load_episode_golden

LR = 0.001


def _bar(d32):
    return max(4.0 * d32, 1e-6)


def _dist(a, b):
    return max(abs(x - y) for x, y in zip(a, b)) if len(a) else 0.0


def _check(name, got, want64, want32):
    d_k, d_32 = _dist(got, want64), _dist(want32, want64)
    print("bic %-28s kernel-vs-fp64 %.3e   fp32-vs-fp64 %.3e   bar %.3e" % (name, d_k, d_32, _bar(d_32)))
    assert d_k <= _bar(d_32), (name, d_k, d_32)


def _run(dev, tag, clip_rows, C, lo, hi, smoothing=0.1, batch=1, n_steps=1, seed=0, no_pos_clips=()):
    from vilco_amd import ops
    from vilco_amd.cl_methods.bic import epoch_orders
    arrays = R.synthetic_cache(seed, clip_rows, C, no_pos_clips)
    d = [a.to(dev) for a in arrays]
    n_clips = len(clip_rows)
    # ---- eval at a point away from (1, 0)
    ab = (1.25, -0.5)
    got = ops.bic_eval(*d, lo, hi, smoothing, torch.tensor(ab, dtype=torch.float32, device=dev)).tolist()
    _check(tag + " eval", got, R.evaluate(arrays, lo, hi, smoothing, ab, torch.float64),
           R.evaluate(arrays, lo, hi, smoothing, ab, torch.float32))
    # ---- fit: whole batches of shuffled epochs laid end to end, cut to n_steps
    per_epoch = max(n_clips // batch, 1)
    order = epoch_orders(n_clips, -(-n_steps // per_epoch), batch, seed=seed)[:n_steps * batch]
    assert len(order) == n_steps * batch
    od = torch.tensor(order, dtype=torch.int32, device=dev)
    runs = []
    for _ in range(2):
        ab_d = torch.tensor([1.0, 0.0], dtype=torch.float32, device=dev)
        losses = ops.bic_fit(*d, od, batch, lo, hi, smoothing, LR, ab_d)
        runs.append((ab_d.clone(), losses.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])       # bit-identical repeats
    ab64, l64 = R.trajectory(arrays, order, batch, lo, hi, smoothing, LR, torch.float64)
    ab32, l32 = R.trajectory(arrays, order, batch, lo, hi, smoothing, LR, torch.float32)
    assert len(l64) == n_steps and runs[0][1].numel() == n_steps
    _check(tag + " fit ab", runs[0][0].double().tolist(), ab64, ab32)
    _check(tag + " fit losses", runs[0][1].tolist(), l64, l32)
    assert tuple(runs[0][0].tolist()) != (1.0, 0.0) or all(v == 0.0 for v in l64)
    return runs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("clip_rows", [[1], [63], [64], [40, 25], [100, 0, 157]], ids=lambda r: "N%d" % sum(r))
def test_rows_at_wave_and_block_edges(dev, clip_rows):
    """N = 1, 63, 64, 65 and 257 rows (257 with an empty clip in the middle), C = 110, the unaligned window [3, 10)"""
    _run(dev, "N%d" % sum(clip_rows), clip_rows, 110, 3, 10, batch=1, n_steps=len(clip_rows), seed=sum(clip_rows))


@pytest.mark.gpu
@pytest.mark.parametrize("C,lo,hi", [(110, 60, 70), (110, 109, 110), (110, 0, 110), (128, 120, 128), (1, 0, 1)])
def test_column_windows(dev, C, lo, hi):
    """across the 64-bit boundary of label_bits, a single column, the whole row, the last columns of C = 128, C = 1"""
    _run(dev, "C%d[%d,%d)" % (C, lo, hi), [100, 0, 157], C, lo, hi, batch=2, n_steps=3, seed=C + lo)


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n_steps,smoothing", [(1, 1, 0.0), (1, 40, 0.1), (3, 1, 0.1), (3, 40, 0.0)])
def test_trajectories_over_seven_clips(dev, batch, n_steps, smoothing):
    """7 clips, one of them empty, two without any positive point: with batch 1 their steps have P = 0 (divisor 1)"""
    rows = [33, 70, 0, 129, 64, 5, 90]
    ab, losses = _run(dev, "b%d s%d sm%.1f" % (batch, n_steps, smoothing), rows, 110, 3, 10, smoothing=smoothing, batch=batch,
                      n_steps=n_steps, seed=11, no_pos_clips=(1, 5))
    assert bool(torch.isfinite(losses).all())


@pytest.mark.gpu
def test_a_step_without_positives_and_an_empty_step(dev):
    """P = 0 in every step (the divisor is clamped to 1), and a step over an empty clip alone (loss 0, no movement)"""
    from vilco_amd import ops
    _run(dev, "P0", [20, 31], 110, 3, 10, batch=2, n_steps=2, seed=3, no_pos_clips=(0, 1))
    arrays = R.synthetic_cache(5, [9, 0, 4], 16)
    d = [a.to(dev) for a in arrays]
    ab = torch.tensor([1.0, 0.0], dtype=torch.float32, device=dev)
    losses = ops.bic_fit(*d, torch.tensor([1], dtype=torch.int32, device=dev), 1, 2, 9, 0.1, LR, ab)
    assert losses.tolist() == [0.0] and ab.tolist() == [1.0, 0.0]


# --------------------------------------------------------------------------------------------------- the driver
def _task_data(task):
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


def _build(dev):
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_episode_golden()
    o = dict(gold['overrides'])
    o['cl_cfg'] = dict(o['cl_cfg'], name='bic')
    cfg = make_config(**o)
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    model.load_state_dict(episode_full_state(gold['init_state']), strict=True)
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    return cfg, model


@pytest.mark.gpu
def test_run_episodes_bic_end_to_end(dev, tmp_path):
    """two tasks of the episode fixture model with cl_cfg.name = 'bic': stage 1, memory, stage 2 on the held-out clips"""
    from vilco_amd.cl_methods.bic import BiCCache, epoch_orders, fit_bias_layer
    from vilco_amd.train_cl import load_best_checkpoint, run_episodes_bic
    from vilco_amd.utils.cl_stream import DistributedBatchLoader, InMemoryBiCStream
    cfg, model = _build(dev)
    cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))           # two epochs per stage
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], path_memory='memory.pkl')
    seen = []

    class Stream(InMemoryBiCStream):
        def __next__(self):
            seen.append(super().__next__())
            return seen[-1]
    stream = Stream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
    random.seed(0)
    folder = str(tmp_path)
    model, opt, sch, log = run_episodes_bic(cfg, model, stream, validate=None, ckpt_folder=folder, gpu_id=0)
    assert len(log) == 2 and 'bic' not in log[0] and seen[0][2] is None
    assert model.list_splits == [cases.EP_NCLS0, cases.EP_NCLS0 + cases.EP_NEW] and len(model.list_bias_layers) == 2
    old, new = model.list_bias_layers
    assert (float(old.alpha), float(old.beta)) == (1.0, 0.0)                   # task 0 has no stage 2
    got = (float(new.alpha), float(new.beta))
    assert got != (1.0, 0.0) and got == (log[1]['bic']['alpha'], log[1]['bic']['beta'])
    hist = [h for e in log for ep in e['history'] for h in ep]
    assert all(bool(torch.isfinite(h['final_loss'])) for h in hist) and 'dist_loss' in log[1]['history'][0][0]

    # ---- the cache of the held-out clips, rebuilt on the (frozen) model the run ended with
    held = seen[1][2]
    walk = DistributedBatchLoader(held.items, held.batch_size, shuffle=False, drop_last=False)
    cache = BiCCache.build(model, walk, 1)
    assert cache.n_clips == len(held.items) == log[1]['bic']['n_clips'] and cache.video_ids == [v['video_id'] for v in held.items]
    model.eval()
    lg, wt, ps = [], [], []
    with torch.no_grad():
        known, model.n_known = model.n_known, 0                               # no correction by another route
        for batch in walk:
            cls_logits, _, masks = model(batch, task_id=1, get_emb=True)
            points = model.point_generator(cls_logits, lengths=[x.shape[1] for x in cls_logits])
            gt_cls, _, w_cls, _ = model.label_points(points, [v['segments'].to(dev) for v in batch],
                                                     [v['labels'].to(dev) for v in batch])
            gt_cls, w_cls, valid = torch.stack(gt_cls), torch.stack(w_cls), torch.cat(masks, dim=1)
            pos_mask = torch.logical_and(gt_cls.sum(-1) > 0, valid)            # PtTransformer.losses
            w_cls = torch.where(pos_mask, w_cls, torch.ones_like(w_cls))
            lg.append(torch.cat(cls_logits, dim=1).reshape(-1, cls_logits[0].shape[-1]))
            wt.append((w_cls * valid.float()).reshape(-1))
            ps.append(pos_mask.reshape(-1))
        model.n_known = known
    assert torch.equal(cache.logits, torch.cat(lg)) and torch.equal(cache.weight, torch.cat(wt))
    assert torch.equal(cache.pos, torch.cat(ps).to(torch.uint8)) and int(cache.pos.sum()) > 0
    assert cache.clip_ptr.tolist() == [i * (cache.logits.shape[0] // cache.n_clips) for i in range(cache.n_clips + 1)]

    # ---- (alpha, beta) and the losses = the restatement's trajectory on that cache
    arrays = tuple(a.cpu() for a in (cache.logits, cache.label_bits, cache.weight, cache.pos, cache.clip_ptr))
    order = epoch_orders(cache.n_clips, 2, held.batch_size, seed=held.seed)
    lo, hi = cases.EP_NCLS0, cases.EP_NCLS0 + cases.EP_NEW
    ab64, l64 = R.trajectory(arrays, order, held.batch_size, lo, hi, cache.smoothing, LR, torch.float64)
    ab32, l32 = R.trajectory(arrays, order, held.batch_size, lo, hi, cache.smoothing, LR, torch.float32)
    _check("driver ab", list(got), ab64, ab32)
    _check("driver losses", log[1]['bic']['losses'].tolist(), l64, l32)

    # ---- the checkpoint carries the splits and the fitted layer
    ck = torch.load(os.path.join(folder, 'best_task_001_performance.pth.tar'), weights_only=False)
    assert ck['list_splits'] == model.list_splits and len(ck['list_bias_layers']) == 2
    model.list_splits, model.list_bias_layers = [], []
    model = load_best_checkpoint(model, folder, 'best_task_001_performance.pth.tar', 1, 0)
    assert model.list_splits == [lo, hi]
    assert [(float(b.alpha), float(b.beta)) for b in model.list_bias_layers] == [(1.0, 0.0), got]
    assert all(b.alpha.device == model.device and not b.alpha.requires_grad for b in model.list_bias_layers)

    # ---- a further fit moves the newest layer only
    with torch.no_grad():
        model.list_bias_layers[0].alpha.fill_(1.3)
        model.list_bias_layers[0].beta.fill_(-0.2)
    before = [(b.alpha.clone(), b.beta.clone()) for b in model.list_bias_layers]
    losses = fit_bias_layer(model, cache, 1, held.batch_size, lr=LR, seed=held.seed)
    assert losses.dtype == torch.float64 and losses.is_cuda and losses.numel() == cache.n_clips // held.batch_size
    assert torch.equal(model.list_bias_layers[0].alpha, before[0][0]) and torch.equal(model.list_bias_layers[0].beta, before[0][1])
    assert not torch.equal(model.list_bias_layers[1].alpha, before[1][0])
