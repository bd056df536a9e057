"""GPU: the herding kernels (`vilco_frob_scale`, `vilco_gram`, `vilco_herd_select`) and `type_sampling = 'herding'` end to end
against the NumPy fp64 restatement (tests/herding_restatement.py).

Error bars.  The Gram kernel is held to NumPy's own fp32 product: `X32 @ X32.T` has some max error against the fp64 product
of the same rounded rows, measured here; the kernel may be at most 4x worse (the factor covers a different summation order; a
dropped part of the split-K would be orders of magnitude beyond it).  Measured on the MI355X over the shapes below: kernel
4.1e-08 .. 9.1e-08 (from D = 1000 up the rounding of the result to fp32; the slabs are added in fp64) against NumPy
8.9e-08 .. 2.5e-06; worst pair N = 5, D = 37: 9.1e-08 against 1.6e-07; at N = 96, D = 2304 * 1024: 6.7e-08 against 2.5e-06.
End to end, `delta` = 4 x the largest difference between the restatement's costs from the fp64 Gram matrices and from NumPy's
fp32 Gram matrices along the device's prefix, measured in the test on the CPU: 3.0e-06 / 3.5e-06 for the two fixture classes.
"""
import os
import random

import numpy as np
import pytest
import torch

import herding_restatement as H
from parity_util import HERE, cases

pytestmark = pytest.mark.gpu


def _rows(seed, N, D):
    """fp32 rows of unit norm: a shared direction plus noise, so the off-diagonal entries are not all near zero"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x += rng.standard_normal(D, dtype=np.float32)[None, :]
    n = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    x /= n[:, None].astype(np.float32)
    return x


def _gram64(x32, chunk=1 << 18):
    g = np.zeros((x32.shape[0], x32.shape[0]))
    for k in range(0, x32.shape[1], chunk):
        c = x32[:, k:k + chunk].astype(np.float64)
        g += c @ c.T
    return g


GRAM_SHAPES = [(3, 64), (5, 37), (17, 1000), (33, 4099), (96, 100000), (97, 70001), (200, 30000), (320, 5000),
               (96, 2304 * 1024)]                     # the last: level 0 of config P, 96 candidates; 64 | D but slabs do not divide it


@pytest.mark.parametrize("N,D", GRAM_SHAPES)
def test_gram_against_fp64(dev, N, D):
    from vilco_amd import ops
    x32 = _rows(100 + N, N, D)
    want = _gram64(x32)
    err_np = float(np.abs((x32 @ x32.T).astype(np.float64) - want).max())
    xd = torch.from_numpy(x32).to(dev)
    g1 = ops.gram(xd)
    g2 = ops.gram(xd)
    assert g1.dtype == torch.float32 and tuple(g1.shape) == (N, N)
    assert torch.equal(g1, g2), "two launches differ"
    assert torch.equal(g1, g1.t()), "not exactly symmetric"
    err = float(np.abs(g1.cpu().numpy().astype(np.float64) - want).max())
    print("gram N=%d D=%d: kernel %.3e  numpy fp32 %.3e" % (N, D, err, err_np))
    assert err <= 4 * err_np, (err, err_np)
    # fp64 output: the same sums before the rounding to fp32
    g64 = ops.gram(xd, out_dtype=torch.float64)
    assert torch.equal(g64.to(torch.float32), g1)
    err64 = float(np.abs(g64.cpu().numpy() - want).max())
    print("          fp64 output %.3e" % err64)
    assert err64 <= 4 * err_np


@pytest.mark.parametrize("N,D", [(7, 333), (96, 36864), (130, 20000)])
def test_frob_scale_and_scaled_gram(dev, N, D):
    """raw rows, the inverse norms from vilco_frob_scale folded into the product: the Gram matrix of the normalised rows"""
    from vilco_amd import ops
    rng = np.random.default_rng(7 + N)
    raw = (rng.standard_normal((N, D)) * rng.uniform(0.1, 30.0, size=(N, 1)) + rng.standard_normal(D)[None, :]).astype(np.float32)
    norm = np.sqrt((raw.astype(np.float64) ** 2).sum(axis=1))
    xd = torch.from_numpy(raw).to(dev)
    inv = ops.frob_scale(xd)
    assert torch.equal(inv, ops.frob_scale(xd))
    rel = float(np.abs(inv.cpu().numpy().astype(np.float64) * norm - 1.0).max())
    print("frob N=%d D=%d: rel %.3e" % (N, D, rel))
    # a thread adds at most 64 fp32 squares in sequence (16384-element segments over 256 threads) before everything turns
    # fp64: (64 + 1) roundings of 2^-24 on the sum at the very worst, half of that on the root, one more for the result
    assert rel <= (65 / 2 + 1) * 2.0 ** -24
    x32 = (raw.astype(np.float64) / norm[:, None]).astype(np.float32)
    want = _gram64(x32)
    err_np = float(np.abs((x32 @ x32.T).astype(np.float64) - want).max())
    g = ops.gram(xd, inv, torch.float64)
    # against the fp64 Gram matrix of the exactly normalised raw rows.  On top of the product's own bar (4 x NumPy's error
    # on the rounded normalised rows) an entry |G_ij| <= 1 carries the relative errors of its two inverse norms
    exact = _gram64(raw) / (norm[:, None] * norm[None, :])
    err = float(np.abs(g.cpu().numpy() - exact).max())
    print("scaled gram N=%d D=%d: kernel %.3e  numpy fp32 %.3e" % (N, D, err, err_np))
    assert err <= 4 * err_np + 2 * (65 / 2 + 1) * 2.0 ** -24
    assert torch.equal(g, ops.gram(xd, inv, torch.float64))


@pytest.mark.parametrize("seed,N,dims", [(1, 24, (300, 120)), (2, 40, (256, 128, 64)), (3, 64, (400, 200, 100, 50)),
                                         (4, 1, (30, 10)), (9, 300, (64, 32))])
def test_select_returns_the_restatements_indices(dev, seed, N, dims):
    from vilco_amd import ops
    G = H.gram_matrices(H.synthetic_class(seed, N, dims))
    gd = torch.from_numpy(G).to(dev)
    for m in (0, 1, N // 2, N, N + 7):
        sel = ops.herd_select(gd, m)
        assert sel.dtype == torch.int32 and sel.is_cuda
        assert sel.tolist() == H.herd_gram(G, m), m
    assert ops.herd_select(list(gd), N).tolist() == H.herd_gram(G, N)              # a list of per-level matrices


def test_select_resolves_an_exact_tie_downwards(dev):
    from vilco_amd import ops
    phis = H.synthetic_class(7, 12, (90, 30))
    first = H.herd_literal(phis, 1)[0]
    lo, hi = (0, first) if first != 0 else (0, 5)
    dup = [p.copy() for p in phis]
    for p, q in zip(dup, phis):
        p[lo] = p[hi] = q[first]
    G = H.tie_grams(dup, lo, hi)
    want = H.herd_gram(G, 12)
    got = ops.herd_select(torch.from_numpy(G).to(dev), 12).tolist()
    assert got == want and got.index(lo) < got.index(hi)
    # all clips equal: every step is a tie over everything that is left
    G1 = np.ones((2, 9, 9))
    assert ops.herd_select(torch.from_numpy(G1).to(dev), 9).tolist() == list(range(9)) == H.herd_gram(G1, 9)


# ------------------------------------------------------------------------------------------------------- end to end
class Stub:
    """the task stream as far as herding uses it: one-clip batches in dataset order"""

    def get_dataloader(self, data, batch_size=1, memory=None, sample_frame=False):
        assert sample_frame is True and batch_size == 1 and memory is None
        return [[v] for vs in data.values() for v in vs]


N_PER = 10


def _class_clips(c, base=200):
    return [cases.icarl_clip(base + 20 * c + k, (c, (c + 1) % cases.IC_NCLS)) for k in range(N_PER)]


def _icarl_model(dev):
    import vilco_amd.modeling as vm
    from vilco_amd.core.config import make_config
    g = torch.load(os.path.join(HERE, "golden", "icarl.pt"), weights_only=False)
    o = dict(g['overrides'])
    o['cl_cfg'] = dict(o['cl_cfg'], type_sampling='herding')
    model = vm.make_meta_arch('LocPointTransformer', **make_config(**o)['model'])
    model.load_state_dict(g['state_dict'])
    return model.to(dev).train()                   # herding switches to eval mode itself, and back


def _descriptors(model, clips):
    """fp64 unit-norm descriptors from the model's own `_pyramid_features` outputs: list over levels of [N, D_l]"""
    was = model.training
    model.eval()
    feats = [[t.reshape(-1).double().cpu().numpy() for t in model._pyramid_features([v])] for v in clips]
    model.train(was)
    return [H.normalise_rows(np.stack([f[l] for f in feats])) for l in range(len(feats[0]))]


def _check_order(order, phis):
    """the device's order against the fp64 restatement along the device's own prefix -> (delta, fraction of decided steps)"""
    G64 = H.gram_matrices(phis)
    G32 = H.gram_matrices([p.astype(np.float32) for p in phis], np.float32)
    N = G64.shape[1]
    assert sorted(order) == list(range(N))
    steps, diff = [], 0.0
    st64, st32 = H.GramState(G64), H.GramState(G32)
    for p in order:
        c64, c32 = st64.costs(), st32.costs()
        free = ~st64.taken
        diff = max(diff, float(np.abs(c64 - c32)[free].max()))
        steps.append((c64, free.copy(), st64.best()))
        st64.add(p)
        st32.add(p)
    delta = 4 * diff
    decided = 0
    for k, (p, (c64, free, best)) in enumerate(zip(order, steps)):
        srt = np.sort(c64[free])
        gap = srt[1] - srt[0] if len(srt) > 1 else np.inf
        assert c64[p] - srt[0] <= delta, (k, p, best, c64[p] - srt[0], delta)
        if gap > delta:
            decided += 1
            assert p == best, (k, p, best, gap, delta)
    return delta, decided / N


def test_herding_memory_end_to_end(dev, capsys):
    model = _icarl_model(dev)
    assert model.type_sampling == 'herding' and model.training
    stub = Stub()
    data = {c: _class_clips(c) for c in (0, 1)}
    ids = {c: [v['video_id'] for v in vs] for c, vs in data.items()}
    orders = {}
    for c, clips in data.items():
        got_clips, sel = model.herding_order(stub, c, clips, 'ALL')
        assert model.training and sel.is_cuda and sel.dtype == torch.int32
        assert [v['video_id'] for v in got_clips] == ids[c]
        orders[c] = sel.tolist()
        delta, frac = _check_order(orders[c], _descriptors(model, clips))
        with capsys.disabled():
            print("herding class %d: order %s  delta %.3e  decided steps %.0f %%" % (c, orders[c], delta, 100 * frac))
        assert frac >= 0.8, "the fixture does not decide enough steps"
    # the memory: m per class in selection order; a second call from scratch is identical
    model.add_samples_to_mem(stub, {c: list(v) for c, v in data.items()}, 4)
    want = {c: [ids[c][i] for i in orders[c][:4]] for c in data}
    assert {c: [v['video_id'] for v in vs] for c, vs in model.memory.items()} == want
    assert all(v['video_id'] == i for c in data for v, i in zip(model.memory[c], want[c]))
    first = {c: list(vs) for c, vs in model.memory.items()}
    model.memory = {}
    model.add_samples_to_mem(stub, {c: list(v) for c, v in data.items()}, 4)
    assert {c: [v['video_id'] for v in vs] for c, vs in model.memory.items()} == want
    assert all(a is b for c in first for a, b in zip(first[c], model.memory[c]))
    # the next task: the old classes shrink in order, without reshuffling; the new class is herded
    random.seed(0)
    new = _class_clips(2)
    model.add_samples_to_mem(stub, {2: list(new)}, 2)
    assert list(model.memory) == [0, 1, 2]
    assert {c: [v['video_id'] for v in model.memory[c]] for c in (0, 1)} == {c: want[c][:2] for c in (0, 1)}
    _, sel2 = model.herding_order(stub, 2, new, 2)
    assert [v['video_id'] for v in model.memory[2]] == [new[i]['video_id'] for i in sel2.tolist()]
    # 'ALL' keeps every clip, still in herding order
    model.memory = {}
    model.add_samples_to_mem(stub, {0: list(data[0])}, 'ALL')
    assert [v['video_id'] for v in model.memory[0]] == [ids[0][i] for i in orders[0]]
    # unequal level shapes are refused by name
    odd = dict(cases.icarl_clip(1), video_id='odd_one')
    model2 = _icarl_model(dev)
    real = model2._pyramid_features
    model2._pyramid_features = lambda vl: [t[:, :-1] for t in real(vl)] if vl[0]['video_id'] == 'odd_one' else real(vl)
    with pytest.raises(ValueError, match="odd_one"):
        model2.herding_order(stub, 0, [cases.icarl_clip(0), odd], 1)


def test_run_episodes_ends_with_the_herded_memory(dev):
    from test_episode import _build, _task_data
    from parity_util import load_episode_golden
    from vilco_amd.train_cl import memory_quota, run_episodes
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    gold = load_episode_golden()
    cfg, model = _build(gold, dev)
    cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], type_sampling='herding')
    model.type_sampling = 'herding'
    tasks = [_task_data(0), _task_data(1)]
    stream = InMemoryQILStream(tasks, batch_size=2, seed=3)
    random.seed(0)
    model, _, _, log = run_episodes(cfg, model, stream, validate=None, ckpt_folder=None, gpu_id=0, keep_history=False)
    assert stream.memory is model.memory and sorted(model.memory) == sorted({**tasks[0], **tasks[1]})
    m = memory_quota(cfg['cl_cfg']['memory_size'], model.cls_head.cls_head.conv.out_channels)
    for c, vs in model.memory.items():
        pool = [v['video_id'] for v in {**tasks[0], **tasks[1]}[c]]
        got = [v['video_id'] for v in vs]
        assert len(got) == min(m, len(pool)) and len(set(got)) == len(got) and set(got) <= set(pool), c
    # the model has not changed since the last task's selection: it can be repeated
    for c in tasks[1]:
        clips, sel = model.herding_order(stream, c, tasks[1][c], m)
        assert [v['video_id'] for v in model.memory[c]] == [clips[i]['video_id'] for i in sel.tolist()], c
