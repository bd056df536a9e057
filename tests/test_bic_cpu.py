"""CPU: the BiC stage-2 contract.  The restatement (tests/bic_restatement.py) equals the classification term of
`PtTransformer.losses`, the held-out split of the task stream follows the reference's rule, the C entry points are
declared, bound and validate their arguments on the host.

No golden of the reference's `BiCQILSetTask` split is recorded: its `__next__` (cl_benchmark.py:198-235) builds both
loaders through `make_dataset` / `make_data_loader` over Ego4D feature files, which tests/golden/_shims does not stand in
for, and it never advances `current_task` after task 0 (:209-213), so driving it yields task 0 for ever.  The rule itself
(:217-221) is three lines and is restated literally in `test_split_rule_is_the_references`."""
import os

import pytest
import torch

import bic_restatement as R

NEW = ("vilco_bic_fit_ws_bytes", "vilco_bic_fit", "vilco_bic_eval_ws_bytes", "vilco_bic_eval")


def test_abi_symbols_declared_and_bound():
    from vilco_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vilco_hip.h")) as h:
        header = h.read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)
    assert callable(ops.bic_fit) and callable(ops.bic_eval)
    with open(os.path.join(root, "vilco_amd", "csrc", "Makefile")) as h:
        assert "bic.hip" in h.read()


def test_entry_points_validate_on_the_host():
    from vilco_amd import _lib, ops
    lib = _lib.load()
    x = 4096                                              # dummy aligned address: every check precedes the launch
    big = 1 << 30

    def fit(C=110, lo=3, hi=10, batch=2, ws=big, n_steps=4):
        return lib.vilco_bic_fit(x, x, x, x, x, 100, 4, x, n_steps, batch, C, lo, hi, 0.1, 0.001, x, x, x, ws, None)

    def ev(C=110, lo=3, hi=10, ws=big):
        return lib.vilco_bic_eval(x, x, x, x, x, 100, 4, C, lo, hi, 0.1, x, x, x, ws, None)
    for f in (fit, ev):
        assert f(C=129, hi=129) == -1                     # C > 128
        assert f(lo=10, hi=10) == -1 and f(lo=11, hi=10) == -1
        assert f(hi=111) == -1                            # hi > C
        assert f(ws=16) == -4
    assert fit(batch=0) == -1 and fit(batch=-3) == -1
    assert fit(n_steps=0) == 0                            # nothing to launch
    assert lib.vilco_bic_fit(None, x, x, x, x, 100, 4, x, 4, 2, 110, 3, 10, 0.1, 0.001, x, x, x, big, None) == -1
    assert lib.vilco_bic_fit(x, x, x, x, x, 1 << 24, 4, x, 4, 2, 110, 3, 10, 0.1, 0.001, x, x, x, big, None) == -2
    assert lib.vilco_bic_fit_ws_bytes(100, 4, 0, 3, 10) == 0 and lib.vilco_bic_fit_ws_bytes(100, 4, 2, 3, 10) > 0
    assert lib.vilco_bic_eval_ws_bytes(100, 4, 10, 3) == 0 and lib.vilco_bic_eval_ws_bytes(100, 4, 0, 128) > 0
    a = R.synthetic_cache(1, [5, 4], 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bic_eval(*a, 0, 7, 0.0, torch.tensor([1.0, 0.0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bic_fit(*a, torch.zeros(2, dtype=torch.int32), 1, 0, 7, 0.0, 0.001, torch.tensor([1.0, 0.0]))


def test_focal_restatement_is_the_librarys():
    from vilco_amd.modeling.losses import sigmoid_focal_loss
    g = torch.Generator().manual_seed(0)
    x, t = 3 * torch.randn(50, 9, generator=g), (torch.rand(50, 9, generator=g) < 0.1).float() * 0.9 + 0.01
    assert torch.equal(R.focal(x, t), sigmoid_focal_loss(x, t, reduction='None'))
    assert (R.focal(x.double(), t.double()) - sigmoid_focal_loss(x, t).double()).abs().max() < 1e-5
    assert R.focal(x.double(), t.double()).dtype == torch.float64


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_objective_is_the_cls_loss_of_losses(smoothing):
    """lo = 0, hi = C, alpha = 1, beta = 0: the restatement = `losses`' classification term (meta_archs.py losses: pos_mask,
    gt_target, w_cls = 1 on negatives, sum over valid points) with dense masks, divided by the batch's own max(num_pos, 1)"""
    from vilco_amd.cl_methods.bic import BiCCache
    from vilco_amd.modeling.losses import sigmoid_focal_loss
    g = torch.Generator().manual_seed(4)
    B, Pn, C = 3, 37, 70
    logits = 3 * torch.randn(B, Pn, C, generator=g)
    gt_cls = (torch.rand(B, Pn, C, generator=g) < 0.03).float()
    valid = torch.arange(Pn)[None, :] < torch.tensor([37, 20, 31])[:, None]
    w_cls = torch.rand(B, Pn, generator=g)
    # -- PtTransformer.losses, sync-free form
    pos_mask = torch.logical_and(gt_cls.sum(-1) > 0, valid)
    gt_target = gt_cls * (1 - smoothing) + smoothing / (C + 1)
    w = torch.where(pos_mask, w_cls, torch.ones_like(w_cls))
    want = (sigmoid_focal_loss(logits.double(), gt_target.double(), reduction='None').double().sum(-1) * w * valid.double()).sum()
    want32 = float(want / pos_mask.sum().clamp(min=1))
    # -- the cache arrays as BiCCache.build packs them
    arrays = (logits.reshape(-1, C), BiCCache.pack_bits(gt_cls).reshape(-1, 2), (w * valid.float()).reshape(-1),
              pos_mask.to(torch.uint8).reshape(-1), torch.tensor([0, Pn, 2 * Pn, 3 * Pn], dtype=torch.int32))
    assert torch.equal(R.unpack_bits(arrays[1], C), gt_cls.reshape(-1, C).double())
    got = float(R.objective(arrays, [0, 1, 2], 0, C, smoothing, R.make_layer((1.0, 0.0), torch.float64), torch.float64))
    assert abs(got - want32) <= 1e-5 * abs(want32), (got, want32)          # `want` went through the library's fp32 focal
    L, ga, gb = R.evaluate(arrays, 0, C, smoothing, (1.0, 0.0), torch.float64)
    assert L == got and ga != 0.0 and gb != 0.0


def test_pack_bits_words():
    from vilco_amd.cl_methods.bic import BiCCache
    t = torch.zeros(3, 128)
    t[0, 0] = t[0, 63] = t[1, 64] = t[1, 127] = t[2, 5] = 1
    t[2, 6] = 0.5                                          # only exact ones count (gt_cls == 1)
    w = BiCCache.pack_bits(t)
    assert w.dtype == torch.int64 and w.tolist() == [[1 - (1 << 63), 0], [0, 1 - (1 << 63)], [32, 0]]
    assert torch.equal(R.unpack_bits(w, 128), (t == 1).double())
    assert BiCCache.pack_bits(torch.ones(2, 1)).tolist() == [[1, 0], [1, 0]]


def _videos(n, tag):
    return [{'id': '%s%d' % (tag, i), 'video_id': '%s%d' % (tag, i)} for i in range(n)]


def test_stream_split():
    from vilco_amd.utils.cl_stream import InMemoryBiCStream, InMemoryQILStream
    tasks = [{0: _videos(10, 'a'), 1: _videos(1, 'b')}, {2: _videos(5, 'c'), 3: _videos(1, 'd')}, {4: _videos(20, 'e')}]
    s = InMemoryBiCStream(tasks, batch_size=2, shuffle=False)
    it = iter(s)
    data, loader, held, nxt = next(it)
    assert held is None and nxt == 2 and data is tasks[0]                  # task 0: one loader over everything
    assert [v['id'] for v in loader.items] == ['a%d' % i for i in range(10)] + ['b0']
    s.memory = {0: tasks[0][0][:3], 1: tasks[0][1][:1]}
    data, loader, held, nxt = next(it)
    assert nxt == 1 and data is tasks[1]
    # memory first, every class cut at int(n * 0.9): 3 -> 2 + 1, 5 -> 4 + 1.  A class with ONE clip has it held out:
    # int(1 * 0.9) = 0 clips go to stage 1 -- what the reference's rule gives (cl_benchmark.py:217-221), kept as it is
    assert [v['id'] for v in loader.items] == ['a0', 'a1', 'c0', 'c1', 'c2', 'c3']
    assert [v['id'] for v in held.items] == ['a2', 'b0', 'c4', 'd0']
    assert [v['is_memory'] for v in loader.items] == [True, True, False, False, False, False]
    assert [v['is_memory'] for v in held.items] == [True, True, False, False]
    assert loader.shuffle is False and held.batch_size == 2
    s.memory = {}
    data, loader, held, nxt = next(it)
    assert nxt is None and len(loader.items) == 18 and len(held.items) == 2          # int(20 * 0.9) = 18
    with pytest.raises(StopIteration):
        next(it)
    # the plain stream is what it was
    d, l, n = next(iter(InMemoryQILStream(tasks, batch_size=2, shuffle=False)))
    assert n == 2 and len(l.items) == 11


def test_split_rule_is_the_references():
    """BiCQILSetTask.__next__ :217-221, literally, against InMemoryBiCStream.split"""
    from vilco_amd.utils.cl_stream import InMemoryBiCStream
    comp = {k: list(range(n)) for k, n in enumerate((1, 2, 9, 10, 11, 19, 20, 21))}
    train_train_data, train_val_data = {}, {}
    for key, values in comp.items():
        total_data_value = len(values)
        len_train_train_data = int(total_data_value * 0.9)
        train_train_data[key] = values[:len_train_train_data]
        train_val_data[key] = values[len_train_train_data:]
    assert InMemoryBiCStream([{}]).split(comp) == (train_train_data, train_val_data)
    assert train_train_data[0] == [] and train_val_data[0] == [0]


def test_epoch_orders_follow_the_loader():
    from vilco_amd.cl_methods.bic import epoch_orders
    from vilco_amd.utils.cl_stream import DistributedBatchLoader
    ld = DistributedBatchLoader(range(7), 3, shuffle=True, seed=5)
    want = []
    for e in range(3):
        ld.sampler.set_epoch(e)
        want += [i for b in ld for i in b]
    got = epoch_orders(7, 3, 3, seed=5)
    assert got == want and len(got) == 18 and sorted(set(got)) == list(range(7))


def test_prev_logits_kind_is_checked():
    from vilco_amd.train_cl import cache_prev_logits
    assert cache_prev_logits(None, [], 0) == {} and cache_prev_logits(None, [], 0, kind='softmax_T2') == {}
    with pytest.raises(ValueError):
        cache_prev_logits(None, [], 0, kind='tanh')
