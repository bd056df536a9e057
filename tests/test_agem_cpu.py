"""A-GEM without a GPU: the float64 restatement (tests/agem_restatement.py) against the one-line formula on the flattened
vector, the inputs of the GPU tests (their conflict is decided far outside the rounding bound), `MemorySampler`, the argument
checks of vilco_agem_project and the combinations the drivers refuse."""
import ctypes

import pytest
import torch

import agem_restatement as A

U = 2.0 ** -24
SIZES = [1, 3, 255, 256, 257, A.CHUNK - 1, A.CHUNK, A.CHUNK + 1, 2 * A.CHUNK + 5]


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------------------------------------------- the restatement
def _pair(kind):
    gen = torch.Generator().manual_seed(7)
    shapes = [(5,), (3, 4), (1,), (2, 3, 2)]
    rs = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    noise = [0.1 * torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    if kind == 'zero':
        return noise, [torch.zeros_like(r) for r in rs]
    k = -0.5 if kind == 'conflict' else 0.5
    return [n + k * r for n, r in zip(noise, rs)], rs


@pytest.mark.parametrize("kind", ["conflict", "agree", "zero"])
def test_restatement_is_the_formula_on_the_concatenated_vector(kind):
    gs, rs = _pair(kind)
    dot, rr, alpha, proj, abs_dot = A.project(gs, rs)
    g, r = torch.cat([x.reshape(-1) for x in gs]), torch.cat([x.reshape(-1) for x in rs])
    assert dot == pytest.approx(float(g @ r), rel=1e-13, abs=1e-300) and rr == pytest.approx(float(r @ r), rel=1e-13, abs=1e-300)
    assert abs_dot == pytest.approx(float((g * r).abs().sum()), rel=1e-13, abs=1e-300)
    want = g - (float(g @ r) / float(r @ r)) * r if kind == 'conflict' else g
    got = torch.cat(proj)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-15)
    if kind == 'conflict':
        assert alpha < 0 and abs(float(got @ r)) <= 1e-12 * abs_dot          # the projected gradient is orthogonal to r
        assert float(got @ got) < float(g @ g)
    else:
        assert alpha == 0.0 and torch.equal(got, g)
    assert [p.numel() for p in proj] == [x.numel() for x in gs]


@pytest.mark.parametrize("k", [-0.5, 0.5])
def test_gpu_inputs_decide_the_branch_far_outside_the_rounding_bound(k):
    gs, rs = A.inputs(SIZES, k, 11)
    assert all(g.dtype == torch.float32 and g.numel() == n for g, n in zip(gs, SIZES))
    dot, rr, alpha, _, abs_dot = A.project(gs, rs)
    bound = gamma(74) * abs_dot + U * abs(dot)
    assert abs(dot) > 100 * bound and rr > 0
    assert (dot < 0) == (k < 0) and (alpha < 0) == (k < 0)


# ------------------------------------------------------------------------------------------------------- MemorySampler
def _memory():
    def clip(i):
        return {'id': 'm%d' % i, 'video_id': 'm%d' % i, 'is_memory': False}
    shared = clip(2)
    return {0: [clip(0), clip(1), shared], 1: [shared, clip(3), clip(4)], 2: [clip(5), {'id': 'm0', 'video_id': 'm0'}, clip(6)]}


def _ids(batch):
    return [v['id'] for v in batch]


def test_memory_sampler():
    from vilco_amd.cl_methods.agem import MemorySampler
    mem = _memory()
    s = MemorySampler(mem, 2, seed=3)
    assert [v['id'] for v in s.items] == ['m%d' % i for i in range(7)], "de-duplicated by id, dataset order"
    assert all(v['is_memory'] is True for v in s.items)
    seq = [_ids(next(s)) for _ in range(9)]
    assert all(len(b) == 2 for b in seq)
    for e in range(3):          # 7 clips, batches of 2: three batches per epoch, the seventh clip of the permutation is dropped
        epoch = [i for b in seq[3 * e:3 * e + 3] for i in b]
        assert len(set(epoch)) == 6, "no clip twice within an epoch"
    assert seq[0:3] != seq[3:6], "every epoch draws its own permutation"
    again = MemorySampler(_memory(), 2, seed=3)
    assert [_ids(next(again)) for _ in range(9)] == seq, "the same (memory, batch_size, seed): the same sequence"
    other = MemorySampler(_memory(), 2, seed=4)
    assert [_ids(next(other)) for _ in range(9)] != seq, "another seed: another order"
    assert iter(s) is s
    # a batch size that divides the memory: every clip exactly once per epoch
    s7 = MemorySampler(_memory(), 7, seed=0)
    assert sorted(_ids(next(s7))) == sorted('m%d' % i for i in range(7))
    s1 = MemorySampler(_memory(), 1, seed=5)
    assert sorted(i for _ in range(7) for i in _ids(next(s1))) == sorted('m%d' % i for i in range(7))
    # a memory smaller than one batch is the batch
    small = MemorySampler({0: _memory()[0]}, 8, seed=1)
    for _ in range(3):
        assert sorted(_ids(next(small))) == ['m0', 'm1', 'm2']
    with pytest.raises(ValueError):
        MemorySampler({}, 2, seed=0)
    with pytest.raises(ValueError):
        MemorySampler(_memory(), 0, seed=0)


# ------------------------------------------------------------------------------------------------------- the C entry point
def test_agem_project_validates_on_the_host():
    """in the style of test_cabi_cpu.py::test_chunk_table_entry_points_validate_on_the_host: refused before anything is launched"""
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096
    ok = dict(ptrs=x, numel=x, chunk_tensor=x, chunk_off=x, n=1, nchunks=1, chunk=1024)
    assert lib.vilco_agem_project(None, x, x, None) == -1
    for bad in (dict(ptrs=None), dict(numel=None), dict(chunk_tensor=None), dict(chunk_off=None), dict(n=-1), dict(nchunks=-1),
                dict(chunk=0), dict(rows=1)):
        tb = ctypes.byref(_lib.ChunkTable(**dict(dict(ok, rows=2), **bad)))
        assert lib.vilco_agem_project(tb, x, x, None) == -1, bad
    tb = ctypes.byref(_lib.ChunkTable(rows=2, **ok))
    assert lib.vilco_agem_project(tb, None, x, None) == -1 and lib.vilco_agem_project(tb, x, None, None) == -1


def test_agem_project_op_refuses_host_tensors_and_mismatches():
    from vilco_amd import ops
    a, b = torch.zeros(4), torch.zeros(4)
    with pytest.raises(RuntimeError):
        ops.agem_project([a], [b])               # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.agem_project([a, a], [b])


# ------------------------------------------------------------------------------------------------------- the drivers
def test_drivers_refuse_what_is_not_supported():
    """the guards stand in front of everything that needs a device: no model, no stream"""
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import agem
    cfg = {'cl_cfg': {'name': 'agem', 'memory_size': 8, 'reg_lambda': 0.0}, 'opt': {'backbone_lr_weight': 1}}
    with pytest.raises(ValueError, match="data parallel"):
        train_cl.run_episodes(cfg, None, None, reducer=object())
    with pytest.raises(ValueError, match="run_episodes_bic"):
        train_cl.run_episodes_bic(cfg, None, None)
    with pytest.raises(ValueError, match="run_episodes_nlq"):
        train_cl.run_episodes_nlq(cfg, None, None, None, None)
    assert agem.check_supported('agem') is True and agem.check_supported('si', reducer=object()) is False
    assert agem.check_supported(None, driver='run_episodes_bic') is False


def test_train_one_epoch_keeps_its_defaults():
    import inspect
    from vilco_amd.utils.train_utils import train_one_epoch
    sig = inspect.signature(train_one_epoch)
    assert sig.parameters['agem'].default is None and list(sig.parameters)[-1] == 'agem'
