"""CPU: the fp64 restatement of the L2P prompt pool (tests/prompt_restatement.py) against the reference's recorded runs
(tests/golden/prompt_pool.npz, made by tests/golden/make_golden_prompt.py from MQ/libs/cl_methods/prompt.py), its tie rules
on hand-built ties, the launcher's limits, and the tensor-op body of vilco_amd.cl_methods.Prompt against the same file."""
import ctypes
import os

import numpy as np
import pytest
import torch

import parity_util  # noqa: F401  (puts tests/golden on the path)
import prompt_restatement as R
from make_golden_prompt import CASES, K, LEN, P

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prompt_pool.npz"))
ENTRIES = ('prompt_norm', 'x_embed_norm', 'similarity', 'selected_key', 'reduce_sim', 'prompted_embedding')
TOL = 1e-6          # fp32 reference against fp64: a few eps = 6e-8 of values of order 1 (sums over C = 96 and L <= 7)


def case(name):
    pre = name + '/'
    return {k[len(pre):]: GOLD[k] for k in GOLD.files if k.startswith(pre)}


def restate(name, g):
    ekey, mode, B, L, with_cls = CASES[name]
    return R.forward(g['x'], g['prompt'], g['key'], idx=g.get('window'), k=K, batchwise=(mode == 'vote'), embedding_key=ekey,
                     cls_features=g.get('cls'))


def test_golden_file_holds_only_decided_cases():
    assert float(GOLD['undecided_share']) == 0.0
    assert {k.split('/')[0] for k in GOLD.files if '/' in k} == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    g = case(name)
    ekey, mode, B, L, with_cls = CASES[name]
    got = restate(name, g)
    assert np.array_equal(got['prompt_idx'], g['prompt_idx'])
    assert got['total_prompt_len'] == int(g['total_prompt_len']) == K * LEN
    for k in ENTRIES:
        assert np.shape(got[k]) == g[k].shape, k
        assert np.max(np.abs(got[k] - g[k])) < TOL, (k, np.max(np.abs(got[k] - g[k])))
    # gradients of prompted.square().sum() - 0.1 reduce_sim
    dp, dk, dx = R.backward(g['x'], g['prompt'], g['key'], got, 2.0 * got['prompted_embedding'], -0.1, embedding_key=ekey,
                            cls_given=with_cls)
    for a, b, n in ((dp, g['d_prompt'], 'd_prompt'), (dk, g['d_key'], 'd_key'), (dx, g['d_x'], 'd_x')):
        assert np.max(np.abs(a - b)) < TOL * max(1.0, np.max(np.abs(b))), (n, np.max(np.abs(a - b)))


def test_equal_similarities_go_to_the_smaller_index():
    assert R.top_by_rank(np.array([0.5, 0.7, 0.5, 0.7, 0.1]), 3).tolist() == [1, 3, 0]
    assert R.rank_desc(np.array([2, 2, 3, 2])).tolist() == [1, 2, 0, 3]
    # two identical keys: the earlier one is picked first, on every row
    rng = np.random.RandomState(0)
    key = rng.uniform(-1, 1, (5, 8))
    key[3] = key[1]
    x = np.broadcast_to(key[1], (2, 3, 8)).copy()
    out = R.forward(x, rng.uniform(-1, 1, (5, 2, 8)), key, k=2, batchwise=False)
    assert out['prompt_idx'].tolist() == [[1, 3], [1, 3]]


def test_an_all_zero_text_row_picks_the_first_prompts():
    rng = np.random.RandomState(1)
    x = np.zeros((1, 4, 8))
    out = R.forward(x, rng.uniform(-1, 1, (6, 2, 8)), rng.uniform(-1, 1, (6, 8)), k=3, batchwise=False)
    assert np.all(out['similarity'] == 0.0) and out['prompt_idx'].tolist() == [[0, 1, 2]]
    assert out['reduce_sim'] == 0.0


def test_equal_counts_at_batch_two_go_to_the_smaller_id():
    # rows pick {4, 2, 0} and {4, 3, 1}: counts 4 -> 2, every other picked id -> 1: the vote keeps 4, then 0 and 1
    sim = np.array([[0.3, 0.0, 0.5, 0.0, 0.9, -1.0],
                    [0.0, 0.2, 0.0, 0.6, 0.9, -1.0]])
    assert R.select(sim, 3, False).tolist() == [[4, 2, 0], [4, 3, 1]]
    assert R.select(sim, 3, True).tolist() == [[4, 0, 1], [4, 0, 1]]


def test_launcher_rejects_each_limit_violation_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                # dummy, suitably aligned addresses: every check precedes any device work

    def call(**kw):
        f = dict(x=x, prompt=x, key=x, idx=x, sim=x, pn=x, xn=x, selkey=x, prompted=x, reduce_sim=x, workspace=x,
                 workspace_bytes=1 << 40, B=2, L=7, C=96, P=10, len=5, k=4, key_mode=0, vote=1)
        f.update(kw)
        return lib.vilco_prompt_fwd(ctypes.byref(_lib.PromptDesc(**f)), None)
    assert lib.vilco_prompt_fwd(None, None) == -1
    for bad in (dict(k=0), dict(k=11), dict(P=65, k=4), dict(P=0, k=0), dict(len=0), dict(B=0), dict(L=0), dict(C=0),
                dict(key_mode=4), dict(key_mode=-1), dict(key_mode=3), dict(x=None), dict(prompted=None), dict(workspace=None)):
        assert call(**bad) == -1, bad
    assert call(P=64, k=64, workspace_bytes=16) == -4          # the pool limit itself is legal: it gets as far as the workspace
    d = _lib.PromptDesc(B=2, L=7, C=96, P=10, len=5, k=4)
    assert lib.vilco_prompt_workspace(ctypes.byref(d)) >= 2 * 96 * 8 + (2 + 10) * 4 + 2 * 4 * 4
    g = _lib.PromptDesc(x=x, prompt=x, key=x, idx=x, sim=x, pn=x, xn=x, selkey=x, prompted=x, reduce_sim=x, workspace=x,
                        workspace_bytes=1 << 40, B=2, L=7, C=96, P=10, len=5, k=11)
    assert lib.vilco_prompt_bwd(ctypes.byref(g), x, x, x, x, x, None) == -1


def test_op_refuses_cpu_tensors_and_the_fifth_key_raises():
    from vilco_amd import ops
    from vilco_amd.cl_methods import Prompt
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.prompt_pool(torch.zeros(2, 3, 8), torch.zeros(4, 2, 8), torch.zeros(4, 8), top_k=2)
    mod = Prompt(length=2, embed_dim=8, embedding_key='median', prompt_pool=True, prompt_key=True, pool_size=4, top_k=2)
    with pytest.raises(NotImplementedError, match="embedding keys"):
        mod(torch.zeros(2, 3, 8))
    with pytest.raises(NotImplementedError):
        Prompt(length=2, embed_dim=8, prompt_pool=False)


@pytest.mark.parametrize("name", sorted(CASES))
def test_module_tensor_op_body_matches_the_reference_on_cpu(name, monkeypatch):
    """VILCO_FUSED_PROMPT=0 (ops.fused_prompt False) keeps the tensor-op body; CPU tensors take it in any case"""
    from vilco_amd import ops
    from vilco_amd.cl_methods import Prompt
    monkeypatch.setattr(ops, "fused_prompt", False)
    g = case(name)
    ekey, mode, B, L, with_cls = CASES[name]
    mod = Prompt(length=LEN, embed_dim=g['x'].shape[2], embedding_key=ekey, prompt_pool=True, prompt_key=True, pool_size=P,
                 top_k=K, batchwise_prompt=(mode == 'vote'))
    with torch.no_grad():
        mod.prompt.copy_(torch.from_numpy(g['prompt']))
        mod.prompt_key.copy_(torch.from_numpy(g['key']))
    x = torch.from_numpy(g['x']).clone().requires_grad_(True)
    res = mod(x, prompt_mask=torch.from_numpy(g['window']) if 'window' in g else None,
              cls_features=torch.from_numpy(g['cls']) if 'cls' in g else None)
    assert sorted(res) == sorted(ENTRIES + ('prompt_idx', 'total_prompt_len'))
    assert res['prompt_idx'].dtype == torch.int64 and np.array_equal(res['prompt_idx'].numpy(), g['prompt_idx'])
    assert res['total_prompt_len'] == int(g['total_prompt_len'])
    for k in ENTRIES:
        assert res[k].dtype == torch.float32 and tuple(res[k].shape) == g[k].shape, k
        assert np.max(np.abs(res[k].detach().numpy() - g[k])) < TOL, k
    (res['prompted_embedding'].square().sum() - 0.1 * res['reduce_sim']).backward()
    for a, n in ((mod.prompt.grad, 'd_prompt'), (mod.prompt_key.grad, 'd_key'), (x.grad, 'd_x')):
        assert np.max(np.abs(a.numpy() - g[n])) < TOL * max(1.0, np.max(np.abs(g[n]))), n
