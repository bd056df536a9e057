"""CPU: CODA-Prompt (vilco_amd/cl_methods/coda.py, ops.coda_prompt's host side, the model / config / driver wiring).

  * the float64 restatement's hand-derived gradients (tests/coda_restatement.py) against torch float64 autograd of the forward
    written with einsum / F.normalize / .detach() -- what ties the formulas to something not derived by hand;
  * the module's tensor-op body (CPU fp32) against the restatement;
  * set_task: Gram-Schmidt rows, frozen rows, seeds;  config, model, optimizer groups, drivers;  the C ABI rows."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import coda_restatement as R
from parity_util import golden_cfg, load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _inputs(B, L, C, M, length, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(B, L, C, generator=g, dtype=dtype)
    prompt = torch.rand(M, length, C, generator=g, dtype=dtype) * 2 - 1
    key = torch.rand(M, C, generator=g, dtype=dtype) * 2 - 1
    attn = torch.rand(M, C, generator=g, dtype=dtype) * 2 - 1
    gp = torch.randn(B, length + L, C, generator=g, dtype=dtype)
    return x, prompt, key, attn, gp


def _torch_forward(x, prompt, key, attn, s, f, want_ortho):
    """the method in tensor ops: rows [0, s) detached, rows [s, f) live, the query a constant"""
    def used(p):
        return torch.cat([p[:s].detach(), p[s:f]], dim=0)
    P, K, A = used(prompt), used(key), used(attn)
    xk = x.detach().mean(dim=1)
    a = torch.einsum('bmc,mc->bm', F.normalize(torch.einsum('bc,mc->bmc', xk, A), dim=2), F.normalize(K, dim=1))
    prompted = torch.cat([torch.einsum('bm,mtc->btc', a, P), x], dim=1)

    def pen(t):
        g = t @ t.t() - torch.eye(t.shape[0], dtype=t.dtype)
        return (g * g).mean()
    ortho = pen(K) + pen(A) + pen(P.reshape(f, -1)) if want_ortho else torch.zeros((), dtype=x.dtype)
    return prompted, ortho, a


CASES = [(1, 1, 6, 1, 1, 0, 1), (3, 5, 7, 4, 2, 0, 4), (2, 5, 24, 10, 3, 4, 6), (3, 7, 16, 10, 5, 9, 10), (2, 3, 12, 6, 2, 2, 4)]


@pytest.mark.parametrize("B,L,C,M,length,s,f", CASES)
@pytest.mark.parametrize("want_ortho", [False, True])
def test_restatement_gradients_equal_float64_autograd(B, L, C, M, length, s, f, want_ortho):
    x, prompt, key, attn, gp = _inputs(B, L, C, M, length)
    g_ortho = 0.37
    leaves = [t.clone().requires_grad_(True) for t in (x, prompt, key, attn)]
    prompted, ortho, a = _torch_forward(*leaves, s, f, want_ortho)
    ((prompted * gp).sum() + g_ortho * ortho).backward()
    fw = R.forward(x, prompt, key, attn, s, f, want_ortho)
    assert rel_err(prompted, torch.from_numpy(fw['prompted'])) < 1e-13
    assert rel_err(a, torch.from_numpy(fw['alpha'][:, :f])) < 1e-13 and not fw['alpha'][:, f:].any()
    assert abs(float(ortho.detach()) - fw['ortho']) <= 1e-13 * max(fw['ortho'], 1.0)
    got = R.backward(x, prompt, key, attn, s, f, gp, g_ortho, want_ortho)
    for name, mine, leaf in zip(('d_prompt', 'd_key', 'd_attn'), got[:3], leaves[1:]):
        want = leaf.grad
        assert rel_err(torch.from_numpy(mine), want) < 1e-10, name
        live = np.zeros(M, dtype=bool)
        live[s:f] = True
        assert not mine[~live].any() and not want[torch.from_numpy(~live)].any(), name      # frozen / unused rows: exact zeros
    assert np.array_equal(got[3], leaves[0].grad.numpy()) and np.array_equal(got[3], gp[:, length:].numpy())


def test_restatement_norms_below_the_clamp_follow_autograd():
    """an all-zero query row and an all-zero key: alpha is an exact 0 and the gradients are autograd's (the clamp's constant)"""
    x, prompt, key, attn, gp = _inputs(2, 3, 8, 4, 2, seed=5)
    x[1] = 0.0
    key[2] = 0.0
    leaves = [t.clone().requires_grad_(True) for t in (x, prompt, key, attn)]
    prompted, ortho, a = _torch_forward(*leaves, 1, 4, True)
    ((prompted * gp).sum() + 0.2 * ortho).backward()
    fw = R.forward(x, prompt, key, attn, 1, 4, True)
    assert not fw['alpha'][1].any() and not fw['alpha'][:, 2].any() and np.isfinite(fw['prompted']).all()
    got = R.backward(x, prompt, key, attn, 1, 4, gp, 0.2, True)
    for mine, leaf in zip(got[:3], leaves[1:]):
        assert np.isfinite(mine).all() and rel_err(torch.from_numpy(mine), leaf.grad) < 1e-10


def _module(M, length, C, n_tasks, ortho, x, prompt, key, attn):
    from vilco_amd.cl_methods import CodaPrompt
    mod = CodaPrompt(M, length, C, n_tasks, ortho=ortho)
    with torch.no_grad():
        mod.prompt.copy_(prompt)
        mod.prompt_key.copy_(key)
        mod.prompt_attn.copy_(attn)
    return mod


@pytest.mark.parametrize("C", [6, 24])
@pytest.mark.parametrize("task,train", [(0, True), (1, True), (2, True), (1, False)])
def test_tensor_op_body_equals_the_restatement(C, task, train):
    """CPU fp32 against float64.  Bar 1e-5 of a tensor's largest element: dot products of C <= 24 (len C <= 72 for the prompt's
    Gram) fp32 terms and at most four chained stages, n u = 72 * 6e-8 = 4e-6 per stage at the very worst."""
    B, L, M, length, n_tasks = 3, 5, 6, 3, 3
    x, prompt, key, attn, gp = _inputs(B, L, C, M, length, seed=C, dtype=torch.float32)
    mod = _module(M, length, C, n_tasks, True, x, prompt, key, attn)
    if not train:
        mod.task_count.fill_(task)
        mod._task = task
    pt = M // n_tasks
    s, f = (task * pt, (task + 1) * pt) if train else ((task + 1) * pt - 1, (task + 1) * pt)
    xin = x.clone().requires_grad_(True)
    res = mod(xin, task_id=task, train=train)
    assert res['total_prompt_len'] == length and set(res) >= {'prompted_embedding', 'total_prompt_len', 'ortho'}
    fw = R.forward(x, prompt, key, attn, s, f, want_ortho=train)
    assert rel_err(res['prompted_embedding'], torch.from_numpy(fw['prompted'])) < 1e-5
    assert torch.equal(res['prompted_embedding'][:, length:], x)
    assert rel_err(res['alpha'], torch.from_numpy(fw['alpha'])) < 1e-5 and not res['alpha'][:, f:].any()
    if not train:
        assert float(res['ortho']) == 0.0                            # the penalty is a training term
        return
    assert abs(float(res['ortho']) - fw['ortho']) < 1e-5 * fw['ortho']
    ((res['prompted_embedding'] * gp).sum() + 0.3 * res['ortho']).backward()
    want = R.backward(x, prompt, key, attn, s, f, gp, 0.3, True)
    for p, w in zip((mod.prompt, mod.prompt_key, mod.prompt_attn), want[:3]):
        assert rel_err(p.grad, torch.from_numpy(w)) < 1e-5
        assert not p.grad[:s].any() and not p.grad[f:].any()
    assert torch.equal(xin.grad, gp[:, length:])


def test_a_task_outside_the_division_raises_while_training():
    x, prompt, key, attn, _ = _inputs(1, 2, 6, 4, 1, dtype=torch.float32)
    mod = _module(4, 1, 6, 2, False, x, prompt, key, attn)
    for bad in (-1, 2, 7):
        with pytest.raises(ValueError, match="task"):
            mod(x, task_id=bad, train=True)
    mod(x, task_id=-1, train=False)                                  # eval does not look at task_id
    with pytest.raises(ValueError):
        mod.set_task(2)


def test_set_task_rows_are_orthonormal_frozen_and_seeded():
    """Every new row q is the fp32 rounding of a float64 unit vector v that is orthogonal (to ~1e-15) to all STORED earlier
    rows e_j, |e_j| <= 1 + u.  Rounding moves element c by at most u |v_c|, so | |q| - 1 | <= u and |<q, e_j>| <= u sum_c |v_c|
    |e_jc| <= u |v| |e_j| <= u (1 + u): the bound below is 1.01 u + 1e-14 for both."""
    from vilco_amd.cl_methods import CodaPrompt
    M, length, C, n = 12, 3, 16, 4
    mod = CodaPrompt(M, length, C, n, seed=7)
    assert int(mod.task_count) == 0 and mod.set_task_calls == 1
    bound = 1.01 * U + 1e-14
    snaps = []
    for t in range(n):
        if t:
            mod.set_task(t)
        assert int(mod.task_count) == t and mod.task_count.dtype == torch.int64
        f = (t + 1) * (M // n)
        for p in (mod.prompt, mod.prompt_key, mod.prompt_attn):
            rows = p.detach().reshape(M, -1).double()
            assert p.dtype == torch.float32
            gram = rows[:f] @ rows[:f].t()
            assert (gram.diagonal().sqrt() - 1).abs().max() <= bound
            assert (gram - torch.diag(gram.diagonal())).abs().max() <= bound
            assert not rows[f:].any()                                # later tasks' rows are untouched (zeros) until their turn
        now = [p.detach().clone() for p in (mod.prompt, mod.prompt_key, mod.prompt_attn)]
        if snaps:
            s = t * (M // n)
            assert all(torch.equal(a[:s], b[:s]) for a, b in zip(snaps, now)), "earlier rows keep their bits"
        snaps = now
    twin = CodaPrompt(M, length, C, n, seed=7)
    for t in range(1, n):
        twin.set_task(t)
    assert all(torch.equal(a, b) for a, b in zip(snaps, (twin.prompt, twin.prompt_key, twin.prompt_attn))), "same seed, same bits"
    other = CodaPrompt(M, length, C, n, seed=8)
    assert not torch.equal(other.prompt_key[:3], twin.prompt_key[:3])
    # set_task(t) again redraws the same rows: the generator is seeded with seed + t
    before = twin.prompt_key.detach().clone()
    twin.set_task(n - 1)
    assert torch.equal(before, twin.prompt_key)


def test_config_defaults_carry_the_coda_keys():
    from vilco_amd.core import config as c
    cfg = c.make_config()
    want = {'prompt_type': 'l2p', 'coda_tasks': None, 'coda_ortho_mu': 0.0, 'coda_seed': 0}
    for k, v in want.items():
        assert cfg['cl_cfg'][k] == v and cfg['model']['cl_cfg'][k] == v and k not in c.DEFAULTS['cl_cfg']
        assert c.EXTRA_DEFAULTS['cl_cfg'][k] == v
    got = c.make_config(cl_cfg=dict(prompt_type='coda', coda_tasks=5))['cl_cfg']
    assert got['prompt_type'] == 'coda' and got['coda_tasks'] == 5 and got['coda_ortho_mu'] == 0.0


def _coda_model(**cl):
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_golden("prompt")
    over = dict(gold['overrides'])
    over['cl_cfg'] = dict(over.get('cl_cfg', {}), **cl)
    m = make_config(**over)['model']
    kw = dict(m)
    if m['use_xl']:
        kw['xlnet_config'] = xlnet_json(m['embd_dim'], 4)
    return vm.make_meta_arch('LocPointTransformer', **kw), gold


def test_model_builds_a_coda_prompt_or_says_why_not():
    from vilco_amd.cl_methods import CodaPrompt, Prompt
    from vilco_amd.utils.train_utils import param_groups
    model, gold = _coda_model(prompt_type='coda', coda_tasks=5, coda_ortho_mu=0.1, coda_seed=3)
    pool = golden_cfg(gold)['cl_cfg']['pool_size']
    assert isinstance(model.prompt, CodaPrompt) and model.prompt.n_tasks == 5 and model.prompt.per_task == pool // 5
    assert model.prompt.want_ortho and model.prompt.seed == 3 and model.coda_ortho_mu == 0.1
    keys = [k for k in model.state_dict() if k.startswith('prompt.')]
    assert sorted(keys) == ['prompt.prompt', 'prompt.prompt_attn', 'prompt.prompt_key', 'prompt.task_count']
    decay, no_decay, remain = param_groups(model)
    for n in ('prompt.prompt', 'prompt.prompt_key', 'prompt.prompt_attn'):
        assert n in no_decay and n not in decay and n not in remain
    # a reloaded checkpoint knows its f
    model.prompt.set_task(2)
    twin, _ = _coda_model(prompt_type='coda', coda_tasks=5)
    twin.load_state_dict(model.state_dict())
    assert int(twin.prompt.task_count) == 2 and twin.prompt._task == 2
    for bad, match in ((dict(prompt_type='coda'), "coda_tasks"), (dict(prompt_type='coda', coda_tasks=3), "multiple"),
                       (dict(prompt_type='coda', coda_tasks=0), "coda_tasks"), (dict(prompt_type='soft'), "prompt_type")):
        with pytest.raises(ValueError, match=match):
            _coda_model(**bad)
    # the L2P model is what it was: its prompt parameters stay in the weight-decayed remainder
    l2p, _ = _coda_model()
    assert isinstance(l2p.prompt, Prompt) and not isinstance(l2p.prompt, CodaPrompt)
    d2, n2, r2 = param_groups(l2p)
    assert 'prompt.prompt' in r2 and 'prompt.prompt_key' in r2
    assert sorted(n for n in no_decay if not n.startswith('prompt.')) == n2 and decay == d2
    assert sorted(n for n in remain) == sorted(n for n in r2 if not n.startswith('prompt.'))


def test_cl_terms_add_the_penalty_and_leave_the_pull_term_out():
    import types
    from vilco_amd.modeling.meta_archs import PtTransformer
    stub = types.SimpleNamespace(n_known=2, cl_name='l2p', _coda_ortho=torch.tensor(0.5), coda_ortho_mu=0.1)
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), [], [], None)
    assert abs(float(out['final_loss']) - 1.05) < 1e-7 and abs(float(out['ortho_loss']) - 0.05) < 1e-8
    stub.coda_ortho_mu = 0.0
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), [], [], None)
    assert float(out['final_loss']) == 1.0 and 'ortho_loss' not in out
    # L2P as before
    stub._coda_ortho = None
    out = PtTransformer._cl_terms(stub, {}, torch.tensor(1.0), [], [], torch.tensor(2.0))
    assert abs(float(out['final_loss']) - 0.8) < 1e-7


def test_check_supported_and_the_refused_drivers():
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import coda
    from vilco_amd.core.config import make_config
    assert coda.check_supported('l2p') is False and coda.check_supported('coda') is True
    assert coda.check_supported('l2p', reducer=object(), driver='run_episodes_bic') is False
    for driver in ('run_episodes_bic', 'run_episodes_nlq'):
        with pytest.raises(ValueError, match=driver):
            coda.check_supported('coda', driver=driver)
    with pytest.raises(ValueError, match="reducer"):
        coda.check_supported('coda', reducer=object())
    cfg = make_config(cl_cfg=dict(prompt_pool=True, prompt_type='coda', coda_tasks=2))
    with pytest.raises(ValueError, match="run_episodes_bic"):
        train_cl.run_episodes_bic(cfg, None, None)
    with pytest.raises(ValueError, match="run_episodes_nlq"):
        train_cl.run_episodes_nlq(cfg, None, None, None, None)
    with pytest.raises(ValueError, match="reducer"):
        train_cl.run_episodes(cfg, None, None, reducer=object())


def test_op_refuses_cpu_tensors():
    from vilco_amd import ops
    x, prompt, key, attn, _ = _inputs(1, 2, 8, 4, 2, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.coda_prompt(x, prompt, key, attn, 0, 2, False)


def test_cabi_rows_exist_and_the_mirror_has_the_struct_s_size():
    from vilco_amd import _lib
    text = open(os.path.join(ROOT, "include", "vilco_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("vilco_coda_workspace", "vilco_coda_fwd", "vilco_coda_bwd"):
        assert n in _lib.SIGNATURES and n + "(" in text and hasattr(lib, n), n
    assert _lib.CodaDesc._cname_ == "vilco_coda_desc" and "} vilco_coda_desc;" in text
    assert ctypes.sizeof(_lib.CodaDesc) == _lib.load().vilco_abi_sizeof(b"vilco_coda_desc") == 104
    body = text[text.index("typedef struct vilco_coda_desc {"):text.index("} vilco_coda_desc;")]
    order = [n for n, _ in _lib.CodaDesc._fields_]
    pos = [body.index(" " + n + ("," if n in ("B", "L", "C", "M", "s") else ";")) for n in order]
    assert pos == sorted(pos), "the mirror lists the fields in the header's order"


def test_entry_points_validate_on_the_host():
    """BADARG before any device work: !(1 <= f <= M <= 128), !(0 <= s < f), len / B / L / C < 1, null operands; a short
    workspace is its own status"""
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                                                     # dummy, suitably aligned addresses
    ok = dict(x=x, prompt=x, key=x, attn=x, B=2, L=5, C=24, M=10, len=3, s=2, f=4, want_ortho=1, alpha=x, prompted=x, ortho=x,
              workspace=x)
    nws = lib.vilco_coda_workspace(ctypes.byref(_lib.CodaDesc(**ok)))
    assert nws >= 8 * (2 * 24 + 3 * 2 * 10 + 10 + 3 * 100) and lib.vilco_coda_workspace(None) == 0

    def fwd(**kw):
        return lib.vilco_coda_fwd(ctypes.byref(_lib.CodaDesc(**dict(ok, **dict(dict(workspace_bytes=nws), **kw)))), None)

    def bwd(g=x, go=x, dp=x, dk=x, da=x, **kw):
        return lib.vilco_coda_bwd(ctypes.byref(_lib.CodaDesc(**dict(ok, **dict(dict(workspace_bytes=nws), **kw)))), g, go, dp, dk, da, None)
    bads = [dict(f=0), dict(f=11), dict(M=129, f=4), dict(M=0, f=0, s=0), dict(s=-1), dict(s=4), dict(s=5), dict(len=0), dict(B=0),
            dict(L=0), dict(C=0), dict(C=-3), dict(x=None), dict(prompt=None), dict(key=None), dict(attn=None), dict(alpha=None),
            dict(prompted=None), dict(ortho=None), dict(workspace=None), dict(workspace=x + 8)]
    for call in (fwd, bwd):
        for bad in bads:
            assert call(**bad) == -1, (call.__name__, bad)
        assert call(workspace_bytes=nws - 1) == -4, call.__name__
    assert lib.vilco_coda_fwd(None, None) == -1 and lib.vilco_coda_bwd(None, x, x, x, x, x, None) == -1
    assert bwd(g=None) == -1 and bwd(go=None) == -1
    assert bwd(go=None, want_ortho=0, dp=None, dk=None, da=None) == 0        # nothing asked for: nothing launched
