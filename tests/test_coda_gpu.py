"""GPU: ops.coda_prompt (csrc/coda.hip) against the float64 restatement (tests/coda_restatement.py, tied to autograd by
test_coda_cpu.py), its footprint, determinism, graph capture, and the op inside the model and the episode loop.

Tolerance, counted.  Every kernel accumulates its fp32 inputs in fp64 and rounds ONCE per stored value.  alpha is written
twice by the forward: rounded to fp32 for the caller, and in fp64 into the workspace; the prompt rows, d_prompt, d_key and
d_attn are all computed from the fp64 copy (with the fp64 query, norms and g_alpha that sit next to it), so NO output passes
through an fp32 intermediate: alpha, the prompt rows of `prompted`, ortho and the three gradients each carry one rounding to
fp32, |got - want| <= u |want|, u = 2^-24.  On top of it the fp64 arithmetic's own error: a sum of n terms is off by at most
n 2^-53 sum |terms|; the longest sums here have n = len C <= 6144 < 2^13 terms and at most three are chained (query, cosine,
gradient), and for the random inputs of this file sum |terms| stays below 2^7 times the tensor's largest element (sqrt(n)
growth of a random sum, n < 2^14): 3 * 2^13 * 2^-53 * 2^7 < 2^-31.  Bound per element, for every compared quantity:

    |got - want| <= 2^-24 |want| + 2^-30 max |want|

The x rows of `prompted` and d_x are bit copies; rows outside [s, f) of the gradients and columns >= f of alpha are exact
zeros.  Cross-check on the same inputs: the op's largest error per quantity may not exceed twice that of the fp32 tensor-op
body (CodaPrompt._forward_tensor_ops on the device)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import coda_restatement as R
from parity_util import GRAD_FLOOR, cases, episode_full_state, golden_cfg, golden_inputs, load_episode_golden, load_golden, rel_err

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SLACK = 2.0 ** -30
QUANT = ('alpha', 'p', 'ortho', 'd_prompt', 'd_key', 'd_attn')

# (C, L, B, len, M, s, f): C below / off / at the vector width, L and B at 1 and above, one and several workgroups, every kind
# of window -- the first component alone, the whole pool, the last component alone, a middle task (pt, 2 pt)
GRID = [(6, 1, 1, 1, 1, 0, 1), (6, 5, 3, 5, 4, 0, 4), (6, 77, 1, 8, 10, 9, 10), (6, 5, 3, 1, 10, 2, 4), (6, 77, 3, 8, 128, 0, 128),
        (67, 1, 3, 1, 4, 0, 1), (67, 5, 1, 5, 10, 0, 10), (67, 77, 3, 8, 4, 3, 4), (67, 5, 3, 5, 10, 2, 4), (67, 77, 1, 8, 128, 32, 64),
        (67, 1, 1, 8, 4, 0, 4), (768, 1, 1, 1, 1, 0, 1), (768, 5, 3, 5, 4, 1, 2), (768, 77, 3, 8, 10, 0, 10), (768, 77, 1, 8, 10, 9, 10),
        (768, 5, 1, 8, 10, 2, 4), (768, 77, 3, 8, 128, 0, 1), (768, 5, 3, 1, 128, 127, 128), (768, 1, 1, 5, 128, 0, 128),
        (768, 77, 3, 8, 128, 32, 64)]
G_ORTHO = 0.375          # exact in fp32: the op is handed its gradient as an fp32 scalar


def make_inputs(C, L, B, length, M, seed=0):
    g = torch.Generator().manual_seed(zlib.crc32(repr((C, L, B, length, M, seed)).encode()) % (1 << 30))
    x = torch.randn(B, L, C, generator=g)
    prompt = 2 * torch.rand(M, length, C, generator=g) - 1
    key = 2 * torch.rand(M, C, generator=g) - 1
    attn = 2 * torch.rand(M, C, generator=g) - 1
    gp = torch.randn(B, length + L, C, generator=g)
    return dict(x=x, prompt=prompt, key=key, attn=attn, gp=gp)


_WANT = {}


def want_for(case, want_ortho):
    """inputs and the restatement's answer, computed once per case and shared"""
    k = (case, want_ortho)
    if k not in _WANT:
        C, L, B, length, M, s, f = case
        inp = make_inputs(C, L, B, length, M)
        a = [inp[n].numpy() for n in ('x', 'prompt', 'key', 'attn')]
        fw = R.forward(*a, s, f, want_ortho)
        assert fw['norm_u'].min() > 1e-3 and fw['norm_k'].min() > 1e-3, "no case sits at the clamp"
        bw = R.backward(*a, s, f, inp['gp'].numpy(), G_ORTHO, want_ortho)
        _WANT[k] = (inp, fw, bw)
    return _WANT[k]


def run_op(dev, inp, s, f, want_ortho):
    from vilco_amd import ops
    leaves = [inp[n].to(dev).requires_grad_(True) for n in ('x', 'prompt', 'key', 'attn')]
    prompted, ortho, alpha = ops.coda_prompt(*leaves, s, f, want_ortho)
    ((prompted * inp['gp'].to(dev)).sum() + G_ORTHO * ortho).backward()
    return prompted.detach(), ortho.detach(), alpha, [t.grad for t in leaves]


def run_tensor_ops(dev, inp, s, f, want_ortho):
    """the module's tensor-op body on the device over the case's tensors (a stand-in for `self`: the module's constructor would
    orthogonalise its rows, which M > C does not allow)"""
    import types
    from vilco_amd.cl_methods import CodaPrompt
    x, prompt, key, attn = (inp[n].to(dev).requires_grad_(True) for n in ('x', 'prompt', 'key', 'attn'))
    stub = types.SimpleNamespace(prompt=prompt, prompt_key=key, prompt_attn=attn, pool_size=prompt.shape[0], _penalty=CodaPrompt._penalty)
    prompted, ortho, alpha = CodaPrompt._forward_tensor_ops(stub, x, s, f, want_ortho)
    ((prompted * inp['gp'].to(dev)).sum() + G_ORTHO * ortho).backward()
    return prompted.detach(), ortho.detach(), alpha, [x.grad, prompt.grad, key.grad, attn.grad]


def quantities(out, length):
    prompted, ortho, alpha, grads = out
    return {'alpha': alpha, 'p': prompted[:, :length], 'ortho': ortho.reshape(1), 'd_prompt': grads[1], 'd_key': grads[2],
            'd_attn': grads[3]}


@pytest.mark.parametrize("want_ortho", [0, 1])
@pytest.mark.parametrize("case", GRID, ids=lambda c: "C%d-L%d-B%d-len%d-M%d-s%d-f%d" % c)
def test_values_copies_and_zero_rows_over_the_shape_grid(dev, case, want_ortho):
    C, L, B, length, M, s, f = case
    inp, fw, bw = want_for(case, bool(want_ortho))
    out = run_op(dev, inp, s, f, bool(want_ortho))
    prompted, ortho, alpha, grads = out
    assert prompted.shape == (B, length + L, C) and alpha.shape == (B, M) and ortho.dim() == 0
    # bit copies
    assert torch.equal(prompted[:, length:].cpu(), inp['x']) and torch.equal(grads[0].cpu(), inp['gp'][:, length:])
    # exact zeros
    assert not alpha[:, f:].any().item()
    for g in grads[1:]:
        assert not g[:s].any().item() and not g[f:].any().item()
    if not want_ortho:
        assert ortho.item() == 0.0
    want = {'alpha': fw['alpha'], 'p': fw['p'], 'ortho': np.array([fw['ortho']]), 'd_prompt': bw[0], 'd_key': bw[1], 'd_attn': bw[2]}
    mine, body = quantities(out, length), quantities(run_tensor_ops(dev, inp, s, f, bool(want_ortho)), length)
    line = []
    for q in QUANT:
        w = want[q]
        err = np.abs(mine[q].detach().double().cpu().numpy() - w)
        berr = np.abs(body[q].detach().double().cpu().numpy() - w)
        bound = U * np.abs(w) + SLACK * np.abs(w).max()
        line.append("%s %.1e/%.1e" % (q, err.max(), berr.max()))
        assert (err <= bound).all(), (q, case, float((err - bound).max()), float(err.max()), float(np.abs(w).max()))
        assert err.max() <= 2 * berr.max(), (q, case, float(err.max()), float(berr.max()))
    print(case, want_ortho, "max |err| op/tensor ops:", " ".join(line))


def test_an_all_zero_query_gives_an_exact_zero_weight_and_a_finite_prompt(dev):
    inp = make_inputs(768, 5, 3, 8, 10, seed=1)
    inp['x'][1] = 0.0
    prompted, ortho, alpha, grads = run_op(dev, inp, 2, 6, True)
    assert not alpha[1].any().item() and alpha[0, :6].abs().min().item() > 0
    assert torch.isfinite(prompted).all().item() and not prompted[1, :8].any().item()
    assert all(torch.isfinite(g).all().item() for g in grads)
    w = R.backward(*[inp[n].numpy() for n in ('x', 'prompt', 'key', 'attn')], 2, 6, inp['gp'].numpy(), G_ORTHO, True)
    for g, ww in zip(grads[1:], w[:3]):
        assert (np.abs(g.double().cpu().numpy() - ww) <= U * np.abs(ww) + SLACK * np.abs(ww).max()).all()


SENT = -1234.5


def _raw(dev, inp, s, f, want_ortho, guard=64):
    """the C entry points over guard-banded buffers (the workspace too) -> the outputs' contents"""
    from vilco_amd import _lib, ops
    lib = _lib.load()
    x, prompt, key, attn = (inp[n].to(dev).contiguous() for n in ('x', 'prompt', 'key', 'attn'))
    B, L, C = x.shape
    M, length = prompt.shape[:2]
    d = ops._coda_desc(x, prompt, key, attn, s, f, want_ortho)

    def banded(n):
        buf = torch.full((n + 2 * guard,), SENT, dtype=torch.float32, device=dev)
        return buf, buf[guard:guard + n]
    bufs = {n: banded(sz) for n, sz in (('alpha', B * M), ('prompted', B * (length + L) * C), ('ortho', 1),
                                        ('d_prompt', M * length * C), ('d_key', M * C), ('d_attn', M * C))}
    nws = lib.vilco_coda_workspace(ctypes.byref(d))
    ws = torch.full((nws + 512,), 0x5A, dtype=torch.uint8, device=dev)          # 256 bytes of band on either side
    assert ws.data_ptr() % 256 == 0
    for n in ('alpha', 'prompted', 'ortho'):
        setattr(d, n, bufs[n][1].data_ptr())
    d.workspace, d.workspace_bytes = ws.data_ptr() + 256, nws
    _lib.check(lib.vilco_coda_fwd(ctypes.byref(d), None))
    gp, go = inp['gp'].to(dev).contiguous(), torch.full((1,), G_ORTHO, device=dev)
    _lib.check(lib.vilco_coda_bwd(ctypes.byref(d), gp.data_ptr(), go.data_ptr(), bufs['d_prompt'][1].data_ptr(),
                                  bufs['d_key'][1].data_ptr(), bufs['d_attn'][1].data_ptr(), None))
    torch.cuda.synchronize()
    for n, (buf, view) in bufs.items():
        band = torch.cat([buf[:guard], buf[guard + view.numel():]])
        assert torch.equal(band, torch.full_like(band, SENT)), n
        assert not (view == SENT).any().item(), n                     # ... and every element inside was written
    assert (ws[:256] == 0x5A).all().item() and (ws[256 + nws:] == 0x5A).all().item(), "workspace bands"
    return {n: v[1].clone() for n, v in bufs.items()}


@pytest.mark.parametrize("C,L,B,length,M,s,f", [(6, 1, 1, 1, 1, 0, 1), (67, 5, 3, 5, 10, 2, 4), (768, 77, 3, 8, 10, 0, 10),
                                                (768, 5, 2, 8, 128, 32, 64)])
def test_nothing_outside_the_footprint_is_written_and_two_calls_give_the_same_bits(dev, C, L, B, length, M, s, f):
    inp = make_inputs(C, L, B, length, M, seed=2)
    for want_ortho in (False, True):
        a, b = _raw(dev, inp, s, f, want_ortho), _raw(dev, inp, s, f, want_ortho)
        for n in a:
            assert torch.equal(a[n], b[n]), n
        # the autograd path returns the same bits as the raw calls
        prompted, ortho, alpha, grads = run_op(dev, inp, s, f, want_ortho)
        assert torch.equal(prompted.reshape(-1), a['prompted']) and torch.equal(ortho.reshape(1), a['ortho'])
        assert torch.equal(alpha.reshape(-1), a['alpha'])
        for g, n in zip(grads[1:], ('d_prompt', 'd_key', 'd_attn')):
            assert torch.equal(g.reshape(-1), a[n]), n


def test_bad_arguments_return_before_any_launch(dev):
    from vilco_amd import _lib, ops
    lib = _lib.load()
    inp = make_inputs(24, 5, 2, 3, 10)
    x, prompt, key, attn = (inp[n].to(dev) for n in ('x', 'prompt', 'key', 'attn'))
    outs = [torch.full((n,), SENT, device=dev) for n in (2 * 10, 2 * 8 * 24, 1, 10 * 3 * 24, 10 * 24, 10 * 24)]
    gp, go = inp['gp'].to(dev), torch.ones(1, device=dev)

    def call(**kw):
        d = ops._coda_desc(x, prompt, key, attn, 2, 4, True)
        nws = lib.vilco_coda_workspace(ctypes.byref(d))
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        d.alpha, d.prompted, d.ortho = (t.data_ptr() for t in outs[:3])
        d.workspace, d.workspace_bytes = ws.data_ptr(), nws
        for k, v in kw.items():
            setattr(d, k, v)
        rc = (lib.vilco_coda_fwd(ctypes.byref(d), None),
              lib.vilco_coda_bwd(ctypes.byref(d), gp.data_ptr(), go.data_ptr(), *(t.data_ptr() for t in outs[3:]), None))
        torch.cuda.synchronize()
        return rc
    for bad in (dict(f=0), dict(f=11), dict(M=129), dict(s=-1), dict(s=4), dict(len=0), dict(B=0), dict(L=0), dict(C=0),
                dict(x=None), dict(prompt=None), dict(key=None), dict(attn=None), dict(alpha=None), dict(prompted=None),
                dict(ortho=None), dict(workspace=None)):
        assert call(**bad) == (-1, -1), bad
        assert all(torch.equal(t, torch.full_like(t, SENT)) for t in outs), bad
    assert call(workspace_bytes=16) == (-4, -4)
    assert all(torch.equal(t, torch.full_like(t, SENT)) for t in outs)
    assert call() == (0, 0) and not any((t == SENT).any().item() for t in outs)


def _module(dev, M=10, length=8, C=768, n_tasks=5, ortho=True):
    from vilco_amd.cl_methods import CodaPrompt
    mod = CodaPrompt(M, length, C, n_tasks, ortho=ortho, seed=11)
    mod.set_task(1)
    return mod.to(dev).train()


def test_forward_and_backward_are_captured_and_replayed_on_a_changed_batch(dev):
    """the module's training forward + backward of task 1, captured with torch.cuda.graph on a side stream after a warm-up
    and replayed on a second batch: outputs and the three gradients equal the eager ones bit for bit"""
    mod = _module(dev)
    g = torch.Generator().manual_seed(5)
    xa, xb = torch.randn(2, 9, 768, generator=g).to(dev), torch.randn(2, 9, 768, generator=g).to(dev)
    gp = torch.randn(2, 17, 768, generator=g).to(dev)
    params = (mod.prompt, mod.prompt_key, mod.prompt_attn)

    def step(x):
        res = mod(x, task_id=1, train=True)
        ((res['prompted_embedding'] * gp).sum() + 0.3 * res['ortho']).backward()
        return res
    # Everything before the capture runs on the capture's stream, and nothing of it outlives the capture's start: a live
    # autograd graph keeps the parameters' AccumulateGrad nodes, which remember the stream they were made on, and a captured
    # backward that reused them would accumulate on a stream outside the capture (vilco_amd/graph.py drops them the same way).
    import gc
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    eager = []
    xs = xa.clone()
    with torch.cuda.stream(side):
        for x in (xa, xb, xa):                            # (the last round is the warm-up of the capture's buffers)
            mod.zero_grad(set_to_none=True)
            xs.copy_(x)
            res = step(xs)
            eager.append([res['prompted_embedding'].detach().clone(), res['ortho'].detach().clone()] + [p.grad.clone() for p in params])
            del res
    torch.cuda.current_stream().wait_stream(side)
    assert not torch.equal(eager[0][2], eager[1][2])
    mod.zero_grad(set_to_none=True)
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = step(xs)
    for x, want in ((xa, eager[0]), (xb, eager[1]), (xa, eager[0])):
        xs.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        got = [res['prompted_embedding'].detach(), res['ortho'].detach()] + [p.grad for p in params]
        for a, b in zip(got, want):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- in the model
def _coda_det_model(dev, gold, task):
    """the prompt fixture model (tests/golden/model_prompt.pt: pool 10, length 20, C = 24) rebuilt with a CodaPrompt"""
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    over = dict(gold['overrides'])
    over['cl_cfg'] = dict(over.get('cl_cfg', {}), prompt_type='coda', coda_tasks=5, coda_ortho_mu=0.1)
    cfg = make_config(**over)
    kw = dict(cfg['model'])
    if kw['use_xl']:
        kw['xlnet_config'] = xlnet_json(kw['embd_dim'], 4)
    m = vm.make_meta_arch('LocPointTransformer', **kw)
    state = {k: v for k, v in gold['state_dict'].items() if not k.startswith('prompt.')}
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert sorted(missing) == ['prompt.prompt', 'prompt.prompt_attn', 'prompt.prompt_key', 'prompt.task_count'] and not unexpected
    m.n_known = gold['n_known']
    for t in range(1, task + 1):
        m.prompt.set_task(t)
    m = m.to(dev).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0
    m.loss_normalizer = golden_cfg(gold)['train_cfg']['init_loss_norm']
    return cfg, m


def _eager_step(model, batch, task):
    for p in model.parameters():
        p.grad = None
    out = model(batch, task_id=task, is_training=True)
    out['final_loss'].backward()
    return ({k: v.detach().clone() for k, v in out.items()},
            {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})


PNAMES = ('prompt.prompt', 'prompt.prompt_key', 'prompt.prompt_attn')


@pytest.mark.parametrize("task", [0, 1])
def test_training_step_in_the_model_replays_and_matches_the_tensor_op_body(dev, task, monkeypatch):
    """A step through GraphedStep, replayed on a changed batch, equals the eager step of a twin bit for bit.  Against
    VILCO_FUSED_PROMPT=0 on the same step: the bars tests/test_prompt_gpu.py uses for this comparison, 1e-6 of the loss and 1e-5
    of a gradient's largest element."""
    from vilco_amd import ops
    from vilco_amd.graph import GraphedStep
    gold = load_golden("prompt")
    batch_a = golden_inputs(gold)
    batch_b = [dict(x, feats=x['feats'] * 0.9 + 0.01, prompt_feature=torch.flip(x['prompt_feature'], dims=(-1,)) * 1.1)
               for x in batch_a]
    (_, ma), (_, mb) = _coda_det_model(dev, gold, task), _coda_det_model(dev, gold, task)
    inp = ma.prepare(batch_a, True, gt_pad=8)
    assert ma.capturable(inp, task, None) and not ma.capturable(inp, 5, None) and not ma.capturable(inp, -1, None)
    with pytest.raises(ValueError, match="task"):
        mb(batch_a, task_id=5, is_training=True)
    gs = GraphedStep(ma, None, eager_steps=1)
    for i, batch in enumerate((batch_a, batch_a, batch_b)):
        got_l = gs(batch, task_id=task)
        torch.cuda.synchronize()
        got_g = {n: p.grad.clone() for n, p in ma.named_parameters() if p.grad is not None}
        want_l, want_g = _eager_step(mb, batch, task)
        assert 'ortho_loss' in want_l and float(want_l['ortho_loss']) > 0
        for k in want_l:
            assert torch.equal(got_l[k], want_l[k]), (i, k, float(got_l[k]), float(want_l[k]))
        assert set(got_g) == set(want_g) and all(n in want_g for n in PNAMES)
        for n in want_g:
            assert torch.equal(got_g[n], want_g[n]), (i, n)
    assert gs.stats['replayed'] == 2 and gs.stats['eager'] == 1, gs.stats
    pt = ma.prompt.per_task
    for n in PNAMES:
        g = want_g[n]
        assert not g[:task * pt].any().item() and not g[(task + 1) * pt:].any().item() and g[task * pt:(task + 1) * pt].any().item()
    # the same step with the tensor-op body
    monkeypatch.setattr(ops, "fused_prompt", False)
    _, mc = _coda_det_model(dev, gold, task)
    assert not mc.capturable(inp, task, None)
    for batch in (batch_a, batch_a, batch_b):              # the same history of the loss normaliser
        plain_l, plain_g = _eager_step(mc, batch, task)
    el = rel_err(want_l['final_loss'], plain_l['final_loss'])
    eg = {n: rel_err(want_g[n], plain_g[n], GRAD_FLOOR) for n in PNAMES}
    print("task", task, "loss rel %.2e" % el, {n: "%.2e" % e for n, e in eg.items()})
    assert el < 1e-6 and all(e < 1e-5 for e in eg.values()), (el, eg)


def test_five_optimizer_steps_of_task_1_leave_task_0_s_rows_alone_and_eval_uses_both(dev):
    from vilco_amd.utils.train_utils import make_optimizer
    gold = load_golden("prompt")
    batch = golden_inputs(gold)
    cfg, m = _coda_det_model(dev, gold, 1)
    pt = m.prompt.per_task
    opt = make_optimizer(m, dict(cfg['opt'], type='AdamW', weight_decay=0.05, learning_rate=1e-3))
    assert all(g['weight_decay'] > 0 for g in (opt.param_groups[0], opt.param_groups[2]))
    before = {n: p.detach().clone() for n, p in m.named_parameters() if n in PNAMES}
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        m(batch, task_id=1, is_training=True)['final_loss'].backward()
        opt.step(clip_grad_l2norm=1.0)
    torch.cuda.synchronize()
    now = dict(m.named_parameters())
    for n in PNAMES:
        assert torch.equal(now[n][:pt], before[n][:pt]), "rows [0, pt) hold their task-0 bits: " + n
        assert torch.equal(now[n][2 * pt:], before[n][2 * pt:]), n
        assert not torch.equal(now[n][pt:2 * pt], before[n][pt:2 * pt]), "rows [pt, 2 pt) have moved: " + n
    # an eval forward after set_task(1) uses f = 2 pt
    seen = {}
    hook = m.prompt.register_forward_hook(lambda mod, i, o: seen.update(alpha=o['alpha'].clone()))
    m.eval()
    with torch.no_grad():
        m(batch[:1], task_id=-1, is_training=False, get_emb=True)      # (inference takes one clip at a time)
    hook.remove()
    a = seen['alpha']
    assert a[:, :2 * pt].abs().min().item() > 0 and not a[:, 2 * pt:].any().item()


# ------------------------------------------------------------------------------------------------- episode
def _task_data(task):
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


def _episode_model(dev, coda_tasks):
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_episode_golden()
    over = dict(gold['overrides'])
    over['cl_cfg'] = dict(over.get('cl_cfg', {}), prompt_type='coda', coda_tasks=coda_tasks, type_sampling='random',
                          path_memory='memory.pkl')
    cfg = make_config(**over)
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    state = {k: v for k, v in episode_full_state(gold['init_state']).items() if not k.startswith('prompt.')}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert all(k.startswith('prompt.') for k in missing) and not unexpected
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    return cfg, model


def test_two_task_episode_sets_the_task_once_per_task_and_its_checkpoint_reloads(dev, tmp_path, monkeypatch):
    import os
    import random
    from vilco_amd import _lib
    from vilco_amd.cl_methods import CodaPrompt
    from vilco_amd.train_cl import run_episodes
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    cfg, model = _episode_model(dev, 2)
    cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))
    cfg['cl_cfg'] = dict(cfg['cl_cfg'], coda_tasks=None)               # the driver fills it from the stream
    calls, real = [], CodaPrompt.set_task

    def spy(self, t):
        calls.append(int(t))
        return real(self, t)
    monkeypatch.setattr(CodaPrompt, 'set_task', spy)
    stream = InMemoryQILStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
    random.seed(0)
    torch.manual_seed(0)
    torch.cuda.manual_seed_all(0)
    seen = []

    def validate(m, epoch, task):
        seen.append(task)
        return 1.0 if seen.count(task) == 2 else 0.1
    try:
        model, opt, sch, log = run_episodes(cfg, model, stream, validate=validate, ckpt_folder=str(tmp_path), gpu_id=0,
                                            use_graph=True, keep_history=True)
        torch.cuda.synchronize()
    finally:
        _lib.check(_lib.load().vilco_seed_word_set(0, None))
        torch.cuda.synchronize()
    assert calls == [0, 1] and cfg['cl_cfg']['coda_tasks'] == 2 and len(log) == 2
    assert all(bool(torch.isfinite(h['final_loss'])) for e in log for ep in e['history'] for h in ep)
    assert int(model.prompt.task_count) == 1
    no_decay = {id(p) for p in opt.param_groups[1]['params']}
    assert all(id(p) in no_decay for p in model.prompt.parameters())
    for j in (0, 1):
        ck = torch.load(os.path.join(str(tmp_path), 'best_task_%03d_performance.pth.tar' % j), map_location='cpu', weights_only=False)
        assert int(ck['state_dict']['prompt.task_count']) == j
    _, twin = _episode_model(dev, 2)
    twin.augment_classification(cases.EP_NEW, dev)
    twin.load_state_dict(ck['state_dict'])
    assert int(twin.prompt.task_count) == 1 and twin.prompt._task == 1
    assert torch.equal(twin.prompt.prompt_key.cpu(), ck['state_dict']['prompt.prompt_key'])


def test_op_time_is_reported_next_to_the_tensor_op_chain(dev):
    """bench.py's configurations hold no prompt pool, so the operator's own time is taken here: forward + backward on resident
    tensors, CUDA events, B = 2, L = 77, C = 768, M = 100, len = 8, f = 10 (s = 0), next to the tensor-op chain on the same
    tensors.  Printed for DESIGN.md; there is no speed-up bar."""
    from vilco_amd import ops
    from vilco_amd.cl_methods import CodaPrompt
    inp = make_inputs(768, 77, 2, 8, 100)
    mod = CodaPrompt(100, 8, 768, 10).to(dev)
    with torch.no_grad():
        mod.prompt.copy_(inp['prompt'])
        mod.prompt_key.copy_(inp['key'])
        mod.prompt_attn.copy_(inp['attn'])
    x, gp = inp['x'].to(dev), inp['gp'].to(dev)

    def step(fused, ortho):
        mod.zero_grad(set_to_none=True)
        if fused:
            prompted, pen, _ = ops.coda_prompt(x, mod.prompt, mod.prompt_key, mod.prompt_attn, 0, 10, ortho)
        else:
            prompted, pen, _ = mod._forward_tensor_ops(x, 0, 10, ortho)
        ((prompted * gp).sum() + 0.1 * pen).backward()

    def timed(fused, ortho, n=30):
        for _ in range(5):
            step(fused, ortho)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            step(fused, ortho)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n * 1e3
    for ortho in (False, True):
        a1, b1, a2, b2 = timed(True, ortho), timed(False, ortho), timed(True, ortho), timed(False, ortho)
        print("coda prompt fwd+bwd, want_ortho=%d, us per call (two runs each): op %.1f %.1f, tensor-op chain %.1f %.1f"
              % (ortho, a1, a2, b1, b2))
        assert all(np.isfinite(v) and v > 0 for v in (a1, a2, b1, b2))
