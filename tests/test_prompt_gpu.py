"""GPU: ops.prompt_pool (csrc/prompt.hip) against the fp64 restatement (tests/prompt_restatement.py, tied to the reference by
test_prompt_cpu.py), the copies' footprint, determinism, graph capture of the selecting path, and the op inside the model.

Bars.  Indices: exactly the restatement's (the rule is a counting rank; inputs are decided by margin or exact ties).  Copies:
bit-equal.  Values (sim, reduce_sim, the three gradients; parity_util.rel_err against fp64): measured, not fixed -- in the same
case the tensor-op body of Prompt (VILCO_FUSED_PROMPT=0) runs on the same device inputs with the restatement's indices as its
window, and the kernel may be at most 4x its error per quantity (the margin the herding Gram test gives a different fp32
summation order).  Measured errors of both paths: DESIGN.md section 3.15."""
import ctypes
import itertools
import zlib

import numpy as np
import pytest
import torch

from parity_util import GRAD_FLOOR, build_hip_model, golden_cfg, golden_inputs, load_golden, rel_err
import prompt_restatement as R

pytestmark = pytest.mark.gpu

CS, LS, BS = (768, 512, 37), (1, 77), (1, 2, 5)
PKL = ((10, 4, 5), (10, 10, 5), (3, 1, 1), (64, 2, 20))
KEYS = (('mean', False), ('max', False), ('mean_max', False), ('cls', False), ('cls', True))
MODES = ('window', 'window_rep', 'topk', 'vote')
QUANT = ('sim', 'reduce_sim', 'd_prompt', 'd_key', 'd_x')
WORST = {}          # (path, quantity) -> worst error seen in this session (printed by the last value test)


def decided(sim, k):
    """every gap between consecutive similarities among a row's k + 1 largest is far above fp32 rounding of a similarity"""
    top = np.abs(sim).max()
    for row in sim:
        s = np.sort(row)[::-1][:k + 1]
        if len(s) > 1 and np.min(s[:-1] - s[1:]) <= 1e-3 * top:
            return False
    return True


def make_inputs(C, L, B, P, k, length, ekey, with_cls, mode, scale=1.0, seed=0):
    """host fp32 inputs whose selection is decided in the restatement (a draw that is not is redrawn)"""
    for attempt in range(200):
        g = torch.Generator().manual_seed(zlib.crc32(repr((C, L, B, P, k, length, ekey, with_cls, mode, seed)).encode()) % (1 << 30) + attempt)
        x = scale * torch.randn(B, L, C, generator=g)
        prompt = 2 * torch.rand(P, length, C, generator=g) - 1
        key = 2 * torch.rand(P, C, generator=g) - 1
        cls = scale * torch.randn(B, C, generator=g) if with_cls else None
        gp = torch.randn(B, k * length + L, C, generator=g)
        idx = None
        if mode == 'window':
            idx = torch.stack([torch.arange(k) + (b * k) % (P - k + 1) for b in range(B)])
        elif mode == 'window_rep':
            idx = (torch.arange(k) + (P - k)).unsqueeze(0).repeat(B, 1)
        want = R.forward(x.numpy(), prompt.numpy(), key.numpy(), idx=None if idx is None else idx.numpy(), k=k,
                         batchwise=(mode == 'vote'), embedding_key=ekey, cls_features=None if cls is None else cls.numpy())
        if idx is not None or decided(want['similarity'], k):
            return dict(x=x, prompt=prompt, key=key, cls=cls, gp=gp, idx=idx, want=want)
    raise RuntimeError("no decided draw")


def run_op(dev, inp, k, mode, ekey, g_rs=-0.1):
    from vilco_amd import ops
    x = inp['x'].to(dev).requires_grad_(True)
    prompt = inp['prompt'].to(dev).requires_grad_(True)
    key = inp['key'].to(dev).requires_grad_(True)
    out = ops.prompt_pool(x, prompt, key, idx=None if inp['idx'] is None else inp['idx'].to(dev), top_k=k,
                          batchwise=(mode == 'vote'), embedding_key=ekey,
                          cls_features=None if inp['cls'] is None else inp['cls'].to(dev))
    ((out[0] * inp['gp'].to(dev)).sum() + g_rs * out[1]).backward()
    return out, (prompt.grad, key.grad, x.grad)


def run_tensor_ops(dev, inp, k, ekey, idx, g_rs=-0.1):
    """today's tensor-op body on the device, with the restatement's indices as its window (its own topk / unique leave the
    order among equal values undefined; the VALUES given the indices are what is measured)"""
    from vilco_amd.cl_methods import Prompt
    P, length, C = inp['prompt'].shape
    mod = Prompt(length=length, embed_dim=C, embedding_key=ekey, prompt_pool=True, prompt_key=True, pool_size=P, top_k=k).to(dev)
    with torch.no_grad():
        mod.prompt.copy_(inp['prompt'])
        mod.prompt_key.copy_(inp['key'])
    x = inp['x'].to(dev).requires_grad_(True)
    res = mod._forward_tensor_ops(x, torch.from_numpy(idx).to(dev), None if inp['cls'] is None else inp['cls'].to(dev))
    ((res['prompted_embedding'] * inp['gp'].to(dev)).sum() + g_rs * res['reduce_sim']).backward()
    return res, (mod.prompt.grad, mod.prompt_key.grad, x.grad)


def errors(sim, rs, grads, want, wgrads):
    t = torch.from_numpy
    return {'sim': rel_err(sim, t(want['similarity'])), 'reduce_sim': rel_err(rs, torch.tensor(want['reduce_sim'])),
            'd_prompt': rel_err(grads[0], t(wgrads[0]), GRAD_FLOOR), 'd_key': rel_err(grads[1], t(wgrads[1]), GRAD_FLOOR),
            'd_x': rel_err(grads[2], t(wgrads[2]), GRAD_FLOOR)}


def check_case(dev, C, L, B, P, k, length, ekey, with_cls, mode, scale=1.0, inp=None):
    inp = inp or make_inputs(C, L, B, P, k, length, ekey, with_cls, mode, scale)
    want = inp['want']
    out, grads = run_op(dev, inp, k, mode, ekey)
    prompted, rs, idx, sim, pn, xn, selkey = out
    tag = (C, L, B, P, k, length, ekey, with_cls, mode, scale)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want['prompt_idx']), (tag, idx.tolist())
    # copies: bit-equal to their sources
    src = torch.cat([inp['prompt'][idx.cpu()].reshape(B, k * length, C), inp['x']], dim=1)
    assert torch.equal(prompted.detach().cpu(), src), tag
    assert torch.equal(selkey.cpu(), pn.cpu()[idx.cpu()]), tag
    assert rs.dim() == 0 and sim.shape == (B, P) and pn.shape == (P, C) and xn.shape == (B, C)
    wgrads = R.backward(inp['x'].numpy(), inp['prompt'].numpy(), inp['key'].numpy(), want, inp['gp'].numpy(), -0.1,
                        embedding_key=ekey, cls_given=with_cls)
    picked = np.zeros(P, dtype=bool)
    picked[want['prompt_idx'].reshape(-1)] = True
    assert torch.count_nonzero(grads[0][torch.from_numpy(~picked).to(dev)]).item() == 0, tag      # exact zeros
    res, agrads = run_tensor_ops(dev, inp, k, ekey, want['prompt_idx'])
    mine = errors(sim, rs, grads, want, wgrads)
    aten = errors(res['similarity'], res['reduce_sim'], agrads, want, wgrads)
    assert rel_err(pn, torch.from_numpy(want['prompt_norm'])) < 1e-6 and rel_err(xn, torch.from_numpy(want['x_embed_norm'])) < 1e-6
    for q in QUANT:
        WORST[('kernel', q)] = max(WORST.get(('kernel', q), 0.0), mine[q])
        WORST[('tensor ops', q)] = max(WORST.get(('tensor ops', q), 0.0), aten[q])
    print(tag, " ".join("%s %.1e/%.1e" % (q, mine[q], aten[q]) for q in QUANT))
    for q in QUANT:
        assert mine[q] <= 4 * aten[q], (tag, q, mine[q], aten[q])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ekey,with_cls", KEYS)
def test_indices_copies_and_values_over_the_shape_grid(dev, ekey, with_cls, mode):
    for C, L, B, (P, k, length) in itertools.product(CS, LS, BS, PKL):
        check_case(dev, C, L, B, P, k, length, ekey, with_cls, mode)
    print("worst so far:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("scale", [1e4, 1e-8])
@pytest.mark.parametrize("mode", ['window_rep', 'vote'])
def test_scaled_inputs(dev, scale, mode):
    """1e-8 drives sum xk^2 below the 1e-12 clamp: xn is xk * 1e6, and the clamp cuts the normalisation's own gradient term"""
    for ekey, with_cls in (('mean', False), ('max', False), ('cls', True)):
        inp = make_inputs(768, 77, 2, 10, 4, 5, ekey, with_cls, mode, scale)
        if scale < 1:
            assert (inp['want']['_ssq_x'] < R.EPS).all()
        check_case(dev, 768, 77, 2, 10, 4, 5, ekey, with_cls, mode, scale, inp=inp)


def _tie_inputs(x, key, k, length=2, vote=False):
    x, key = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(key, dtype=torch.float32)
    g = torch.Generator().manual_seed(3)
    P, C = key.shape
    prompt = 2 * torch.rand(P, length, C, generator=g) - 1
    gp = torch.randn(x.shape[0], k * length + x.shape[1], C, generator=g)
    want = R.forward(x.numpy(), prompt.numpy(), key.numpy(), k=k, batchwise=vote)
    return dict(x=x, prompt=prompt, key=key, cls=None, gp=gp, idx=None, want=want)


def test_hand_built_ties(dev):
    rng = np.random.RandomState(0)
    # equal similarities: two identical keys
    key = rng.uniform(-1, 1, (5, 8)).astype(np.float32)
    key[3] = key[1]
    inp = _tie_inputs(np.broadcast_to(key[1], (2, 3, 8)).copy(), key, 2)
    assert inp['want']['prompt_idx'].tolist() == [[1, 3], [1, 3]]
    out, _ = run_op(dev, inp, 2, 'topk', 'mean')
    assert out[2].tolist() == [[1, 3], [1, 3]] and out[3][0, 1].item() == out[3][0, 3].item()
    # an all-zero text row: every similarity is 0, prompts 0 .. k-1 win
    inp = _tie_inputs(np.zeros((1, 4, 8)), rng.uniform(-1, 1, (6, 8)), 3)
    out, grads = run_op(dev, inp, 3, 'topk', 'mean')
    assert out[2].tolist() == [[0, 1, 2]] and torch.count_nonzero(out[3]).item() == 0 and out[1].item() == 0.0
    assert all(torch.isfinite(g).all().item() for g in grads)
    # equal counts at B = 2: unit keys, the text rows ARE the wanted similarities (up to their norm)
    sim = np.zeros((2, 1, 8), dtype=np.float32)
    sim[0, 0, :6] = [0.3, 0.0, 0.5, 0.0, 0.9, -1.0]
    sim[1, 0, :6] = [0.0, 0.2, 0.0, 0.6, 0.9, -1.0]
    inp = _tie_inputs(sim, np.eye(6, 8), 3, vote=True)
    assert inp['want']['prompt_idx'].tolist() == [[4, 0, 1], [4, 0, 1]]
    out, _ = run_op(dev, inp, 3, 'vote', 'mean')
    assert out[2].tolist() == [[4, 0, 1], [4, 0, 1]]
    inp = _tie_inputs(sim, np.eye(6, 8), 3, vote=False)
    out, _ = run_op(dev, inp, 3, 'topk', 'mean')
    assert out[2].tolist() == [[4, 2, 0], [4, 3, 1]]


@pytest.mark.parametrize("ekey", ['max', 'mean_max'])
def test_a_maximum_attained_twice_sends_its_gradient_to_the_first_position(dev, ekey):
    """positions 2 and 5 hold the same row maximum in every channel.  Bound (derived): d_x = g + a few fp32 operations on a dot
    product over C = 64 terms, C eps = 4e-6 of the largest element at the very worst; a misplaced gradient is an O(1) error."""
    inp = make_inputs(64, 7, 2, 6, 2, 3, ekey, False, 'window_rep')
    x = inp['x']
    x[:, 2] = x.max(dim=1)[0] + 1.0
    x[:, 5] = x[:, 2]
    inp['want'] = R.forward(x.numpy(), inp['prompt'].numpy(), inp['key'].numpy(), idx=inp['idx'].numpy(), embedding_key=ekey)
    assert (inp['want']['_arg'] == 2).all()
    out, grads = run_op(dev, inp, 2, 'window_rep', ekey)
    wg = R.backward(x.numpy(), inp['prompt'].numpy(), inp['key'].numpy(), inp['want'], inp['gp'].numpy(), -0.1, embedding_key=ekey)
    assert rel_err(grads[2], torch.from_numpy(wg[2]), GRAD_FLOOR) < 1e-5
    path = grads[2].cpu() - inp['gp'][:, 2 * 3:]
    if ekey == 'max':
        assert torch.count_nonzero(path[:, 5]).item() == 0 and torch.count_nonzero(path[:, 2]).item() > 0


def _raw(dev, inp, k, mode, ekey, guard=64):
    """the C entry points over guard-banded buffers -> (outputs, gradients, the untouched-band checks)"""
    from vilco_amd import _lib, ops
    lib = _lib.load()
    x, prompt, key = (inp[n].to(dev).contiguous() for n in ('x', 'prompt', 'key'))
    B, L, C = x.shape
    P, length = prompt.shape[:2]
    idx_in = None if inp['idx'] is None else inp['idx'].to(dev).contiguous()
    d = ops._prompt_desc(x, prompt, key, idx_in, None, (k, ops.PROMPT_KEY_MODES[ekey], mode == 'vote'))
    SENT = -1234.5

    def banded(n):
        buf = torch.full((n + 2 * guard,), SENT, dtype=torch.float32, device=dev)
        return buf, buf[guard:guard + n]
    bufs = {n: banded(sz) for n, sz in (('sim', B * P), ('pn', P * C), ('xn', B * C), ('selkey', B * k * C),
                                        ('prompted', B * (k * length + L) * C), ('reduce_sim', 1), ('d_prompt', P * length * C),
                                        ('d_key', P * C), ('d_x', B * L * C))}
    idx = torch.full((B * k + 2 * guard,), -77, dtype=torch.int64, device=dev)
    nws = lib.vilco_prompt_workspace(ctypes.byref(d))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    d.idx = idx[guard:].data_ptr()
    for n in ('sim', 'pn', 'xn', 'selkey', 'prompted', 'reduce_sim'):
        setattr(d, n, bufs[n][1].data_ptr())
    d.workspace, d.workspace_bytes = ws.data_ptr(), nws
    _lib.check(lib.vilco_prompt_fwd(ctypes.byref(d), None))
    gp, g_rs = inp['gp'].to(dev).contiguous(), torch.full((1,), -0.1, device=dev)
    _lib.check(lib.vilco_prompt_bwd(ctypes.byref(d), gp.data_ptr(), g_rs.data_ptr(), bufs['d_prompt'][1].data_ptr(),
                                    bufs['d_key'][1].data_ptr(), bufs['d_x'][1].data_ptr(), None))
    torch.cuda.synchronize()
    for n, (buf, view) in bufs.items():
        band = torch.cat([buf[:guard], buf[guard + view.numel():]])
        assert torch.equal(band, torch.full_like(band, SENT)), n
        assert not (view == SENT).any().item(), n                     # ... and every element inside was written
    assert (idx[:guard] == -77).all().item() and (idx[guard + B * k:] == -77).all().item()
    return {n: v[1].clone() for n, v in bufs.items()}, idx[guard:guard + B * k].reshape(B, k).clone()


@pytest.mark.parametrize("C,L,B,P,k,length", [(37, 1, 5, 3, 1, 1), (37, 77, 2, 10, 4, 5), (768, 77, 5, 64, 2, 20), (512, 1, 1, 10, 10, 5)])
def test_nothing_outside_the_footprint_is_written_and_two_calls_give_the_same_bits(dev, C, L, B, P, k, length):
    for mode, ekey in (('vote', 'mean_max'), ('window_rep', 'mean'), ('topk', 'max')):
        inp = make_inputs(C, L, B, P, k, length, ekey, False, mode)
        a, ia = _raw(dev, inp, k, mode, ekey)
        b, ib = _raw(dev, inp, k, mode, ekey)
        assert torch.equal(ia, ib) and np.array_equal(ia.cpu().numpy(), inp['want']['prompt_idx'])
        for n in a:
            assert torch.equal(a[n], b[n]), n
        src = torch.cat([inp['prompt'][ia.cpu()].reshape(B, k * length, C), inp['x']], dim=1)
        assert torch.equal(a['prompted'].cpu().reshape(src.shape), src)
        # the autograd path returns the same bits as the raw calls
        out, grads = run_op(dev, inp, k, mode, ekey)
        assert torch.equal(out[0].detach().reshape(-1), a['prompted']) and torch.equal(out[1].detach().reshape(1), a['reduce_sim'])
        for g, n in zip(grads, ('d_prompt', 'd_key', 'd_x')):
            assert torch.equal(g.reshape(-1), a[n]), n


def test_a_window_outside_the_pool_raises_the_status_word_and_reads_nothing_out_of_bounds(dev):
    from vilco_amd import ops
    inp = make_inputs(37, 3, 2, 5, 2, 2, 'mean', False, 'window_rep')
    ops.status_word_take()
    run_op(dev, inp, 2, 'window_rep', 'mean')
    assert ops.status_word_take() == 0
    inp['idx'] = torch.tensor([[0, 5], [-1, 4]])
    out, _ = run_op(dev, inp, 2, 'window_rep', 'mean')
    assert ops.status_word_take() & 1 and out[2].tolist() == [[0, 4], [0, 4]]          # clamped into the pool
    assert ops.status_word_take() == 0                                                  # taken: cleared


def _eval_module(dev, C=768, P=10, k=4, length=5):
    from vilco_amd.cl_methods import Prompt
    torch.manual_seed(11)
    return Prompt(length=length, embed_dim=C, embedding_key='mean', prompt_pool=True, prompt_key=True, pool_size=P, top_k=k,
                  batchwise_prompt=True).to(dev).eval()


def _two_batches_with_different_votes(mod):
    """two text batches, each decided under the module's keys, whose voted SETS differ"""
    prompt, key = mod.prompt.detach().cpu().numpy(), mod.prompt_key.detach().cpu().numpy()
    found = []
    for seed in range(200):
        x = torch.randn(2, 9, 768, generator=torch.Generator().manual_seed(500 + seed))
        w = R.forward(x.numpy(), prompt, key, k=4, batchwise=True)
        if decided(w['similarity'], 4) and (not found or sorted(found[0][1]['prompt_idx'][0].tolist()) != sorted(w['prompt_idx'][0].tolist())):
            found.append((dict(x=x), w))
            if len(found) == 2:
                return found[0] + found[1]
    raise RuntimeError("no pair of batches with different votes")


def test_the_selecting_forward_is_captured_and_replayed_on_a_batch_whose_vote_differs(dev):
    """eval-mode forward, prompt_mask=None, batchwise vote: captured on a side stream after one warm-up call and replayed on
    a second batch.  (The tensor-op body cannot be captured: torch.unique reads its output size on the host.)"""
    mod = _eval_module(dev)
    a, wa, b, wb = _two_batches_with_different_votes(mod)
    xs = torch.empty(2, 9, 768, device=dev)
    with torch.no_grad():
        eager = []
        for inp in (a, b):
            res = mod(inp['x'].to(dev))
            eager.append((res['prompt_idx'].clone(), res['prompted_embedding'].clone(), res['reduce_sim'].clone()))
        # the module votes in the reference's order among equal counts (Prompt._forward_fused): the SET is the restatement's
        for got, w in ((eager[0][0], wa), (eager[1][0], wb)):
            assert all(sorted(r) == sorted(w['prompt_idx'][0].tolist()) for r in got.tolist())
        xs.copy_(a['x'])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mod(xs)                                       # warm-up
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            res = mod(xs)
        for inp, want in ((a, eager[0]), (b, eager[1]), (a, eager[0])):
            xs.copy_(inp['x'])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(res['prompt_idx'], want[0]) and torch.equal(res['prompted_embedding'], want[1])
            assert torch.equal(res['reduce_sim'], want[2])


def _det_model(dev, gold):
    m = build_hip_model(gold, dev).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0
    m.loss_normalizer = golden_cfg(gold)['train_cfg']['init_loss_norm']
    return m


@pytest.mark.parametrize("where", ["inside", "past"])
def test_training_step_in_the_model_replays_and_matches_the_tensor_op_body(dev, where, monkeypatch):
    """The prompt fixture model (tests/golden/model_prompt.pt: pool 10, top_k 4, length 20, C = 24), task 1 (window inside the
    pool) and task 2 (past it: top-k + vote while training).  A step through GraphedStep, replayed on a changed batch, equals
    the eager step bit for bit.  Against VILCO_FUSED_PROMPT=0 on the same step: prepended rows are bit copies either way, so
    the paths differ by fp32 rounding of reduce_sim (weight 0.1 in the loss) and of d key -- bars (derived): 1e-6 of the loss,
    1e-5 of a gradient's largest element (a dot product over C = 24 terms and a sum over B k <= 8 rows, eps = 6e-8 each).
    Past the pool the module's vote keeps the order torch.topk gives equal counts on the tensor-op body's count array
    (Prompt._vote), so the two paths pick the same list there too."""
    from vilco_amd import ops
    from vilco_amd.graph import GraphedStep
    gold = load_golden("prompt")
    task = 1 if where == "inside" else 2
    batch_a = golden_inputs(gold)
    batch_b = [dict(x, feats=x['feats'] * 0.9 + 0.01, prompt_feature=torch.flip(x['prompt_feature'], dims=(-1,)) * 1.1)
               for x in batch_a]
    ma, mb = _det_model(dev, gold), _det_model(dev, gold)
    assert (task + 1) * ma.prompt.top_k <= ma.prompt.pool_size if where == "inside" else (task + 1) * ma.prompt.top_k > ma.prompt.pool_size
    gs = GraphedStep(ma, None, eager_steps=1)
    seen = {}
    hook = mb.prompt.register_forward_hook(lambda m, i, o: seen.__setitem__(True, o['prompt_idx'].clone()))

    def eager(model, batch):
        for p in model.parameters():
            p.grad = None
        out = model(batch, task_id=task, is_training=True)
        out['final_loss'].backward()
        return ({k: v.detach().clone() for k, v in out.items()},
                {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    for i, batch in enumerate((batch_a, batch_a, batch_b)):
        got_l = gs(batch, task_id=task)
        torch.cuda.synchronize()
        got_g = {n: p.grad.clone() for n, p in ma.named_parameters() if p.grad is not None}
        want_l, want_g = eager(mb, batch)
        for k in want_l:
            assert torch.equal(got_l[k], want_l[k]), (i, k, float(got_l[k]), float(want_l[k]))
        assert set(got_g) == set(want_g)
        for n in want_g:
            assert torch.equal(got_g[n], want_g[n]), (i, n)
    assert gs.stats['replayed'] == 2 and gs.stats['eager'] == 1, gs.stats
    assert 'prompt.prompt' in want_g and 'prompt.prompt_key' in want_g
    # the same step with the tensor-op body
    monkeypatch.setattr(ops, "fused_prompt", False)
    mc = _det_model(dev, gold)
    hook2 = mc.prompt.register_forward_hook(lambda m, i, o: seen.__setitem__(False, o['prompt_idx'].clone()))
    for batch in (batch_a, batch_a, batch_b):              # the same history of the loss normaliser
        plain_l, plain_g = eager(mc, batch)
    hook.remove(); hook2.remove()
    same = torch.equal(seen[True], seen[False])
    print(where, "indices fused", seen[True].tolist(), "tensor ops", seen[False].tolist())
    assert same                 # also past the pool: the module's vote keeps the tensor-op body's order among equal counts
    if True:
        el = rel_err(want_l['final_loss'], plain_l['final_loss'])
        eg = {n: rel_err(want_g[n], plain_g[n], GRAD_FLOOR) for n in ('prompt.prompt', 'prompt.prompt_key')}
        print(where, "loss rel %.2e" % el, {n: "%.2e" % e for n, e in eg.items()})
        assert el < 1e-6 and all(e < 1e-5 for e in eg.values()), (el, eg)


def test_op_time_is_reported_next_to_the_tensor_op_chain(dev):
    """bench.py's configurations hold no prompt pool, so the operator's own time is taken here: forward + backward on resident
    tensors, CUDA events, B = 2, L = 77, C = 768, pool 10, k = 4, length 5 (the ViLCo recipe's sizes), next to the tensor-op
    chain (VILCO_FUSED_PROMPT=0) on the same tensors.  Printed for DESIGN_LOG.md; there is no speed-up bar."""
    from vilco_amd import ops
    from vilco_amd.cl_methods import Prompt
    inp = make_inputs(768, 77, 2, 10, 4, 5, 'mean', False, 'window_rep')
    mod = Prompt(length=5, embed_dim=768, embedding_key='mean', prompt_pool=True, prompt_key=True, pool_size=10, top_k=4).to(dev)
    x, gp, idx = inp['x'].to(dev), inp['gp'].to(dev), inp['idx'].to(dev)

    def step(fused):
        mod.zero_grad(set_to_none=True)
        if fused:
            out = ops.prompt_pool(x, mod.prompt, mod.prompt_key, idx=idx)
            loss = (out[0] * gp).sum() - 0.1 * out[1]
        else:
            res = mod._forward_tensor_ops(x, idx)
            loss = (res['prompted_embedding'] * gp).sum() - 0.1 * res['reduce_sim']
        loss.backward()

    def timed(fused, n=30):
        for _ in range(5):
            step(fused)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            step(fused)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n * 1e3
    a1, b1, a2, b2 = timed(True), timed(False), timed(True), timed(False)
    print("prompt pool fwd+bwd, us per call (two runs each): op %.1f %.1f, tensor-op chain %.1f %.1f" % (a1, a2, b1, b2))
    assert all(np.isfinite(v) and v > 0 for v in (a1, a2, b1, b2))
