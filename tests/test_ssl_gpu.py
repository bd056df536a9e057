"""Narration SSL on the device (csrc/ssl.hip through ops.ssl_pool / ops.ssl_nce / MemoryBank) against the float64
restatement (tests/ssl_restatement.py) on the same inputs, the reference golden's three steps replayed through the device
path, and the model's fused path against the tensor-expression path it replaces.

Bars: 1e-5 relative in max norm for the kernels (the bar tests/test_cl_parts.py holds this branch to), 1e-3 for the
model-level parity of two paths that differ in summation order and in the encoder's GEMM format (README: the parity bar)."""
import os

import numpy as np
import pytest
import torch

import ssl_restatement as R
from parity_util import GRAD_FLOOR, build_hip_model, golden_inputs, load_golden, rel_err

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 1e-5


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------- pooling
POOL_CASES = {
    # three levels, C a multiple of 4 but not of the 256 * 4 columns a workgroup covers per pass; lengths 0, 1 and full
    "levels": dict(T=[16, 8, 4], C=36, lens=[[16, 8, 4], [1, 0, 2], [0, 5, 1]]),
    # the narration use: one level, C not a multiple of 4 (scalar loads)
    "narration": dict(T=[5], C=10, lens=[[5], [0], [1]]),
    # 72 slabs of 32 rows per clip; 1000 = 31 slabs + 8 rows ends inside a slab
    "split": dict(T=[2304], C=1024, lens=[[2304], [1000]]),
}


@pytest.mark.parametrize("name", sorted(POOL_CASES))
def test_pool_forward_backward_vs_restatement(dev, name):
    from vilco_amd import ops
    case = POOL_CASES[name]
    g = torch.Generator().manual_seed(7)
    B = len(case['lens'])
    feats_h = [0.25 + torch.randn(B, T, case['C'], generator=g) for T in case['T']]
    dout_h = torch.randn(B, case['C'], generator=g)
    lens = torch.tensor(case['lens'], dtype=torch.int32, device=dev)
    runs = []
    for _ in range(2):
        feats = [f.to(dev).requires_grad_(True) for f in feats_h]
        out = ops.ssl_pool(feats, lens)
        out.backward(dout_h.to(dev))
        runs.append((out.detach().clone(), [f.grad.clone() for f in feats]))
    want = R.pool([f.numpy() for f in feats_h], case['lens'])
    wgrads = R.pool_grad(dout_h.double().numpy(), case['T'], case['lens'])
    out, grads = runs[0]
    print(name, "fwd", rel_err(out, t64(want)), "bwd", [rel_err(a, t64(b)) for a, b in zip(grads, wgrads)])
    assert rel_err(out, t64(want)) < BAR
    for l, (a, b) in enumerate(zip(grads, wgrads)):
        assert rel_err(a, t64(b)) < BAR, l
        for bi, row in enumerate(case['lens']):
            assert not a[bi, row[l]:].any(), "gradient rows at or beyond the length must be exact zeros"
    assert torch.equal(out, runs[1][0]) and all(torch.equal(a, b) for a, b in zip(grads, runs[1][1]))


def test_pool_ignores_what_lies_beyond_the_length(dev):
    """NaN above the length must not reach the output: those elements are not read"""
    from vilco_amd import ops
    f = torch.randn(2, 70, 16, device=dev)
    lens = torch.tensor([[33], [0]], dtype=torch.int32, device=dev)
    clean = ops.ssl_pool([f], lens)
    f2 = f.clone()
    f2[0, 33:] = float('nan')
    f2[1] = float('nan')
    assert torch.equal(ops.ssl_pool([f2], lens), clean) and not clean[1].any()


# ----------------------------------------------------------------------------------------------------------------- nce
NCE_SIZES = [(1, 4, 1), (3, 36, 4), (3, 100, 67), (16, 1024, 1010)]       # smallest; wrap + gap; no multiple of 64; the recipe


def _mask(kind, B):
    if kind == "none":
        return [0.0] * B
    if kind == "all":
        return [1.0] * B
    return [1.0 if b % 2 == 0 else 0.0 for b in range(B)]                  # a gap in the mask (B = 1: the one row)


def _nce_inputs(B, D, M):
    g = torch.Generator().manual_seed(1000 * B + D + M)
    return (torch.randn(B, D, generator=g), 0.3 + torch.randn(B, D, generator=g), torch.randn(M, D, generator=g))


@pytest.mark.parametrize("kind", ["none", "some", "all"])
@pytest.mark.parametrize("B,D,M", NCE_SIZES)
def test_nce_vs_restatement(dev, B, D, M, kind):
    from vilco_amd import ops
    from vilco_amd.modeling.meta_archs import MemoryBank
    text_h, video_h, bank_h = _nce_inputs(B, D, M)
    mask_h = _mask(kind, B)
    scale = 1.7                                                              # an upstream gradient other than 1
    want = R.nce(text_h.numpy(), video_h.numpy(), mask_h, bank_h.numpy(), M - 1)
    runs = []
    for _ in range(2):
        mb = MemoryBank(M, D, device=dev)
        mb.memory.copy_(bank_h)
        mb.ptr = M - 1                                                       # a wrap inside one update
        text, video = text_h.to(dev).requires_grad_(True), video_h.to(dev).requires_grad_(True)
        loss, xn = ops.ssl_nce(text, video, torch.tensor(mask_h, device=dev), mb.memory, mb.ring)
        (scale * loss).backward()
        runs.append((loss.detach().clone(), text.grad.clone(), video.grad.clone(), mb.memory.clone(), mb.ptr, xn.clone()))
    loss, dt, dv, bank, ptr, xn = runs[0]
    n = int(sum(mask_h))
    if n == 0:
        assert float(loss) == 0.0 and not dt.any() and not dv.any()
        assert torch.equal(bank.cpu(), bank_h) and ptr == M - 1
    else:
        print((B, D, M, kind), "loss", abs(float(loss) - want['loss']) / want['loss'], "dt", rel_err(dt, t64(want['dtext']) * scale),
              "dv", rel_err(dv, t64(want['dvideo']) * scale), "bank", rel_err(bank, t64(want['bank'])))
        assert abs(float(loss) - want['loss']) <= BAR * want['loss']
        assert rel_err(dt, t64(want['dtext']) * scale) < BAR and rel_err(dv, t64(want['dvideo']) * scale) < BAR
        assert ptr == want['ptr'] == (M - 1 + n) % M
        assert rel_err(bank, t64(want['bank'])) < BAR and rel_err(xn[0], t64(want['tn'])) < BAR
        rows = [b for b in range(B) if mask_h[b]]
        written = {(M - 1 + r) % M: b for r, b in enumerate(rows)}
        for j in range(M):                                                   # bit-equal: the rows written, and the rest untouched
            assert torch.equal(bank[j], xn[0, written[j]] if j in written else bank_h[j].to(dev)), j
        for b in range(B):
            if not mask_h[b]:
                assert not dt[b].any() and not dv[b].any()
    for a, b in zip(runs[0], runs[1]):
        assert a == b if isinstance(a, int) else torch.equal(a, b)


def test_memory_bank_keeps_its_contract_and_updates_masked(dev):
    from vilco_amd.modeling.meta_archs import MemoryBank
    mb = MemoryBank(4, 8, device=dev)
    assert mb.ptr == 0 and mb.get_all() is mb.memory
    mb.update(torch.ones(3, 8, device=dev))
    mb.update(2 * torch.ones(3, 8, device=dev))
    assert mb.ptr == 2 and mb.memory[:, 0].tolist() == [2.0, 2.0, 1.0, 2.0]
    rows = torch.arange(3, device=dev, dtype=torch.float32)[:, None].expand(3, 8) + 5
    mb.update_masked(rows, torch.tensor([1.0, 0.0, 1.0], device=dev))
    assert mb.ptr == 0 and mb.memory[:, 0].tolist() == [2.0, 2.0, 5.0, 7.0]
    before = mb.memory.clone()
    mb.update_masked(rows, torch.zeros(3, device=dev))
    assert mb.ptr == 0 and torch.equal(mb.memory, before)
    with pytest.raises(RuntimeError, match="narration SSL"):
        mb.update_masked(torch.ones(5, 8, device=dev), torch.ones(5, device=dev))          # more rows than the bank holds


def test_golden_steps_replayed_through_the_device_path(dev):
    """tests/golden/ssl_step.npz (reference MemoryBank + masked_contrastive_loss + the pooling lines of its forward): bank,
    pointer, loss and input gradients after each of the three steps.  The maskless step, which the reference skips, is an
    exact-zero loss here and leaves bank and pointer alone."""
    from vilco_amd import ops
    from vilco_amd.modeling.meta_archs import MemoryBank
    g = np.load(os.path.join(HERE, "golden", "ssl_step.npz"))
    mb = MemoryBank(4, 8, device=dev)
    mb.memory.copy_(torch.from_numpy(g['bank0']))
    w, bias = torch.from_numpy(g['enc_w']).to(dev), torch.from_numpy(g['enc_b']).to(dev)
    for s in range(3):
        tokens = torch.from_numpy(g['tokens%d' % s]).to(dev).requires_grad_(True)
        feats = [torch.from_numpy(g['feats%d_%d' % (s, l)]).to(dev).requires_grad_(True) for l in range(2)]
        tok = (tokens.permute(0, 2, 1) @ w.t() + bias).contiguous()                       # the encoder itself: test_model parity
        text = ops.ssl_pool([tok], torch.from_numpy(g['tok_lens'][s]).to(dev).reshape(-1, 1))
        video = ops.ssl_pool(feats, torch.from_numpy(g['feat_lens'][s]).to(dev))
        loss, _ = ops.ssl_nce(text, video, torch.from_numpy(g['masks'][s]).to(dev), mb.memory, mb.ring)
        loss.backward()
        assert mb.ptr == int(g['ptr%d' % s]) and rel_err(mb.memory, torch.from_numpy(g['bank%d' % s])) < BAR, s
        if g['skipped'][s]:
            assert float(loss) == 0.0 and not tokens.grad.any() and not any(f.grad.any() for f in feats)
            continue
        assert abs(float(loss.detach()) - float(g['loss%d' % s])) <= BAR * float(g['loss%d' % s]), s
        assert rel_err(tokens.grad, torch.from_numpy(g['d_tokens%d' % s])) < BAR, s
        for l, f in enumerate(feats):
            assert rel_err(f.grad, torch.from_numpy(g['d_feats%d_%d' % (s, l)])) < BAR, (s, l)


# --------------------------------------------------------------------------------------------------------------- model
def _ssl_model(dev, fused):
    from vilco_amd.modeling.meta_archs import MemoryBank
    model = build_hip_model(load_golden("noxl"), dev).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    g = torch.Generator().manual_seed(31)
    model.narration_ssl, model.fused_ssl, model.ssl_factor = True, fused, 0.03
    model.narration_encoder = torch.nn.Linear(24, 32).to(dev)
    with torch.no_grad():
        model.narration_encoder.weight.copy_(0.3 * torch.randn(32, 24, generator=g))
        model.narration_encoder.bias.copy_(0.1 * torch.randn(32, generator=g))
    model._memory_bank_cfg = (10, 32)
    model.memory_bank = MemoryBank(10, 32, device=dev)
    model.memory_bank.memory.copy_(torch.randn(10, 32, generator=g))
    model.memory_bank.ptr = 8
    model.loss_normalizer = 100.0
    return model


def _ssl_batch(gold):
    g = torch.Generator().manual_seed(32)
    return [dict(x, narration_feats=torch.randn(24, 3 + 2 * i, generator=g), narration_mask=float(i != 1))
            for i, x in enumerate(golden_inputs(gold))]


def test_model_fused_ssl_equals_the_unfused_path(dev):
    gold = load_golden("noxl")
    batch = _ssl_batch(gold)
    assert len(batch) >= 2
    res = []
    for fused in (True, False):
        model = _ssl_model(dev, fused)
        out = model(batch, task_id=gold['task_id'], is_training=True)
        out['final_loss'].backward()
        res.append((out, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None},
                    model.memory_bank.memory.clone(), model.memory_bank.ptr))
    (oa, ga, ba, pa), (ob, gb, bb, pb) = res
    assert float(ob['ssl_loss']) > 0 and rel_err(oa['ssl_loss'], ob['ssl_loss']) < 1e-3
    assert rel_err(oa['final_loss'], ob['final_loss']) < 1e-3
    assert pa == pb and rel_err(ba, bb) < 1e-3
    assert set(ga) == set(gb) and 'narration_encoder.weight' in ga
    # (a constant shift of every key cancels in softmax: these biases' gradients are analytically zero, rounding noise on
    # both paths -- left out as in tests/test_loss_gpu.py, tests/test_episode.py)
    noise = ('key_norm.bias', '.key.bias')
    worst = max((rel_err(ga[n], gb[n], GRAD_FLOOR), n) for n in ga if not n.endswith(noise))
    print("worst gradient", worst)
    assert worst[0] < 1e-3, worst


def test_model_without_any_narration_has_a_zero_ssl_loss(dev):
    gold = load_golden("noxl")
    batch = [dict(x, narration_mask=0.0) for x in _ssl_batch(gold)]
    model = _ssl_model(dev, True)
    before = model.memory_bank.memory.clone()
    out = model(batch, task_id=gold['task_id'], is_training=True)
    out['final_loss'].backward()
    assert float(out['ssl_loss']) == 0.0 and model.memory_bank.ptr == 8 and torch.equal(model.memory_bank.memory, before)
    assert not model.narration_encoder.weight.grad.any()


def test_get_emb_pass_in_train_mode_leaves_the_bank_alone(dev):
    """cache_prev_logits (train_cl.py) runs `model(..., get_emb=True)` over the whole loader with the model in train mode: the
    SSL loss is not consumed there, so the bank and its pointer must come out bit-identical (the reference writes the bank only
    inside the training-loss branch, meta_archs.py:939-945)"""
    gold = load_golden("noxl")
    batch = _ssl_batch(gold)
    for fused in (True, False):
        model = _ssl_model(dev, fused)
        before, ring = model.memory_bank.memory.clone(), model.memory_bank.ring.clone()
        with torch.no_grad():
            out = model(batch, task_id=gold['task_id'], is_training=True, get_emb=True)
        assert isinstance(out, tuple) and model.training
        assert torch.equal(model.memory_bank.memory, before) and torch.equal(model.memory_bank.ring, ring), fused
        model(batch, task_id=gold['task_id'], is_training=True)['final_loss'].backward()          # the training step does write it
        assert model.memory_bank.ptr == (8 + 1) % 10 and not torch.equal(model.memory_bank.memory, before), fused


def test_batches_outside_the_kernel_limits_take_the_unfused_branch(dev):
    """more clips than the bank has rows (the kernels need B <= M): the tensor-expression branch runs, as before"""
    gold = load_golden("noxl")
    batch = _ssl_batch(gold)
    model = _ssl_model(dev, True)
    assert model.prepare(batch, True).narr_cf is not None
    model._memory_bank_cfg = (len(batch) - 1, 32)
    assert not model._ssl_fused(len(batch)) and model._ssl_fused(len(batch) - 1)
    inp = model.prepare(batch, True)
    assert inp.narr_cf is None and inp.narr is not None and not model.capturable(inp, gold['task_id'])
    model._memory_bank_cfg = (10, 30)                                                             # D % 4 != 0
    assert not model._ssl_fused(1)
