"""CPU: tests/xl_attention_restatement.py pinned from outside, all in float64 (the bars are float64 roundoff):

1. its shift (glue_restatement.relshift) against the gather form pos[i][j] = bd[i][T - i + j], and against the formula as
   tests/test_ops_gpu.py::test_rel_attention.ref writes it out (ibnd einsums, the reshape of rel_shift_bnij, the mask from a
   float pad vector minus the identity): the same o and the same five gradients;
2. entries of bd outside band_mask(T) have no influence: moved by 1e3, every output stays bit-identical;
3. row 0 of dkr is exactly zero (position p = 0 is picked by no (i, j));
4. the attention core of oracle.mq_oracle.xlnet_layer, which tests/test_oracle_model.py pins to the reference goldens.  The
   layer's signature does not expose the core (projections in front, output projection, LayerNorm and feed-forward behind), so
   the tensors its three core einsums take and give are recorded on the way through, as
   test_local_attention_restatement_cpu.py records the band core of the NLQ oracle.

T in {1, 2, 5, 64, 65}, kr shared and per clip, lens with T, 1 and a value in between (and 0: the empty clip)."""
import pytest
import torch

import xl_attention_restatement as XL

EPS = 1e-12
TS = [1, 2, 5, 64, 65]


def _lens(T):
    return torch.tensor([T, 1, max(1, T // 2)], dtype=torch.int32)


def _inputs(T, per_clip, B=3, H=2, hd=4, seed=0):
    g = torch.Generator().manual_seed(100 * T + 7 * int(per_clip) + seed)
    qw, qr, k, v, dout = [torch.randn(B, T, H * hd, generator=g, dtype=torch.float64) for _ in range(5)]
    kr = torch.randn(*((B,) if per_clip else ()), 2 * T, H * hd, generator=g, dtype=torch.float64)
    return qw, qr, k, v, kr, dout


def _grads(fn, tensors, dout):
    leaves = [t.clone().requires_grad_(True) for t in tensors]
    o = fn(*leaves)
    o.backward(dout)
    return dict(zip(XL.NAMES, [o.detach()] + [t.grad for t in leaves[:4]] + [leaves[4].grad]))


def _gather_form(qw, qr, k, v, kr, lens, H, scale, keep=None):
    B, T, C = qw.shape
    hd = C // H
    qh, kh, vh = [t.view(B, T, H, hd).transpose(1, 2) for t in (qw, k, v)]
    bd = XL.position_scores(qr, kr, H)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    pos = bd.gather(3, (T - i + j).expand(B, H, T, T))
    s = (qh @ kh.transpose(-1, -2) + pos) * scale
    s = s - 1e30 * ((j[None] >= lens.long()[:, None, None]) & (j != i)[None]).double()[:, None]
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep
    return (p @ vh).transpose(1, 2).reshape(B, T, C)


def _ibnd_form(qw, qr, k, v, kr, lens, H, scale):
    """test_ops_gpu.py::test_rel_attention.ref, with kr of either layout"""
    B, T, C = qw.shape
    hd = C // H
    f = lambda x: x.view(B, T, H, hd).permute(1, 0, 2, 3)          # ibnd
    ac = torch.einsum("ibnd,jbnd->bnij", f(qw), f(k))
    if kr.dim() == 2:
        krr = kr.view(2 * T, 1, H, hd).expand(2 * T, B, H, hd)
    else:
        krr = kr.view(B, 2 * T, H, hd).permute(1, 0, 2, 3)
    bd = torch.einsum("ibnd,jbnd->bnij", f(qr), krr)
    xs = bd.shape
    bd = bd.reshape(xs[0], xs[1], xs[3], xs[2])[:, :, 1:, :].reshape(xs[0], xs[1], xs[2], xs[3] - 1)[:, :, :, :T]
    score = (ac + bd) * scale
    pad = (~(torch.arange(T)[None, :] < lens.long()[:, None])).double()                          # [B, T(j)]
    mask = ((pad[:, None, None, :] - torch.eye(T, dtype=torch.float64)[None, None]) > 0).double()
    score = score - 1e30 * mask
    p = torch.softmax(score, dim=3)
    o = torch.einsum("bnij,jbnd->ibnd", p, f(v))
    return o.permute(1, 0, 2, 3).reshape(B, T, C)


@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("T", TS)
def test_gather_form_equals_reshape_form(T, per_clip):
    H, scale = 2, 0.4
    qw, qr, k, v, kr, dout = _inputs(T, per_clip)
    lens = _lens(T)
    want = XL.reference(qw, qr, k, v, kr, lens, H, scale, dout)
    for tag, form in (("gather", _gather_form), ("ibnd", _ibnd_form)):
        got = _grads(lambda *t: form(*t, lens, H, scale), (qw, qr, k, v, kr), dout)
        for n in XL.NAMES:
            e = float((got[n] - want[n]).abs().max())
            print("T %d %-6s %-3s max abs difference %.3e" % (T, tag, n, e))
            assert got[n].shape == want[n].shape and e < EPS, (tag, n, e)
    keep = (torch.rand(3, H, T, T, generator=torch.Generator().manual_seed(5)) >= 0.3).double() / 0.7
    want = XL.reference(qw, qr, k, v, kr, lens, H, scale, dout, keep)
    got = _grads(lambda *t: _gather_form(*t, lens, H, scale, keep), (qw, qr, k, v, kr), dout)
    for n in XL.NAMES:
        assert float((got[n] - want[n]).abs().max()) < EPS, ("keep", n)


@pytest.mark.parametrize("T", TS)
def test_band_mask(T):
    m = XL.band_mask(T)
    assert m.shape == (T, 2 * T) and m.dtype == torch.bool
    assert m.sum(dim=1).tolist() == [T] * T
    picked = torch.zeros(T, 2 * T, dtype=torch.bool)
    for i in range(T):
        for j in range(T):
            picked[i, T - i + j] = True
    assert torch.equal(m, picked)
    assert not bool(m[:, 0].any())


@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("T", TS)
def test_scores_outside_the_band_have_no_influence(T, per_clip):
    H, scale = 2, 0.4
    qw, qr, k, v, kr, dout = _inputs(T, per_clip, seed=1)
    lens = _lens(T)
    outside = (~XL.band_mask(T)).double()

    def run(hook):
        return _grads(lambda *t: XL.attention(*t, lens, H, scale, bd_hook=hook), (qw, qr, k, v, kr), dout)
    plain = run(None)
    moved = run(lambda bd: bd + 1e3 * outside)
    inside = run(lambda bd: bd + 1e3 * (1.0 - outside) * torch.arange(2 * T, dtype=torch.float64))
    for n in XL.NAMES:
        assert torch.equal(plain[n], moved[n]), n
    if T > 1:
        assert not torch.equal(plain["o"], inside["o"])           # (the hook does reach the scores)


@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("T", TS)
def test_position_zero_takes_no_gradient_and_one_key_rows_none_at_all(T, per_clip):
    H, scale = 2, 0.4
    qw, qr, k, v, kr, dout = _inputs(T, per_clip, seed=2)
    r = XL.reference(qw, qr, k, v, kr, _lens(T), H, scale, dout)
    assert int(torch.count_nonzero(r["dkr"][..., 0, :])) == 0
    if T > 1:
        assert int(torch.count_nonzero(r["dkr"][..., 1, :])) > 0
    for t in r.values():
        assert bool(torch.isfinite(t).all())
    # clip 1 has len 1: row 0 sees one key.  An empty clip: every row does.
    assert int(torch.count_nonzero(r["dqw"][1, 0])) == 0 and int(torch.count_nonzero(r["dqr"][1, 0])) == 0
    r0 = XL.reference(qw, qr, k, v, kr, torch.tensor([T, 0, 1], dtype=torch.int32), H, scale, dout)
    for n in ("dqw", "dqr", "dk"):
        assert int(torch.count_nonzero(r0[n][1])) == 0, n
    if per_clip:
        assert int(torch.count_nonzero(r0["dkr"][1])) == 0
    assert torch.equal(r0["dv"][1], dout[1])                       # p = 1 on the diagonal: o = v, dv = dout
    assert XL.rel(r0["o"][1:2], v[1:2]) == 0.0


def test_restatement_equals_the_oracle_attention_core(monkeypatch):
    """oracle.mq_oracle.xlnet_layer on random parameters, with the dropout factors of the probabilities given: the operands of
    its two score einsums (q + r_w_bias with k, q + r_r_bias with kr) and of its value einsum are recorded on the way through;
    a loss on the value einsum's output gives the gradients of exactly those operands."""
    from oracle import mq_oracle as M
    B, T, D, H, hd, inner = 2, 7, 8, 2, 4, 8
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = {"x.rel_attn." + n: rn(D, H, hd) * 0.5 for n in ("q", "k", "v", "r", "o")}
    p.update({"x.rel_attn.r_w_bias": rn(H, hd), "x.rel_attn.r_r_bias": rn(H, hd),
              "x.rel_attn.layer_norm.weight": rn(D), "x.rel_attn.layer_norm.bias": rn(D),
              "x.ff.layer_1.weight": rn(inner, D), "x.ff.layer_1.bias": rn(inner), "x.ff.layer_2.weight": rn(D, inner),
              "x.ff.layer_2.bias": rn(D), "x.ff.layer_norm.weight": rn(D), "x.ff.layer_norm.bias": rn(D)})
    for t in p.values():
        t.requires_grad_(True)                                      # so that every recorded operand is on the graph
    lens = torch.tensor([T, 3], dtype=torch.int32)
    mask = torch.arange(T)[None, :] < lens[:, None]
    keep =(torch.rand(B, H, T, T, generator=g) >= 0.25).double() / 0.75
    ones = lambda *s: torch.ones(*s, dtype=torch.float64)
    drop = {"xl_input": ones(B, T, D), "xl_pos_emb": (torch.rand(B, 2 * T, D, generator=g) >= 0.25).double() / 0.75,
            "attn_prob": keep, "xl_attn_out": ones(B, T, D), "xl_ff_inner": ones(B, T, inner), "xl_ff_out": ones(B, T, D),
            "xl_output": ones(B, T, D)}
    seen = []
    einsum = torch.einsum

    def recording(eq, *ops):
        y = einsum(eq, *ops)
        if eq in ("ibnd,jbnd->bnij", "bnij,jbnd->ibnd"):
            for t in ops:
                t.retain_grad()
            seen.append((eq, ops, y))
        return y
    monkeypatch.setattr(torch, "einsum", recording)
    M.xlnet_layer(p, "x.", rn(B, T, D).requires_grad_(True), mask, H, drop)
    monkeypatch.undo()
    assert [s[0] for s in seen] == ["ibnd,jbnd->bnij", "ibnd,jbnd->bnij", "bnij,jbnd->ibnd"]
    (qw, k), (qr, kr), (_, v) = [s[1] for s in seen]                # [T (2T), B, H, hd]
    vec = seen[2][2]
    tm = lambda t: t.detach().permute(1, 0, 2, 3).reshape(B, t.shape[0], H * hd)      # token-major [B, T, C]
    w = rn(B, T, H * hd)
    (vec.permute(1, 0, 2, 3).reshape(B, T, H * hd) * w).sum().backward()
    r = XL.reference(tm(qw), tm(qr), tm(k), tm(v), tm(kr), lens, H, 1.0 / hd ** 0.5, w, keep)
    got = dict(o=tm(vec), dqw=tm(qw.grad), dqr=tm(qr.grad), dk=tm(k.grad), dv=tm(v.grad), dkr=tm(kr.grad))
    for n in XL.NAMES:
        e = XL.rel(got[n], r[n])
        print("%-3s %.3e" % (n, e))
        assert e < EPS, (n, e)
