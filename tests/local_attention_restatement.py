"""Plain float64 PyTorch restatement of sliding-window attention (mask mode 4 of vilco_attn_fwd / vilco_attn_bwd,
ops.MASK_LOCAL: NLQ's LocalMaskedMHCA), its gradients by autograd, and the error measure its tests share.  No call into
vilco_amd.

The operation, per clip b and head h (heads are channel slices of the token-major tensors):
    s[i][j] = scale * q_i . k_j            for keys j < len[b] with |i - j| <= window, -inf for every other key
    p       = softmax over the remaining keys (times the optional keep mask, already scaled by 1 / (1 - drop_p))
    o_i     = sum_j p[i][j] v_j
A query row with no remaining key (i - window >= len[b], or len[b] = 0) gives an all-zero output row and takes part in no
gradient: the kernels' `inv = l_run > 0 ? 1 / l_run : 0`.

tests/test_local_attention_restatement_cpu.py holds this file to a per-row loop and to the band core of
oracle.nlq_oracle.local_mhca; tests/test_local_attention_edges_gpu.py holds the HIP kernels to it."""
import math

import torch


def band(lens, T, window):
    """[B, T, T] bool: key j is visible to query i of clip b  (j < len[b] and |i - j| <= window)"""
    idx = torch.arange(T)
    near = (idx[:, None] - idx[None, :]).abs() <= int(window)
    return near[None] & (idx[None, None, :] < lens.long().cpu()[:, None, None])


def row_has_key(lens, T, window):
    """[B, T] bool: query row i of clip b has at least one visible key"""
    return band(lens, T, window).any(dim=-1)


def attention(q, k, v, lens, H, scale, window, keep=None):
    """q, k, v [B, T, H*hd] (any float dtype; computed in float64), lens [B], keep [B, H, T, T] or None -> o [B, T, H*hd]
    (float64, on the autograd graph of q, k, v when they are float64 leaves)."""
    q, k, v = q.double(), k.double(), v.double()
    B, T, C = q.shape
    hd = C // H
    qh, kh, vh = [t.view(B, T, H, hd).transpose(1, 2) for t in (q, k, v)]
    ok = band(lens, T, window)[:, None]                                   # [B, 1, T, T]
    live = ok.any(dim=-1, keepdim=True)                                   # [B, 1, T, 1]
    s = (scale * qh) @ kh.transpose(-1, -2)
    s = s.masked_fill(~ok, float("-inf"))
    s = s.masked_fill(~live, 0.0)                                         # a dead row: any finite number, zeroed below
    p = torch.softmax(s, dim=-1).masked_fill(~live, 0.0)                  # masked_fill: no gradient through a dead row
    if keep is not None:
        p = p * keep.double()
    return (p @ vh).transpose(1, 2).reshape(B, T, C)


def reference(q, k, v, lens, H, scale, window, dout, keep=None):
    """-> dict o, dq, dk, dv (float64) for the upstream gradient dout"""
    qd, kd, vd = [t.detach().double().cpu().clone().requires_grad_(True) for t in (q, k, v)]
    o = attention(qd, kd, vd, lens, H, scale, window, None if keep is None else keep.detach().cpu())
    o.backward(dout.detach().double().cpu())
    return dict(o=o.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)


def rel(got, want):
    """The measure of tests/test_ops_gpu.py -- max|got - want| / max|want| -- taken per batch element (dim 0); returns the
    worst.  A slice whose reference is identically zero has no scale: it must be identically zero in `got` too (either sign;
    NaN is not zero), else AssertionError."""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert g.shape == w.shape, (tuple(g.shape), tuple(w.shape))
    worst = 0.0
    for b in range(g.shape[0]):
        gb, wb = g[b], w[b]
        if gb.numel() == 0:
            continue
        m = float(wb.abs().max())
        if m == 0.0:
            bad = int(torch.count_nonzero(gb)) + int(torch.isnan(gb).sum())
            assert bad == 0, "batch element %d: %d non-zero entries where the reference is identically zero (max |got| %.3e)" % (
                b, bad, float(gb.abs().nan_to_num(nan=math.inf).max()))
            continue
        if bool(torch.isnan(gb).any()):
            return math.inf
        worst = max(worst, float((gb - wb).abs().max()) / m)
    return worst
