"""Plain float64 PyTorch restatement of XLNet's relative attention core (ops.rel_attention; modeling_xlnet_x.py:256-320, bi, no
mems / segments), its gradients by autograd, and the error measure its tests share.  No call into vilco_amd.

The operation, per clip b and head h (heads are channel slices of the token-major tensors; T queries, T keys, 2T positions):
    bd[i][p]  = qr_i . kr_p                      kr [2T, C] shared by the batch, or [B, 2T, C] per clip
    pos[i][j] = bd[i][T - i + j]                 rel_shift_bnij (glue_restatement.relshift): only p in [T - i, 2T - i) is picked
    s[i][j]   = (qw_i . k_j + pos[i][j]) * scale - 1e30 * ((j >= len[b]) & (j != i))
    p         = softmax over j (times the optional keep mask, already scaled by 1 / (1 - drop_p))
    o_i       = sum_j p[i][j] v_j
A query always sees its own position, so no row is empty; a row with ONE visible key (len 0: every row; len 1: row 0; T = 1)
has the constant softmax 1 and takes no part in dqw, dqr, dk or dkr: in float64 these come out exactly zero (1e30 swallows any
score, exp(-1e30 - max) is 0, and autograd's p (g - sum p g) is g_i - g_i).  Position p = 0 is picked by no (i, j) (T - i + j >= 1):
row 0 of dkr is exactly zero.

tests/test_xl_attention_restatement_cpu.py holds this file to the gather form of the shift, to the formula as
tests/test_ops_gpu.py::test_rel_attention writes it out, and to the attention core of oracle.mq_oracle.xlnet_layer;
tests/test_xl_attention_edges_gpu.py holds the HIP kernels to it."""
import torch

import glue_restatement as G
from local_attention_restatement import rel          # noqa: F401  (the measure: per batch element, exact zeros where the reference is zero)

NAMES = ("o", "dqw", "dqr", "dk", "dv", "dkr")


def band_mask(T):
    """[T, 2T] bool: p in [T - i, 2T - i), the entries of row i of the unshifted scores that rel_shift_bnij keeps"""
    i, p = torch.arange(T)[:, None], torch.arange(2 * T)[None, :]
    return (p >= T - i) & (p < 2 * T - i)


def position_scores(qr, kr, H):
    """qr [B, T, H*hd], kr [2T, H*hd] or [B, 2T, H*hd] -> bd [B, H, T, 2T] in the dtype of the inputs"""
    B, T, C = qr.shape
    hd = C // H
    qh = qr.view(B, T, H, hd).transpose(1, 2)                               # [B, H, T, hd]
    if kr.dim() == 2:
        kh = kr.view(2 * T, H, hd).transpose(0, 1)[None]                    # [1, H, 2T, hd]
    else:
        kh = kr.view(B, 2 * T, H, hd).transpose(1, 2)                       # [B, H, 2T, hd]
    return qh @ kh.transpose(-1, -2)


def xl_mask(lens, T):
    """[B, 1, T, T] bool: key j is hidden from query i of clip b  (j >= len[b] and j != i)"""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    return ((j[None] >= lens.long().cpu()[:, None, None]) & (j != i)[None])[:, None]


def attention(qw, qr, k, v, kr, lens, H, scale, keep=None, bd_hook=None):
    """qw, qr, k, v [B, T, H*hd], kr [2T, H*hd] or [B, 2T, H*hd] (any float dtype; computed in float64), lens [B],
    keep [B, H, T, T] or None -> o [B, T, H*hd] (float64, on the autograd graph of float64 leaves).
    bd_hook(bd) -> bd: lets a test disturb the unshifted scores before the shift."""
    qw, qr, k, v, kr = [t.double() for t in (qw, qr, k, v, kr)]
    B, T, C = qw.shape
    hd = C // H
    qh, kh, vh = [t.view(B, T, H, hd).transpose(1, 2) for t in (qw, k, v)]
    bd = position_scores(qr, kr, H)
    if bd_hook is not None:
        bd = bd_hook(bd)
    pos = G.relshift(bd.reshape(B * H, T, 2 * T)).reshape(B, H, T, T)
    s = (qh @ kh.transpose(-1, -2) + pos) * scale - 1e30 * xl_mask(lens, T).double()
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep.double()
    return (p @ vh).transpose(1, 2).reshape(B, T, C)


def reference(qw, qr, k, v, kr, lens, H, scale, dout, keep=None):
    """-> dict o, dqw, dqr, dk, dv, dkr (float64) for the upstream gradient dout"""
    leaves = [t.detach().double().cpu().clone().requires_grad_(True) for t in (qw, qr, k, v, kr)]
    o = attention(*leaves, lens, H, scale, None if keep is None else keep.detach().cpu())
    o.backward(dout.detach().double().cpu())
    return dict(o=o.detach(), dqw=leaves[0].grad, dqr=leaves[1].grad, dk=leaves[2].grad, dv=leaves[3].grad, dkr=leaves[4].grad)


def rel_of(name, got, want):
    """rel() of one of NAMES: a shared kr's gradient ([2T, C]) is measured over the whole tensor, everything else per batch
    element.  AssertionError where a zero reference slice is not zero in `got`."""
    if name == "dkr" and want.dim() == 2:
        return rel(got[None], want[None])
    return rel(got, want)
