"""XLNet's relative attention at hd = 64 (mask mode 3, fp16 x2) through the C ABI where ops.rel_attention never goes: the
forward on the hd = 64 XL kernel, then a backward that asks for NO dS (dbias, dbias_amax and ds_planes null).  The XL backward
kernels exist to produce dS, so this backward runs the general dQ and dK/dV kernels -- the only ones that read the transposed
planes of q, dO and k, which the call must therefore have packed -- behind the XL forward's o and lse.

B 1, H 2, T 130: two query workgroups of the forward (128 rows each), three query tiles of the general backward, a ragged
tail everywhere, Tk no multiple of 64, 11 masked keys.  Outputs sit NaN-filled between canaries, the workspace between guard
bytes.  Compared with a float64 restatement of modeling_xlnet_x.py:256-320 (unshifted position scores, XLNet mask, dropout on
the probabilities with the kernels' own mask) at tests/test_ops_gpu.py's attention tolerance."""
import ctypes

import pytest
import torch

from glue_restatement import guarded

pytestmark = pytest.mark.gpu

TOL_GEMM = 2e-5            # tests/test_ops_gpu.py: its bar for every attention comparison, and its measure


def rel(got, want):
    want, got = want.double().cpu(), got.double().cpu()
    return ((got - want).abs().max() / (want.abs().max() + 1e-12)).item()


B, H, HD, T, LEN = 1, 2, 64, 130, 119
C = H * HD
SCALE = 0.125
MODE_XL, F16X2 = 3, 3
WS_PAD = 512


def reference(q, k, v, bd, g, keep):
    """float64: o and the gradients of q, k, v for upstream g; keep: dropout factors [B, H, T, T] or None"""
    qd, kd, vd = [t.double().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = [t.view(B, T, H, HD).transpose(1, 2) for t in (qd, kd, vd)]
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    pos = bd.double().gather(3, (T - i + j).expand(B, H, T, T))          # rel_shift: bd[b, h, i, T - i + j]
    s = (qh @ kh.transpose(-1, -2) + pos) * SCALE
    s = s - 1e30 * ((j >= LEN) & (j != i)).double()                      # padded keys, except a query's own position
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep.double()
    o = (p @ vh).transpose(1, 2).reshape(B, T, C)
    o.backward(g.double())
    return o.detach(), qd.grad, kd.grad, vd.grad


def run(dev, drop_p):
    """the two calls with guarded buffers -> ({name: output}, float64 reference (o, dq, dk, dv))"""
    from vilco_amd import _lib, ops
    lib = _lib.load()
    torch.manual_seed(41)
    q, k, v, g = [torch.randn(B, T, C) for _ in range(4)]
    bd = torch.randn(B, H, T, 2 * T)
    seed = 1234
    assert lib.vilco_attn_planes_supported(T, T, HD, MODE_XL, F16X2, 1, drop_p) == 1, "not the hd = 64 XL forward"
    keep = ops.dropout_mask(drop_p, seed, (B, H, T, T), dev, "attn_prob").cpu() if drop_p else None
    want = reference(q, k, v, bd, g, keep)

    qg, kg, vg, gg, bdg = [t.to(dev) for t in (q, k, v, g, bd)]
    lens = torch.tensor([LEN], dtype=torch.int32, device=dev)
    (o, c_o), (lse, c_lse) = guarded(B * T * C, dev), guarded(B * H * T, dev)
    (dq, c_dq), (dk, c_dk), (dv, c_dv) = [guarded(B * T * C, dev) for _ in range(3)]
    nws = max(int(lib.vilco_attn_fwd_workspace(B, H, T, T, HD, F16X2)), int(lib.vilco_attn_bwd_workspace(B, H, T, T, HD, F16X2)))
    ws = torch.full((nws + 2 * WS_PAD,), 0xA5, dtype=torch.uint8, device=dev)
    ws_off = (-ws.data_ptr()) % 256 + 256

    def call(fn, nbytes, **kw):
        d = _lib.AttnDesc(q=qg.data_ptr(), k=kg.data_ptr(), v=vg.data_ptr(), bias=bdg.data_ptr(), kv_len=lens.data_ptr(),
                          o=o.data_ptr(), lse=lse.data_ptr(), B=B, H=H, Tq=T, Tk=T, hd=HD, scale=SCALE, mode=MODE_XL,
                          precision=F16X2, drop_p=drop_p, drop_seed=seed, workspace=ws.data_ptr() + ws_off,
                          workspace_bytes=int(nbytes), **kw)
        rc = fn(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()
        return rc

    assert call(lib.vilco_attn_fwd, lib.vilco_attn_fwd_workspace(B, H, T, T, HD, F16X2)) == 0
    assert call(lib.vilco_attn_bwd, lib.vilco_attn_bwd_workspace(B, H, T, T, HD, F16X2),
                dout=gg.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr()) == 0
    for c in (c_o, c_lse, c_dq, c_dk, c_dv):
        c()
    w = ws.cpu()
    assert bool((w[:ws_off] == 0xA5).all()), "write in front of the workspace"
    assert bool((w[ws_off + nws:] == 0xA5).all()), "write past the end of the workspace"
    return dict(o=o, dq=dq, dk=dk, dv=dv, lse=lse), want


@pytest.mark.parametrize("drop_p", [0.0, 0.2])
def test_xl64_forward_then_backward_without_ds(dev, drop_p):
    got, want = run(dev, drop_p)
    assert bool(torch.isfinite(got["lse"]).all())
    for name, ref in zip(("o", "dq", "dk", "dv"), want):
        e = rel(got[name].view(B, T, C), ref)
        print("drop_p %.1f  %-2s  %.3e (bar %.1e)" % (drop_p, name, e, TOL_GEMM))
        assert e < TOL_GEMM, (name, e)
