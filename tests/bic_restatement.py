"""Restatement of BiC stage 2 (csrc/bic.hip, vilco_amd/cl_methods/bic.py) in plain torch on the CPU, in any dtype: the
objective through a `BiasLayer` and the focal loss, its gradient by autograd, the trajectory by torch.optim.SGD.  It reads
the same cache arrays and the same `order` as the kernels.

`focal` is `vilco_amd.modeling.losses.sigmoid_focal_loss` without that function's cast to float32 (which would make a
float64 run impossible); tests/test_bic_cpu.py checks that the two agree in float32.
"""
import torch
import torch.nn.functional as F

from vilco_amd.modeling.meta_archs import BiasLayer


def focal(inputs, targets, alpha=0.25, gamma=2.0):
    p = torch.sigmoid(inputs)
    ce = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * ((1 - p_t) ** gamma)
    return (alpha * targets + (1 - alpha) * (1 - targets)) * loss


def unpack_bits(label_bits, C):
    """int64 [N, 2] -> 0/1 [N, C] (float64)"""
    c = torch.arange(C)
    return ((label_bits[:, c // 64] >> (c % 64)) & 1).to(torch.float64)


def rows_of(clip_ptr, clips):
    ptr = clip_ptr.tolist()
    idx = [torch.arange(ptr[c], ptr[c + 1]) for c in clips]
    return torch.cat(idx) if idx else torch.zeros(0, dtype=torch.int64)


def objective(arrays, clips, lo, hi, smoothing, layer, dtype):
    """L over the clips `clips`; arrays = (logits, label_bits, weight, pos, clip_ptr) as CPU tensors"""
    logits, bits, weight, pos, clip_ptr = arrays
    C = logits.shape[1]
    r = rows_of(clip_ptr, clips)
    x = logits[r][:, lo:hi].to(dtype)
    t = (unpack_bits(bits[r], C)[:, lo:hi] * (1 - smoothing) + smoothing / (C + 1)).to(dtype)
    w = weight[r].to(dtype)
    P = max(float(pos[r].sum()), 1.0)
    return (focal(layer(x), t).sum(-1) * w).sum() / P


def make_layer(ab, dtype):
    layer = BiasLayer().to(dtype)
    with torch.no_grad():
        layer.alpha.fill_(ab[0])
        layer.beta.fill_(ab[1])
    return layer


def evaluate(arrays, lo, hi, smoothing, ab, dtype):
    """(L, dL/dalpha, dL/dbeta) over all clips, as python floats"""
    layer = make_layer(ab, dtype)
    L = objective(arrays, range(arrays[4].numel() - 1), lo, hi, smoothing, layer, dtype)
    L.backward()
    return float(L), float(layer.alpha.grad), float(layer.beta.grad)


def trajectory(arrays, order, batch_clips, lo, hi, smoothing, lr, dtype, ab0=(1.0, 0.0)):
    """plain SGD over order[k * batch_clips : (k + 1) * batch_clips] per step -> ((alpha, beta), [loss of every step])"""
    layer = make_layer(ab0, dtype)
    opt = torch.optim.SGD(layer.parameters(), lr=lr)
    losses = []
    for k in range(len(order) // batch_clips):
        opt.zero_grad()
        L = objective(arrays, order[k * batch_clips:(k + 1) * batch_clips], lo, hi, smoothing, layer, dtype)
        L.backward()
        opt.step()
        losses.append(float(L))
    return (float(layer.alpha), float(layer.beta)), losses


def synthetic_cache(seed, clip_rows, C, no_pos_clips=()):
    """logits ~ N(0, 3), about 5 % of the label bits set, weights in [0, 1] with a fifth of the rows exactly 0; pos = a row
    with a label and a weight.  The clips in `no_pos_clips` carry no label at all (their steps have P = 0)."""
    g = torch.Generator().manual_seed(seed)
    N = sum(clip_rows)
    ptr = torch.tensor([0] + list(clip_rows), dtype=torch.int64).cumsum(0).to(torch.int32)
    logits = 3.0 * torch.randn(N, C, generator=g)
    on = torch.rand(N, C, generator=g) < 0.05
    for c in no_pos_clips:
        on[ptr[c]:ptr[c + 1]] = False
    weight = torch.rand(N, generator=g)
    weight[torch.rand(N, generator=g) < 0.2] = 0.0
    pos = (on.any(-1) & (weight > 0)).to(torch.uint8)
    from vilco_amd.cl_methods.bic import BiCCache
    bits = BiCCache.pack_bits(on.to(torch.float32))
    return logits.contiguous(), bits.contiguous(), weight.contiguous(), pos.contiguous(), ptr
