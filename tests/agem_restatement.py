"""float64 restatement of the A-GEM projection (Chaudhry et al., ICLR 2019, "Efficient Lifelong Learning with A-GEM", eq. 11) as
vilco_agem_project defines it (include/vilco_hip.h), in plain torch on the CPU, written from the definition.  Nothing here is
shared with the code under test.

g = all gradients, r = all reference gradients, each taken as ONE vector over the tensors of the call:
  g.r < 0 and r.r > 0:   g <- g - alpha r,  alpha = g.r / r.r   (negative)
  otherwise:             alpha = 0, g unchanged."""
import optim_restatement as R

CHUNK = R.CHUNK          # elements per chunk of the multi-tensor kernels (the tests' own statement of it)


def _d(x):
    return x.detach().double().cpu().reshape(-1)


def project(grads, refs):
    """-> (dot, rr, alpha, projected, abs_dot): the two sums over all tensors, alpha as above, the projected gradients (flat
    float64 tensors, one per input) and sum |g r|, the magnitude the rounding bound of the dot is made of."""
    assert len(grads) == len(refs)
    dot = rr = abs_dot = 0.0
    for g, r in zip(grads, refs):
        g, r = _d(g), _d(r)
        assert g.numel() == r.numel()
        dot += float((g * r).sum())
        rr += float((r * r).sum())
        abs_dot += float((g * r).abs().sum())
    alpha = dot / rr if (dot < 0.0 and rr > 0.0) else 0.0
    projected = [_d(g) - alpha * _d(r) for g, r in zip(grads, refs)]
    return dot, rr, alpha, projected, abs_dot


def inputs(sizes, k, seed):
    """the GPU tests' inputs: per size a reference gradient r ~ N(0, 1) and g = noise + k r (fp32 CPU tensors).  k = -0.5: g.r is
    about -0.5 r.r, a conflict decided far outside any rounding bound; k = +0.5: the two agree as clearly."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    gs, rs = [], []
    for n in sizes:
        r = torch.randn(n, generator=gen)
        gs.append(torch.randn(n, generator=gen) + k * r)
        rs.append(r)
    return gs, rs
