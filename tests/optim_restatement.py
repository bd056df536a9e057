"""float64 restatement of what vilco_amd/csrc/optim.hip computes at the end of every training iteration: the global-norm clip
coefficient (torch.nn.utils.clip_grad_norm_), one AdamW / SGD-momentum update (torch.optim) and the EWC / MAS penalty with the
gradient it adds (EWC.py:6-22 / MAS.py:5-21), in plain torch on the CPU.  Nothing here is shared with the code under test.

Hyperparameters (max_norm, lr, weight_decay, betas, eps, momentum, lambda) enter as their fp32-rounded values: the C ABI
carries `float`, so that rounding is by design and not an error of the kernels.  Every function rounds them itself (`f32`); a
caller that compares with torch.optim hands torch.optim the rounded values too.  The clip coefficient `coef` is taken as it
comes: the kernels read it from device memory, a test of one update hands over the device's fp32 value.

Besides the result every function returns the magnitudes the rounding bounds of tests/test_optim_edges_gpu.py are made of:
|p_old|, the size of the update with its addends taken absolutely, and the absolute addends of each moving average."""
import math

import numpy as np
import torch


CHUNK = 16384          # elements per chunk of the multi-tensor kernels, stated here on its own: not read from the library


def chunk_lists(numels, chunk=CHUNK):
    """(chunk_tensor, chunk_off, first) of a vilco_chunk_table as host lists: tensor i is cut into chunks of `chunk` elements at
    offsets 0, chunk, ...; first[i] .. first[i + 1] are its chunks (first has len(numels) + 1 entries).  The tests' own
    statement of the walking convention: vilco_amd.ops.ChunkPlan is held against it, and is not used to build it."""
    ct, co, first = [], [], []
    for i, n in enumerate(numels):
        first.append(len(ct))
        for off in range(0, n, chunk):
            ct.append(i)
            co.append(off)
    first.append(len(ct))
    return ct, co, first


class Table:
    """a vilco_chunk_table on the device, built by hand: `ptr_rows` = the address rows [rows][n], `numels` = elements per entry;
    empty lists are padded to one element so that no address is null.  `struct()` is the ctypes mirror of it."""

    def __init__(self, dev, ptr_rows, numels):
        self.numels, self.n, self.nrows, self.dev = list(numels), len(numels), len(ptr_rows), dev
        ct, co, self.first = chunk_lists(self.numels)
        self.nchunks = len(ct)
        self.ptrs = torch.tensor(ptr_rows if self.n else [[0]] * self.nrows, dtype=torch.int64).to(dev)
        self.numel = torch.tensor(self.numels or [0], dtype=torch.int64).to(dev)
        self.ct = torch.tensor(ct or [0], dtype=torch.int32).to(dev)
        self.co = torch.tensor(co or [0], dtype=torch.int64).to(dev)
        self.partial = torch.full((max(self.nchunks, 1),), float('nan'), device=dev)

    def struct(self, **kw):
        from vilco_amd import _lib
        f = dict(ptrs=self.ptrs.data_ptr(), numel=self.numel.data_ptr(), chunk_tensor=self.ct.data_ptr(), chunk_off=self.co.data_ptr(),
                 rows=self.nrows, n=self.n, nchunks=self.nchunks, chunk=CHUNK)
        f.update(kw)
        return _lib.ChunkTable(**f)


def f32(x):
    """the double that a C `float` argument carries"""
    return float(np.float32(x))


def _d(x):
    return x.detach().double().cpu()


def clip(grads, max_norm):
    """(norm, coef): norm = sqrt(sum over all tensors of sum g^2), coef = min(1, max_norm / (norm + 1e-6)), or 1 when
    max_norm <= 0 (no clipping)."""
    sq = 0.0
    for g in grads:
        g = _d(g)
        sq += float((g * g).sum())
    norm = math.sqrt(sq)
    max_norm = f32(max_norm)
    coef = 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + 1e-6))
    return norm, coef


def adamw_step(p, g, m, v, step, lr, wd, beta1, beta2, eps, coef=1.0):
    """torch.optim.AdamW (decoupled decay), one tensor, one step; `step` is the count AFTER this update, `coef` scales g.
    Returns (p_new, m_new, v_new, mags) with mags = {'p_old', 'delta', 'm_terms', 'v_terms'}: |p_old|; the update
    step_size * (|beta1 m| + |(1 - beta1) g|) / denom, which is |p_new - decayed p| when the two addends of m agree in sign
    and larger otherwise; the two absolute addends of m and of v."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    lr, wd, beta1, beta2, eps = f32(lr), f32(wd), f32(beta1), f32(beta2), f32(eps)
    g = g * coef
    m1, m2 = beta1 * m, (1.0 - beta1) * g
    v1, v2 = beta2 * v, (1.0 - beta2) * g * g
    m_new, v_new = m1 + m2, v1 + v2
    bc1, bc2 = 1.0 - beta1 ** float(step), 1.0 - beta2 ** float(step)
    step_size = lr / bc1
    denom = v_new.sqrt() / math.sqrt(bc2) + eps
    p_new = p * (1.0 - lr * wd) - step_size * (m_new / denom)
    mags = dict(p_old=p.abs(), delta=step_size * (m1.abs() + m2.abs()) / denom, m_terms=(m1.abs(), m2.abs()),
                v_terms=(v1.abs(), v2.abs()))
    return p_new, m_new, v_new, mags


def sgd_step(p, g, buf, step, lr, wd, momentum, coef=1.0):
    """torch.optim.SGD with momentum (no dampening, no nesterov): d = coef g + wd p; buf = d on the parameter's first step
    (step <= 1: what `buf` holds is not read), else momentum buf + d; p -= lr buf.
    Returns (p_new, buf_new, mags) with mags = {'p_old', 'delta', 'buf_terms'}: delta = lr * (sum of the absolute addends of
    buf_new), buf_terms = (|momentum buf| or 0, |coef g|, |wd p|)."""
    p, g = _d(p), _d(g)
    lr, wd, momentum = f32(lr), f32(wd), f32(momentum)
    t_g, t_p = coef * g, wd * p
    t_b = torch.zeros_like(p) if step <= 1 else momentum * _d(buf)
    buf_new = t_b + (t_g + t_p)
    p_new = p - lr * buf_new
    terms = (t_b.abs(), t_g.abs(), t_p.abs())
    return p_new, buf_new, dict(p_old=p.abs(), delta=lr * (terms[0] + terms[1] + terms[2]), buf_terms=terms)


def penalty(params, grads, entries, lam):
    """lam * sum over entries of sum F (opt - p[:len(opt)])^2 and the gradients after -2 lam F (opt - p) was added to them.
    entries: (param index, importance, optpar) triples; importance and optpar cover the first optpar.numel() elements of the
    flattened parameter (rows a class head gained in dim 0 since the task was consolidated are not touched).
    Returns (value, new_grads, mags): new_grads in the parameters' shapes, mags = {'abs_sum': per parameter |g_old| + sum of
    the absolute added terms, 'touched': per parameter the number of entries that touch each element, 'value_abs': lam * sum of
    |F| (opt - p)^2}."""
    lam = f32(lam)
    new = [_d(g).clone() for g in grads]
    abs_sum = [g.abs() for g in new]
    touched = [torch.zeros(g.shape, dtype=torch.int64) for g in new]
    value = value_abs = 0.0
    for idx, imp, opt in entries:
        imp, opt = _d(imp).reshape(-1), _d(opt).reshape(-1)
        n = opt.numel()
        d = opt - _d(params[idx]).reshape(-1)[:n]
        value += lam * float((imp * d * d).sum())
        value_abs += lam * float((imp.abs() * d * d).sum())
        term = -2.0 * lam * imp * d
        new[idx].view(-1)[:n] += term
        abs_sum[idx].view(-1)[:n] += term.abs()
        touched[idx].view(-1)[:n] += 1
    return value, new, dict(abs_sum=abs_sum, touched=touched, value_abs=value_abs)


# ------------------------------------------------------------------------------------------------------------------
# a whole optimizer made of the functions above, stepping the way torch.optim walks its groups
class Stepper:
    """param_groups like torch.optim's ({'params': [...], 'lr', 'weight_decay'}); parameters are float64 tensors carrying
    `.grad` (None: skipped, its step count does not advance); a parameter listed k times is stepped k times per `step()`.
    State per parameter (by id): 'step', and 'exp_avg' / 'exp_avg_sq' or 'momentum_buffer'.
    torch.optim.SGD collects every occurrence's momentum buffer BEFORE it updates any: a parameter listed k times that has no
    buffer yet starts it from the gradient at all k occurrences of that iteration, and keeps the last."""

    def __init__(self, groups, kind, betas=(0.9, 0.999), eps=1e-8, momentum=0.9):
        assert kind in ("AdamW", "SGD")
        self.groups, self.kind, self.betas, self.eps, self.momentum, self.state = groups, kind, betas, eps, momentum, {}

    def step(self, max_norm=-1.0):
        seen, grads = set(), []
        for g in self.groups:
            for p in g['params']:
                if p.grad is not None and id(p) not in seen:
                    seen.add(id(p))
                    grads.append(p.grad)
        norm, coef = clip(grads, max_norm)
        fresh = {i for i in seen if 'momentum_buffer' not in self.state.get(i, {})}
        for g in self.groups:
            for p in g['params']:
                if p.grad is None:
                    continue
                st = self.state.setdefault(id(p), {'step': 0})
                st['step'] += 1
                if self.kind == "AdamW":
                    m = st.get('exp_avg', torch.zeros_like(p))
                    v = st.get('exp_avg_sq', torch.zeros_like(p))
                    new, st['exp_avg'], st['exp_avg_sq'], _ = adamw_step(p, p.grad, m, v, st['step'], g['lr'], g['weight_decay'],
                                                                        self.betas[0], self.betas[1], self.eps, coef)
                else:
                    new, st['momentum_buffer'], _ = sgd_step(p, p.grad, st.get('momentum_buffer'), 1 if id(p) in fresh else st['step'], g['lr'],
                                                             g['weight_decay'], self.momentum, coef)
                p.data.copy_(new)
        return norm, coef
