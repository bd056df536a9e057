"""CPU: tests/local_attention_restatement.py against two independent formulations of sliding-window attention -- a per-row
Python loop (gather the row's window, softmax, weighted sum) and the band core of oracle.nlq_oracle.local_mhca on the NLQ
golden inputs -- plus the conventions the GPU tests rely on: a query row with no key is an all-zero row without gradients,
and a window of T - 1 or more is plain key masking.  All float64; the bars are float64 roundoff."""
import math

import pytest
import torch

import local_attention_restatement as LA
from parity_util import HERE, cases

EPS = 1e-12


def _inputs(B, T, H, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, T, H * hd, generator=g, dtype=torch.float64) for _ in range(4)]       # q, k, v, dout


def _loop(q, k, v, lens, H, scale, window, keep=None):
    """one row at a time: the visible keys are gathered, the softmax is over exactly those"""
    B, T, C = q.shape
    hd = C // H
    rows = []
    for b in range(B):
        L = int(lens[b])
        for i in range(T):
            lo, hi = max(0, i - window), min(L, i + window + 1)
            for h in range(H):
                sl = slice(h * hd, (h + 1) * hd)
                if hi <= lo:
                    rows.append(q[b, i, sl] * 0.0)
                    continue
                p = torch.softmax(scale * (k[b, lo:hi, sl] @ q[b, i, sl]), dim=0)
                if keep is not None:
                    p = p * keep[b, h, i, lo:hi]
                rows.append(p @ v[b, lo:hi, sl])
    return torch.stack(rows).view(B, T, C)


@pytest.mark.parametrize("T,window,lens", [(13, 0, [13, 5]), (13, 1, [13, 1]), (13, 3, [9, 0]), (20, 4, [20, 7]), (20, 19, [20, 3]),
                                           (20, 50, [11, 20])])
@pytest.mark.parametrize("drop", [False, True])
def test_restatement_equals_a_per_row_loop(T, window, lens, drop):
    B, H, hd = 2, 2, 4
    q, k, v, dout = _inputs(B, T, H, hd, 100 + T + window)
    lens = torch.tensor(lens, dtype=torch.int32)
    keep = None
    if drop:
        keep = (torch.rand(B, H, T, T, generator=torch.Generator().manual_seed(5)) >= 0.2).double() / 0.8
    want = LA.reference(q, k, v, lens, H, 0.4, window, dout, keep)
    ql, kl, vl = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o = _loop(ql, kl, vl, lens, H, 0.4, window, keep)
    o.backward(dout)
    for name, got in (("o", o), ("dq", ql.grad), ("dk", kl.grad), ("dv", vl.grad)):
        e = float((got.detach() - want[name]).abs().max())
        print("%-3s max abs difference %.3e" % (name, e))
        assert e < EPS, (name, e)
    has = LA.row_has_key(lens, T, window)
    want_has = torch.tensor([[max(0, i - window) < min(int(L), i + window + 1) for i in range(T)] for L in lens])
    assert torch.equal(has, want_has)


def test_rows_without_a_key_are_zero_and_carry_no_gradient():
    B, T, H, hd, window = 2, 24, 2, 4, 3
    q, k, v, dout = _inputs(B, T, H, hd, 7)
    lens = torch.tensor([10, 0], dtype=torch.int32)
    has = LA.row_has_key(lens, T, window)
    assert has[0].tolist() == [i < 13 for i in range(T)] and not bool(has[1].any())
    r = LA.reference(q, k, v, lens, H, 0.5, window, dout)
    for t in r.values():
        assert bool(torch.isfinite(t).all())
    assert torch.count_nonzero(r["o"][~has]) == 0 and torch.count_nonzero(r["dq"][~has]) == 0
    assert torch.count_nonzero(r["o"][has]) > 0 and torch.count_nonzero(r["dq"][0, :13]) > 0
    assert torch.count_nonzero(r["dk"][0, 10:]) == 0 and torch.count_nonzero(r["dv"][0, 10:]) == 0
    for name in ("o", "dq", "dk", "dv"):
        assert torch.count_nonzero(r[name][1]) == 0, name                  # the empty clip
    # whatever the dead rows hold upstream and in q changes nothing
    q2, d2 = q.clone(), dout.clone()
    q2[~has] += 3.0
    d2[~has] -= 2.0
    r2 = LA.reference(q2, k, v, lens, H, 0.5, window, d2)
    for name in ("o", "dq", "dk", "dv"):
        assert torch.equal(r[name], r2[name]), name


@pytest.mark.parametrize("window", [16, 17, 1000, 2 ** 31 - 1])
def test_a_window_of_T_minus_1_or_more_is_plain_key_masking(window):
    B, T, H, hd = 2, 17, 2, 4
    q, k, v, dout = _inputs(B, T, H, hd, 9)
    lens = torch.tensor([17, 6], dtype=torch.int32)
    r = LA.reference(q, k, v, lens, H, 0.5, window, dout)
    qd, kd, vd = [t.clone().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = [t.view(B, T, H, hd).transpose(1, 2) for t in (qd, kd, vd)]
    s = (0.5 * qh) @ kh.transpose(-1, -2)
    km = (torch.arange(T)[None, :] < lens[:, None])[:, None, None, :]
    o = (torch.softmax(s.masked_fill(~km, float("-inf")), dim=-1) @ vh).transpose(1, 2).reshape(B, T, H * hd)
    o.backward(dout)
    for name, got in (("o", o), ("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        assert float((got.detach() - r[name]).abs().max()) < EPS, name
    assert bool(LA.row_has_key(lens, T, window).all())


@pytest.mark.parametrize("stride", [1, 2])
def test_restatement_equals_the_oracle_band_core_below_len(stride, monkeypatch):
    """oracle.nlq_oracle.local_mhca on cases.nlq_inputs() with the golden block's parameters: the tensors its band core takes
    (the outputs of the query / key / value projections) and gives (the input of the output projection) are recorded on
    the way through.  The oracle adds -1e4 to a key at or beyond len where the restatement removes it -- exp(-1e4) is 0 in
    float64 next to the always-present key j = i -- and zeroes the query rows at or beyond len, so the two agree on the
    rows below len, and so do the gradients of a loss that weighs only those rows."""
    from oracle import mq_oracle as M
    from oracle import nlq_oracle as N
    import os
    c = torch.load(os.path.join(HERE, "golden", "nlq_blocks.pt"), weights_only=False)["local_s%d" % stride]
    p = {"a." + n: (t.double() if t.is_floating_point() else t) for n, t in c["state"].items()}
    x, mask, _, _ = cases.nlq_inputs()
    seen = []
    conv1x1 = M.conv1x1

    def recording(p_, pre, t):
        y = conv1x1(p_, pre, t)
        if pre.endswith("proj."):
            t.retain_grad()
        else:
            y.retain_grad()
        seen.append((pre, t, y))
        return y
    monkeypatch.setattr(M, "conv1x1", recording)
    y, om = N.local_mhca(p, "a.", x.double().requires_grad_(True), mask, cases.NLQ_H, stride, cases.NLQ_WIN)
    assert [s[0] for s in seen] == ["a.query.", "a.key.", "a.value.", "a.proj."]
    q, k, v = [s[2] for s in seen[:3]]                       # channel-first [B, C, T']
    core = seen[3][1]
    B, C, T = q.shape
    lens = om[:, 0, :].sum(dim=1).to(torch.int32)
    assert T == cases.NLQ_T // stride and int(lens[1]) < T
    below = (torch.arange(T)[None, :] < lens[:, None])
    w = torch.randn(B, T, C, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * below[:, :, None]
    (core.transpose(1, 2) * w).sum().backward()
    tm = [t.detach().transpose(1, 2).contiguous() for t in (q, k, v)]
    r = LA.reference(*tm, lens, cases.NLQ_H, 1.0 / math.sqrt(C // cases.NLQ_H), cases.NLQ_WIN // 2, w)
    got = dict(o=core.detach().transpose(1, 2), dq=q.grad.transpose(1, 2), dk=k.grad.transpose(1, 2), dv=v.grad.transpose(1, 2))
    for name in ("o", "dq", "dk", "dv"):
        a, b = got[name] * below[:, :, None], r[name] * below[:, :, None]
        e = float((a - b).abs().max() / b.abs().max())
        print("stride %d %-3s %.3e" % (stride, name, e))
        assert e < 1e-12, (name, e)
    # beyond len the two differ by design: the oracle's rows are zeroed, the restatement's still see the keys below len
    assert torch.count_nonzero(got["o"][1, int(lens[1]):]) == 0
    assert torch.count_nonzero(r["o"][1, int(lens[1]):int(lens[1]) + cases.NLQ_WIN // 2]) > 0
