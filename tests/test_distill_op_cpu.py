"""CPU side of the fused distillation op (csrc/distill.hip, ops.cl_distill; reference MQ/libs/modeling/meta_archs.py:1482-1519):
the fp64 restatement the GPU tests compare with equals the oracle (itself tied to the reference by tests/golden/distill.pt),
the entry points validate on the host, and train_cl.cache_prev_logits hands out views of one buffer per clip."""
import ctypes

import numpy as np
import pytest
import torch

from parity_util import rel_err  # noqa: F401  (puts the repository root on sys.path)
from distill_restatement import distill_grad, distill_loss

LEVEL_T = (5, 2, 1)


def _layout(sep):
    rows, o = [], 0
    for T in LEVEL_T:
        rows.append(o)
        o += T + sep
    return rows, o - sep


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sep", [0, 1])
def test_restatement_equals_the_oracle(mode, sep):
    from oracle import mq_oracle as O
    g = torch.Generator().manual_seed(7 + mode)
    B, C, ldt, n_known, n_classes = 2, 9, 11, 6, 9
    rows, R = _layout(sep)
    logits = (3 * torch.randn(B, R, C, generator=g, dtype=torch.float64)).requires_grad_(True)
    targets = torch.rand(sum(LEVEL_T), ldt, generator=g, dtype=torch.float64)       # rows do not sum to 1
    levels = [logits[:, r:r + T] for r, T in zip(rows, LEVEL_T)]
    prev = list(targets.split(LEVEL_T))
    scale = 0.01 * n_known / n_classes
    want = O.cl_distill(levels, prev if mode else [prev], n_known, 'bic' if mode else 'icarl', n_classes)
    got = distill_loss(logits.detach(), rows, LEVEL_T, targets, n_known, mode, scale)
    assert abs(float(got) - float(want.detach())) <= 1e-13 * abs(float(want.detach()))
    (1.7 * want).backward()
    grad = distill_grad(logits.detach(), rows, LEVEL_T, targets, n_known, mode, scale, g=1.7)
    assert (grad - logits.grad).abs().max().item() <= 1e-13 * logits.grad.abs().max().item()
    assert torch.count_nonzero(grad[1]) == 0 and torch.count_nonzero(grad[0, :, n_known:]) == 0


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                                     # dummy aligned address: every check precedes the launch
    L = 3

    def desc(rows=(0, 6, 9), lens=LEVEL_T, **kw):
        hr, ht = (ctypes.c_int32 * len(rows))(*rows), (ctypes.c_int32 * len(lens))(*lens)
        f = dict(logits=x, targets=x, level_row=ctypes.addressof(hr), level_T=ctypes.addressof(ht), level_dev=x,
                 B=2, R=10, C=7, L=L, clip=0, ldt=7, n_known=3, mode=0, scale=0.01)
        f.update(kw)
        d = _lib.DistillDesc(**f)
        d._keep = (hr, ht)
        return d

    def fwd(d, out=x, ws=x, nws=1 << 20):
        return lib.vilco_cl_distill_fwd(ctypes.byref(d) if d is not None else None, out, ws, nws, None)

    def bwd(d, g=x, dl=x):
        return lib.vilco_cl_distill_bwd(ctypes.byref(d) if d is not None else None, g, dl, None)

    bad = [dict(logits=None), dict(targets=None), dict(level_row=None), dict(level_T=None), dict(level_dev=None),
           dict(L=0), dict(L=-1), dict(n_known=0), dict(n_known=8), dict(n_known=5, ldt=4), dict(clip=2), dict(clip=-1),
           dict(rows=(0, 6, 10)), dict(rows=(0, 6, 9), lens=(5, 2, 2)), dict(rows=(-1, 6, 9)), dict(lens=(5, 0, 1)),
           dict(mode=2), dict(mode=-1)]
    for kw in bad:
        assert fwd(desc(**kw)) == -1, kw
        assert bwd(desc(**kw)) == -1, kw
    assert fwd(None) == -1 and bwd(None) == -1
    assert fwd(desc(), out=None) == -1 and fwd(desc(), ws=None) == -1
    assert bwd(desc(), g=None) == -1 and bwd(desc(), dl=None) == -1
    assert fwd(desc(), nws=4) == -4                                   # a legal call gets as far as the workspace check
    assert lib.vilco_cl_distill_workspace(sum(LEVEL_T)) >= 8 and lib.vilco_cl_distill_workspace(-1) == 0


def test_ops_cl_distill_refuses_host_tensors_and_mismatched_levels():
    from vilco_amd import ops
    logits, targets = torch.zeros(2, 10, 7), torch.zeros(8, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cl_distill(logits, (0, 6, 9), LEVEL_T, targets, 3, 0, 0.0)
    with pytest.raises(ValueError, match="level lengths"):
        ops.cl_distill(logits, (0, 6, 9), LEVEL_T, [np.zeros((5, 7), np.float32), np.zeros((3, 7), np.float32)], 3, 0, 0.0)
    with pytest.raises(ValueError, match="rows of the levels"):
        ops.cl_distill(logits, (0, 6, 9), LEVEL_T, torch.zeros(9, 7), 3, 0, 0.0)


class _Stub:
    """what cache_prev_logits needs of a model: fixed per-level logits for every batch"""
    n_known = 3

    def __init__(self, levels):
        self.levels = levels

    def __call__(self, video_list, task_id=0, get_emb=False):
        assert get_emb
        return self.levels, None, None


@pytest.mark.parametrize("kind", ["sigmoid", "softmax_T2"])
def test_cached_targets_are_views_of_one_buffer_per_clip(kind):
    from vilco_amd.train_cl import cache_prev_logits
    g = torch.Generator().manual_seed(3)
    levels = [torch.randn(2, T, 5, generator=g) for T in LEVEL_T]
    loader = [[{'video_id': 'a'}, {'video_id': 'b'}]]
    got = cache_prev_logits(_Stub(levels), loader, 0, kind=kind)
    assert sorted(got) == ['a', 'b']
    for i, vid in enumerate(('a', 'b')):
        clip = got[vid]
        assert isinstance(clip, list) and [tuple(t.shape[:1]) for t in clip] == [(T,) for T in LEVEL_T]
        ld, off = clip[0].shape[1], clip[0].storage_offset()
        for t, lvl in zip(clip, levels):
            want = torch.sigmoid(lvl[i]) if kind == 'sigmoid' else torch.softmax(lvl[i][:, :3] / 2, dim=1)
            assert torch.equal(t, want)
            assert t.is_contiguous() and t.untyped_storage().data_ptr() == clip[0].untyped_storage().data_ptr()
            assert t.storage_offset() == off
            off += t.shape[0] * ld
    assert got['a'][0].untyped_storage().data_ptr() != got['b'][0].untyped_storage().data_ptr()
    host = cache_prev_logits(_Stub(levels), loader, 0, as_numpy=True, kind=kind)
    for vid in ('a', 'b'):
        for a, t in zip(host[vid], got[vid]):
            assert isinstance(a, np.ndarray) and np.array_equal(a, t.numpy())
