"""The operand hints of vilco_amd/ops.py on their own: the per-tensor record (max|x| partials + remembered operand planes), its
validity rules, its trip across a stage cut and across Function.apply.  Plain CPU tensors; no library call."""
import pytest
import torch

from vilco_amd import ops


@pytest.fixture
def flags():
    saved = ops.produce_amax, ops._pack_cache, ops.seg_tape
    yield
    ops.produce_amax, ops._pack_cache, ops.seg_tape = saved


def _tagged(B=2, T=5, C=8):
    """x [B, T, C] carrying amax partials and fake planes in both layouts"""
    x = torch.randn(B, T, C)
    parts, nat, seq = torch.ones(4), torch.zeros(16, dtype=torch.uint8), torch.zeros(24, dtype=torch.uint8)
    assert ops._tag_amax(x, parts, 3) is x
    assert ops._remember_planes(x, "nat", (B * T, C), 3, nat) is nat
    assert ops._remember_planes(x, "seq", (B, T, C), 3, seq) is seq
    return x, parts, nat, seq


def test_same_key_hits_and_any_other_key_misses(flags):
    x, parts, nat, seq = _tagged()
    got = ops._amax_of(x)
    assert got[0] is parts and got[1] == 3
    assert ops._planes_of(x, "nat", (10, 8), 3) is nat
    assert ops._planes_of(x, "seq", (2, 5, 8), 3) is seq
    assert ops._planes_of(x, "seq", x.shape, 3) is seq              # (a torch.Size is the same key)
    assert ops._planes_of(x, "nat", (5, 8), 3) is None              # other rows
    assert ops._planes_of(x, "nat", (10, 16), 3) is None            # other cols
    assert ops._planes_of(x, "nat", (10, 8), 2) is None             # other precision
    assert ops._planes_of(x, "seq", (10, 8), 3) is None             # the other layout's shape
    assert ops._planes_of(x, "nat", (2, 5, 8), 3) is None
    assert ops._planes_of(x, "seq", (2, 5, 8), 0) is None
    assert ops._planes_of(x, "seq", (1, 10, 8), 3) is None
    assert ops._amax_of(torch.randn(3)) == (None, 0)                # nothing was ever hung on this one
    assert ops._amax_of(ops._tag_amax(torch.randn(3), parts, 0)) == (None, 0)      # no partials: no tag


def test_in_place_edit_kills_amax_and_both_plane_layouts(flags):
    x, parts, nat, seq = _tagged()
    x.add_(1)
    assert ops._amax_of(x) == (None, 0)
    assert ops._planes_of(x, "nat", (10, 8), 3) is None
    assert ops._planes_of(x, "seq", (2, 5, 8), 3) is None
    # what is remembered after the edit stands alone: the dead record's other entries do not come back with it
    again = torch.zeros(16, dtype=torch.uint8)
    ops._remember_planes(x, "nat", (10, 8), 3, again)
    assert ops._planes_of(x, "nat", (10, 8), 3) is again
    assert ops._amax_of(x) == (None, 0) and ops._planes_of(x, "seq", (2, 5, 8), 3) is None


def test_produce_amax_off_hides_amax_only(flags):
    x, parts, nat, seq = _tagged()
    ops.produce_amax = False
    assert ops._amax_of(x) == (None, 0)
    assert ops._planes_of(x, "nat", (10, 8), 3) is nat and ops._planes_of(x, "seq", (2, 5, 8), 3) is seq
    ops.produce_amax = True
    assert ops._amax_of(x)[0] is parts


def test_pack_cache_off_remembers_nothing(flags):
    ops._pack_cache = False
    x, parts, nat, seq = _tagged()
    assert ops._planes_of(x, "nat", (10, 8), 3) is None and ops._planes_of(x, "seq", (2, 5, 8), 3) is None
    ops._pack_cache = True                                          # nothing was stored while it was off
    assert ops._planes_of(x, "nat", (10, 8), 3) is None and ops._planes_of(x, "seq", (2, 5, 8), 3) is None
    assert ops._amax_of(x)[0] is parts                              # (amax is not the pack cache's business)
    y, _, nat, _ = _tagged()
    ops._pack_cache = False                                         # ... and what was stored before is not looked at
    assert ops._planes_of(y, "nat", (10, 8), 3) is None


def test_seg_cut_hands_the_record_to_the_leaf(flags):
    x, parts, nat, seq = _tagged()
    x.requires_grad_(True)
    assert ops.seg_cut(x) is x                                      # no tape: no cut
    ops.seg_tape = tape = ops.SegTape()
    leaf = ops.seg_cut(x, next_stage=True)
    assert leaf is not x and leaf.is_leaf and leaf.requires_grad and leaf.data_ptr() == x.data_ptr()
    assert len(tape.records) == 1 and tape.records[0][0] is x and tape.records[0][1] is leaf and tape.records[0][2] == 0
    assert tape.stage == 1
    for t in (leaf, x):
        got = ops._amax_of(t)
        assert got[0] is parts and got[1] == 3
        assert ops._planes_of(t, "nat", (10, 8), 3) is nat and ops._planes_of(t, "seq", (2, 5, 8), 3) is seq
    # planes packed for the leaf later are the leaf's own
    other = torch.zeros(16, dtype=torch.uint8)
    ops._remember_planes(leaf, "nat", (10, 8), 3, other)
    assert ops._planes_of(leaf, "nat", (10, 8), 3) is other and ops._planes_of(x, "nat", (10, 8), 3) is nat


# ---- across Function.apply
_PARTS = torch.ones(2)


class _Two(torch.autograd.Function):
    """two outputs; `hint`: leaves amax for output 1 only"""

    @staticmethod
    def forward(ctx, x, hint):
        if hint:
            ops._leave(_Two, 1, amax=(_PARTS, 2))
        return x * 2, x * 3

    @staticmethod
    def backward(ctx, da, db):
        return da * 2 + db * 3, None


class _Raises(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ops._leave(_Raises, 0, amax=(_PARTS, 2), planes=torch.zeros(8, dtype=torch.uint8))
        raise RuntimeError("after leaving a hint")

    @staticmethod
    def backward(ctx, dy):
        return dy


class _Outer(torch.autograd.Function):
    """calls the wrapped _Two from inside its forward, and leaves hints of its own before and after that"""
    inner = None

    @staticmethod
    def forward(ctx, x):
        ops._leave(_Outer, 0, amax=(_PARTS, 1))
        _Outer.inner = ops._apply(_Two, x, True)
        ops._leave(_Outer, 0, planes=torch.zeros(8, dtype=torch.uint8), layout="seq")
        return x + 1

    @staticmethod
    def backward(ctx, dy):
        return dy


def _untagged(t):
    return ops._amax_of(t) == (None, 0) and ops._hints(t) is None


def test_apply_hangs_hints_on_outputs_by_position(flags):
    x = torch.randn(2, 3, 8, requires_grad=True)
    a, b = ops._apply(_Two, x, True)
    assert torch.equal(a, x * 2) and torch.equal(b, x * 3)
    got = ops._amax_of(b)
    assert got[0] is _PARTS and got[1] == 2 and _untagged(a)
    (a.sum() + b.sum()).backward()                                   # the outputs are still on the tape
    assert torch.equal(x.grad, torch.full_like(x, 5.0))
    assert not ops._handover


def test_a_forward_that_raises_leaves_nothing_behind(flags):
    x = torch.randn(2, 3, 8)
    with pytest.raises(RuntimeError, match="after leaving a hint"):
        ops._apply(_Raises, x)
    assert not ops._handover
    a, b = ops._apply(_Two, x, False)
    assert _untagged(a) and _untagged(b)


def test_nested_calls_keep_their_own_hints(flags):
    x = torch.randn(2, 3, 8)
    y = ops._apply(_Outer, x)
    ia, ib = _Outer.inner
    _Outer.inner = None
    got = ops._amax_of(ib)
    assert got[0] is _PARTS and got[1] == 2 and _untagged(ia)         # the inner call got its own
    got = ops._amax_of(y)
    assert got[0] is _PARTS and got[1] == 1                           # the outer one's, from before and after the inner call
    assert ops._planes_of(y, "seq", (2, 3, 8), 3) is not None and ops._planes_of(y, "nat", (6, 8), 3) is None
    assert not ops._handover


def test_a_function_called_without_the_wrapper_tags_nothing(flags):
    x = torch.randn(2, 3, 8)
    a, b = _Two.apply(x, True)
    assert _untagged(a) and _untagged(b) and not ops._handover
