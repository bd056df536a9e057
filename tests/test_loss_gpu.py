"""ops.mq_loss (vilco_mq_loss_fwd / _bwd: point labelling + focal / DIoU / al losses + loss_normalizer EMA in two
launches each way) against the fp64 oracle restatement of meta_archs.py:1253-1344 / 1374-1447 (oracle.label_points_single,
oracle.losses -- themselves pinned to the reference goldens through tests/test_oracle_model.py)."""
import pytest
import torch

from loss_cases import _case
from parity_util import rel_err

pytestmark = pytest.mark.gpu


GT2 = [([[10.0, 40.0], [60.5, 130.25]], [1, 5]), ([[10.0, 40.0], [60.5, 130.25]], [1, 5])]


@pytest.mark.parametrize("gaps", [True, False])
def test_loss_basic(dev, gaps):
    _case(dev, 22, 256, GT2, [256, 239], gaps)


def test_loss_ragged_gt_counts_ties_and_smoothing(dev):
    gts = [([[5.0, 25.0], [5.0, 25.0005], [100.0, 101.0], [30.0, 200.0]], [3, 7, 3, 0]),      # two GT within 1e-3 of each other: multi-hot
           ([[50.0, 58.0]], [2]),
           ([[0.0, 256.0], [120.0, 136.0], [121.0, 135.0]], [9, 9, 1])]
    _case(dev, 10, 256, gts, [256, 100, 255], True, smoothing=0.1, seed=3)


def test_loss_no_positive_anywhere(dev):
    """GT far outside every regression range / beyond the clip: num_pos = 0 -> normaliser uses max(num_pos, 1), reg loss 0"""
    gts = [([[300.0, 300.5]], [0]), ([[400.0, 400.2]], [1])]
    _case(dev, 4, 64, gts, [64, 40], True, seed=5)


def test_loss_center_sample_none_and_many_classes(dev):
    _case(dev, 110, 128, [([[3.0, 90.0], [20.0, 30.0]], [109, 64]), ([[40.0, 44.0]], [33])], [128, 128], False, radius=0.0,
          seed=7, al=0.5, loss_weight=2.0)


def test_model_fused_equals_tensor_expression_path(dev):
    """the whole model with the fused loss kernels vs VILCO_FUSED_LOSS=0 (the tensor-expression losses the round-1
    goldens were checked with): same losses, same gradients"""
    from parity_util import GRAD_FLOOR, build_hip_model, golden_cfg, golden_inputs, load_golden
    gold = load_golden("noxl")
    outs = []
    for fused in (True, False):
        model = build_hip_model(gold)
        model.fused_loss = fused
        model.loss_normalizer = golden_cfg(gold)['train_cfg']['init_loss_norm']
        losses = model(golden_inputs(gold), task_id=gold['task_id'], is_training=True)
        losses['final_loss'].backward()
        outs.append((losses, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, model.loss_normalizer))
    (la, ga, na), (lb, gb, nb) = outs
    assert abs(na - nb) < 1e-4
    for k in ('cls_loss', 'reg_loss', 'al_loss', 'final_loss'):
        assert rel_err(la[k], lb[k]) < 1e-5, k
    assert sorted(ga) == sorted(gb)
    for k in ga:
        if not k.endswith(('key_norm.bias', '.key.bias')):          # analytically zero: 1e-11-level noise both ways
            assert rel_err(ga[k], gb[k], GRAD_FLOOR) < 1e-4, k


def test_parameter_gradients_of_the_loss_are_the_same_bits_on_every_launch(dev):
    """Round 6: the gradients of the per-level regression scales and of the gaussian-weight parameters (mu / sigma) leave
    vilco_mq_loss_bwd through per-row shares and a fixed-order second launch (loss_bwd_finish_kernel) instead of float atomicAdds --
    the last sums of a step whose order changed from launch to launch.  Eight backward passes of the golden model from one state:
    every gradient tensor bit-equal to the first pass's, the atomics' former targets included."""
    from parity_util import build_hip_model, golden_cfg, golden_inputs, load_golden
    gold = load_golden("xl")
    model = build_hip_model(gold)
    ref = None
    for it in range(8):
        model.zero_grad(set_to_none=True)
        model.loss_normalizer = golden_cfg(gold)['train_cfg']['init_loss_norm']
        model(golden_inputs(gold), task_id=gold['task_id'], is_training=True)['final_loss'].backward()
        g = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        if ref is None:
            ref = g
            assert any(k.startswith(('mu', 'sigma')) for k in g) and any(k.startswith('reg_head.scale.') for k in g)
            assert any(float(g[k].abs().max()) > 0 for k in g if k.startswith('reg_head.scale.'))      # (levels without a positive point: 0)
        else:
            assert sorted(g) == sorted(ref)
            for k in g:
                assert torch.equal(g[k], ref[k]), (it, k)
