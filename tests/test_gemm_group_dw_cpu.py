"""CPU: the inputs of tests/test_gemm_group_dw_gpu.py::test_model_gradients_grouped_replayed_and_ungrouped keep every gradient
it bounds RELATIVELY away from zero -- the float64 restatement (oracle/mq_oracle.py) on the same clips (the golden ones reversed
in time), every weight of a matrix product: a bound relative to max|gradient| means nothing on a zero tensor."""
import torch

from parity_util import golden_cfg, golden_inputs, load_golden


def test_every_matrix_gradient_of_the_reversed_clips_is_far_from_zero():
    from oracle import mq_oracle
    gold = load_golden("noxl")
    cfg = golden_cfg(gold)
    p = {k: (v.double() if v.is_floating_point() else v).clone().requires_grad_(v.is_floating_point())
         for k, v in gold['state_dict'].items()}
    vl = [dict(d, feats=d['feats'].flip(-1).contiguous()) for d in golden_inputs(gold)]
    vl = [{k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()} for d in vl]
    losses, _ = mq_oracle.forward_losses(p, cfg, vl, task_id=gold['task_id'], n_known=gold['n_known'])
    losses['final_loss'].backward()
    # (the predicate of the GPU test: weights of matrix products -- not the [1, C, 1] LayerNorm affines, not biases)
    mats = {k: v.grad for k, v in p.items() if v.is_floating_point() and v.grad is not None and k.endswith("weight")
            and v.dim() >= 2 and v.shape[0] > 1 and v.shape[1] > 1}
    assert len(mats) >= 10
    top = max(float(g.abs().max()) for g in mats.values())
    for k, g in mats.items():
        assert float(g.abs().max()) > 1e-6 * top, (k, float(g.abs().max()), top)
