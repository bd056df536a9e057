"""The ViLCo recipe's step -- narration SSL on -- replayed as hipGraphs is the step the eager path runs.

The episode model and helpers of tests/test_graph_gpu.py with `narration_ssl` switched on, a seeded narration encoder and
memory bank, and the episode batches extended by seeded narration tokens whose masks' counts differ from batch to batch (one
batch has none).  What a host-side ring pointer, a host read of the mask sum or a stale captured reduction would break:
every loss bit for bit, the final weights, the bank and its pointer."""
import pytest
import torch

from parity_util import cases
from test_graph_gpu import _episode_model, seed_word_zero  # noqa: F401  (the fixture is used by name)

pytestmark = pytest.mark.gpu

MASKS = ([1.0, 0.0], [0.0, 0.0], [1.0, 1.0], [0.0, 1.0])      # per batch: 1, 0, 2, 1 narrated clips
NARR_DIM, BANK = 24, 5                                       # 5 rows: the eight steps' eight rows wrap the ring


def _ssl_episode_model(dev):
    from vilco_amd.modeling.meta_archs import MemoryBank
    cfg, model = _episode_model(dev)
    D = cfg['model']['fpn_dim']
    g = torch.Generator().manual_seed(77)
    model.narration_ssl, model.narration_dim, model.ssl_factor = True, NARR_DIM, 0.03
    model.narration_encoder = torch.nn.Linear(NARR_DIM, D).to(dev)
    with torch.no_grad():
        model.narration_encoder.weight.copy_(0.3 * torch.randn(D, NARR_DIM, generator=g))
        model.narration_encoder.bias.copy_(0.1 * torch.randn(D, generator=g))
    model._memory_bank_cfg = (BANK, D)
    model.memory_bank = MemoryBank(BANK, D, device=dev)
    model.memory_bank.memory.copy_(torch.randn(BANK, D, generator=g))
    return cfg, model


def _ssl_batches():
    g = torch.Generator().manual_seed(78)
    out = []
    for bi, batch in enumerate(cases.episode_batches(0)):
        out.append([dict(x, narration_feats=torch.randn(NARR_DIM, 3 + (2 * bi + ci) % 5, generator=g),
                         narration_mask=MASKS[bi][ci]) for ci, x in enumerate(batch)])
    return out


def _train(dev, use_graph):
    from vilco_amd.graph import GraphedStep
    from vilco_amd.utils.train_utils import make_optimizer, make_scheduler, train_one_epoch
    cfg, model = _ssl_episode_model(dev)
    batches = _ssl_batches()
    opt = make_optimizer(model, cfg['opt'])
    sch = make_scheduler(opt, cfg['opt'], len(batches))
    clip = cfg['train_cfg']['clip_grad_l2norm']
    graph = GraphedStep(model, opt, clip_grad_l2norm=clip, eager_steps=1) if use_graph else None
    losses = []
    for epoch in range(2):
        model.pre_train_epoch(task_id=0, current_epoch=epoch)
        hist = train_one_epoch(batches, model, opt, sch, epoch, 1, clip_grad_l2norm=clip, cl_name=cfg['cl_cfg']['name'],
                               reg_lambda=cfg['cl_cfg']['reg_lambda'], prev_out_cls_logits_dict={}, current_task_id=0,
                               graph=graph)
        losses += [{k: float(v) for k, v in h.items()} for h in hist]
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return losses, sd, model.memory_bank.memory.clone(), model.memory_bank.ptr, graph


def test_graphed_ssl_training_equals_eager_training(dev, seed_word_zero):
    la, sa, ba, pa, _ = _train(dev, False)
    lb, sb, bb, pb, graph = _train(dev, True)
    assert graph.stats['captured'] == 1 and graph.stats['replayed'] == 7 and graph.stats['eager'] == 1, graph.stats
    assert len(la) == len(lb) == 8
    for i, (a, b) in enumerate(zip(la, lb)):
        assert set(a) == set(b) and 'ssl_loss' in a
        for k in a:
            assert a[k] == b[k], (i, k, a[k], b[k])
    assert [l['ssl_loss'] == 0.0 for l in la] == [False, True, False, False] * 2        # the maskless batch: an exact zero
    assert 'narration_encoder.weight' in sa
    for k in sa:      # (tests/test_graph_gpu.py's rule: loss.hip accumulates the mu / sigma / scale gradients with float atomics)
        assert torch.equal(sa[k], sb[k]) or (any(t in k for t in ("mu", "sigma", "scale")) and
                                             torch.allclose(sa[k], sb[k], rtol=1e-5, atol=1e-9)), k
    assert pa == pb == 8 % BANK and torch.equal(ba, bb)


def test_unfused_ssl_stays_eager(dev, seed_word_zero, monkeypatch):
    monkeypatch.setenv("VILCO_FUSED_SSL", "0")
    losses, _, _, ptr, graph = _train(dev, True)
    assert graph.stats['captured'] == 0 and graph.stats['replayed'] == 0 and graph.stats['eager'] == 8, graph.stats
    assert ptr == 8 % BANK and sum('ssl_loss' in l for l in losses) == 6        # the reference's form: no key without a narration
