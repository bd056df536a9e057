"""ER-ACE in the captured step (vilco_amd/cl_methods/ace.py, PtTransformer._fused_losses' 'er_ace' route, graph.GraphedStep), on
the small episode model the DER and distillation graph tests build: a step captured with one window table and replayed with
others follows the table of ITS batch -- losses and every gradient bit for bit the eager step on the same batch."""
import pytest
import torch

from parity_util import cases, episode_full_state, load_episode_golden

pytestmark = pytest.mark.gpu


@pytest.fixture
def seed_word_zero():
    """the dropout step word is process-wide device state: leave it at 0 for the other tests"""
    from vilco_amd import _lib
    yield
    _lib.check(_lib.load().vilco_seed_word_set(0, None))
    torch.cuda.synchronize()


def _ace_model(dev, name='er_ace'):
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_episode_golden()
    over = dict(gold['overrides'])
    over['cl_cfg'] = dict(over.get('cl_cfg', {}), name=name, type_sampling='random')
    cfg = make_config(**over)
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    model.load_state_dict(episode_full_state(gold['init_state']), strict=True)
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    assert model.cl_name == name
    model.train()
    for mod in model.modules():
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0            # stochastic depth draws from torch's generator: not what is compared here
    model.pre_train_epoch(task_id=0, current_epoch=0)
    return model


def _step(model, batch):
    for p in model.parameters():
        p.grad = None
    out = model(batch, task_id=0)
    out['final_loss'].backward()
    torch.cuda.synchronize()
    return ({k: v.detach().reshape(()).float().clone() for k, v in out.items()},
            {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})


def test_replayed_step_follows_the_window_table_of_its_batch(dev, seed_word_zero):
    """graph calls over the two clips of one batch with the memory in four states: {task clip, memory clip} (call 0 eager, call 1
    captures and replays), {memory clip, task clip}, two task clips, two memory clips.  Every call equals the eager step of a twin
    model in the same state; the old-class rows of the classification head's last conv get exactly zero gradient when no memory
    clip is in the batch, and the windows change the loss."""
    from vilco_amd.cl_methods import ace
    from vilco_amd.graph import GraphedStep
    batch = cases.episode_batches(0)[0]
    assert len(batch) == 2
    ma, mb = _ace_model(dev), _ace_model(dev)
    n_known = 2
    C_ = ma.cls_head.cls_head.conv.out_channels
    assert n_known < C_
    for m in (ma, mb):
        m.n_known = n_known
    states = [(1,), (1,), (0,), (), (0, 1)]            # which rows of the batch are memory clips

    def set_state(model, rows):
        model.memory = {0: [batch[r] for r in rows]} if rows else {}

    gs = GraphedStep(ma, None, eager_steps=1)
    got = []
    for rows in states:
        set_state(ma, rows)
        assert ace.step_table(ma, batch).tolist() == [0 if r in rows else n_known for r in range(2)]
        out = gs(batch, task_id=0)
        torch.cuda.synchronize()
        got.append(({k: v.clone() for k, v in out.items()},
                    {n: p.grad.clone() for n, p in ma.named_parameters() if p.grad is not None}))
    assert gs.stats['captured'] == 1 and gs.stats['replayed'] == 4 and gs.stats['eager'] == 1, gs.stats
    print("cls_loss per table:", [float(o['cls_loss']) for o, _ in got])      # (the normaliser EMA moves from call to call)
    for rows, (out, grads) in zip(states, got):
        set_state(mb, rows)
        want, wg = _step(mb, batch)
        assert set(out) == set(want)
        for k in want:
            assert torch.equal(out[k].reshape(()), want[k]), (rows, k, float(out[k]), float(want[k]))
        assert set(wg) == set(grads)
        for n in wg:
            assert torch.equal(grads[n], wg[n]), (rows, n)
        w, b = grads['cls_head.cls_head.conv.weight'], grads['cls_head.cls_head.conv.bias']
        if rows == ():
            assert bool((w[:n_known] == 0).all()) and bool((b[:n_known] == 0).all()) and bool((w[n_known:] != 0).any())
        else:
            assert bool((w[:n_known] != 0).any()) and bool((b[:n_known] != 0).all())
    # two memory clips: the plain loss, bit for bit what a model without the method computes at its fifth step (the normaliser
    # EMA has moved four times by then, by the same #pos: the windows do not touch the assignment); the steps before differ
    plain = _ace_model(dev, None)
    plain.n_known = n_known
    for i, (out, grads) in enumerate(got):
        want, wg = _step(plain, batch)
        same = all(torch.equal(out[k].reshape(()), want[k]) for k in want) and all(torch.equal(grads[n], wg[n]) for n in wg)
        assert torch.equal(out['reg_loss'].reshape(()), want['reg_loss']), i
        assert same == (i == 4), (i, float(out['cls_loss']), float(want['cls_loss']))
        if i < 4:
            assert float(out['cls_loss']) < float(want['cls_loss']), "a window only removes non-negative focal terms"
    # a step without the slot filled is not capturable; without known classes the method does not ask for it
    inp = ma.prepare(batch, True, gt_pad=8)
    assert inp.ace_lo is None and not ma.capturable(inp, 0, None)
    inp.ace_lo = ace.step_table(ma, batch)
    assert ma.capturable(inp, 0, None) and not ma.capturable(inp, 0, [[torch.zeros(1)]])
    assert ("ace_lo", (2,)) in inp.signature()
    ma.n_known = 0
    inp.ace_lo = None
    assert ma.capturable(inp, 0, None)
