"""Elastic Response Distillation in the step and in the episode loop (vilco_amd/cl_methods/erd.py, PtTransformer._cl_terms' 'erd'
branch, graph.GraphedStep, train_cl.run_episodes), on the small episode model the DER and POD graph tests build.

  * a step captured with one `erd_tab` and replayed with others -- one of them all zeros -- follows the table of ITS batch: bit for
    bit the eager step of a twin model, losses and gradients (the fused loss route: raw offsets and the per-level Scale);
  * the two-task stream run eager and with use_graph=True: the same losses and the same final state_dict, bit for bit;
    `erd_recorded` and `erd_bytes` in the second task's entry; the records of a task are released only after the next task's are
    in place."""
import random

import pytest
import torch

import erd_restatement as E
from parity_util import cases, episode_full_state, load_episode_golden

pytestmark = pytest.mark.gpu


def _erd_model(dev, **cl):
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_episode_golden()
    over = dict(gold['overrides'])
    over['cl_cfg'] = dict(over.get('cl_cfg', {}), name='erd', type_sampling='random', **cl)
    cfg = make_config(**over)
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    model.load_state_dict(episode_full_state(gold['init_state']), strict=True)
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    assert model.cl_name == 'erd' and model.erd_bank is None
    return cfg, model


def _random_records(dev, levels, n_old, valid_rows, seed):
    """records of independent random teachers, selected by the restatement -> per clip the arguments of ERDBank.record"""
    g = torch.Generator().manual_seed(seed)
    P = sum(levels)
    out = []
    for valid in valid_rows:
        z = torch.randn(P, n_old, generator=g)
        ok = E.valid_positions(levels, valid)
        pick = torch.randperm(len(ok), generator=g)[:max(2, len(ok) // 12)].numpy()
        z[torch.from_numpy(ok[pick]), 0] += 6.0
        o = torch.rand(P, 2, generator=g) * 3.0
        sel = E.select(z.numpy(), o.numpy(), levels, valid, n_old, 2.0, 2.0)
        assert E.margin(sel) >= 1e-6 and sel['S_cls'] and sel['S_reg']
        r = E.make_record(z.numpy(), o.numpy(), sel, n_old)
        out.append((torch.from_numpy(r['map_cls']).to(dev), torch.from_numpy(r['map_reg']).to(dev),
                    torch.from_numpy(r['val_cls']).to(dev), torch.from_numpy(r['val_reg']).to(dev),
                    len(sel['S_cls']), len(sel['S_reg'])))
    return out


@pytest.fixture
def seed_word_zero():
    """the dropout step word is process-wide device state: leave it at 0 for the other tests"""
    from vilco_amd import _lib
    yield
    _lib.check(_lib.load().vilco_seed_word_set(0, None))
    torch.cuda.synchronize()


def test_replayed_step_follows_the_table_of_its_batch(dev, seed_word_zero):
    from vilco_amd.cl_methods import erd
    from vilco_amd.graph import GraphedStep
    batch = cases.episode_batches(0)[0]
    assert len(batch) == 2
    twins = []
    for _ in range(2):
        _, m = _erd_model(dev, erd_lambda_reg=0.5)
        m.train()
        for mod in m.modules():
            if hasattr(mod, "drop_prob"):
                mod.drop_prob = 0.0            # stochastic depth draws from torch's generator: not what is compared here
        m.pre_train_epoch(task_id=0, current_epoch=0)
        m.n_known = 2
        m.erd_bank = erd.ERDBank()
        twins.append(m)
    ma, mb = twins
    assert ma.erd_lambda_reg == 0.5 and ma.erd_lambda_cls == 1.0
    levels = tuple(ma.max_seq_len // s for s in ma.fpn_strides)
    was = ma.training
    ma.eval()
    with torch.no_grad():
        _, _, masks = ma(batch, task_id=0, get_emb=True)
    ma.train(was)
    valid = torch.stack([m.reshape(m.shape[0], -1).sum(1) for m in masks], dim=1).tolist()
    recs = _random_records(dev, levels, 2, valid, seed=3)
    states = [(0,), (0,), (1,), (), (0, 1)]

    def set_state(model, rows):
        model.erd_bank.clear()
        for r in rows:
            model.erd_bank.record(batch[r]['video_id'], *recs[r], 2, erd.clip_len(batch[r]), levels)

    gs = GraphedStep(ma, None, eager_steps=1)
    got = []
    for rows in states:
        set_state(ma, rows)
        tab = erd.step_table(ma, batch)
        assert [int(a != 0) for a in tab[:, 0].tolist()] == [int(r in rows) for r in range(2)]
        out = gs(batch, task_id=0)
        torch.cuda.synchronize()
        got.append(({k: v.clone() for k, v in out.items()},
                    {n: p.grad.clone() for n, p in ma.named_parameters() if p.grad is not None}))
    assert gs.stats['captured'] == 1 and gs.stats['replayed'] == 4 and gs.stats['eager'] == 1, gs.stats
    vals = [(float(o['erd_loss']), float(o['erd_cls_loss']), float(o['erd_reg_loss'])) for o, _ in got]
    print("erd_loss, cls, reg per table:", vals)
    assert vals[0][1] > 0 and vals[0][2] > 0 and vals[2][0] > 0 and vals[1] != vals[2] and vals[3] == (0.0, 0.0, 0.0) and vals[4][0] > 0
    assert ma.erd_bank.skipped == 0
    for rows, (out, grads) in zip(states, got):
        set_state(mb, rows)
        for p in mb.parameters():
            p.grad = None
        want = mb(batch, task_id=0)
        want['final_loss'].backward()
        torch.cuda.synchronize()
        assert set(out) == set(want) and {'erd_loss', 'erd_cls_loss', 'erd_reg_loss'} <= set(want)
        for k in want:
            assert torch.equal(out[k].reshape(()), want[k].detach().reshape(()).float()), (rows, k, float(out[k]), float(want[k]))
        wg = {n: p.grad for n, p in mb.named_parameters() if p.grad is not None}
        assert set(wg) == set(grads)
        for n in wg:        # (the gaussian-weight gradients are float atomics in loss_bwd: equal up to summation order)
            assert torch.equal(grads[n], wg[n]) or (any(t in n for t in ("mu", "sigma", "scale")) and
                                                    torch.allclose(grads[n], wg[n], rtol=1e-5, atol=1e-9)), (rows, n)
    # a step without the slot filled is not capturable
    inp = ma.prepare(batch, True, gt_pad=8)
    assert inp.erd_tab is None and not ma.capturable(inp, 0, None)
    inp.erd_tab = erd.step_table(ma, batch)
    assert ma.capturable(inp, 0, None) and ("erd_tab", (2, 5)) in inp.signature()


# ------------------------------------------------------------------------------------------------- episode
def _task_data(task):
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


def _episode(dev, folder, use_graph, spy_order=None):
    from vilco_amd import _lib
    from vilco_amd.cl_methods import erd
    from vilco_amd.train_cl import run_episodes
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    mp = pytest.MonkeyPatch()
    if spy_order is not None:
        real_record, real_release = erd.record_clips, erd.ERDBank.release

        def record(model, bank, loader, j, opts=None):
            spy_order.append(('record begins', len(bank), sum(len(r) for r in bank.retired)))
            out = real_record(model, bank, loader, j, opts)
            spy_order.append(('record ends', len(bank), sum(len(r) for r in bank.retired)))
            return out

        def release(self):
            spy_order.append(('release', len(self), sum(len(r) for r in self.retired)))
            return real_release(self)
        mp.setattr(erd, 'record_clips', record)
        mp.setattr(erd.ERDBank, 'release', release)
    try:
        cfg, model = _erd_model(dev)
        cfg = dict(cfg, opt=dict(cfg['opt'], epochs=1, warmup_epochs=1))
        cfg['cl_cfg'] = dict(cfg['cl_cfg'], path_memory='memory.pkl')
        stream = InMemoryQILStream([_task_data(0), _task_data(1)], batch_size=2, seed=3)
        random.seed(0)                      # the memory's random selection
        torch.manual_seed(0)                # the new rows of the class head (augment_classification)
        torch.cuda.manual_seed_all(0)
        calls = []

        def validate(m, epoch, task):
            calls.append(task)
            return 1.0 if calls.count(task) == 2 else 0.1
        model, opt, sch, log = run_episodes(cfg, model, stream, validate=validate, ckpt_folder=str(folder), gpu_id=0,
                                            use_graph=use_graph, keep_history=True)
        torch.cuda.synchronize()
    finally:
        mp.undo()
        _lib.check(_lib.load().vilco_seed_word_set(0, None))
        torch.cuda.synchronize()
    return model, log


def test_two_task_episode_eager_and_replayed(dev, tmp_path):
    """run_episodes with cl_cfg.name = 'erd' over the two-task in-memory stream, eager and with replayed steps: task 0 adds nothing;
    at the start of task 1 every clip its loader yields is recorded (`erd_recorded`, `erd_bytes`); every loss of every iteration
    and the final state_dict are the same bits in both runs"""
    order = []
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    me, le = _episode(dev, tmp_path / "a", False)
    mg, lg = _episode(dev, tmp_path / "b", True, spy_order=order)
    for log in (le, lg):
        assert len(log) == 2 and 'erd_recorded' not in log[0] and 'erd_bytes' not in log[0]
        assert all('erd_loss' not in h for ep in log[0]['history'] for h in ep)
        assert log[1]['erd_recorded'] > 0 and log[1]['erd_bytes'] >= 8 * log[1]['erd_recorded']
    assert le[1]['erd_recorded'] == lg[1]['erd_recorded'] and le[1]['erd_bytes'] == lg[1]['erd_bytes']
    assert 0 < len(mg.erd_bank) <= lg[1]['erd_recorded'] and mg.erd_bank.nbytes() <= lg[1]['erd_bytes']
    he = [h for e in le for ep in e['history'] for h in ep]
    hg = [h for e in lg for ep in e['history'] for h in ep]
    erds = [float(h['erd_loss']) for h in hg if 'erd_loss' in h]
    print("erd_loss per iteration of task 1: %s; recorded %d, %d bytes, skipped %d" %
          (["%.4g" % d for d in erds], lg[1]['erd_recorded'], lg[1]['erd_bytes'], mg.erd_bank.skipped))
    assert erds and all(d == d and abs(d) != float('inf') and d >= 0.0 for d in erds)
    assert len(he) == len(hg)
    for i, (a, b) in enumerate(zip(he, hg)):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k].detach().reshape(()).float(), b[k].detach().reshape(()).float()), (i, k, float(a[k]), float(b[k]))
    se, sg = me.state_dict(), mg.state_dict()
    assert set(se) == set(sg)
    diff = [k for k in se if not torch.equal(se[k], sg[k])]
    assert not diff, diff
    # the hook's order at the one task boundary with known classes: cleared, recorded, then released
    assert [o[0] for o in order] == ['record begins', 'record ends', 'release'] and order[0][1] == 0 and order[1][1] > 0


def test_rerecording_drops_the_old_buffers_only_after_the_new_are_in_place(dev):
    """a third task: begin_task retires the second task's records, records the third's, and only then lets the old buffers go --
    a table built at any moment names live memory"""
    import weakref
    from vilco_amd.cl_methods import erd, hooks
    cfg, model = _erd_model(dev)
    hook = hooks.ERD(cfg)
    hook.begin_run(model, None)
    model.n_known = 2
    b0, b1 = cases.episode_batches(0)[0], cases.episode_batches(1)[0]
    entry = {}
    hook.begin_task(1, model, None, [b0], entry)
    assert entry['erd_recorded'] == len(b0) and entry['erd_bytes'] == model.erd_bank.nbytes() > 0
    old = [weakref.ref(t) for r in model.erd_bank.records.values() for t in r.buffers()]
    seen = {}
    real = erd.record_clips

    def spy(m, bank, loader, j, opts=None):
        out = real(m, bank, loader, j, opts)
        seen['alive'] = all(w() is not None for w in old)
        seen['new'] = len(bank)
        return out
    mp = pytest.MonkeyPatch()
    mp.setattr(erd, 'record_clips', spy)
    try:
        entry = {}
        hook.begin_task(2, model, None, [b1], entry)
    finally:
        mp.undo()
    torch.cuda.synchronize()
    assert seen == {'alive': True, 'new': len(b1)} and all(w() is None for w in old) and model.erd_bank.retired == []
    assert {erd.clip_key(v) for v in b1} == set(model.erd_bank.records)
