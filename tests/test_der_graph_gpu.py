"""Dark Experience Replay in the step and in the episode loop (vilco_amd/cl_methods/der.py, PtTransformer._cl_terms' 'der'
branch, graph.GraphedStep, train_cl.run_episodes), on the small episode model the A-GEM and distillation graph tests build.

  * a step captured with one `der_tab` and replayed with others follows the table of ITS batch: bit for bit the eager step;
  * a two-task episode records the memory clips' logits at the task boundary, at the head's width of that time, and task 1
    trains against them -- eagerly and with replayed steps, ending in the same parameter bits;
  * the term of the first task-1 iteration against the float64 restatement (tests/der_restatement.py) on the same logits,
    within the bounds tests/test_der_op_gpu.py derives."""
import random

import pytest
import torch

import der_restatement as D
from parity_util import cases, episode_full_state, load_episode_golden

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ALPHA = 0.5


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture
def seed_word_zero():
    """the dropout step word is process-wide device state: leave it at 0 for the other tests"""
    from vilco_amd import _lib
    yield
    _lib.check(_lib.load().vilco_seed_word_set(0, None))
    torch.cuda.synchronize()


def _der_model(dev):
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_episode_golden()
    over = dict(gold['overrides'])
    over['cl_cfg'] = dict(over.get('cl_cfg', {}), name='der', type_sampling='random', der_alpha=ALPHA)
    cfg = make_config(**over)
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    state = episode_full_state(gold['init_state'])
    model.load_state_dict(state, strict=True)
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    assert model.cl_name == 'der' and model.der_alpha == ALPHA and model.der_bank is None
    return cfg, model


def _levels(model):
    return tuple(model.max_seq_len // s for s in model.fpn_strides)


# ------------------------------------------------------------------------------------------------- one step, changing tables
def test_replayed_step_follows_the_table_of_its_batch(dev, seed_word_zero):
    """graph calls over the SAME clips with the bank in four states: a record for row 0 (call 0 eager, call 1 captures and
    replays); a record (another one, narrower) for row 1 only; no record at all (all-zero addresses); both rows.  Every call equals the
    eager step of a twin model in the same state: losses and every gradient, bit for bit."""
    from vilco_amd.cl_methods import der
    from vilco_amd.graph import GraphedStep
    batch = cases.episode_batches(0)[0]
    assert len(batch) == 2
    twins = []
    for _ in range(2):
        _, m = _der_model(dev)
        m.train()
        for mod in m.modules():
            if hasattr(mod, "drop_prob"):
                mod.drop_prob = 0.0            # stochastic depth draws from torch's generator: not what is compared here
        m.pre_train_epoch(task_id=0, current_epoch=0)
        m.n_known = 2
        m.der_bank = der.DERBank()
        twins.append(m)
    ma, mb = twins
    levels = _levels(ma)
    C_ = ma.cls_head.cls_head.conv.out_channels
    g = torch.Generator().manual_seed(3)
    recs = [torch.randn(sum(levels), C_, generator=g).to(dev), torch.randn(sum(levels), max(C_ - 1, 1), generator=g).to(dev)]
    states = [(0,), (0,), (1,), (), (0, 1)]

    def set_state(model, rows):
        model.der_bank.records = {}
        for r in rows:
            assert model.der_bank.record(batch[r]['video_id'], recs[r], der.clip_len(batch[r]), levels)

    gs = GraphedStep(ma, None, eager_steps=1)
    got = []
    for rows in states:
        set_state(ma, rows)
        tab = der.step_table(ma, batch)
        assert [int(a != 0) for a in tab[:, 0].tolist()] == [int(r in rows) for r in range(2)]
        out = gs(batch, task_id=0)
        torch.cuda.synchronize()
        got.append(({k: v.clone() for k, v in out.items()},
                    {n: p.grad.clone() for n, p in ma.named_parameters() if p.grad is not None}))
    assert gs.stats['captured'] == 1 and gs.stats['replayed'] == 4 and gs.stats['eager'] == 1, gs.stats
    ders = [float(o['der_loss']) for o, _ in got]
    print("der_loss per table:", ders)
    assert ders[0] > 0 and ders[2] > 0 and ders[1] != ders[2] and ders[3] == 0.0 and ders[4] > 0
    assert ma.der_bank.skipped == 0
    for rows, (out, grads) in zip(states, got):
        set_state(mb, rows)
        for p in mb.parameters():
            p.grad = None
        want = mb(batch, task_id=0)
        want['final_loss'].backward()
        torch.cuda.synchronize()
        assert set(out) == set(want) and 'der_loss' in want
        for k in want:
            assert torch.equal(out[k].reshape(()), want[k].detach().reshape(()).float()), (rows, k, float(out[k]), float(want[k]))
        wg = {n: p.grad for n, p in mb.named_parameters() if p.grad is not None}
        assert set(wg) == set(grads)
        for n in wg:        # (the gaussian-weight gradients are float atomics in loss_bwd: equal up to summation order)
            assert torch.equal(grads[n], wg[n]) or (any(t in n for t in ("mu", "sigma", "scale")) and
                                                    torch.allclose(grads[n], wg[n], rtol=1e-5, atol=1e-9)), (rows, n)
    # a step without the slot filled is not capturable; without known classes the method does not key on it
    inp = ma.prepare(batch, True, gt_pad=8)
    assert inp.der_tab is None and not ma.capturable(inp, 0, None)
    inp.der_tab = der.step_table(ma, batch)
    assert ma.capturable(inp, 0, None) and not ma.capturable(inp, 0, [[recs[0]]])
    assert ("der_tab", (2, 2)) in inp.signature()


# ------------------------------------------------------------------------------------------------- episode
def _task_data(task):
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


@pytest.fixture(scope="module")
def episodes(dev, tmp_path_factory):
    """run_episodes with cl_cfg.name = 'der' over the two-task in-memory stream of tests/test_agem_gpu.py, eagerly and with
    replayed steps: {use_graph: (log, final parameters, GraphedStep stats, bank, folder)}.  The eager run also keeps what the
    FIRST der term of task 1 was given and returned (`probe`)."""
    from vilco_amd import _lib, ops
    from vilco_amd import graph as graph_mod
    from vilco_amd.train_cl import run_episodes
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    runs, probe, cur = {}, {}, {}
    real_step, real_op = graph_mod.GraphedStep, ops.der_replay
    made = []

    class Spy(real_step):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    def spy_op(logits, level_row, level_T, valid_lens, der_tab, alpha, **kw):
        if not probe:
            x = logits.detach().clone().requires_grad_(True)
            loss, count = real_op(x, level_row, level_T, valid_lens, der_tab, alpha, return_count=True)
            (grad,) = torch.autograd.grad(loss, x)
            probe.update(records={r[0].data_ptr(): r[0] for r in cur['model'].der_bank.records.values()},
                         x=x.detach(), level_row=list(level_row), level_T=list(level_T), valid=valid_lens.clone(),
                         tab=der_tab.clone(), alpha=alpha, loss=loss.detach().clone(), count=count.clone(), grad=grad)
        return real_op(logits, level_row, level_T, valid_lens, der_tab, alpha, **kw)
    mp = pytest.MonkeyPatch()
    mp.setattr(graph_mod, 'GraphedStep', Spy)
    try:
        for use_graph in (False, True):
            del made[:]
            cfg, model = _der_model(dev)
            cur['model'] = model
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
            folder = str(tmp_path_factory.mktemp("der%d" % use_graph))
            if not use_graph:
                mp.setattr(ops, 'der_replay', spy_op)
            model, opt, sch, log = run_episodes(cfg, model, stream, validate=validate, ckpt_folder=folder, gpu_id=0,
                                                use_graph=use_graph, keep_history=True)
            if not use_graph:
                mp.setattr(ops, 'der_replay', real_op)
            torch.cuda.synchronize()
            runs[use_graph] = (log, {n: p.detach().clone() for n, p in model.named_parameters()}, [dict(g.stats) for g in made],
                               model.der_bank, folder, model.memory)
    finally:
        mp.undo()
        _lib.check(_lib.load().vilco_seed_word_set(0, None))
        torch.cuda.synchronize()
    runs['probe'] = probe
    return runs


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_task_episode_under_der(episodes, use_graph):
    import os
    from vilco_amd.cl_methods.der import DERBank
    from vilco_amd.train_cl import DER_BANK_FILE
    log, params, stats, bank, folder, memory = episodes[use_graph]
    assert len(log) == 2
    # task 0: nothing to replay
    hist0 = [h for ep in log[0]['history'] for h in ep]
    assert hist0 and all('der_loss' not in h or float(h['der_loss']) == 0.0 for h in hist0)
    # task 1: the term is in every step's loss dictionary, positive where the batch holds a memory clip
    hist1 = [h for ep in log[1]['history'] for h in ep]
    ders = [float(h['der_loss']) for h in hist1]
    print("use_graph=%s: der_loss per iteration of task 1: %s" % (use_graph, ["%.4g" % d for d in ders]))
    assert len(ders) > 0 and all(d >= 0.0 for d in ders) and max(ders) > 0.0
    assert all(bool(torch.isfinite(h['final_loss'])) for e in log for ep in e['history'] for h in ep)
    assert all(bool(torch.isfinite(p).all()) for p in params.values())
    # the bank: one record per memory clip, task-0 clips at task-0 width
    mem_ids = {v['video_id'] for vs in memory.values() for v in vs}
    assert mem_ids and set(bank.records) == mem_ids and bank.skipped == 0
    assert log[0]['der_recorded'] > 0 and log[0]['der_dropped'] == 0
    ids0 = {v['video_id'] for c, vs in memory.items() if c < cases.EP_NCLS0 for v in vs}
    new1 = {v['video_id'] for c, vs in memory.items() if c >= cases.EP_NCLS0 for v in vs} - ids0
    assert ids0, "task 0's classes are still in the memory"
    for vid in ids0:
        buf, n, lv = bank.get(vid)
        assert buf.shape[1] == cases.EP_NCLS0 and buf.dtype == torch.float32 and buf.is_cuda and buf.is_contiguous()
        assert buf.shape[0] == sum(lv) and bool(torch.isfinite(buf).all())
    for vid in new1:
        assert bank.get(vid)[0].shape[1] == cases.EP_NCLS0 + cases.EP_NEW
    # written next to the memory pickle
    path = os.path.join(folder, DER_BANK_FILE)
    assert os.path.exists(path) and os.path.exists(os.path.join(folder, 'memory.pkl'))
    back = DERBank().load_state_dict(torch.load(path, weights_only=False))
    assert set(back.records) == mem_ids
    assert all(torch.equal(back.get(k)[0], bank.get(k)[0].cpu()) for k in mem_ids)
    if use_graph:
        assert len(stats) == 2, "a GraphedStep per task"
        print("replay counters:", stats)
        assert stats[1]['replayed'] > 0 and stats[1]['captured'] > 0, stats
        assert stats[1]['replayed'] + stats[1]['eager'] == len(hist1)
    else:
        assert stats == []


def test_replayed_episode_ends_where_the_eager_one_does(episodes):
    """equal bits, with the proviso tests/test_graph_gpu.py makes for the gaussian-weight parameters and regression scales
    (loss.hip accumulates their gradients with float atomics)"""
    eager, replayed = episodes[False][1], episodes[True][1]
    assert sorted(eager) == sorted(replayed) and len(eager) > 50
    d0 = [float(h['der_loss']) for ep in episodes[False][0][1]['history'] for h in ep]
    d1 = [float(h['der_loss']) for ep in episodes[True][0][1]['history'] for h in ep]
    assert d0 == d1
    for vid, rec in episodes[False][3].records.items():
        assert torch.equal(rec[0], episodes[True][3].get(vid)[0]), vid
    for n in eager:
        assert torch.equal(eager[n], replayed[n]) or (any(t in n for t in ("mu", "sigma", "scale")) and
                                                      torch.allclose(eager[n], replayed[n], rtol=1e-5, atol=1e-12)), n


def test_first_task1_term_against_the_restatement(episodes):
    """the first der term of task 1, on the logits the step gave it: loss within gamma(4) + u of the float64 restatement's,
    every element of the logit gradient within gamma(3) + ulp(c) / c of its value, N equal (tests/test_der_op_gpu.py)"""
    p = episodes['probe']
    assert p and p['alpha'] == ALPHA
    by_addr = p['records']           # the bank as it was at that step (task 1's end evicts some of these clips)
    tab = p['tab'].tolist()
    records = [by_addr[a] if a else None for a, _ in tab]
    assert any(r is not None for r in records), "the first batch of task 1 holds a memory clip"
    assert all(r is None or r.shape[1] == n == cases.EP_NCLS0 for r, (_, n) in zip(records, tab))
    assert p['x'].shape[2] == cases.EP_NCLS0 + cases.EP_NEW, "the head has grown since the records were made"
    w_loss, w_N, w_grad, mask, _ = D.der_term(p['x'], p['level_row'], p['level_T'], p['valid'].tolist(), records, ALPHA)
    assert int(p['count']) == w_N > 0
    got = float(p['loss'].double())
    print("loss %.6g, restatement %.6g, err / bound %.3f" % (got, w_loss, abs(got - w_loss) / ((gamma(4) + U) * w_loss)))
    assert abs(got - w_loss) <= (gamma(4) + U) * w_loss
    grad = p['grad'].double().cpu()
    assert bool((grad[~mask] == 0).all())
    bound = (gamma(3) + 2 * U) * w_grad[mask].abs() + 2.0 ** -149
    assert bool(((grad[mask] - w_grad[mask]).abs() <= bound).all())
