"""Pooled feature distillation in the step and in the episode loop (vilco_amd/cl_methods/pod.py, PtTransformer._cl_terms' 'pod'
branch, graph.GraphedStep, train_cl.run_episodes), on the small episode model the DER and distillation graph tests build.

  * a step captured with one `pod_tab` and replayed with others -- one of them all zeros -- follows the table of ITS batch:
    bit for bit the eager step;
  * ops.pod_distill on the model's own pyramid against cl_methods.pod.pod_term and the float64 restatement, within the loss
    bound tests/test_pod_op_gpu.py derives; record_clips' records are the restatement's;
  * a two-task episode records every clip of task 1 from the incoming model and trains against the records with replayed steps."""
import random

import pytest
import torch

import pod_restatement as P
from parity_util import cases, episode_full_state, load_episode_golden

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LAMBDA = 0.5


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture
def seed_word_zero():
    """the dropout step word is process-wide device state: leave it at 0 for the other tests"""
    from vilco_amd import _lib
    yield
    _lib.check(_lib.load().vilco_seed_word_set(0, None))
    torch.cuda.synchronize()


def _pod_model(dev):
    import vilco_amd.modeling as vm
    from ref_import import xlnet_json
    from vilco_amd.core.config import make_config
    gold = load_episode_golden()
    over = dict(gold['overrides'])
    over['cl_cfg'] = dict(over.get('cl_cfg', {}), name='pod', type_sampling='random', pod_lambda=LAMBDA)
    cfg = make_config(**over)
    model = vm.make_meta_arch('LocPointTransformer', **dict(cfg['model'], xlnet_config=xlnet_json(cfg['model']['embd_dim'], cases.EP_H)))
    state = episode_full_state(gold['init_state'])
    model.load_state_dict(state, strict=True)
    model = model.to(dev)
    model.loss_normalizer = cfg['model']['train_cfg']['init_loss_norm']
    assert model.cl_name == 'pod' and model.pod_lambda == LAMBDA and model.pod_bank is None
    return cfg, model


def _levels(model):
    return tuple(model.max_seq_len // s for s in model.fpn_strides)


def _pyramid(model, batch):
    """the pyramid an eval-mode pass of `model` gives `batch` -> (features, level lengths)"""
    model._pod_step = None
    was = model.training
    model.eval()
    with torch.no_grad():
        model(batch, task_id=0, get_emb=True)
    model.train(was)
    (feats, level_len), model._pod_step = model._pod_step, None
    return feats, level_len


# ------------------------------------------------------------------------------------------------- one step, changing tables
def test_replayed_step_follows_the_table_of_its_batch(dev, seed_word_zero):
    """graph calls over the SAME clips with the bank in five states: a record for row 0 (call 0 eager, call 1 captures and
    replays); a record for row 1 only; no record at all (all-zero addresses); both rows.  Every call equals the eager step of a
    twin model in the same state: losses and every gradient, bit for bit."""
    from vilco_amd.cl_methods import pod
    from vilco_amd.graph import GraphedStep
    batch = cases.episode_batches(0)[0]
    assert len(batch) == 2
    twins = []
    for _ in range(2):
        _, m = _pod_model(dev)
        m.train()
        for mod in m.modules():
            if hasattr(mod, "drop_prob"):
                mod.drop_prob = 0.0            # stochastic depth draws from torch's generator: not what is compared here
        m.pre_train_epoch(task_id=0, current_epoch=0)
        m.n_known = 2
        m.pod_bank = pod.PODBank()
        twins.append(m)
    ma, mb = twins
    levels = _levels(ma)
    feats, _ = _pyramid(ma, batch)
    assert tuple(int(f.shape[1]) for f in feats) == levels
    C_ = int(feats[0].shape[2])
    g = torch.Generator().manual_seed(3)
    recs = []
    for _ in range(2):
        parts = [torch.randn(C_ + T, generator=g) for T in levels]
        recs.append(torch.cat([p / p.norm() for p in parts]).to(dev))
    states = [(0,), (0,), (1,), (), (0, 1)]

    def set_state(model, rows):
        model.pod_bank.clear()
        for r in rows:
            model.pod_bank.record(batch[r]['video_id'], recs[r], pod.clip_len(batch[r]), levels, C_)

    gs = GraphedStep(ma, None, eager_steps=1)
    got = []
    for rows in states:
        set_state(ma, rows)
        tab = pod.step_table(ma, batch)
        assert [int(a != 0) for a in tab.tolist()] == [int(r in rows) for r in range(2)]
        out = gs(batch, task_id=0)
        torch.cuda.synchronize()
        got.append(({k: v.clone() for k, v in out.items()},
                    {n: p.grad.clone() for n, p in ma.named_parameters() if p.grad is not None}))
    assert gs.stats['captured'] == 1 and gs.stats['replayed'] == 4 and gs.stats['eager'] == 1, gs.stats
    pods = [float(o['pod_loss']) for o, _ in got]
    print("pod_loss per table:", pods)
    assert pods[0] > 0 and pods[2] > 0 and pods[1] != pods[2] and pods[3] == 0.0 and pods[4] > 0
    assert ma.pod_bank.skipped == 0
    for rows, (out, grads) in zip(states, got):
        set_state(mb, rows)
        for p in mb.parameters():
            p.grad = None
        want = mb(batch, task_id=0)
        want['final_loss'].backward()
        torch.cuda.synchronize()
        assert set(out) == set(want) and 'pod_loss' in want
        for k in want:
            assert torch.equal(out[k].reshape(()), want[k].detach().reshape(()).float()), (rows, k, float(out[k]), float(want[k]))
        wg = {n: p.grad for n, p in mb.named_parameters() if p.grad is not None}
        assert set(wg) == set(grads)
        for n in wg:        # (the gaussian-weight gradients are float atomics in loss_bwd: equal up to summation order)
            assert torch.equal(grads[n], wg[n]) or (any(t in n for t in ("mu", "sigma", "scale")) and
                                                    torch.allclose(grads[n], wg[n], rtol=1e-5, atol=1e-9)), (rows, n)
    # a step without the slot filled is not capturable
    inp = ma.prepare(batch, True, gt_pad=8)
    assert inp.pod_tab is None and not ma.capturable(inp, 0, None)
    inp.pod_tab = pod.step_table(ma, batch)
    assert ma.capturable(inp, 0, None) and not ma.capturable(inp, 0, [[recs[0]]])
    assert ("pod_tab", (2,)) in inp.signature()


def test_op_equals_the_tensor_op_body_on_the_models_pyramid(dev):
    """ops.pod_distill and cl_methods.pod.pod_term on the pyramid the model gives a batch, against independent random records:
    both within the loss bound of tests/test_pod_op_gpu.py (eta = gamma(4) per compared pair, absolute, plus the final fp32
    rounding), the body's widened by its fp32 norms (gamma(k + 4) each, k = C + T_0); record_clips' records are the
    restatement's u to gamma(4) and give the op an exact zero"""
    from vilco_amd import ops
    from vilco_amd.cl_methods import pod
    _, model = _pod_model(dev)
    batch = cases.episode_batches(0)[0]
    feats, level_len = _pyramid(model, batch)
    levels, C_, L = [int(f.shape[1]) for f in feats], int(feats[0].shape[2]), len(feats)
    valid = level_len.tolist()
    g = torch.Generator().manual_seed(11)
    recs = []
    for _ in range(len(batch)):
        parts = [torch.randn(C_ + T, generator=g) for T in levels]
        recs.append(torch.cat([p / p.norm() for p in parts]).to(dev))
    tab = torch.tensor([r.data_ptr() for r in recs], dtype=torch.int64, device=dev)
    scale = 1.25
    w = P.pod_term(feats, valid, recs, scale)
    assert min(w['dist'][b][l] for b, l in w['gv']) > 0.1
    loss, count = ops.pod_distill(feats, level_len, tab, scale, return_count=True)
    body, n = pod.pod_term(feats, valid, recs, scale)
    npairs = len(w['gv'])
    Wt = scale / (L * len(batch))
    b_op = Wt * npairs * gamma(4) + U * w['loss']
    b_body = Wt * npairs * (2 * gamma(C_ + max(levels) + 4) + gamma(4)) + gamma(npairs + 2) * w['loss']
    print("op %.7g body %.7g restatement %.7g (bounds %.3g / %.3g)" % (float(loss), float(body), w['loss'], b_op, b_body))
    assert int(count) == n == len(batch)
    assert abs(float(loss) - w['loss']) <= b_op and abs(float(body) - w['loss']) <= b_body
    # the records record_clips writes for these clips
    bank = pod.PODBank()
    assert pod.record_clips(model, bank, [batch], 0) == len(batch) == len(bank)
    for b, v in enumerate(batch):
        buf, n_len, lv, c = bank.get(v['video_id'])
        assert (n_len, lv, c) == (pod.clip_len(v), tuple(levels), C_) and buf.is_cuda
        want = P.make_record([f[b].cpu() for f in feats], valid[b])
        assert bool(((buf.double().cpu() - want).abs() <= gamma(4) * want.abs() + 2.0 ** -149).all())
    tab = bank.table_for(batch, [pod.clip_len(v) for v in batch], device=dev, level_T=levels, C=C_)
    torch.cuda.synchronize()
    assert all(int(a) != 0 for a in tab.tolist())
    assert float(ops.pod_distill(feats, level_len, tab, scale)) == 0.0


# ------------------------------------------------------------------------------------------------- episode
def _task_data(task):
    data = {}
    for b in cases.episode_batches(task):
        for v in b:
            for c in v['labels'].tolist():
                if (task == 0 and c < cases.EP_NCLS0) or (task == 1 and c >= cases.EP_NCLS0):
                    data.setdefault(c, []).append(v)
    return data


def test_two_task_episode_under_pod(dev, tmp_path):
    """run_episodes with cl_cfg.name = 'pod' over the two-task in-memory stream, with replayed steps: task 0 adds nothing; at the
    start of task 1 every clip its loader yields is recorded, and the term is finite and non-zero in task 1's steps"""
    from vilco_amd import _lib
    from vilco_amd import graph as graph_mod
    from vilco_amd.train_cl import run_episodes
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    made = []
    real_step = graph_mod.GraphedStep

    class Spy(real_step):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    mp = pytest.MonkeyPatch()
    mp.setattr(graph_mod, 'GraphedStep', Spy)
    try:
        cfg, model = _pod_model(dev)
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
        model, opt, sch, log = run_episodes(cfg, model, stream, validate=validate, ckpt_folder=str(tmp_path), gpu_id=0,
                                            use_graph=True, keep_history=True)
        torch.cuda.synchronize()
    finally:
        mp.undo()
        _lib.check(_lib.load().vilco_seed_word_set(0, None))
        torch.cuda.synchronize()
    assert len(log) == 2 and model.training
    assert 'pod_recorded' not in log[0]
    hist0 = [h for ep in log[0]['history'] for h in ep]
    assert hist0 and all('pod_loss' not in h for h in hist0)
    assert log[1]['pod_recorded'] > 0 and len(model.pod_bank) > 0 and len(model.pod_bank) <= log[1]['pod_recorded']
    hist1 = [h for ep in log[1]['history'] for h in ep]
    pods = [float(h['pod_loss']) for h in hist1]
    print("pod_loss per iteration of task 1: %s; recorded %d, skipped %d; replay counters %s"
          % (["%.4g" % d for d in pods], log[1]['pod_recorded'], model.pod_bank.skipped, [dict(g.stats) for g in made]))
    assert pods and all(d == d and abs(d) != float('inf') and d >= 0.0 for d in pods) and max(pods) > 0.0
    assert all(bool(torch.isfinite(h['final_loss'])) for e in log for ep in e['history'] for h in ep)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert len(made) == 2 and made[1].stats['replayed'] > 0 and made[1].stats['captured'] > 0, [g.stats for g in made]
