"""GPU: the HIP NLQ scorer (`vilco_nlq_recall` via vilco_amd.utils.metrics_nlq) against the imported reference's goldens
(tests/golden/nlq_metrics.npz) and the NumPy restatement: recall tables and per-query flags equal, first-row IoU bit-equal, mIoU
within (n - 1) * 2**-53; record dicts and the device-resident stream score identically; `evaluate_segments` equals the prefix
evaluations; the validation functions return the same numbers on the stream path as on the dict path, with one scoring launch
and no host copy while records are appended.

Appends are checked under `torch.cuda.set_sync_debug_mode("error")` when this torch build honours it (probed with an `.item()`
that has to raise); otherwise `Tensor.cpu`, `.item` and `.tolist` are patched to raise for the duration of the appends.  The
mode that was used is printed; on the MI355X with torch-ROCm it was `set_sync_debug_mode` (it is honoured there: it refused the
pageable host-to-device copy an earlier version of `append` made)."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import nlq_metrics_restatement as R
from parity_util import HERE, cases

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture()
def evs(dev, tmp_path):
    from vilco_amd.utils import ReferringRecall, make_nlq_evaluator
    g = R.golden()
    gt = R.text(g, 'gt')
    ego = make_nlq_evaluator(R.write_ego4d(gt, tmp_path))
    anet = ReferringRecall(dataset="tacos", gt_file=R.write_jsonl(R.to_jsonl_gt(gt), tmp_path))
    return g, gt, ego, anet


def _to_stream(ev, recs, seg=None, dev="cuda"):
    st = ev.new_stream(capacity=4)                                   # small: the buffer has to grow
    for i, r in enumerate(recs):
        t = torch.tensor(r['predicted_times'], dtype=torch.float32, device=dev)
        st.append((r['clip_uid'], r['annotation_uid'], r['query_idx']), t[:, :2], t[:, 2], 0 if seg is None else int(seg[i]))
    return st


def _fp32_records(recs):
    """the records as the validation loop builds them: fp32 rows widened by .tolist()"""
    return [dict(r, predicted_times=torch.tensor(r['predicted_times'], dtype=torch.float32).tolist()) for r in recs]


@pytest.mark.parametrize("case", R.EGO_CASES)
def test_device_matches_reference_goldens(evs, case):
    from vilco_amd.utils import evaluate_nlq_performance
    g, gt, ego, anet = evs
    recs = R.text(g, case + '_pred')
    frac, s0 = ego.evaluate(recs, verbose=False)
    pct, s1 = ego.evaluate(recs, verbose=True)
    print(case, frac.tolist(), pct.tolist())
    assert s0 is None and isinstance(s1, str) and "Rank@1" in s1
    np.testing.assert_array_equal(frac, g[case + '_frac'])
    np.testing.assert_array_equal(pct, g[case + '_pct'])                        # percent when verbose
    mean, miou, per = evaluate_nlq_performance(recs, gt, list(R.THRESHOLDS), list(R.TOPK), per_instance=True)
    np.testing.assert_array_equal(mean, g[case + '_mean'])
    np.testing.assert_array_equal(np.array(per['results'], dtype=bool), g[case + '_flags'])
    np.testing.assert_array_equal(_bits(np.array(per['average_IoU']).reshape(-1)), _bits(g[case + '_avg']))
    np.testing.assert_array_equal(_bits(per['overlap']), _bits(g[case + '_overlap']))
    n, want = len(recs), float(g[case + '_miou'])
    print(case, "mIoU", float(miou), want, "bound", (n - 1) * 2.0 ** -53)
    if np.isnan(want):
        assert np.isnan(miou)
    else:
        assert abs(float(miou) - want) <= (n - 1) * 2.0 ** -53
    mean2, miou2 = evaluate_nlq_performance({str(i): r for i, r in enumerate(recs)}, gt, list(R.THRESHOLDS), list(R.TOPK))
    assert np.array_equal(mean2, mean) and _bits(miou2) == _bits(miou)
    # evaluate_anet: the fp32 mode
    sub = R.to_submission(recs)
    a0 = anet.evaluate_anet(sub, verbose=False)
    a1 = anet.evaluate_anet(sub, verbose=True)
    assert a0.dtype == torch.float32 and tuple(a0.shape) == (3, 2)
    np.testing.assert_array_equal(a0.numpy(), g[case + '_anet_frac'])
    np.testing.assert_array_equal(a1.numpy(), g[case + '_anet_pct'])


def test_unknown_key_raises(evs):
    g, gt, ego, anet = evs
    with pytest.raises(AssertionError, match="Instance not present!"):
        ego.evaluate(R.text(g, 'unknown_pred'), verbose=False)
    with pytest.raises(AssertionError, match="Instance not present!"):
        _to_stream(ego, R.text(g, 'unknown_pred'))


def test_dict_and_stream_inputs_score_identically(evs):
    from vilco_amd.utils import metrics_nlq as M
    g, gt, ego, anet = evs
    for case in R.EGO_CASES:
        recs = _fp32_records(R.text(g, case + '_pred'))
        st = _to_stream(ego, recs)
        assert len(st) == len(recs) and st.seg.shape[0] >= len(recs)
        for verbose in (False, True):
            a, _ = ego.evaluate(recs, verbose=verbose)
            b, _ = ego.evaluate(st, verbose=verbose)
            assert a.tobytes() == b.tobytes()
        d = ego._score(recs, M.MODE_NUMPY64, want_flags=True)
        s = ego._score(st, M.MODE_NUMPY64, want_flags=True)
        assert torch.equal(d['flags'], s['flags']) and torch.equal(d['hits'], s['hits'])
        assert d['top1'].cpu().numpy().tobytes() == s['top1'].cpu().numpy().tobytes()
        assert d['top1_sum'].cpu().numpy().tobytes() == s['top1_sum'].cpu().numpy().tobytes()
        # the stream gives the records back (first 10 rows) and the submission content
        back = st.records()
        assert [r['predicted_times'] for r in back] == [r['predicted_times'][:10] for r in recs]
        assert M.submission(back) == M.submission(recs)


def test_evaluate_segments_equals_prefix_evaluations(evs):
    from vilco_amd.utils import metrics_nlq as M
    g, gt, ego, anet = evs
    recs, seg = R.text(g, 'seg_pred'), g['seg_id']
    # the reference's 13 prefix tables, from record dicts (13 launches) ...
    for k in range(13):
        pct, _ = ego.evaluate([r for r, s in zip(recs, seg) if s <= k], verbose=True)
        np.testing.assert_array_equal(pct, g['seg_pct'][k])
    # ... and from ONE launch over the stream
    st = _to_stream(ego, _fp32_records(recs), seg)
    before = M.LAUNCHES
    tables = ego.evaluate_segments(st, verbose=True)
    assert M.LAUNCHES == before + 1 and len(tables) == 13
    f32 = _fp32_records(recs)
    for k, (pct, s) in enumerate(tables):
        want, _ = ego.evaluate([r for r, sg in zip(f32, seg) if sg <= k], verbose=True)
        assert pct.tobytes() == want.tobytes() and isinstance(s, str)
    frac = ego.evaluate_segments(st, verbose=False, n_seg=15)
    assert len(frac) == 15 and frac[14][0].tobytes() == frac[12][0].tobytes() and frac[0][1] is None
    np.testing.assert_array_equal(frac[12][0] * 100, tables[12][0])


@pytest.mark.parametrize("mode,fp32", [(0, False), (0, True), (1, False), (1, True)])
def test_large_random_against_restatement(dev, mode, fp32):
    from vilco_amd.utils import metrics_nlq as M
    rng = np.random.default_rng(11 + 2 * mode + fp32)
    n, k_cap, n_seg = 200_000, 10, 13
    gs = np.round(rng.uniform(0, 400, n), 3)
    gt = np.stack([gs, gs + np.round(rng.uniform(0, 60, n), 3)], axis=1)
    zero = rng.uniform(size=n) < 0.01
    gt[zero, 0] = np.round(gt[zero, 0] * 8) / 8                                      # (exact in fp32 too)
    gt[zero, 1] = gt[zero, 0]                                                        # zero-length ground truth
    w = (gt[:, 1] - gt[:, 0])[:, None]
    ps = gt[:, None, 0] + rng.normal(0, 0.5, (n, k_cap)) * (w + 1)
    pe = gt[:, None, 1] + rng.normal(0, 0.5, (n, k_cap)) * (w + 1)
    pred = np.stack([np.minimum(ps, pe), np.maximum(ps, pe)], axis=2)
    exact = rng.uniform(size=(n, k_cap)) < 0.05                                      # the window itself: 0/0 on zero length
    pred[exact] = np.broadcast_to(gt[:, None, :], pred.shape)[exact]
    third = rng.uniform(size=(n, k_cap)) < 0.05                                      # IoU at a threshold
    pred[third, 0] = np.broadcast_to(gt[:, None, 0], third.shape)[third]
    pred[third, 1] = (np.broadcast_to(gt[:, None, 0], third.shape) + 0.5 * np.broadcast_to(w, third.shape))[third]
    if fp32:
        pred = pred.astype(np.float32)
    cnt = rng.integers(0, k_cap + 1, n).astype(np.int32)
    seg = rng.integers(0, n_seg, n).astype(np.int32)
    thr, ranks = (0.3, 0.5, 0.7), (1, 3, 5, 10, 25)
    args = (torch.as_tensor(pred).cuda(), torch.as_tensor(cnt).cuda(), torch.as_tensor(gt).cuda(), thr, ranks, mode)
    out = M.nlq_recall_device(*args, seg_id=torch.as_tensor(seg).cuda(), n_seg=n_seg, want_flags=True)
    flags, top1 = R.flags_and_top1(pred, cnt, gt, thr, ranks, mode)
    got = out['flags'].cpu().numpy().astype(bool)
    assert got.shape == flags.shape and flags.any() and not flags.all()
    np.testing.assert_array_equal(got, flags)
    np.testing.assert_array_equal(_bits(out['top1'].cpu().numpy()), _bits(top1))
    assert np.isnan(top1[cnt > 0]).any()
    hits = np.stack([flags[seg == s].sum(axis=0) for s in range(n_seg)])
    np.testing.assert_array_equal(out['hits'].cpu().numpy(), hits)
    np.testing.assert_array_equal(out['n'].cpu().numpy(), np.bincount(seg, minlength=n_seg))
    again = M.nlq_recall_device(*args, seg_id=torch.as_tensor(seg).cuda(), n_seg=n_seg, want_flags=True)
    for k in ('hits', 'n', 'top1', 'top1_sum', 'flags'):
        assert out[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
    # one segment, no ids: the totals; finite sums agree with NumPy's to the summation-order bound
    one = M.nlq_recall_device(*args)
    np.testing.assert_array_equal(one['hits'][0].cpu().numpy(), hits.sum(axis=0))
    assert int(one['n'][0]) == n
    fin = np.isfinite(top1)
    sel = torch.as_tensor(np.flatnonzero(fin)).cuda()
    part = M.nlq_recall_device(args[0][sel], args[1][sel], args[2][sel], thr, ranks, mode)
    m = int(fin.sum())
    assert abs(float(part['top1_sum'][0]) / m - np.mean(top1[fin])) <= (m - 1) * 2.0 ** -53
    # no queries at all
    empty = M.nlq_recall_device(args[0][:0], args[1][:0], args[2][:0], thr, ranks, mode, n_seg=2)
    assert int(empty['hits'].abs().sum()) == 0 and empty['n'].tolist() == [0, 0] and empty['top1_sum'].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------- validation functions
@contextlib.contextmanager
def no_host_copies():
    """see the module docstring"""
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    no_host_copies.used = "set_sync_debug_mode" if honoured else "patched Tensor.cpu/.item/.tolist"
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
        try:
            yield
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return
    saved = {k: getattr(torch.Tensor, k) for k in ("cpu", "item", "tolist")}

    def refuse(*a, **k):
        raise AssertionError("host copy while appending to the record stream")
    for k in saved:
        setattr(torch.Tensor, k, refuse)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(torch.Tensor, k, v)


class _ValTasks:
    def get_valSet_by_taskNum(self, n):
        return [([[q] for q in list(cases.nlq_episode_data(k).values())[0]], 1) for k in range(n)]


class _DictOnly:
    """the same evaluator without the stream interface: the validation functions take the record-dict path"""

    def __init__(self, ev):
        self.ev, self.dataset, self.calls = ev, ev.dataset, []

    def evaluate(self, results, verbose=True):
        self.calls.append(len(results))
        return self.ev.evaluate(results, verbose=verbose)


def _episode_model(dev):
    import vilco_amd.modeling_nlq as nlq
    gold = torch.load(os.path.join(HERE, "golden", "nlq_episode.pt"), weights_only=False)
    model = nlq.make_meta_arch('LocPointTransformer', **cases.nlq_model_cfg())
    model.load_state_dict(gold['init_state'], strict=True)
    return model.to(dev), gold


def _guard_appends(monkeypatch):
    from vilco_amd.utils import metrics_nlq as M
    inner = M.NLQRecordStream.extend
    count = []

    def extend(self, *a, **k):
        with no_host_copies():
            count.append(1)
            return inner(self, *a, **k)
    monkeypatch.setattr(M.NLQRecordStream, "extend", extend)
    return count


def test_validation_stream_path_equals_dict_path(dev, tmp_path, monkeypatch):
    from vilco_amd.utils import make_nlq_evaluator, metrics_nlq as M, train_utils_nlq as tu
    model, gold = _episode_model(dev)
    ev = make_nlq_evaluator(R.write_ego4d(R.episode_gt(), tmp_path))
    # the reference evaluator's table for the reference's own recorded final-validation records
    final = gold['tasks'][-1]['results']
    g = R.golden()
    np.testing.assert_array_equal(ev.evaluate(final, verbose=True)[0], g['episode_pct'])
    np.testing.assert_array_equal(ev.evaluate(final, verbose=False)[0], g['episode_frac'])
    flags, _ = R.evaluate(final, R.gt_windows(R.episode_gt()))
    np.testing.assert_array_equal(R.recall(flags) * 100, g['episode_pct'])
    appends = _guard_appends(monkeypatch)
    vt, plain = _ValTasks(), _DictOnly(ev)
    for task in range(cases.NLQ_EP_TASKS):
        a = tu.valid_one_epoch_cl_single_gpu(vt, model, 0, task, evaluator=plain)
        before = M.LAUNCHES
        b = tu.valid_one_epoch_cl_single_gpu(vt, model, 0, task, evaluator=ev)
        assert M.LAUNCHES == before + 1
        print("valid", task, a, b)
        assert np.float64(a).tobytes() == np.float64(b).tobytes()
    task = cases.NLQ_EP_TASKS - 1
    ra, rb = {'val': [50.0, 37.5], 'test': []}, {'val': [50.0, 37.5], 'test': []}
    plain.calls.clear()
    n_app = len(appends)
    a = tu.final_validate(vt, model, 0, task, evaluator=plain, list_val_recall_ii=ra)
    assert plain.calls == [4, 8, 12] and len(appends) == n_app                       # the accumulated lists, scored 3 times
    before = M.LAUNCHES
    b = tu.final_validate(vt, model, 0, task, evaluator=ev, list_val_recall_ii=rb)
    assert M.LAUNCHES == before + 1                                                  # ONE scoring launch
    assert len(appends) == n_app + 12
    print("final", a, b, ra, rb, "appends checked with", no_host_copies.used)
    assert np.float64(a).tobytes() == np.float64(b).tobytes() and np.isfinite(b)
    assert ra == rb and len(rb['val']) == 3


def test_valid_one_epoch_nlq_singlegpu_writes_submission(dev, tmp_path, monkeypatch):
    from vilco_amd.utils import ReferringRecall, metrics_nlq as M, train_utils_nlq as tu
    g = R.golden()
    gt = R.text(g, 'gt')
    for video in gt['videos']:                        # the stand-in loader's query ids are split at '_'
        for clip in video['clips']:
            for ann in clip['annotations']:
                ann['annotation_uid'] = ann['annotation_uid'].replace('_', '-')
    ev = ReferringRecall(dataset="ego4d", gt_file=R.write_ego4d(gt, tmp_path))
    records = R.text(g, 'sub_records')

    class Model:
        def eval(self):
            return self

        def __call__(self, video_list, is_training=False):
            t = torch.tensor(records[video_list[0]['i']]['predicted_times'], dtype=torch.float32, device=dev)
            return [{'segments': t[:, :2].contiguous(), 'scores': t[:, 2].contiguous()}]
    loader = [[{'i': i, 'query_id': '%s_%d' % (r['annotation_uid'], r['query_idx']), 'video_id': r['clip_uid']}]
              for i, r in enumerate(records)]
    _guard_appends(monkeypatch)
    out = str(tmp_path / "sub.json")
    perf, s = tu.valid_one_epoch_nlq_singlegpu(loader, Model(), 0, evaluator=ev, output_file=out)
    with open(out) as f:
        assert json.load(f) == R.text(g, 'sub_json')
    want, _ = ev.evaluate(records, verbose=True)
    assert perf.tobytes() == want.tobytes() and isinstance(s, str)
    plain = _DictOnly(ev)
    perf2, _ = tu.valid_one_epoch_nlq_singlegpu(loader, Model(), 0, evaluator=plain)
    assert perf2.tobytes() == perf.tobytes()
    # the 'rows' case itself, whose fp64 rows these fp32 records were made from, scores the same table here
    assert M.LAUNCHES > 0


def test_run_episodes_nlq_with_device_evaluator(dev, tmp_path, monkeypatch):
    """one short episode (three templates, two epochs each) with make_nlq_evaluator: every validation's R@1 equals the
    restatement's on the records of that validation, read back from the stream"""
    from vilco_amd.train_cl import run_episodes_nlq
    from vilco_amd.utils import make_nlq_evaluator, metrics_nlq as M
    from vilco_amd.utils.cl_stream import InMemoryQILStream
    model, gold = _episode_model(dev)
    mcfg = cases.nlq_model_cfg()
    cfg = {'opt': cases.nlq_episode_opt(0.5), 'train_cfg': mcfg['train_cfg'],
           'cl_cfg': dict(mcfg['cl_cfg'], memory_size=cases.NLQ_EP_MEMORY, path_memory='mem.pkl')}
    stream = InMemoryQILStream([cases.nlq_episode_data(j) for j in range(cases.NLQ_EP_TASKS)], batch_size=cases.NLQ_EP_BATCH,
                               shuffle=False)
    ev = make_nlq_evaluator(R.write_ego4d(R.episode_gt(), tmp_path))
    win = R.gt_windows(R.episode_gt())
    inner = M.ReferringRecall.evaluate_segments
    seen, calls = [], []

    def evaluate_segments(self, st, verbose=True, n_seg=None):
        flags, _ = R.evaluate(st.records(), win)
        seg = np.array(st.seg_id)
        seen.append([R.recall(flags[seg <= s])[0, 0] * 100 for s in range(n_seg)])
        return inner(self, st, verbose=verbose, n_seg=n_seg)
    monkeypatch.setattr(M.ReferringRecall, "evaluate_segments", evaluate_segments)
    _guard_appends(monkeypatch)
    before = M.LAUNCHES
    model, opt, sch, log = run_episodes_nlq(cfg, model, stream, _ValTasks(), ev, ckpt_folder=str(tmp_path), ckpt_freq=2,
                                            on_validate=lambda kind, j, epoch, r1: calls.append((kind, j, epoch, r1)))
    assert len(log) == cases.NLQ_EP_TASKS and len(calls) == len(seen) == M.LAUNCHES - before
    for (kind, j, epoch, r1), prefixes in zip(calls, seen):
        assert len(prefixes) == j + 1
        want = float(np.mean(prefixes)) if kind == 'final' else prefixes[-1]
        print(kind, j, epoch, r1, want)
        assert np.isfinite(r1) and r1 == want
    for j, entry in enumerate(log):
        finals = [r1 for kind, jj, _, r1 in calls if kind == 'final' and jj == j]
        others = [r1 for kind, jj, _, r1 in calls if kind != 'final' and jj == j]
        assert np.isfinite(entry['final_R1']) and entry['final_R1'] == finals[0]
        assert np.isfinite(entry['best_R1']) and entry['best_R1'] == max(others)
