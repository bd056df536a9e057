"""NLQ evaluation on the device: the reference's `ReferringRecall` (NLQ/libs/utils/metrics.py:10-177) and
`evaluate_nlq_performance` (NLQ/evaluate_ego4d_nlq.py:61-116) with their signatures, scored by `vilco_nlq_recall`
(csrc/evaluate.hip), and `NLQRecordStream`, the device-resident form of the validation records.

The host maps record keys to ground-truth indices (dictionary work) and packs the first max(topK) rows of dict records; the
IoU, the threshold tests and the per-segment counts run on the GPU.  No CPU fallback, as in `ops`.

Reference behaviour kept on purpose (DESIGN.md sections 3.9 and 7): `evaluate(verbose=True)` returns the table in PERCENT
(display_results multiplies the array in place) and a fraction otherwise; a 0/0 IoU is NaN, never a hit, and as a first row
it makes the mean IoU NaN; `evaluate_anet` works in fp32 with an unclamped hull.
"""
import ctypes as C
import json

import numpy as np
import torch

from .. import _lib

MODE_NUMPY64, MODE_TORCH32 = 0, 1
SUBMISSION_ROWS = 10            # rows of `predicted_times` the challenge file keeps (train_utils.py:682)
LAUNCHES = 0                    # calls of vilco_nlq_recall since import (tests assert one launch per final validation)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def load_jsonl(filename):
    with open(filename, "r") as f:
        return [json.loads(line.strip("\n")) for line in f.readlines()]


def nlq_recall_device(pred, cnt, gt, thresholds, ranks, mode=MODE_NUMPY64, seg_id=None, n_seg=1, want_flags=False):
    """One scoring launch.  pred [n, k_cap, 2] fp32 or fp64, cnt [n] int32, gt [n, 2] fp64, seg_id [n] int32 or None, all on
    the device.  Returns device tensors {'hits' [n_seg, n_thr, n_rank] int64, 'n' [n_seg] int64, 'top1' [n] fp64,
    'top1_sum' [n_seg] fp64, 'flags' [n, n_thr, n_rank] uint8 or None}; nothing is copied to the host here."""
    global LAUNCHES
    lib = _lib.load()
    thr = [float(x) for x in thresholds]
    rk = [int(x) for x in ranks]
    n, k_cap = int(pred.shape[0]), int(pred.shape[1])
    assert pred.dtype in (torch.float32, torch.float64) and pred.is_contiguous() and pred.shape[2] == 2
    assert cnt.dtype == torch.int32 and gt.dtype == torch.float64 and gt.is_contiguous()
    assert seg_id is None or seg_id.dtype == torch.int32
    dev = pred.device
    hits = torch.empty((n_seg, len(thr), len(rk)), dtype=torch.int64, device=dev)
    nq = torch.empty(n_seg, dtype=torch.int64, device=dev)
    top1 = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    top1_sum = torch.empty(n_seg, dtype=torch.float64, device=dev)
    flags = torch.empty((max(n, 1), len(thr), len(rk)), dtype=torch.uint8, device=dev) if want_flags else None
    nws = lib.vilco_nlq_recall_workspace(n, len(rk))
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
    thr_c = (C.c_double * len(thr))(*thr)
    rk_c = (C.c_int32 * len(rk))(*rk)
    LAUNCHES += 1
    _lib.check(lib.vilco_nlq_recall(pred.data_ptr() if n else None, int(pred.dtype == torch.float32),
                                    cnt.data_ptr() if n else None, k_cap, gt.data_ptr() if n else None,
                                    None if seg_id is None else seg_id.data_ptr(), n, n_seg, thr_c, len(thr), rk_c, len(rk),
                                    mode, hits.data_ptr(), nq.data_ptr(), top1.data_ptr(), top1_sum.data_ptr(),
                                    None if flags is None else flags.data_ptr(), ws.data_ptr(), nws, _stream()))
    return {'hits': hits, 'n': nq, 'top1': top1[:n], 'top1_sum': top1_sum, 'flags': None if flags is None else flags[:n]}


class NLQRecordStream(object):
    """Validation records kept on the device.  Per query: the first k_cap rows of `segments` and `scores` as the model
    returned them (fp32), the row count, the index of its ground truth and its segment id (the template it belongs to).
    Only these rows can influence a result: the evaluator cuts at K <= 10 and the submission file keeps 10 rows.
    `append` never synchronises: rows that are on the device are copied device to device; rows the model already left on
    the host (its postprocessing ends with the reference's copy to the host) are staged in a host mirror of the buffer and
    go up together when the stream is scored.  The buffers double when they are full."""

    def __init__(self, gt_index, k_cap=SUBMISSION_ROWS, capacity=256, device='cuda', dataset='ego4d_cl'):
        self.gt_index = gt_index              # key -> ground-truth row; raises for an unknown key
        self.k_cap = int(k_cap)
        self.dataset = dataset
        self.device = torch.device(device)
        self.seg = torch.zeros((capacity, self.k_cap, 2), dtype=torch.float32, device=self.device)
        self.score = torch.zeros((capacity, self.k_cap), dtype=torch.float32, device=self.device)
        self._host_seg = self._host_score = None      # the host mirror, made when the first host rows arrive
        self._pending = []                            # rows of the mirror not yet uploaded
        self.keys, self.video_ids, self.cnt, self.gt_idx, self.seg_id = [], [], [], [], []

    def __len__(self):
        return len(self.keys)

    @property
    def n_seg(self):
        return (max(self.seg_id) + 1) if self.seg_id else 1

    def _grow(self):
        for name in ('seg', 'score', '_host_seg', '_host_score'):
            old = getattr(self, name)
            if old is None:
                continue
            new = torch.zeros((2 * old.shape[0],) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
            new[:old.shape[0]].copy_(old)
            setattr(self, name, new)

    def append(self, key, segments, scores, seg_id=0, video_id=None):
        """key: (clip_uid, annotation_uid, query_idx), or the query id of the jsonl datasets"""
        rows = int(segments.shape[0])
        assert rows > 0
        gi = self.gt_index(key)
        i = len(self.keys)
        if i == self.seg.shape[0]:
            self._grow()
        m = min(rows, self.k_cap)
        if segments.is_cuda:
            self.seg[i, :m].copy_(segments[:m])
            self.score[i, :m].copy_(scores[:m])
        else:
            if self._host_seg is None:
                self._host_seg = torch.zeros(tuple(self.seg.shape), dtype=torch.float32)
                self._host_score = torch.zeros(tuple(self.score.shape), dtype=torch.float32)
            self._host_seg[i, :m].copy_(segments[:m])
            self._host_score[i, :m].copy_(scores[:m])
            self._pending.append(i)
        self.keys.append(key)
        self.video_ids.append(video_id)
        self.cnt.append(m)
        self.gt_idx.append(gi)
        self.seg_id.append(int(seg_id))

    def flush(self):
        """upload the staged host rows (one copy per buffer)"""
        if self._pending:
            idx = torch.tensor(self._pending, dtype=torch.int64)
            on_dev = idx.to(self.device)
            self.seg.index_copy_(0, on_dev, self._host_seg[idx].to(self.device))
            self.score.index_copy_(0, on_dev, self._host_score[idx].to(self.device))
            self._pending = []

    def extend(self, video_list, output, seg_id=0):
        """the records of one validation batch (the stream form of train_utils_nlq.prediction_records)"""
        for v, o in zip(video_list, output):
            if self.dataset in ("ego4d", "ego4d_cl"):
                uid, idx = v['query_id'].split("_")[:2]
                key = (v['video_id'], uid, int(idx))
            else:
                key = v['query_id']
            self.append(key, o['segments'], o['scores'], seg_id, v['video_id'])
        return self

    def device_columns(self):
        """(pred [n, k_cap, 2] fp32, cnt, gt index, segment id) on the device; the three small columns go up in one copy"""
        n = len(self)
        self.flush()
        small = torch.tensor([self.cnt, self.gt_idx, self.seg_id], dtype=torch.int64).reshape(3, n).to(self.device)
        return self.seg[:n], small[0].int(), small[1], small[2].int()

    def records(self):
        """the reference's list of record dicts; ONE host copy of the whole stream"""
        n = len(self)
        self.flush()
        rows = torch.cat([self.seg[:n], self.score[:n, :, None]], dim=2).cpu().tolist()
        out = []
        for key, vid, c, r in zip(self.keys, self.video_ids, self.cnt, rows):
            if self.dataset in ("ego4d", "ego4d_cl"):
                out.append({'query_idx': key[2], 'annotation_uid': key[1], 'predicted_times': r[:c], 'clip_uid': key[0]})
            else:
                out.append({'query_id': key, 'predicted_times': r[:c], 'video_id': vid})
        return out


def submission(results):
    """the Ego4D challenge file content of train_utils.py:676-690: every `predicted_times` cut to 10 rows"""
    save = []
    for item in results:
        new_item = item.copy()
        new_item["predicted_times"] = new_item["predicted_times"][:SUBMISSION_ROWS]
        save.append(new_item)
    return {"version": "1.0", "challenge": "ego4d_nlq_challenge", "results": save}


def _load_gt_from_json(ground_truth):
    gt_dict, num_gt_queries = {}, 0
    for video_datum in ground_truth["videos"]:
        for clip_datum in video_datum["clips"]:
            clip_uid = clip_datum["clip_uid"]
            for ann_datum in clip_datum["annotations"]:
                gt_dict[(clip_uid, ann_datum["annotation_uid"])] = ann_datum
                num_gt_queries += len(ann_datum["language_queries"])
    return gt_dict, num_gt_queries


class _QueryGT(object):
    """ground-truth windows as one fp64 table (on the device once it is needed) and the key -> row lookup"""

    def __init__(self, gt_dict, ego4d):
        self.ego4d = ego4d
        self.first, self.count, rows = {}, {}, []
        nan = float('nan')
        if ego4d:
            for key, ann in gt_dict.items():
                self.first[key] = len(rows)
                self.count[key] = len(ann["language_queries"])
                for q in ann["language_queries"]:
                    ok = "clip_start_sec" in q and "clip_end_sec" in q
                    rows.append([q["clip_start_sec"], q["clip_end_sec"]] if ok else None)
        else:
            for key, ts in gt_dict.items():
                self.first[key] = len(rows)
                rows.append([ts[0], ts[1]])
        self.missing = {i for i, r in enumerate(rows) if r is None}
        self.table = np.array([[nan, nan] if r is None else r for r in rows], dtype=np.float64).reshape(-1, 2)
        self._dev = None

    def index(self, key):
        if not self.ego4d:
            return self.first[key]                           # KeyError for an unknown query id, as the reference's dict
        assert key[:2] in self.first, "Instance not present!"
        i = self.first[key[:2]] + range(self.count[key[:2]])[key[2]]      # a list index: IndexError, negatives wrap
        if i in self.missing:
            raise KeyError("clip_start_sec")
        return i

    def device(self):
        if self._dev is None:
            self._dev = torch.as_tensor(self.table).cuda()
        return self._dev


def _pack_records(rows_of, k_cap):
    """[n, k_cap, 2] fp64 and the counts from per-record row lists ([[start, end, ...], ...] or one flat [start, end])"""
    n = len(rows_of)
    pred = np.zeros((n, k_cap, 2), dtype=np.float64)
    cnt = np.zeros(n, dtype=np.int32)
    for i, rows in enumerate(rows_of):
        assert isinstance(rows, list)
        if not isinstance(rows[0], list):
            rows = [rows]
        rows = rows[:k_cap]
        a = np.array(rows)                                   # as compute_IoU: the rows' dtype decides (ints become exact doubles)
        pred[i, :len(rows)] = a[:, :2]
        cnt[i] = len(rows)
    return pred, cnt


def _table_str(header, cells, title=None):
    """plain-text table: the reference's cells with two decimals (it used terminaltables)"""
    width = [max(len(h), len(c)) for h, c in zip(header, cells)]
    line = "+" + "+".join("-" * (w + 2) for w in width) + "+"
    row = lambda xs: "|" + "|".join(" " + x.center(w) + " " for x, w in zip(xs, width)) + "|"   # noqa: E731
    return "\n".join(([title] if title else []) + [line, row(header), line, row(cells), line])


class ReferringRecall(object):
    """NLQ/libs/utils/metrics.py:10-177 on the device."""
    thresholds = np.array([0.3, 0.5])
    topK = np.array([1, 5, 10])

    def __init__(self, dataset="ego4d", gt_file="./ego4d_data/ego4d_nlq_v2_ori_data/nlq_val.json"):
        self.dataset = dataset
        self.gt_file = gt_file
        ego4d = self.dataset in ("ego4d", "ego4d_cl")
        if ego4d:
            with open(self.gt_file) as file_id:
                self.gt_dict, self.num_gt_queries = self.load_gt_from_json(json.load(file_id))
        else:
            self.gt_dict = {}
            for d in load_jsonl(self.gt_file):
                self.gt_dict[d['query_id']] = d["timestamps"]
            self.num_gt_queries = len(self.gt_dict)
        self._gt = _QueryGT(self.gt_dict, ego4d)

    def load_gt_from_json(self, ground_truth):
        return _load_gt_from_json(ground_truth)

    # ------------------------------------------------------------------------------------------------------- stream interface
    def new_stream(self, capacity=256):
        """an empty NLQRecordStream bound to this evaluator's ground truth (the validation loops append to it)"""
        k_cap = max(int(np.max(self.topK)), SUBMISSION_ROWS)
        return NLQRecordStream(self._gt.index, k_cap=k_cap, capacity=capacity, dataset=self.dataset)

    def _score(self, predictions, mode, by_segment=0, want_flags=False):
        """by_segment: the number of segments to count separately (0: all records as one)"""
        if isinstance(predictions, NLQRecordStream):
            pred, cnt, gi, seg = predictions.device_columns()
            n_seg = by_segment if by_segment else 1
            return nlq_recall_device(pred, cnt, self._gt.device()[gi], self.thresholds, self.topK, mode,
                                     seg_id=seg if by_segment else None, n_seg=n_seg, want_flags=want_flags)
        assert not by_segment
        if mode == MODE_NUMPY64:
            gi, rows_of = [], []
            for pred_datum in predictions:
                gi.append(self._gt.index((pred_datum["clip_uid"], pred_datum["annotation_uid"], pred_datum["query_idx"])))
                rows_of.append(pred_datum["predicted_times"])
        else:
            gi = [self._gt.index(k['query_id']) for k in predictions]
            rows_of = [k["predicted_times"] for k in predictions]
        pred, cnt = _pack_records(rows_of, int(np.max(self.topK)))
        gt = self._gt.device()[torch.tensor(gi, dtype=torch.int64).cuda()] if gi else torch.zeros((0, 2), dtype=torch.float64).cuda()
        return nlq_recall_device(torch.as_tensor(pred).cuda(), torch.as_tensor(cnt).cuda(), gt, self.thresholds, self.topK,
                                 mode, want_flags=want_flags)

    # ------------------------------------------------------------------------------------------------------------ display
    def display_results(self, results, title=None):
        header = ["Rank@%s mIoU@%s" % (ii, jj) for ii in self.topK for jj in self.thresholds]
        results *= 100                                                   # in place: the caller's table becomes percent
        cells = ["%.02f" % results[jj][ii] for ii in range(len(self.topK)) for jj in range(len(self.thresholds))]
        return _table_str(header, cells, title)

    def display_results_anet(self, results, title=None):
        header = ["Rank@%s mIoU@%.1f" % (ii, jj) for ii in self.topK for jj in self.thresholds]
        results *= 100
        cells = ["%.02f" % results[ii][jj] for ii in range(len(self.topK)) for jj in range(len(self.thresholds))]
        return _table_str(header, cells, title)

    # ----------------------------------------------------------------------------------------------------------- evaluate
    def evaluate(self, predictions, verbose=True):
        """(mean_results[n_thr][n_rank], score_str) as :107-140; predictions: the list of record dicts or an NLQRecordStream"""
        out = self._score(predictions, MODE_NUMPY64)
        hits, n = out['hits'][0].cpu().numpy(), len(predictions)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean_results = hits.astype(np.float64) / np.float64(n)       # the mean of booleans: an exact sum over n
        score_str = None
        if verbose:
            print(f"Evaluated: {n} / {self.num_gt_queries} instances")
            score_str = self.display_results(mean_results)
            print(score_str, flush=True)
        return mean_results, score_str

    def evaluate_segments(self, stream, verbose=True, n_seg=None):
        """ONE launch for the whole stream: a list, per segment s, of what `evaluate` returns for the records of segments
        0..s (the accumulated list the continual-learning validation scores after each template), from prefix sums of the
        per-segment integer counts.  n_seg: at least this many segments (templates without queries at the end)"""
        out = self._score(stream, MODE_NUMPY64, by_segment=max(stream.n_seg, n_seg or 1))
        hits = np.cumsum(out['hits'].cpu().numpy(), axis=0)
        n = np.cumsum(out['n'].cpu().numpy())
        res = []
        for s in range(hits.shape[0]):
            with np.errstate(invalid='ignore', divide='ignore'):
                mean_results = hits[s].astype(np.float64) / np.float64(n[s])
            score_str = None
            if verbose:
                print(f"Evaluated: {n[s]} / {self.num_gt_queries} instances")
                score_str = self.display_results(mean_results)
                print(score_str, flush=True)
            res.append((mean_results, score_str))
        return res

    def evaluate_anet(self, submission, verbose=True):
        """recall[n_rank][n_thr] (float32 tensor) as :149-177, in the fp32 arithmetic of `_iou`"""
        out = self._score(submission, MODE_TORCH32)
        recall_x_iou = torch.tensor(out['hits'][0].cpu().numpy().T.copy(), dtype=torch.float32)
        recall_x_iou /= len(submission)
        if verbose:
            print(f"Evaluated: {len(submission)} / {self.num_gt_queries} instances")
            score_str = self.display_results_anet(recall_x_iou)
            print(score_str, flush=True)
        return recall_x_iou


def _host_overlap(rows, gt):
    """compute_IoU of one record (evaluate_ego4d_nlq.py:37-58); only for the `overlap` entry of the per-instance output,
    which is the reference's loop variable after its last iteration"""
    pred, gt = np.array(rows if isinstance(rows[0], list) else [rows]), np.array([gt])
    inter = np.maximum(0.0, np.minimum(pred[:, 1, None], gt[None, :, 1]) - np.maximum(pred[:, 0, None], gt[None, :, 0]))
    union = np.maximum(0.0, np.maximum(pred[:, 1, None], gt[None, :, 1]) - np.minimum(pred[:, 0, None], gt[None, :, 0]))
    with np.errstate(invalid='ignore', divide='ignore'):
        return 1.0 * inter / union                                       # [rows, 1]: the ground truth is a list of one


def evaluate_nlq_performance(predictions, ground_truth, thresholds, topK, per_instance=False):
    """evaluate_ego4d_nlq.py:61-116: (mean_results[n_thr][n_rank], mIoU) as fractions, plus with per_instance the dict
    {'overlap' (of the last record), 'average_IoU' (first-row IoU per record), 'results' [n_thr][n_rank][n] booleans}"""
    gt_dict, num_gt_queries = _load_gt_from_json(ground_truth)
    lookup = _QueryGT(gt_dict, True)
    records = [p if isinstance(p, dict) else predictions[p] for p in predictions]
    gi = [lookup.index((p["clip_uid"], p["annotation_uid"], p["query_idx"])) for p in records]
    k_cap = max(int(np.max(topK)) if len(topK) else 1, 1)
    pred, cnt = _pack_records([p["predicted_times"] for p in records], k_cap)
    gt = torch.as_tensor(lookup.table[gi].reshape(-1, 2)).cuda()
    out = nlq_recall_device(torch.as_tensor(pred).cuda(), torch.as_tensor(cnt).cuda(), gt, thresholds, topK, MODE_NUMPY64,
                            want_flags=per_instance)
    n = len(records)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean_results = out['hits'][0].cpu().numpy().astype(np.float64) / np.float64(n)
        mIoU = np.float64(out['top1_sum'].cpu().numpy()[0]) / np.float64(n)
    print(f"Evaluated: 0 / {num_gt_queries} instances")                 # the reference never counts its instances
    if not per_instance:
        return mean_results, mIoU
    flags = out['flags'].cpu().numpy().astype(bool)                      # [n, n_thr, n_rank]
    per_instance_results = {
        "overlap": _host_overlap(records[-1]["predicted_times"], lookup.table[gi[-1]].tolist()),
        "average_IoU": [np.array([x]) for x in out['top1'].cpu().numpy()],   # overlap[0] of a [rows, 1] array
        "results": [[list(flags[:, t, r]) for r in range(len(topK))] for t in range(len(thresholds))],
    }
    return mean_results, mIoU, per_instance_results


def make_nlq_evaluator(cfg_or_path, dataset=None):
    """the evaluator `run_episodes_nlq` and the validation functions take (NLQ/train_cl.py:127): from a config dict
    ({'dataset_name', 'dataset': {'json_file'}}) or from the ground-truth file's path (dataset defaults to 'ego4d_cl')"""
    if isinstance(cfg_or_path, dict):
        return ReferringRecall(dataset=dataset or cfg_or_path["dataset_name"], gt_file=cfg_or_path["dataset"]["json_file"])
    return ReferringRecall(dataset=dataset or "ego4d_cl", gt_file=cfg_or_path)
