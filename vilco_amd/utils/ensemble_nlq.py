"""NLQ model ensembling on the device: the reference's challenge-submission recipe (NLQ/ensemble.py:7-101, 123-143 with
NLQ/temporal_nms.py:6-74) for M models and all queries in one launch of `vilco_nlq_ensemble` (csrc/ensemble.hip).

Per query: the first `top1_max_input` rows of every model are clustered by their centres into new proposals, the proposals are
appended to the first `max_input` rows of every model, a greedy temporal NMS (`nms_thd`, at most `max_after_nms` rows) runs
over that list and the result is padded with its last row.  The rules, the accidental ones included (the span in place of the
union, chains of centres, the dict keyed by centre), are those of the reference and are written out in include/vilco_hip.h.
The arithmetic is fp64 in the reference's order, so results are bit-equal to the reference's for FINITE inputs; Python's
`sorted` has no defined answer for NaN, so there is nothing to match for it.  Every model must supply at least one row per
query.  Rows are [start, end, score].

Records are paired by KEY -- (clip_uid, annotation_uid, query_idx), or query_id for the jsonl datasets -- not by position as in
the reference; the output follows the first input's order and inputs whose key sets differ raise ValueError.
No CPU fallback, as in `ops`.

Command line (replaces the reference's hard-coded `__main__`): writes the challenge file and, with --gt, prints the
evaluator's table:
  python -m vilco_amd.utils.ensemble_nlq OUT.json A.json B.json [C.json ...] [--gt nlq_val.json] [--max-input 4 ...]
"""
import argparse
import json

import numpy as np
import torch

from .. import _lib
from .metrics_nlq import NLQRecordStream, ReferringRecall

DEFAULTS = dict(max_input=4, top1_max_input=1, distance=2, nms_thd=0.5, max_after_nms=5, pad=True)
MAX_MODELS, MAX_INPUT, MAX_TOP1_ROWS, MAX_CANDIDATES = 8, 10, 64, 128       # the kernel's limits (include/vilco_hip.h)
LAUNCHES = 0                    # calls of vilco_nlq_ensemble since import (tests assert one launch per ensemble)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _params(kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown ensemble parameter(s): %s" % ", ".join(sorted(unknown)))
    return dict(DEFAULTS, **kw)


def nlq_ensemble_device(pred, cnt, want_proposals=False, **params):
    """One ensemble launch.  pred [n_model, n_query, k_cap, 3] fp32 or fp64 and cnt [n_model, n_query] int32 on the device.
    Returns device tensors (out [n_query, max_after_nms, 3] fp64, out_cnt [n_query] int32: the rows kept before padding);
    with want_proposals also (prop [n_query, n_model * top1_max_input, 4] fp64: start, end, score, total; prop_cnt).
    Nothing is copied to the host and nothing waits for the device."""
    global LAUNCHES
    p = _params(params)
    assert pred.dim() == 4 and pred.shape[3] == 3 and pred.is_contiguous() and pred.dtype in (torch.float32, torch.float64)
    n_model, n, k_cap = int(pred.shape[0]), int(pred.shape[1]), int(pred.shape[2])
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (n_model, n) and cnt.is_contiguous()
    dev = pred.device
    out = torch.empty((n, p["max_after_nms"], 3), dtype=torch.float64, device=dev)
    out_cnt = torch.empty(n, dtype=torch.int32, device=dev)
    prop = prop_cnt = None
    if want_proposals:
        prop = torch.zeros((n, max(n_model * p["top1_max_input"], 1), 4), dtype=torch.float64, device=dev)
        prop_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    if n:
        LAUNCHES += 1
    _lib.check(_lib.load().vilco_nlq_ensemble(
        pred.data_ptr() if n else None, int(pred.dtype == torch.float32), cnt.data_ptr() if n else None, n_model, n, k_cap,
        int(p["max_input"]), int(p["top1_max_input"]), float(p["distance"]), float(p["nms_thd"]), int(p["max_after_nms"]),
        int(bool(p["pad"])), out.data_ptr() if n else None, out_cnt.data_ptr() if n else None,
        prop.data_ptr() if want_proposals else None, prop_cnt.data_ptr() if want_proposals else None, _stream()))
    return (out, out_cnt, prop, prop_cnt) if want_proposals else (out, out_cnt)


# ---------------------------------------------------------------------------------------------------------------- streams
class NLQEnsembleStream(NLQRecordStream):
    """The ensemble of several record streams, on the device.  Keys, ground-truth indices and segment ids are those of the
    first stream; `table` [n, max_after_nms, 3] fp64 holds (start, end, score), `kept` [n] the rows before padding.
    `ReferringRecall.evaluate` / `evaluate_segments` take it like any NLQRecordStream."""

    def __init__(self, first, table, kept, params):
        self.gt_index, self.k_cap, self.dataset, self.device = first.gt_index, int(table.shape[1]), first.dataset, table.device
        self.keys, self.video_ids = list(first.keys), list(first.video_ids)
        self.gt_idx, self.seg_id = list(first.gt_idx), list(first.seg_id)
        self.table, self.kept, self.params = table, kept, dict(params)
        self.cnt = None                                   # the row counts live on the device: `kept`, or k_cap when padded

    def append(self, *a, **k):
        raise TypeError("an NLQEnsembleStream is the result of ensemble_streams(); append to the input streams")

    def flush(self):
        pass

    def device_columns(self):
        """(pred [n, max_after_nms, 2] fp64, cnt, gt index, segment id) on the device"""
        n = len(self)
        small = torch.tensor([self.gt_idx, self.seg_id], dtype=torch.int64).reshape(2, n).to(self.device)
        cnt = torch.full_like(self.kept, self.k_cap) if self.params["pad"] else self.kept
        return self.table[:, :, :2].contiguous(), cnt, small[0], small[1].int()

    def records(self):
        """the reference's output records ([start, end] rows); ONE host copy of the table"""
        rows = self.table[:, :, :2].cpu().tolist()
        kept = [self.k_cap] * len(self) if self.params["pad"] else self.kept.cpu().tolist()
        out = []
        for key, vid, r, c in zip(self.keys, self.video_ids, rows, kept):
            if self.dataset in ("ego4d", "ego4d_cl"):
                out.append({'query_idx': key[2], 'annotation_uid': key[1], 'predicted_times': r[:c], 'clip_uid': key[0]})
            else:
                out.append({'query_id': key, 'predicted_times': r[:c], 'video_id': vid})
        return out


def _pair(key_lists):
    """per input the positions of the first input's keys; ValueError unless all inputs hold the same keys once"""
    first = key_lists[0]
    if len(set(first)) != len(first):
        raise ValueError("input 0 holds a query twice")
    out = [list(range(len(first)))]
    for m, keys in enumerate(key_lists[1:], 1):
        pos = {k: i for i, k in enumerate(keys)}
        if len(pos) != len(keys):
            raise ValueError("input %d holds a query twice" % m)
        if set(pos) != set(first):
            diff = sorted(map(str, set(pos) ^ set(first)))
            raise ValueError("inputs 0 and %d hold different queries (%d differ, e.g. %s)" % (m, len(diff), diff[0]))
        out.append([pos[k] for k in first])
    return out


def _check_sizes(n_model, k_cap, p):
    """the kernel's limits, as ValueError before anything is built"""
    if not 1 <= n_model <= MAX_MODELS:
        raise ValueError("1 to %d models can be ensembled, not %d" % (MAX_MODELS, n_model))
    if not 1 <= p["max_input"] <= MAX_INPUT or p["max_input"] > k_cap:
        raise ValueError("max_input must be in 1..%d and at most the rows kept per query (%d)" % (MAX_INPUT, k_cap))
    t = min(p["top1_max_input"], k_cap)
    if p["top1_max_input"] < 0 or n_model * p["top1_max_input"] > MAX_TOP1_ROWS or n_model * (p["max_input"] + t) > MAX_CANDIDATES:
        raise ValueError("too many rows per query for the ensemble kernel")
    if not 1 <= p["max_after_nms"] <= MAX_CANDIDATES:
        raise ValueError("max_after_nms must be in 1..%d" % MAX_CANDIDATES)


def ensemble_streams(streams, **params):
    """The ensemble of M NLQRecordStreams holding the same queries (paired by key; the first stream's order): one launch,
    no host copy of any row.  Returns an NLQEnsembleStream."""
    p = _params(params)
    streams = list(streams)
    if not streams:
        raise ValueError("no streams to ensemble")
    order = _pair([s.keys for s in streams])
    k_cap = min(s.k_cap for s in streams)
    _check_sizes(len(streams), k_cap, p)
    if any(c < 1 for s in streams for c in s.cnt):
        raise ValueError("every model must supply at least one row per query")
    first, n = streams[0], len(streams[0])
    dev = first.device
    preds, cnts = [], []
    for s, idx in zip(streams, order):
        s.flush()
        rows = torch.cat([s.seg[:n, :k_cap], s.score[:n, :k_cap, None]], dim=2).to(dev)
        if idx != list(range(n)):
            rows = rows[torch.tensor(idx, dtype=torch.int64).to(dev)]
        preds.append(rows)
        cnts.append([min(s.cnt[i], k_cap) for i in idx])
    pred = torch.stack(preds).contiguous()
    cnt = torch.tensor(cnts, dtype=torch.int32).reshape(len(streams), n).to(dev)
    table, kept = nlq_ensemble_device(pred, cnt, **p)
    return NLQEnsembleStream(first, table, kept, p)


# ------------------------------------------------------------------------------------------------------ records and files
def load_predictions(path):
    """the record list of a prediction file: the challenge file's 'results', or a bare list"""
    with open(path) as f:
        data = json.load(f)
    return data["results"] if isinstance(data, dict) else data


def challenge_file(records):
    """the content of the reference's submission file (NLQ/ensemble.py:145-153)"""
    return {"version": "1.0", "challenge": "ego4d_nlq_challenge", "results": records}


def write_challenge_file(path, records):
    with open(path, "w") as f:
        json.dump(challenge_file(records), f)


def _key(rec):
    return rec["query_id"] if "query_id" in rec else (rec["clip_uid"], rec["annotation_uid"], rec["query_idx"])


def _pack(rows_of, k_cap):
    """[n, k_cap, 3] fp64 and the counts from per-query row lists"""
    pred = np.zeros((len(rows_of), k_cap, 3), dtype=np.float64)
    cnt = np.zeros(len(rows_of), dtype=np.int32)
    for i, rows in enumerate(rows_of):
        if len(rows) < 1:
            raise ValueError("every model must supply at least one row per query")
        rows = rows[:k_cap]
        pred[i, :len(rows)] = [[r[0], r[1], r[2]] for r in rows]
        cnt[i] = len(rows)
    if not np.isfinite(pred).all():
        raise ValueError("predicted_times must be finite")
    return pred, cnt


def ensemble_predictions(inputs, **params):
    """inputs: M record lists or paths of prediction files.  Returns the reference-shaped record list: every field of the
    first input's record, `predicted_times` replaced by the ensemble's [start, end] rows."""
    p = _params(params)
    lists = [load_predictions(x) if isinstance(x, str) else list(x) for x in inputs]
    if not lists:
        raise ValueError("no predictions to ensemble")
    order = _pair([[_key(r) for r in recs] for recs in lists])
    k_cap = max(p["max_input"], p["top1_max_input"], 1)
    _check_sizes(len(lists), k_cap, p)
    packed = [_pack([recs[i]["predicted_times"] for i in idx], k_cap) for recs, idx in zip(lists, order)]
    pred = torch.as_tensor(np.stack([a for a, _ in packed])).cuda()
    cnt = torch.as_tensor(np.stack([c for _, c in packed])).cuda()
    table, kept = nlq_ensemble_device(pred, cnt, **p)
    rows = table[:, :, :2].cpu().tolist()
    kept = [p["max_after_nms"]] * len(rows) if p["pad"] else kept.cpu().tolist()
    out = []
    for rec, r, c in zip(lists[0], rows, kept):
        new = rec.copy()
        new["predicted_times"] = r[:c]
        out.append(new)
    return out


# ------------------------------------------------------------------------------------------- the reference's two functions
def _rows3(rows):
    """[start, end, score] of a list or host tensor of rows; the score is the last column, as the generator reads it"""
    rows = rows.tolist() if torch.is_tensor(rows) else rows
    return [[float(r[0]), float(r[1]), float(r[-1])] for r in rows]


def _split(rows, per_model):
    """one list as consecutive models of per_model rows: [n_model, 1, per_model, 3] fp64 and the counts, on the device"""
    n_model = -(-len(rows) // per_model)
    pred = np.zeros((n_model, 1, per_model, 3), dtype=np.float64)
    cnt = np.zeros((n_model, 1), dtype=np.int32)
    for m in range(n_model):
        part = rows[m * per_model:(m + 1) * per_model]
        pred[m, 0, :len(part)] = part
        cnt[m, 0] = len(part)
    return torch.as_tensor(pred).cuda(), torch.as_tensor(cnt).cuda()


def temporal_nms(predictions, nms_thd, max_after_nms=100):
    """NLQ/temporal_nms.py:25-74 for one list of [start, end, score] rows (a list or a host tensor; at most 80 rows): the rows
    kept, by score.  Runs through the ensemble kernel with the generator switched off."""
    rows = _rows3(predictions)
    if not rows:
        return []
    if len(rows) > MAX_MODELS * MAX_INPUT:
        raise ValueError("temporal_nms takes at most %d rows" % (MAX_MODELS * MAX_INPUT))
    pred, cnt = _split(rows, MAX_INPUT)
    out, kept = nlq_ensemble_device(pred, cnt, max_input=MAX_INPUT, top1_max_input=0, nms_thd=nms_thd,
                                    max_after_nms=min(int(max_after_nms), MAX_CANDIDATES), pad=False)
    return out[0, :int(kept[0])].cpu().tolist()


def top1_generator(input_list):
    """NLQ/ensemble.py:30-101 for one list of rows (start, end, ..., score; at most 64): the proposals
    [start, end, score, 0, total] by total.  Runs through the ensemble kernel, which also returns its proposals."""
    rows = _rows3(input_list)
    if not 1 <= len(rows) <= MAX_TOP1_ROWS:
        raise ValueError("top1_generator takes 1 to %d rows" % MAX_TOP1_ROWS)
    per_model = -(-len(rows) // MAX_MODELS)
    pred, cnt = _split(rows, per_model)
    _, _, prop, prop_cnt = nlq_ensemble_device(pred, cnt, want_proposals=True, max_input=1, top1_max_input=per_model)
    return [[s, e, w, 0, t] for s, e, w, t in prop[0, :int(prop_cnt[0])].cpu().tolist()]


# ------------------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    ap = argparse.ArgumentParser(description="Ensemble NLQ prediction files into one challenge file (the reference's NLQ/ensemble.py).")
    ap.add_argument("out", help="the challenge file to write")
    ap.add_argument("inputs", nargs="+", help="prediction files of the models, in model order")
    ap.add_argument("--gt", help="ground-truth file: print the evaluator's table for the ensemble")
    ap.add_argument("--dataset", default="ego4d")
    ap.add_argument("--max-input", type=int, default=DEFAULTS["max_input"])
    ap.add_argument("--top1-max-input", type=int, default=DEFAULTS["top1_max_input"])
    ap.add_argument("--distance", type=float, default=DEFAULTS["distance"])
    ap.add_argument("--nms-thd", type=float, default=DEFAULTS["nms_thd"])
    ap.add_argument("--max-after-nms", type=int, default=DEFAULTS["max_after_nms"])
    ap.add_argument("--no-pad", action="store_true")
    a = ap.parse_args(argv)
    records = ensemble_predictions(a.inputs, max_input=a.max_input, top1_max_input=a.top1_max_input, distance=a.distance,
                                   nms_thd=a.nms_thd, max_after_nms=a.max_after_nms, pad=not a.no_pad)
    write_challenge_file(a.out, records)
    print("wrote %d records to %s" % (len(records), a.out))
    if a.gt:
        ReferringRecall(dataset=a.dataset, gt_file=a.gt).evaluate(records, verbose=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
