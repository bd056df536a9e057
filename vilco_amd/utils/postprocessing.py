"""External classification scores for MQ validation: the library's counterpart of the reference's
MQ/libs/utils/postprocessing.py (loaders, `results_to_dict`, `results_to_array`, `postprocess_results`), with the
expansion itself on the device (csrc/fuse.hip, `vilco_score_fuse`).

Per video the `num_pred` best rows by score are kept, the `topk` best classes of the video's external class-score
vector are taken, and topk x rows new rows come out: label = the external class, score = sqrt(class score * row score),
the segments repeated.  Row order as in the reference: videos in sorted(set(video-id)) order, inside a video the classes
by rank, inside a class the kept rows by rank.

Ties: the reference ranks with `np.argsort(x)[::-1]`, an unstable sort that defines no order among equal values.  Here
both rankings are: descending value, equal values with the larger original index first (the reverse of a stable
ascending sort; NaN ranks first).  A negative class score gives a NaN fused score, as `np.sqrt` does.

`fuse_external_scores` returns the fused columns as device tensors that `ANETdetection.evaluate` takes as they are;
`postprocess_results` keeps the reference's signature and return value (host columns).  No CPU fallback."""
import ctypes as C
import json
import os
import pickle

import numpy as np
import torch

from .. import _lib

def load_results_from_pkl(filename):
    assert os.path.isfile(filename)
    with open(filename, "rb") as f:
        return pickle.load(f)


def load_results_from_json(filename):
    """a JSON result / score file; ActivityNet-style files keep their content under a top-level 'results' key"""
    assert os.path.isfile(filename)
    with open(filename, "r") as f:
        results = json.load(f)
    if 'results' in results:
        results = results['results']
    return results


def load_cls_scores(cls_score_file):
    """{video id: class-score vector}; a path with '.json' in it is JSON, anything else a pickle (the reference's test)"""
    if '.json' in cls_score_file:
        return load_results_from_json(cls_score_file)
    return load_results_from_pkl(cls_score_file)


def _host(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).reshape(-1)


def _by_video(results):
    """(sorted distinct video ids, per-row video index, stable row permutation that groups the rows by video)"""
    vids = np.asarray(results['video-id'], dtype=object).reshape(-1)
    uniq = sorted(set(vids.tolist()))
    index = {v: i for i, v in enumerate(uniq)}
    vidx = np.fromiter((index[v] for v in vids), dtype=np.int64, count=len(vids))
    return uniq, vidx, np.argsort(vidx, kind='stable')


def results_to_dict(results):
    """result columns -> {video id: [{'label', 'score', 'segment': [start, end]}, ...]} (rows in result order)"""
    uniq, _, _ = _by_video(results)
    out = {v: [] for v in uniq}
    for vid, s, e, lab, sc in zip(results['video-id'], _host(results['t-start']), _host(results['t-end']),
                                  _host(results['label']), _host(results['score'])):
        out[vid].append({"label": int(lab), "score": float(sc), "segment": [float(s), float(e)]})
    return out


def results_to_array(results, num_pred):
    """result columns -> {video id: {'label' [m], 'score' [m], 'segment' [m, 2]}}, the m = min(num_pred, rows) best rows
    of each video by score (the module's tie rule), as int64 / float64 arrays"""
    uniq, vidx, perm = _by_video(results)
    cnt = np.bincount(vidx, minlength=len(uniq))
    off = np.r_[0, np.cumsum(cnt)]
    lab = _host(results['label']).astype(np.int64)[perm]
    sc = _host(results['score']).astype(np.float64)[perm]
    seg = np.stack([_host(results['t-start']).astype(np.float64)[perm],
                    _host(results['t-end']).astype(np.float64)[perm]], 1)
    out = {}
    for i, v in enumerate(uniq):
        a, b = off[i], off[i + 1]
        inds = np.argsort(sc[a:b], kind='stable')[::-1][:num_pred]
        out[v] = {'label': lab[a:b][inds], 'score': sc[a:b][inds], 'segment': seg[a:b][inds]}
    return out


def _score_table(cls_scores, uniq):
    """dense fp64 [n_vid, n_cls] table of the videos, in their order; KeyError for a video without scores"""
    rows = [np.asarray(cls_scores[v], dtype=np.float64).reshape(-1) for v in uniq]
    if rows and any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("external class-score vectors differ in length")
    return np.stack(rows) if rows else np.zeros((0, 1), dtype=np.float64)


def fuse_external_scores(results, cls_scores, num_pred=200, topk=2):
    """The fused rows on the device.  results: the evaluator's result columns (dict, as `collect_results` returns them;
    columns may be numpy arrays or tensors on any device); cls_scores: {video id: class-score vector}.
    Returns a dict: 'video-id' = the distinct video ids, sorted (ONE entry per video); 'offsets' = int32 [n_vid + 1], video v
    owns fused rows offsets[v] .. offsets[v + 1]; 'video-index' (int32), 'label' (int32), 't-start', 't-end', 'score'
    (float64) = the fused columns as device tensors.  `ANETdetection.evaluate` takes this dict as it is."""
    lib = _lib.load()
    uniq, vidx, perm = _by_video(results)
    table = _score_table(cls_scores, uniq)              # before any device work: a missing video raises KeyError here
    n, n_vid, n_cls = len(vidx), len(uniq), table.shape[1]
    num_pred, topk = int(num_pred), int(topk)
    cnt = np.bincount(vidx, minlength=n_vid).astype(np.int64)
    pred_off = np.r_[0, np.cumsum(cnt)].astype(np.int32)
    out_off = np.r_[0, np.cumsum(topk * np.minimum(cnt, num_pred))].astype(np.int32)
    n_out = int(out_off[-1])
    perm_d = torch.as_tensor(perm, device='cuda')
    cols = [torch.as_tensor(results[k]).detach().reshape(-1).to(device='cuda', dtype=torch.float64)[perm_d].contiguous()
            for k in ('score', 't-start', 't-end')]
    cols = [c if c.numel() else torch.zeros(1, dtype=torch.float64, device='cuda') for c in cols]
    table_d = torch.as_tensor(table).cuda() if table.size else torch.zeros(1, dtype=torch.float64, device='cuda')
    out = {'video-index': torch.empty(max(n_out, 1), dtype=torch.int32, device='cuda'),
           'label': torch.empty(max(n_out, 1), dtype=torch.int32, device='cuda')}
    for k in ('t-start', 't-end', 'score'):
        out[k] = torch.empty(max(n_out, 1), dtype=torch.float64, device='cuda')
    if n_vid == 0:
        return dict({k: v[:0] for k, v in out.items()}, **{'video-id': uniq, 'offsets': out_off})
    nws = lib.vilco_score_fuse_workspace(n, n_vid)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device='cuda')
    i32p = C.POINTER(C.c_int32)
    _lib.check(lib.vilco_score_fuse(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                                    pred_off.ctypes.data_as(i32p), n, n_vid, table_d.data_ptr(), n_cls, num_pred, topk,
                                    out_off.ctypes.data_as(i32p), n_out, out['video-index'].data_ptr(),
                                    out['label'].data_ptr(), out['t-start'].data_ptr(), out['t-end'].data_ptr(),
                                    out['score'].data_ptr(), ws.data_ptr(), nws,
                                    torch.cuda.current_stream().cuda_stream))
    fused = {k: v[:n_out] for k, v in out.items()}
    fused['video-id'] = uniq
    fused['offsets'] = out_off
    return fused


def fused_to_host(fused):
    """the device dict of `fuse_external_scores` as the reference's host columns (one video id per row, int64 labels)"""
    cnt = np.diff(fused['offsets'])
    vids = [v for v, c in zip(fused['video-id'], cnt) for _ in range(int(c))]
    return {'video-id': vids, 't-start': fused['t-start'].cpu().numpy(), 't-end': fused['t-end'].cpu().numpy(),
            'label': fused['label'].cpu().numpy().astype(np.int64), 'score': fused['score'].cpu().numpy()}


def postprocess_results(results, cls_score_file, num_pred=200, topk=2):
    """The reference's entry point: results (a result dict or the path of a pickled one) re-scored with the external
    class scores of cls_score_file (JSON or pickle).  Returns {'video-id': list, 't-start', 't-end', 'label', 'score':
    numpy columns}.  A video without external scores raises KeyError."""
    if isinstance(results, str):
        results = load_results_from_pkl(results)
    return fused_to_host(fuse_external_scores(results, load_cls_scores(cls_score_file), num_pred=num_pred, topk=topk))
