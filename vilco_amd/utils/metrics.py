"""MQ evaluation on the device: the reference's `ANETdetection` (MQ/libs/utils/metrics.py:152-272) and
`evaluation_retrieval` (MQ/libs/utils/get_retrieval_performance.py:7-195) with their signatures, scored by the HIP kernels of
csrc/evaluate.hip (`vilco_det_ap`, `vilco_retrieval_hits`).  Ground truth is parsed once on the host and kept on the device
per task; per call the host only maps video ids / labels to indices and packs the columns (vectorised), the matching and the
AP / recall arithmetic run on the GPU.  No CPU fallback, as in `ops`.

Reference behaviour kept on purpose: the label remap is pandas' simultaneous dict map (a label
missing from the ground truth stays raw and is scored as whichever class index it equals); with use_cl the reference's
`replace(list_of_dicts)` changes nothing, so labels are taken as class indices as they are; a 0/0 tIoU is NaN, which the
detection match treats as the best overlap and the retrieval metric as no overlap.  Ties: the later row ranks first
(DESIGN.md section 7).
"""
import ctypes as C
import json
import os
import pickle as pkl
import time

import numpy as np
import torch

from .. import _lib

RETRIEVAL_TIOUS = (0.1, 0.2, 0.3, 0.4, 0.5)       # get_retrieval_performance.py:117-118 (fixed there)
RETRIEVAL_RANKS = (1, 5)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _nonempty(t):
    """kernels take a valid pointer even for zero rows"""
    return t if t.numel() > 0 else torch.zeros(1, dtype=t.dtype, device=t.device)


# ------------------------------------------------------------------------------------------------------------------ loaders
def remove_duplicate_annotations(ants, tol=1e-3):
    """metrics.py:14-30: drop events with the same label and start / end within tol of an earlier kept one"""
    valid_events = []
    for event in ants:
        s, e, lab = event['segment'][0], event['segment'][1], event['label_id']
        if not any(abs(s - p['segment'][0]) <= tol and abs(e - p['segment'][1]) <= tol and lab == p['label_id']
                   for p in valid_events):
            valid_events.append(event)
    return valid_events


def _label_id(event, label, label_offset):
    if isinstance(event[label], (tuple, list)):
        label_id = 0
        for i, x in enumerate(event[label][::-1]):
            label_id += label_offset ** i + int(x)
        return label_id
    return int(event[label])


def _remap(labels, index):
    """pandas' Series.replace(dict): a simultaneous map, keys not in the dict stay as they are"""
    labels = np.asarray(labels, dtype=np.int64)
    if labels.size == 0 or not index:
        return labels.copy()
    keys = np.array(sorted(index), dtype=np.int64)
    vals = np.array([index[k] for k in keys], dtype=np.int64)
    pos = np.clip(np.searchsorted(keys, labels), 0, len(keys) - 1)
    hit = keys[pos] == labels
    return np.where(hit, vals[pos], labels)


def _gt_table(vids, starts, stops, labels):
    activity_index = {j: i for i, j in enumerate(sorted(set(int(x) for x in labels)))}
    return ({'video-id': list(vids), 't-start': np.asarray(starts, dtype=np.float64).reshape(-1),
             't-end': np.asarray(stops, dtype=np.float64).reshape(-1), 'label': _remap(labels, activity_index)},
            activity_index)


def load_gt_seg_from_json(json_file, split=None, label='label_id', label_offset=0, debug_video_id=None, use_cl=False):
    """metrics.py:33-107.  Returns (ground_truth, activity_index) as the reference does, the ground truth as a dict of columns
    {'video-id': list, 't-start', 't-end': float64 arrays, 'label': int64 array (remapped)} in the reference's row order;
    with use_cl, lists of both, one per task of the pickle's 'val' entry.  Like the reference, the CL columns accumulate over
    the tasks (task i holds the rows of tasks 0..i)."""
    if use_cl:
        with open(json_file, 'rb') as f:
            data = pkl.load(f)['val']
        ground_truth, activity_index = [], []
        vids, starts, stops, labels = [], [], [], []
        for sub in data:
            for video in sub['dict_db']:
                for idx, lab in enumerate(video['labels']):
                    vids.append(video['id'])
                    starts.append(float(video['segments'][idx][0]))
                    stops.append(float(video['segments'][idx][1]))
                    labels.append(lab)
            gt, ai = _gt_table(vids, starts, stops, labels)
            ground_truth.append(gt)
            activity_index.append(ai)
        return ground_truth, activity_index
    with open(json_file, 'r', encoding='utf8') as f:
        json_db = json.load(f)
    if 'database' in json_db.keys():
        json_db = json_db['database']
    vids, starts, stops, labels = [], [], [], []
    for k, v in json_db.items():
        if debug_video_id is not None and v['clip_id'] != debug_video_id[-1]:
            continue
        if (split is not None) and v['subset'].lower() != split:
            continue
        ants = remove_duplicate_annotations(v['annotations'])
        for event in ants:
            starts.append(float(event['segment'][0]))
            stops.append(float(event['segment'][1]))
            labels.append(_label_id(event, label, label_offset))
        vids += [k] * len(ants)
    return _gt_table(vids, starts, stops, labels)


def load_pred_seg_from_json(json_file, label='label_id', label_offset=0):
    """metrics.py:110-149, as a dict of columns {'video-id', 't-start', 't-end', 'label', 'score'}"""
    with open(json_file, 'r', encoding='utf8') as f:
        json_db = json.load(f)['database']
    vids, starts, stops, labels, scores = [], [], [], [], []
    for k, v in json_db.items():
        vids += [k] * len(v)
        for event in v:
            starts.append(float(event['segment'][0]))
            stops.append(float(event['segment'][1]))
            labels.append(_label_id(event, label, label_offset))
            scores.append(float(event['scores']))
    return {'video-id': vids, 't-start': np.asarray(starts, dtype=np.float64), 't-end': np.asarray(stops, dtype=np.float64),
            'label': np.asarray(labels, dtype=np.int64), 'score': np.asarray(scores, dtype=np.float64)}


def _column(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(dtype, copy=False).reshape(-1)


def _pred_columns(preds):
    """the three input forms of ANETdetection.evaluate -> (video ids, start, end, label, score) host columns"""
    if isinstance(preds, str) and os.path.isfile(preds):
        preds = load_pred_seg_from_json(preds)
    elif not isinstance(preds, dict):
        import pandas as pd   # only a DataFrame needs pandas
        if not isinstance(preds, pd.DataFrame):
            raise TypeError("preds must be a result dict, a prediction JSON path or a DataFrame")
        assert 'label' in preds
        preds = {k: preds[k].to_numpy() for k in ('video-id', 't-start', 't-end', 'label', 'score')}
    vids = preds['video-id']
    if isinstance(vids, torch.Tensor):
        vids = vids.cpu().numpy()
    return (np.asarray(vids, dtype=object).reshape(-1), _column(preds['t-start'], np.float64),
            _column(preds['t-end'], np.float64), _column(preds['label'], np.int64), _column(preds['score'], np.float64))


def _video_index(vids, index):
    """vectorised id -> index (-1: not in the ground truth); the dict lookup runs once per distinct id"""
    if len(vids) == 0:
        return np.zeros(0, dtype=np.int32)
    uniq, inv = np.unique(vids.astype(str), return_inverse=True)
    lut = np.array([index.get(u, -1) for u in uniq], dtype=np.int32)
    return lut[inv.reshape(-1)]


# ------------------------------------------------------------------------------------------------------------- detection AP
class _DetGT:
    """one task's ground truth on the device: rows grouped by (class, video), each group in the reference's row order"""

    def __init__(self, gt, activity_index):
        vids = np.asarray(gt['video-id'], dtype=object).astype(str)
        uniq = sorted(set(vids.tolist()))
        self.video_index = {v: i for i, v in enumerate(uniq)}
        vidx = np.array([self.video_index[v] for v in vids], dtype=np.int64)
        cls = np.asarray(gt['label'], dtype=np.int64)
        self.n_cls, self.n_vid, self.n_gt = len(activity_index), len(uniq), len(cls)
        order = np.lexsort((vidx, cls))                   # stable: (class, video), row order inside
        c, v = cls[order], vidx[order]
        if len(order):
            start = np.flatnonzero(np.r_[True, (c[1:] != c[:-1]) | (v[1:] != v[:-1])])
        else:
            start = np.zeros(0, dtype=np.int64)
        self.n_grp = len(start)
        self.npos = np.bincount(cls, minlength=self.n_cls)[:self.n_cls].astype(np.int32)
        self.gs = _nonempty(_dev(np.asarray(gt['t-start'], np.float64)[order], torch.float64))
        self.ge = _nonempty(_dev(np.asarray(gt['t-end'], np.float64)[order], torch.float64))
        self.grp_off = _dev(np.r_[start, len(order)], torch.int32)
        self.grp_cls = _nonempty(_dev(c[start], torch.int32))
        self.grp_vid = _nonempty(_dev(v[start], torch.int32))
        self.cls_npos = _nonempty(_dev(self.npos, torch.int32))


def _is_device_columns(preds):
    """the output of postprocessing.fuse_external_scores: fused rows that are already on the device"""
    return isinstance(preds, dict) and 'video-index' in preds and 'offsets' in preds


def _remap_device(labels, index):
    """`_remap` on a device column"""
    if labels.numel() == 0 or not index:
        return labels
    keys = torch.tensor(sorted(index), dtype=torch.int64, device=labels.device)
    vals = torch.tensor([index[int(k)] for k in sorted(index)], dtype=torch.int64, device=labels.device)
    lab = labels.to(torch.int64)
    pos = torch.searchsorted(keys, lab).clamp_(0, len(keys) - 1)
    return torch.where(keys[pos] == lab, vals[pos], lab).to(torch.int32)


def _dev_col(a, dtype):
    """a prediction column for vilco_det_ap: host arrays are uploaded, device tensors are passed as they are"""
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return _nonempty(a.to(dtype).contiguous())           # no copy when the dtype and layout already fit
    return _nonempty(_dev(a, dtype))


def det_ap_device(gt, vidx, cls, ts, te, score, tiou_thresholds, want_flags=False):
    """AP[n_thr, n_cls] (and the TP flags [n_thr, n_pred] in input order) of prediction columns against a _DetGT.  The
    columns are host arrays or device tensors; class indices outside [0, n_cls) are ignored by the kernel."""
    lib = _lib.load()
    thr = np.asarray(tiou_thresholds, dtype=np.float64).reshape(-1)
    n, n_thr = len(cls), len(thr)
    cols = [_dev_col(vidx, torch.int32), _dev_col(cls, torch.int32), _dev_col(ts, torch.float64),
            _dev_col(te, torch.float64), _dev_col(score, torch.float64)]
    ap = torch.empty((n_thr, max(gt.n_cls, 1)), dtype=torch.float64, device='cuda')
    flags = torch.empty((n_thr, max(n, 1)), dtype=torch.uint8, device='cuda') if want_flags else None
    nws = lib.vilco_det_ap_workspace(n, gt.n_gt, n_thr)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device='cuda')
    thr_c = (C.c_double * n_thr)(*thr.tolist())
    _lib.check(lib.vilco_det_ap(*[t.data_ptr() for t in cols], n, gt.gs.data_ptr(), gt.ge.data_ptr(), gt.grp_off.data_ptr(),
                                gt.grp_cls.data_ptr(), gt.grp_vid.data_ptr(), gt.n_grp, gt.n_gt, gt.cls_npos.data_ptr(),
                                gt.n_cls, gt.n_vid, thr_c, n_thr, ap.data_ptr(),
                                flags.data_ptr() if want_flags else None, ws.data_ptr(), nws, _stream()))
    ap_h = ap[:, :gt.n_cls].cpu().numpy()
    if want_flags:
        return ap_h, flags[:, :n].cpu().numpy().astype(bool)
    return ap_h


class ANETdetection(object):
    """metrics.py:152-272 on the device.  `num_workers` is accepted and ignored."""

    def __init__(self, ant_file, split=None, tiou_thresholds=np.linspace(0.1, 0.5, 5), label='label_id', label_offset=0,
                 num_workers=8, dataset_name=None, debug_video_id=None, use_cl=False):
        self.tiou_thresholds = tiou_thresholds
        self.ap = None
        self.num_workers = num_workers
        self.use_cl = use_cl
        self.dataset_name = dataset_name if dataset_name is not None else os.path.basename(ant_file).replace('.json', '')
        self.split = split
        self.ground_truth, self.activity_index = load_gt_seg_from_json(
            ant_file, split=self.split, label=label, label_offset=label_offset, debug_video_id=debug_video_id,
            use_cl=self.use_cl)
        self._dev_gt = {}
        self.last_times = {}      # seconds of the last evaluate(): 'host' (column preparation), 'device' (kernels + copy)

    def _task(self, current_task_id):
        key = current_task_id if self.use_cl else None
        if key not in self._dev_gt:
            gt = self.ground_truth[key] if self.use_cl else self.ground_truth
            ai = self.activity_index[key] if self.use_cl else self.activity_index
            self._dev_gt[key] = _DetGT(gt, ai)
        return self._dev_gt[key]

    def prepare(self, preds, current_task_id=None):
        """host part of evaluate(): the packed prediction columns (video index, class index, start, end, score); device
        tensors when preds is the output of postprocessing.fuse_external_scores"""
        gt = self._task(current_task_id)
        if _is_device_columns(preds):
            # fused rows stay where they are: the video id -> GT index lookup runs once per video on the host and is
            # expanded by the video-index column; labels are range-checked by the kernel
            lut = _dev(_video_index(np.asarray(preds['video-id'], dtype=object), gt.video_index), torch.int32)
            vidx = lut[preds['video-index'].long()] if len(preds['video-id']) else preds['video-index']
            cls = preds['label'] if self.use_cl else _remap_device(preds['label'], self.activity_index)
            return gt, (vidx, cls, preds['t-start'], preds['t-end'], preds['score'])
        vids, ts, te, labels, score = _pred_columns(preds)
        # with use_cl the reference's preds['label'].replace(list_of_dicts) is a no-op: labels are class indices as given
        cls = labels if self.use_cl else _remap(labels, self.activity_index)
        cls = np.where((cls >= 0) & (cls < gt.n_cls), cls, -1).astype(np.int32)
        return gt, (_video_index(vids, gt.video_index), cls, ts, te, score)

    def evaluate(self, preds, current_task_id=None, verbose=True):
        """(mAP[n_thr], average_mAP, tiou_thresholds) as metrics.py:222-271"""
        self.ap = None
        t0 = time.perf_counter()
        gt, cols = self.prepare(preds, current_task_id)
        t1 = time.perf_counter()
        self.ap = det_ap_device(gt, *cols, self.tiou_thresholds)
        t2 = time.perf_counter()
        self.last_times = {'host': t1 - t0, 'device': t2 - t1}
        mAP = self.ap.mean(axis=1)
        average_mAP = mAP.mean()
        if verbose:
            print('[RESULTS] Action detection results on {:s}.'.format(self.dataset_name))
            block = ''
            for tiou, tiou_mAP in zip(self.tiou_thresholds, mAP):
                block += '\n|tIoU = {:.2f}: mAP = {:.2f} (%)'.format(tiou, tiou_mAP * 100)
            print(block)
            print('Avearge mAP: {:.2f} (%)'.format(average_mAP * 100))
        return mAP, average_mAP, self.tiou_thresholds


# ---------------------------------------------------------------------------------------------------------------- Recall@K
def _load_retrieval_gt(ground_truth_filename, subset, use_cl):
    """get_retrieval_performance.py:46-88: {video: {label name: [[s, e], ...]}} (a list of them, one per task, with use_cl)"""
    if use_cl:
        with open(ground_truth_filename, 'rb') as f:
            data = pkl.load(f)['val']
        out = []
        for sub in data:
            names = {v: k for k, v in sub['label_dict'].items()}
            task = {}
            for video in sub['dict_db']:
                ann = {}
                for idx, lab in enumerate(video['labels']):
                    ann.setdefault(names[lab], []).append([video['segments'][idx][0], video['segments'][idx][1]])
                task[video['id']] = ann
            out.append(task)
        return out
    with open(ground_truth_filename, 'r') as f:
        data = json.load(f)
    gt = {}
    for _, v in data.items():
        if not v['subset'] in subset:
            continue
        ann = {}
        for a in v['annotations']:
            ann.setdefault(a['label'], []).append([a['segment'][0], a['segment'][1]])
        gt[v['clip_id']] = ann
    return gt


def _load_retrieval_pred(prediction):
    if not isinstance(prediction, dict):
        with open(prediction, 'r') as f:
            prediction = json.load(f)
    if not all(k in prediction for k in Moment_Retrieval.PREDICTION_FIELDS):
        raise IOError('Please input a valid prediction file.')
    return prediction['results']


class Moment_Retrieval(object):
    """get_retrieval_performance.py:6-183 on the device.  prediction_filename may be the in-memory object of
    results_to_anet_json.  A ground-truth video without predictions raises KeyError (the reference stops in pdb)."""
    GROUND_TRUTH_FIELDS = ['database']
    PREDICTION_FIELDS = ['results', 'version', 'external_data']

    def __init__(self, ground_truth_filename=None, prediction_filename=None, ground_truth_fields=GROUND_TRUTH_FIELDS,
                 prediction_fields=PREDICTION_FIELDS, tiou_thresholds=np.linspace(0.5, 0.95, 10), subset='test',
                 verbose=False, check_status=False, use_cl=False, _ground_truth=None):
        if not ground_truth_filename and _ground_truth is None:
            raise IOError('Please input a valid ground truth file.')
        if prediction_filename is None or (isinstance(prediction_filename, str) and not prediction_filename):
            raise IOError('Please input a valid prediction file.')
        self.subset = subset
        self.tiou_thresholds = tiou_thresholds
        self.verbose = verbose
        self.use_cl = use_cl
        self.ground_truth = (_ground_truth if _ground_truth is not None
                             else _load_retrieval_gt(ground_truth_filename, subset, use_cl))
        self.prediction = _load_retrieval_pred(prediction_filename)
        if self.verbose:
            print('[INIT] Loaded annotations from {} subset.'.format(subset))
            nr_gt = sum(len(g) for g in self.ground_truth) if self.use_cl else len(self.ground_truth)
            print('\tNumber of ground truth instances: {}'.format(nr_gt))
            print('\tNumber of predictions: {}'.format(len(self.prediction)))
            print('\tFixed threshold for tiou score: {}'.format(self.tiou_thresholds))

    def pack(self, current_task_id=None):
        """host part: GT groups (video, label name) and their predictions in result order, as flat columns"""
        gt = self.ground_truth[current_task_id] if self.use_cl else self.ground_truth
        pred_rows = {}        # (video, label) -> row count; rows packed per group
        ps, pe, poff, pcnt, gs, ge, goff = [], [], [], [], [], [], [0]
        npred = 0
        for vid, ann in gt.items():
            if vid not in self.prediction:
                raise KeyError("no predictions for ground-truth video %r" % (vid,))
            rows = self.prediction[vid]
            by_label = pred_rows.get(vid)
            if by_label is None:
                by_label = {}
                for r in rows:
                    by_label.setdefault(r['label'], []).append(r['segment'])
                pred_rows[vid] = by_label
            for lab, segs in ann.items():
                p = by_label.get(lab, ())
                poff.append(npred)
                pcnt.append(len(p))
                for s in p:
                    ps.append(s[0]); pe.append(s[1])
                npred += len(p)
                for s in segs:
                    gs.append(s[0]); ge.append(s[1])
                goff.append(len(gs))
        return (np.asarray(ps, np.float64), np.asarray(pe, np.float64), np.asarray(poff, np.int32),
                np.asarray(pcnt, np.int32), np.asarray(gs, np.float64), np.asarray(ge, np.float64), np.asarray(goff, np.int32))

    def hits(self, current_task_id=None):
        """(hit counts [5 tIoU, 2 ranks], GT count)"""
        ps, pe, poff, pcnt, gs, ge, goff = self.pack(current_task_id)
        return retrieval_hits_device(ps, pe, poff, pcnt, gs, ge, goff, RETRIEVAL_TIOUS, RETRIEVAL_RANKS)

    def evaluate(self, current_task_id=None):
        hits, total = self.hits(current_task_id)
        if total == 0:
            return np.full(hits.shape, np.nan)
        return hits / float(total)


def retrieval_hits_device(ps, pe, poff, pcnt, gs, ge, goff, tious, ranks):
    lib = _lib.load()
    n_grp, n_thr, n_rank = len(poff), len(tious), len(ranks)
    t = [_nonempty(_dev(a, torch.float64)) for a in (ps, pe)]
    g = [_nonempty(_dev(a, torch.int32)) for a in (poff, pcnt)]
    gg = [_nonempty(_dev(a, torch.float64)) for a in (gs, ge)]
    off = _dev(goff, torch.int32)
    hits = torch.empty((n_thr, n_rank), dtype=torch.int64, device='cuda')
    total = torch.empty(1, dtype=torch.int64, device='cuda')
    nws = lib.vilco_retrieval_hits_workspace(n_grp, n_thr, n_rank)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device='cuda')
    thr_c = (C.c_double * n_thr)(*[float(x) for x in tious])
    rk_c = (C.c_int32 * n_rank)(*[int(x) for x in ranks])
    _lib.check(lib.vilco_retrieval_hits(t[0].data_ptr(), t[1].data_ptr(), g[0].data_ptr(), g[1].data_ptr(), gg[0].data_ptr(),
                                        gg[1].data_ptr(), off.data_ptr(), n_grp, thr_c, n_thr, rk_c, n_rank, hits.data_ptr(),
                                        total.data_ptr(), ws.data_ptr(), nws, _stream()))
    return hits.cpu().numpy(), int(total.item())


def evaluation_retrieval(gt, pred, subset, tiou, use_cl=False, current_task_id=None):
    """get_retrieval_performance.py:185-195: recall[5 tIoU, 2 ranks]; pred may be a file path or the JSON object"""
    mr = Moment_Retrieval(ground_truth_filename=gt, prediction_filename=pred, subset=subset, tiou_thresholds=tiou,
                          verbose=True, check_status=False, use_cl=use_cl)
    return mr.evaluate(current_task_id=current_task_id)


def make_mq_evaluators(ann_file, split='val', tiou_thresholds=(0.1, 0.2, 0.3, 0.4, 0.5), use_cl=True):
    """(evaluator, retrieval_eval) for valid_one_epoch_cl_single_gpu / final_validate; both parse ann_file once"""
    tious = np.asarray(tiou_thresholds, dtype=np.float64)
    evaluator = ANETdetection(ann_file, split, tiou_thresholds=tious, use_cl=use_cl)
    gt = _load_retrieval_gt(ann_file, split, use_cl)

    def retrieval_eval(json_obj, current_task_id=None):
        return Moment_Retrieval(prediction_filename=json_obj, subset=split, tiou_thresholds=tious, use_cl=use_cl,
                                _ground_truth=gt).evaluate(current_task_id=current_task_id)

    return evaluator, retrieval_eval
