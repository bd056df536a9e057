"""Pooled Outputs Distillation (Douillard, Cord, Ollion, Robert, Valle: "PODNet: Pooled Outputs Distillation for Small-Tasks
Incremental Learning", ECCV 2020) on the pyramid between the neck and the heads -- feature-level distillation, which the
reference does not have.

The pyramid is one-dimensional, [B, T_l, C] per level, so POD's two spatial poolings of the squared features are a sum over
time (p, C entries) and a sum over channels (q, one entry per valid position).  Their concatenation is L2-normalised and
compared, by Euclidean distance, with what the model that ENTERS the task produced for the same clip:

    pod_loss = scale / (L N_rec) * sum_b sum_l || normalize([p ; q]) - record_bl ||,   scale = pod_lambda sqrt(n_classes / n_new)

(PODNet's adaptive factor, computed on the host once per task; `pod_lambda`, cl_cfg, default 1.0, is not tuned here.)  The
records are written at the START of every task with known classes: one eval-mode, no-grad pass of the incoming model over
every clip the task's loader yields (`record_clips` -- the method's cost: one inference pass over the task's clips per task).
A record is sum_l (C + T_l) floats, far smaller than a DER record.  On the device the term is ONE op over the level list
(`ops.pod_distill`, csrc/pod.hip: three launches forward, one backward, the record addresses read from a device table), so a
captured step replays it and follows whatever table the next batch brings.  A batch row has no record -- address 0 -- when its
clip is not in the bank or its length or level layout in this step differs from the recorded one (counted in
`PODBank.skipped`).  PODNet's cosine classifier and its flat-embedding term are not part of this."""
import math

import torch

from . import hooks      # (which imports this module: both use the other's names in calls only)
from .der import clip_key, clip_len, labelled


class PODBank:
    """{video_id: record} with the table a step needs.  The buffers are never moved or rewritten while their clip is in the
    bank: a captured step reads their addresses from the table of the batch, which is built from the bank alone."""

    def __init__(self):
        self.records = {}          # video_id -> (buffer [sum (C + T_l)], clip length, (T_l, ...), C)
        self.skipped = 0           # rows that had a record the step could not use (length / layout mismatch)

    def __len__(self):
        return len(self.records)

    def __contains__(self, video_id):
        return video_id in self.records

    def get(self, video_id):
        return self.records.get(video_id)

    def clear(self):
        self.records = {}

    def record(self, video_id, vector, length, level_lens, C):
        """vector: the clip's normalised record [sum (C + T_l)] (a row of ops.pod_record).  It is copied into a buffer of
        its own; a later record of the same clip replaces the earlier one."""
        level_lens = tuple(int(t) for t in level_lens)
        buf = vector.detach().to(torch.float32).reshape(-1).contiguous().clone()
        if buf.numel() != sum(int(C) + t for t in level_lens):
            raise ValueError("PODBank.record: %d floats do not hold the levels %s at C = %d" % (buf.numel(), level_lens, C))
        self.records[video_id] = (buf, int(length), level_lens, int(C))

    def rows_for(self, video_list, lens, level_T=None, C=None):
        """the record address (or 0) per clip, on the host; bumps `skipped` for records of another length / layout / width"""
        rows = []
        for v, n in zip(video_list, lens):
            rec = self.records.get(clip_key(v))
            if rec is None:
                rows.append(0)
            elif (rec[1] != int(n) or (level_T is not None and rec[2] != tuple(int(t) for t in level_T))
                  or (C is not None and rec[3] != int(C))):
                self.skipped += 1
                rows.append(0)
            else:
                rows.append(rec[0].data_ptr())
        return rows

    def table_for(self, video_list, lens, device=None, level_T=None, C=None):
        """the step's `pod_tab`: int64 [B] on `device` (default: where the records live) -- staged in pinned memory and
        uploaded without blocking, like the other small input tables"""
        host = torch.tensor(self.rows_for(video_list, lens, level_T, C), dtype=torch.int64).reshape(len(video_list))
        if device is None:
            device = next((r[0].device for r in self.records.values()), torch.device('cpu'))
        device = torch.device(device)
        if device.type != 'cuda':
            return host.to(device)
        return host.pin_memory().to(device, non_blocking=True)


def empty_table(batch, device):
    """a `pod_tab` that names no record"""
    return torch.zeros(int(batch), dtype=torch.int64, device=device)


def adaptive_scale(pod_lambda, n_classes, n_known):
    """PODNet's factor: pod_lambda * sqrt(n_classes / (n_classes - n_known)), on the host"""
    n_new = int(n_classes) - int(n_known)
    if n_new < 1:
        raise ValueError("cl_name 'pod': the head holds %d classes, %d of them known: no new class" % (n_classes, n_known))
    return float(pod_lambda) * math.sqrt(int(n_classes) / n_new)


def step_table(model, video_list, level_T=None):
    """`pod_tab` of a training step of `model` over `video_list`: all zeros while there is nothing to distil from (no bank,
    no known classes), the bank's table otherwise"""
    vids = labelled(video_list)
    bank = getattr(model, 'pod_bank', None)
    if bank is None or model.n_known == 0 or not len(bank):
        return empty_table(len(vids), model.device)
    if level_T is None:
        level_T = model._der_levels()      # before the forward (a step prepared for replay): the layout of every training step
    return bank.table_for(vids, [clip_len(v) for v in vids], device=model.device, level_T=level_T)


def pooled_records(feats, level_len):
    """ops.pod_record in tensor ops (a CPU model): feats = list of [B, T_l, C], level_len [B, L] -> [B, sum (C + T_l)]"""
    out = []
    for l, h in enumerate(feats):
        T = h.shape[1]
        V = level_len[:, l].to(h.device).clamp(0, T)
        keep = (torch.arange(T, device=h.device)[None, :] < V[:, None]).to(h.dtype)
        s = h * h * keep[:, :, None]
        v = torch.cat([s.sum(1), s.sum(2)], dim=1)
        out.append(v / v.norm(dim=1, keepdim=True).clamp_min(1e-12))
    return torch.cat(out, dim=1)


@torch.no_grad()
def record_clips(model, bank, loader_or_videos, task_id):
    """Every labelled clip of `loader_or_videos` (a loader that yields clip lists, or a list of clips) goes through an
    eval-mode, no-grad forward of `model` -- the incoming model of the task -- padded as a training step pads it, and its
    pooled, normalised pyramid is recorded (ops.pod_record on the device).  -> number of records written.  The model's
    train / eval state is restored."""
    from .. import ops
    batches = loader_or_videos
    if isinstance(batches, (list, tuple)) and batches and isinstance(batches[0], dict):
        batches = [[v] for v in batches]
    was_training = model.training
    model.eval()
    n = 0
    try:
        for video_list in batches:
            vids = labelled(video_list)
            if not vids:
                continue
            model._pod_step = None
            model(vids, task_id=task_id, get_emb=True)
            (feats, level_len), model._pod_step = model._pod_step, None
            feats = [f.detach() for f in feats]
            rec = ops.pod_record(feats, level_len) if feats[0].is_cuda else pooled_records(feats, level_len)
            level_T, C = [int(f.shape[1]) for f in feats], int(feats[0].shape[2])
            for b, v in enumerate(vids):
                bank.record(clip_key(v), rec[b], clip_len(v), level_T, C)
                n += 1
    finally:
        model._pod_step = None
        model.train(was_training)
    return n


def pod_term(feats, valid_lens, records, scale):
    """The term in tensor ops, for a CPU model and as the A/B reference of ops.pod_distill.  feats: list of [B, T_l, C];
    valid_lens [B, L]; records: per batch row None or the record [sum (C + T_l)].  -> (loss, N_rec): the loss in the
    features' dtype (autograd gives the gradient), N_rec a Python int; an exact zero when no row has a record."""
    valid = valid_lens.tolist() if torch.is_tensor(valid_lens) else valid_lens
    L, C = len(feats), int(feats[0].shape[2])
    n_rec = sum(1 for r in records if r is not None)
    if n_rec == 0:
        return sum(f.sum() for f in feats) * 0.0, 0
    total = feats[0].new_zeros(())
    for b, rec in enumerate(records):
        if rec is None:
            continue
        off = 0
        for l, f in enumerate(feats):
            T = int(f.shape[1])
            V = max(0, min(int(valid[b][l]), T))
            if V:
                s = f[b, :V] * f[b, :V]
                v = torch.cat([s.sum(0), s.sum(1)])
                u = v / v.norm().clamp_min(1e-12)
                e = u - rec[off:off + C + V].to(f.dtype)
                d2 = (e * e).sum()
                # ||e|| with the gradient e / max(||e||, 1e-12): an exact zero, not NaN, at e = 0
                total = total + _Norm.apply(e, d2)
            off += C + T
    return total * (float(scale) / (L * n_rec)), n_rec


class _Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, d2):
        d = d2.sqrt()
        ctx.save_for_backward(e, d)
        return d

    @staticmethod
    def backward(ctx, g):
        e, d = ctx.saved_tensors
        return g * e / d.clamp_min(1e-12), None


def check_supported(cl_name, reducer=None, driver='run_episodes', type_sampling=None, start_epoch=0):
    """the combinations this implementation refuses, by name: the BiC / NLQ drivers and data parallelism (hooks.SUPPORT_MORE), iCaRL's
    target cache, and a resume inside a task (the incoming model the records come from is gone once a task is under way)"""
    if cl_name != 'pod':
        return False
    drivers, takes_reducer = hooks.support('pod')
    if driver not in drivers:
        raise ValueError("cl_cfg.name 'pod' is not supported by %s: only run_episodes records the incoming model's pyramid"
                         % driver)
    if reducer is not None and not takes_reducer:
        raise ValueError("cl_cfg.name 'pod' does not support data parallelism (reducer is not None): the records live on one "
                         "rank's device and no multi-GPU node has run it")
    if type_sampling == 'icarl':
        raise ValueError("cl_cfg.name 'pod' with type_sampling 'icarl': that setting caches iCaRL's distillation targets for "
                         "every step; choose 'random' or 'herding' for the memory")
    if start_epoch > 0:
        raise ValueError("cl_cfg.name 'pod' cannot resume inside a task (start_epoch = %d): the records come from the model "
                         "that entered the task, which is gone once the task is under way; resume at a task boundary"
                         % start_epoch)
    return True
