"""Elastic Response Distillation (Feng, Wang, Yuan: "Overcoming Catastrophic Forgetting in Incremental Object Detection via
Elastic Response Distillation", CVPR 2022) for the one-stage, anchor-free temporal detector -- the one method here that holds
the REGRESSION head to what it knew.  The reference does not have it.

At the START of every task with known classes the incoming model answers on every clip the task's loader yields
(`record_clips`: one eval-mode, no-grad pass per task, where POD records).  Per clip, over the valid positions V of all levels:

    c_i = max_{y < n_old} z_iy,   mu = mean_V c,   sigma = the population standard deviation of c over V      (fp64)
    S_cls = {i in V : c_i > mu + erd_alpha_cls sigma}                                   (strict: sigma = 0 selects nothing)
    S_reg = {i in V : c_i > mu + erd_alpha_reg sigma  and  o^_i0 + o^_i1 > 0}

A record keeps only the selected rows in ascending position -- logits [K_c, n_old], finished offsets [K_r, 2] -- and one int32
map [sum T_l] from position to slot (-1: not selected) per set; the dense outputs are dropped.  Every step of the task adds

    erd_loss = erd_lambda_cls A / N_c + erd_lambda_reg D / N_r
    A = sum_b sum_{i in S_cls(b)} sum_{y < n_b} (x_iy - z_iy)^2,   N_c = sum_b |S_cls(b)| n_b
    D = sum_b sum_{i in S_reg(b)} diou(o_i, o^_i),                 N_r = sum_b |S_reg(b)|      (losses.ctr_diou_loss_1d)

over the batch rows with a usable record; a part whose count is 0 is an exact zero with an exactly zero gradient.  On the
device the selection is ops.erd_select and the term ONE op over the concatenated head output (ops.erd_distill, csrc/erd.hip:
two launches forward, one backward, everything per batch read through a device table), so a captured step replays it.

Departures from the paper, which is written for GFL: the classification part is the squared distance of the selected logits
(the paper's too) but the regression part is the library's DIoU between the student's and the teacher's offsets, not a KL
divergence between GFL's discretised box distributions, which this head does not predict; the selection statistic is the
maximum logit over the OLD classes; mu and sigma are taken per clip over the valid positions; the paper's NMS over the
regression set is left out.  erd_alpha_cls = erd_alpha_reg = 2 are the paper's values; erd_lambda_cls = erd_lambda_reg = 1
are NOT tuned here."""
import math

import torch

from . import hooks      # (which imports this module: both use the other's names in calls only)
from .der import clip_key, clip_len, labelled

TAB_COLS = 5             # map_cls, map_reg, val_cls, val_reg (addresses), n_b

OPTIONS = {'erd_alpha_cls': 2.0, 'erd_alpha_reg': 2.0, 'erd_lambda_cls': 1.0, 'erd_lambda_reg': 1.0}


def options(cl_cfg):
    """the four options of cl_cfg (read with .get) -> dict; a value that is not finite, or a negative lambda, raises"""
    out = {}
    for k, dflt in OPTIONS.items():
        raw = cl_cfg.get(k, dflt)
        try:
            v = float(raw)
        except (TypeError, ValueError):
            v = float('nan')
        if not math.isfinite(v):
            raise ValueError("cl_cfg.%s must be a finite number, got %r" % (k, raw))
        if 'lambda' in k and v < 0.0:
            raise ValueError("cl_cfg.%s must be a finite number >= 0, got %r" % (k, raw))
        out[k] = v
    return out


class Record:
    """what the bank keeps of one clip: the two maps, the selected rows, and what a usable record is matched by"""
    __slots__ = ("map_cls", "map_reg", "val_cls", "val_reg", "k_cls", "k_reg", "n_old", "length", "level_lens")

    def __init__(self, map_cls, map_reg, val_cls, val_reg, k_cls, k_reg, n_old, length, level_lens):
        self.map_cls, self.map_reg, self.val_cls, self.val_reg = map_cls, map_reg, val_cls, val_reg
        self.k_cls, self.k_reg, self.n_old, self.length, self.level_lens = int(k_cls), int(k_reg), int(n_old), int(length), level_lens

    def nbytes(self):
        """bytes of the record: two int32 maps and the selected rows (an empty set's unused row is not counted)"""
        return 8 * int(self.map_cls.numel()) + 4 * self.k_cls * self.n_old + 8 * self.k_reg

    def row(self):
        return (self.map_cls.data_ptr(), self.map_reg.data_ptr(), self.val_cls.data_ptr(), self.val_reg.data_ptr(), self.n_old)

    def buffers(self):
        return (self.map_cls, self.map_reg, self.val_cls, self.val_reg)


class ERDBank:
    """{video_id: Record} with the table a step needs.  The buffers are never moved or rewritten while their clip is in the
    bank: a captured step reads their addresses from the table of the batch, which is built from the bank alone.  `clear`
    only RETIRES the records: their buffers stay alive until `release`, which the hook calls once the new records -- and so
    every table built from then on -- are in place."""

    def __init__(self):
        self.records = {}
        self.retired = []          # record dictionaries cleared but not yet released
        self.skipped = 0           # rows that had a record the step could not use (length / layout mismatch)

    def __len__(self):
        return len(self.records)

    def __contains__(self, video_id):
        return video_id in self.records

    def get(self, video_id):
        return self.records.get(video_id)

    def clear(self):
        if self.records:
            self.retired.append(self.records)
        self.records = {}

    def release(self):
        """drop the buffers of the records cleared earlier -> how many records that were"""
        n = sum(len(r) for r in self.retired)
        self.retired = []
        return n

    def nbytes(self):
        return sum(r.nbytes() for r in self.records.values())

    def record(self, video_id, map_cls, map_reg, val_cls, val_reg, k_cls, k_reg, n_old, length, level_lens):
        """the buffers are taken as they are (ops.erd_select / select_rows made them for this record); a later record of the
        same clip replaces the earlier one"""
        level_lens = tuple(int(t) for t in level_lens)
        P = sum(level_lens)
        for m in (map_cls, map_reg):
            if m.dtype != torch.int32 or tuple(m.shape) != (P,) or not m.is_contiguous():
                raise ValueError("ERDBank.record: a map %s %s does not cover the %d positions of the levels %s"
                                 % (m.dtype, tuple(m.shape), P, level_lens))
        if (val_cls.dtype != torch.float32 or val_cls.dim() != 2 or val_cls.shape[0] < max(int(k_cls), 1)
                or val_cls.shape[1] != int(n_old) or not val_cls.is_contiguous()):
            raise ValueError("ERDBank.record: logits %s do not hold %d rows of %d classes" % (tuple(val_cls.shape), k_cls, n_old))
        if (val_reg.dtype != torch.float32 or val_reg.dim() != 2 or val_reg.shape[0] < max(int(k_reg), 1)
                or val_reg.shape[1] != 2 or not val_reg.is_contiguous()):
            raise ValueError("ERDBank.record: offsets %s do not hold %d rows of 2" % (tuple(val_reg.shape), k_reg))
        self.records[video_id] = Record(map_cls, map_reg, val_cls, val_reg, k_cls, k_reg, n_old, length, level_lens)

    def usable(self, video_list, lens, level_T=None):
        """per clip its Record or None; bumps `skipped` for records of another length / level layout (DER's rule)"""
        out = []
        for v, n in zip(video_list, lens):
            rec = self.records.get(clip_key(v))
            if rec is not None and (rec.length != int(n) or
                                    (level_T is not None and rec.level_lens != tuple(int(t) for t in level_T))):
                self.skipped += 1
                rec = None
            out.append(rec)
        return out

    def rows_for(self, video_list, lens, level_T=None):
        """[(four addresses, n_b) or zeros] per clip, on the host"""
        return [rec.row() if rec is not None else (0,) * TAB_COLS for rec in self.usable(video_list, lens, level_T)]

    def table_for(self, video_list, lens, device=None, level_T=None):
        """the step's `erd_tab`: int64 [B, 5] on `device` (default: where the records live) -- staged in pinned memory and
        uploaded without blocking, like the other small input tables"""
        host = torch.tensor(self.rows_for(video_list, lens, level_T), dtype=torch.int64).reshape(len(video_list), TAB_COLS)
        if device is None:
            device = next((r.map_cls.device for r in self.records.values()), torch.device('cpu'))
        device = torch.device(device)
        if device.type != 'cuda':
            return host.to(device)
        return host.pin_memory().to(device, non_blocking=True)


def empty_table(batch, device):
    """an `erd_tab` that names no record"""
    return torch.zeros(int(batch), TAB_COLS, dtype=torch.int64, device=device)


def step_table(model, video_list, level_T=None):
    """`erd_tab` of a training step of `model` over `video_list`: all zeros while there is nothing to distil from (no bank,
    no known classes), the bank's table otherwise"""
    vids = labelled(video_list)
    bank = getattr(model, 'erd_bank', None)
    if bank is None or model.n_known == 0 or not len(bank):
        return empty_table(len(vids), model.device)
    if level_T is None:
        level_T = model._der_levels()      # before the forward (a step prepared for replay): the layout of every training step
    return bank.table_for(vids, [clip_len(v) for v in vids], device=model.device, level_T=level_T)


def valid_mask(level_T, level_len_row, device=None):
    """bool [sum T_l]: the positions below their level's valid length (clamped to the level), levels end to end"""
    parts = []
    for T, V in zip(level_T, level_len_row):
        V = max(0, min(int(V), int(T)))
        parts.append(torch.arange(int(T), device=device) < V)
    return torch.cat(parts)


def select_rows(logits, offsets, level_T, level_len, n_old, alpha_cls, alpha_reg):
    """ops.erd_select in tensor ops (a CPU model): logits [B, P, C], offsets [B, P, 2], level_len [B, L] -> per clip
    (map_cls, map_reg, val_cls, val_reg, K_c, K_r) in ops.erd_select's layout; the statistics in fp64, the mean first"""
    valid = level_len.tolist() if torch.is_tensor(level_len) else level_len
    out = []
    for b in range(logits.shape[0]):
        V = valid_mask(level_T, valid[b], logits.device)
        c = logits[b, :, :int(n_old)].max(dim=1)[0].double()
        sel_c = torch.zeros_like(V)
        sel_r = torch.zeros_like(V)
        if bool(V.any()):
            cv = c[V]
            mu = cv.sum() / cv.numel()
            sigma = (((cv - mu) ** 2).sum() / cv.numel()).sqrt()
            sel_c = V & (c > mu + float(alpha_cls) * sigma)
            sel_r = V & (c > mu + float(alpha_reg) * sigma) & ((offsets[b, :, 0].double() + offsets[b, :, 1].double()) > 0)
        rec = []
        for sel in (sel_c, sel_r):
            m = torch.full((V.numel(),), -1, dtype=torch.int32, device=logits.device)
            m[sel] = torch.arange(int(sel.sum()), dtype=torch.int32, device=logits.device)
            rec.append(m)
        kc, kr = int(sel_c.sum()), int(sel_r.sum())
        vc = torch.zeros(max(kc, 1), int(n_old), dtype=torch.float32, device=logits.device)
        vr = torch.zeros(max(kr, 1), 2, dtype=torch.float32, device=logits.device)
        vc[:kc] = logits[b, sel_c, :int(n_old)].float()
        vr[:kr] = offsets[b, sel_r].float()
        out.append((rec[0], rec[1], vc, vr, kc, kr))
    return out


def record_bound(n_clips, level_T, n_old, alpha_cls, alpha_reg):
    """an upper bound of the bytes `n_clips` records take: at most 1 / (1 + alpha^2) of a clip's positions lie more than
    alpha > 0 standard deviations above its mean (Cantelli's inequality); any number of them otherwise"""
    P = sum(int(t) for t in level_T)

    def most(alpha):
        return P if alpha <= 0 else min(P, int(P / (1.0 + alpha * alpha)))
    return int(n_clips) * (8 * P + 4 * int(n_old) * most(alpha_cls) + 8 * most(alpha_reg))


def _count_clips(batches):
    """the clips a pass over `batches` will see, without making the pass -- or None when the loader does not say"""
    if isinstance(batches, (list, tuple)):
        return sum(len(labelled(b)) for b in batches)
    ds = getattr(batches, 'dataset', None)
    try:
        return len(ds) if ds is not None else None
    except TypeError:
        return None


def check_room(model, batches, opts):
    """raises before the recording pass starts when the records of the task cannot fit the device's free memory (the way
    herding does for its descriptors); a CPU model, or a loader that does not say how many clips it holds, is not checked"""
    dev = model.device
    n = _count_clips(batches)
    if dev.type != 'cuda' or not n:
        return
    need = record_bound(n, model._der_levels(), model.n_known, opts['erd_alpha_cls'], opts['erd_alpha_reg'])
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if need > free:
        raise RuntimeError("cl_cfg.name 'erd': the records of the task's %d clips may need %d bytes, %d bytes of device memory "
                           "are free" % (n, need, free))


@torch.no_grad()
def record_clips(model, bank, loader_or_videos, task_id, opts=None):
    """Every labelled clip of `loader_or_videos` (a loader that yields clip lists, or a list of clips) goes through an
    eval-mode, no-grad forward of `model` -- the incoming model of the task -- padded as a training step pads it; the
    confident positions are selected (ops.erd_select on the device) and the selected rows recorded.  -> (records written,
    their bytes).  The model's train / eval state is restored."""
    from .. import ops
    opts = opts or options({})
    n_old = int(model.n_known)
    batches = loader_or_videos
    if isinstance(batches, (list, tuple)) and batches and isinstance(batches[0], dict):
        batches = [[v] for v in batches]
    check_room(model, batches, opts)
    was_training = model.training
    model.eval()
    n = nbytes = 0
    try:
        for video_list in batches:
            vids = labelled(video_list)
            if not vids:
                continue
            cls_logits, offsets, masks = model(vids, task_id=task_id, get_emb=True)
            level_T = [int(x.shape[1]) for x in cls_logits]
            z = torch.cat([x.detach().float() for x in cls_logits], dim=1).contiguous()
            o = torch.cat([x.detach().float() for x in offsets], dim=1).contiguous()
            level_len = torch.stack([m.reshape(m.shape[0], -1).sum(1) for m in masks], dim=1).to(torch.int32).contiguous()
            select = ops.erd_select if z.is_cuda else select_rows
            recs = select(z, o, level_T, level_len, n_old, opts['erd_alpha_cls'], opts['erd_alpha_reg'])
            for v, r in zip(vids, recs):
                bank.record(clip_key(v), r[0], r[1], r[2], r[3], r[4], r[5], n_old, clip_len(v), level_T)
                nbytes += bank.get(clip_key(v)).nbytes()
                n += 1
    finally:
        model.train(was_training)
    return n, nbytes


def erd_term(logits, offsets, scale, level_row, level_T, valid_lens, records, lambda_cls, lambda_reg):
    """The term in tensor ops, for a CPU model and as the A/B reference of ops.erd_distill.  logits [B, R, C]; offsets
    [B, R, 2], finished -- or raw with scale [L]: o = relu(scale_l raw); valid_lens [B, L]; records: per batch row None or a
    Record.  -> (erd_loss, cls part, reg part, N_c, N_r): the losses in the logits' dtype (autograd gives the gradients), the
    counts Python ints; a part whose count is 0 is an exact zero with a zero gradient."""
    from ..modeling.losses import ctr_diou_loss_1d
    valid = valid_lens.tolist() if torch.is_tensor(valid_lens) else valid_lens
    dev = logits.device
    rows = torch.cat([int(r) + torch.arange(int(T), device=dev) for r, T in zip(level_row, level_T)])
    level_of = torch.cat([torch.full((int(T),), l, dtype=torch.long, device=dev) for l, T in enumerate(level_T)])
    A, D, Nc, Nr = logits.new_zeros(()), logits.new_zeros(()), 0, 0
    for b, rec in enumerate(records):
        if rec is None or not 1 <= rec.n_old <= logits.shape[2]:
            continue
        V = valid_mask(level_T, valid[b], dev)
        mc, mr = rec.map_cls.to(dev).long(), rec.map_reg.to(dev).long()
        sc, sr = V & (mc >= 0), V & (mr >= 0)
        if bool(sc.any()):
            d = logits[b, rows[sc], :rec.n_old] - rec.val_cls.to(dev)[mc[sc]].to(logits.dtype)
            A = A + (d * d).sum()
            Nc += int(sc.sum()) * rec.n_old
        if bool(sr.any()):
            o = offsets[b, rows[sr]]
            if scale is not None:
                o = torch.relu(o * scale[level_of[sr]][:, None])
            D = D + ctr_diou_loss_1d(o, rec.val_reg.to(dev)[mr[sr]].to(o.dtype), reduction='sum', check=False)
            Nr += int(sr.sum())
    zero = logits.sum() * 0.0 + offsets.sum() * 0.0
    cls = A * (float(lambda_cls) / Nc) if Nc else zero
    reg = D * (float(lambda_reg) / Nr) if Nr else zero
    return cls + reg, cls, reg, Nc, Nr


def check_supported(cl_name, reducer=None, driver='run_episodes', type_sampling=None, start_epoch=0):
    """the combinations this implementation refuses, by name: the BiC / NLQ drivers and data parallelism (hooks.SUPPORT_MORE),
    iCaRL's target cache, and a resume inside a task (the incoming model the records come from is gone once a task is under way)"""
    if cl_name != 'erd':
        return False
    drivers, takes_reducer = hooks.support('erd')
    if driver not in drivers:
        raise ValueError("cl_cfg.name 'erd' is not supported by %s: only run_episodes records the incoming model's responses"
                         % driver)
    if reducer is not None and not takes_reducer:
        raise ValueError("cl_cfg.name 'erd' does not support data parallelism (reducer is not None): the records live on one "
                         "rank's device and no multi-GPU node has run it")
    if type_sampling == 'icarl':
        raise ValueError("cl_cfg.name 'erd' with type_sampling 'icarl': that setting caches iCaRL's distillation targets for "
                         "every step; choose 'random' or 'herding' for the memory")
    if start_epoch > 0:
        raise ValueError("cl_cfg.name 'erd' cannot resume inside a task (start_epoch = %d): the records come from the model "
                         "that entered the task, which is gone once the task is under way; resume at a task boundary"
                         % start_epoch)
    return True
