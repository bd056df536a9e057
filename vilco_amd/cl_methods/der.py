"""Dark Experience Replay (Buzzega, Boschini, Porrello, Abati, Calderara: "Dark Experience for General Continual Learning",
NeurIPS 2020) on the replay memory the episode loop already keeps -- logit replay, which the reference does not have.

When a clip enters the memory, the classification logits the model gives it THEN are recorded (`record_memory`, at the task
boundary: after the memory was updated and the best checkpoint reloaded, before the head grows).  From the next task on,
every step adds  der_alpha * mean (x - z)^2  over the memory clips of its batch: x the head's logits now, z the record, over
the positions the loss kernels treat as valid and the classes the head had when the record was made.  On the device that is
ONE op over the concatenated head output (`ops.der_replay`, csrc/der.hip: two launches forward, one backward, the record
addresses read from a device table), so a captured step replays it and follows whatever table the next batch brings.

DER and DER++.  The DER++ label term is the detection loss on the memory clips themselves, which the task loader already
mixes into the batches of a stream built with train_enable=True: that configuration IS DER++.  With train_enable=False no
memory clip reaches a batch, no row has a record and the term is an exact zero.  `der_alpha` (cl_cfg, default 0.1) is a
hyper-parameter; it is not tuned here.

A record is [sum T_l, n] fp32 on the device, the pyramid levels end to end, n the head's width at insertion time; with it the
clip's length and level lengths.  A clip recorded earlier keeps its record (insertion-time logits are the method), a clip
dropped from the memory loses it.  A batch row has no record -- address 0 in the table -- when its clip is not in the bank
or its length in this step differs from the recorded one (a re-cropped long clip: counted in `DERBank.skipped`)."""
import torch

from . import hooks      # (which imports this module: both use the other's names in calls only)


def clip_key(video):
    return video['video_id']


def clip_len(video):
    return int(video['feats'].shape[-1])


class DERBank:
    """{video_id: record} with the table a step needs.  The buffers are never moved or rewritten while their clip is in the
    bank: a captured step reads their addresses from the table of the batch, which is built from the bank alone."""

    def __init__(self):
        self.records = {}          # video_id -> (buffer [sum T_l, n], clip length, (T_l, ...))
        self.skipped = 0           # rows that had a record the step could not use (length mismatch)

    def __len__(self):
        return len(self.records)

    def __contains__(self, video_id):
        return video_id in self.records

    def get(self, video_id):
        return self.records.get(video_id)

    def record(self, video_id, logits, length, level_lens):
        """logits: [sum T_l, n] or the per-level list of [T_l, n].  A clip that already has a record keeps it -> False."""
        if video_id in self.records:
            return False
        if not torch.is_tensor(logits):
            logits = torch.cat([t.reshape(t.shape[0], -1) for t in logits], dim=0)
        level_lens = tuple(int(t) for t in level_lens)
        buf = logits.detach().to(torch.float32).contiguous().clone()
        if buf.dim() != 2 or buf.shape[0] != sum(level_lens) or buf.shape[1] < 1:
            raise ValueError("DERBank.record: logits %s do not hold the %d rows of the levels %s"
                             % (tuple(buf.shape), sum(level_lens), level_lens))
        self.records[video_id] = (buf, int(length), level_lens)
        return True

    def drop_missing(self, memory):
        """forget the records of clips that are no longer in `memory` ({class: [videos]}) -> number dropped"""
        alive = {clip_key(v) for videos in memory.values() for v in videos}
        gone = [k for k in self.records if k not in alive]
        for k in gone:
            del self.records[k]
        return len(gone)

    def rows_for(self, video_list, lens, level_T=None):
        """[(address or 0, n)] per clip, on the host; bumps `skipped` for records of another length / level layout"""
        rows = []
        for v, n in zip(video_list, lens):
            rec = self.records.get(clip_key(v))
            if rec is None:
                rows.append((0, 0))
            elif rec[1] != int(n) or (level_T is not None and rec[2] != tuple(int(t) for t in level_T)):
                self.skipped += 1
                rows.append((0, 0))
            else:
                rows.append((rec[0].data_ptr(), int(rec[0].shape[1])))
        return rows

    def table_for(self, video_list, lens, device=None, level_T=None):
        """the step's `der_tab`: int64 [B, 2] on `device` (default: where the records live) -- staged in pinned memory and
        uploaded without blocking, like the other small input tables"""
        host = torch.tensor(self.rows_for(video_list, lens, level_T), dtype=torch.int64).reshape(len(video_list), 2)
        if device is None:
            device = next((r[0].device for r in self.records.values()), torch.device('cpu'))
        device = torch.device(device)
        if device.type != 'cuda':
            return host.to(device)
        return host.pin_memory().to(device, non_blocking=True)

    def state_dict(self):
        return {'records': {k: {'logits': buf.detach().cpu().clone(), 'length': n, 'level_lens': tuple(lv)}
                            for k, (buf, n, lv) in self.records.items()},
                'skipped': int(self.skipped)}

    def load_state_dict(self, state, device=None):
        self.records = {}
        for k, r in state['records'].items():
            buf = r['logits'].to(dtype=torch.float32)
            buf = (buf.to(device) if device is not None else buf.clone()).contiguous()
            self.records[k] = (buf, int(r['length']), tuple(int(t) for t in r['level_lens']))
        self.skipped = int(state.get('skipped', 0))
        return self


def empty_table(batch, device):
    """a `der_tab` that names no record"""
    return torch.zeros(int(batch), 2, dtype=torch.int64, device=device)


def labelled(video_list):
    """the clips of a batch that become its rows (PtTransformer._batch_cf drops unlabelled clips)"""
    return [v for v in video_list if len(v['labels']) > 0]


def step_table(model, video_list, level_T=None):
    """`der_tab` of a training step of `model` over `video_list`: all zeros while there is nothing to replay (no bank, no
    known classes), the bank's table otherwise"""
    vids = labelled(video_list)
    bank = getattr(model, 'der_bank', None)
    if bank is None or model.n_known == 0 or not len(bank):
        return empty_table(len(vids), model.device)
    if level_T is None and hasattr(model, '_der_levels'):
        level_T = model._der_levels()      # before the forward (a step prepared for replay): the layout of every training step
    return bank.table_for(vids, [clip_len(v) for v in vids], device=model.device, level_T=level_T)


@torch.no_grad()
def record_memory(model, bank, memory, task_id, batch_size=1):
    """Every clip of `memory` ({class: [videos]}) that has no record yet goes through an eval-mode forward of `model` (the
    route train_cl.cache_prev_logits takes: padded to max_seq_len, get_emb=True) and its raw classification logits are
    recorded at the head's present width.  -> number of new records.  The model's train / eval state is restored."""
    from ..utils.cl_stream import InMemoryQILStream
    todo = [v for v in InMemoryQILStream.flatten(memory) if clip_key(v) not in bank and len(v['labels']) > 0]
    was_training = model.training
    model.eval()
    try:
        for i in range(0, len(todo), max(int(batch_size), 1)):
            video_list = todo[i:i + max(int(batch_size), 1)]
            cls_logits, _, _ = model(video_list, task_id=task_id, get_emb=True)
            level_lens = [int(lvl.shape[1]) for lvl in cls_logits]
            for b, v in enumerate(video_list):
                bank.record(clip_key(v), [lvl[b] for lvl in cls_logits], clip_len(v), level_lens)
    finally:
        model.train(was_training)
    return len(todo)


def der_term(logits, level_row, level_T, valid_lens, records, alpha):
    """The term in tensor ops, for a CPU model and as the A/B reference of ops.der_replay.  logits [B, R, C]; valid_lens
    [B, L]; records: per batch row None or the record [sum T_l, n_b].  -> (loss, N): alpha * S / N in the logits' dtype
    (autograd gives the gradient), N a Python int; an exact zero when nothing is compared."""
    S, N = logits.new_zeros(()), 0
    valid = valid_lens.tolist() if torch.is_tensor(valid_lens) else valid_lens
    for b, z in enumerate(records):
        if z is None:
            continue
        n_b = int(z.shape[1])
        if not 1 <= n_b <= logits.shape[2]:
            continue
        off = 0
        for l, (row, T) in enumerate(zip(level_row, level_T)):
            V = max(0, min(int(valid[b][l]), int(T)))
            if V:
                d = logits[b, int(row):int(row) + V, :n_b] - z[off:off + V].to(logits.dtype)
                S = S + (d * d).sum()
                N += n_b * V
            off += int(T)
    if N == 0:
        return logits.sum() * 0.0, 0
    return S * (float(alpha) / N), N


def check_supported(cl_name, reducer=None, driver='run_episodes', type_sampling=None):
    """the combinations this implementation refuses, by name: the BiC / NLQ drivers and data parallelism (hooks.SUPPORT), and iCaRL's target
    cache (type_sampling 'icarl' hands every step the previous model's outputs, which a 'der' step has no term for)"""
    if cl_name != 'der':
        return False
    drivers, takes_reducer = hooks.SUPPORT['der']
    if driver not in drivers:
        raise ValueError("cl_cfg.name 'der' is not supported by %s: only run_episodes records the memory's logits" % driver)
    if reducer is not None and not takes_reducer:
        raise ValueError("cl_cfg.name 'der' does not support data parallelism (reducer is not None): the records live on one "
                         "rank's device and no multi-GPU node has run it")
    if type_sampling == 'icarl':
        raise ValueError("cl_cfg.name 'der' with type_sampling 'icarl': that setting caches iCaRL's distillation targets for "
                         "every step; choose 'random' or 'herding' for the memory")
    return True
