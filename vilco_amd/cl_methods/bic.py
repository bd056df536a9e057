"""BiC stage 2 (Wu et al., "Large Scale Incremental Learning", 2019; the reference's MQ/train_bic.py:602-649): with the
network frozen, fit alpha and beta of the newest `BiasLayer` on the held-out split of the task.

The reference runs the whole model forward, `losses` and a backward to two scalars in every step.  A frozen network's raw
logits do not change, so `BiCCache.build` computes them once, together with what `PtTransformer.losses` derives from the
labels, and keeps everything on the device; `fit_bias_layer` then runs all steps of all epochs as ONE call of
`ops.bic_fit` (csrc/bic.hip) that never waits for the host.  The stage-2 objective is the focal classification term,
normalised by the step's own number of positive points; DESIGN.md 3.11 / 7 say what that leaves out and why.
"""
import torch

from .. import ops
from ..utils.cl_stream import DistributedBatchLoader


class BiCCache:
    """logits [N, C] fp32 (before the bias correction), label_bits [N, 2] int64 (uint64 bit patterns: bit c of the row =
    gt_cls[n, c] == 1), weight [N] fp32 (valid * w_cls, w_cls = 1 on negatives), pos [N] uint8 (pos_mask), clip_ptr
    [n_clips + 1] int32 -- all points of all clips, the pyramid levels concatenated, clip after clip; video_ids in order."""

    def __init__(self, logits, label_bits, weight, pos, clip_ptr, video_ids, smoothing):
        self.logits, self.label_bits, self.weight, self.pos, self.clip_ptr = logits, label_bits, weight, pos, clip_ptr
        self.video_ids, self.smoothing = list(video_ids), float(smoothing)

    @property
    def n_clips(self):
        return int(self.clip_ptr.numel()) - 1

    @staticmethod
    def pack_bits(gt_cls):
        """[..., C] 0/1 targets -> [..., 2] int64 words (two's complement wraps bit 63 into the sign: the same 64 bits)"""
        C = gt_cls.shape[-1]
        on = (gt_cls == 1).to(torch.int64)
        words = []
        for w in range(2):
            part = on[..., 64 * w:min(C, 64 * w + 64)]
            shifts = torch.arange(part.shape[-1], dtype=torch.int64, device=gt_cls.device)
            words.append((part << shifts).sum(-1) if part.shape[-1] else torch.zeros(on.shape[:-1], dtype=torch.int64,
                                                                                        device=gt_cls.device))
        return torch.stack(words, dim=-1)

    @classmethod
    @torch.no_grad()
    def build(cls, model, loader, task_id):
        """one forward per batch of the held-out loader (eval mode, get_emb=True, the bias correction bypassed), the
        model's own `label_points` for gt_cls / w_cls; nothing per point goes to the host"""
        was_training, model.bic_raw_logits = model.training, True
        model.eval()
        dev = model.device
        logits, bits, weight, pos, ids = [], [], [], [], []
        try:
            for video_list in loader:
                vl = [v for v in video_list if len(v['labels']) > 0]
                if not vl:
                    continue
                cls_logits, _, fpn_masks = model(vl, task_id=task_id, get_emb=True)
                points = model.point_generator(cls_logits, lengths=[x.shape[1] for x in cls_logits])
                gt_cls, _, w_cls, _ = model.label_points(points, [v['segments'].to(dev) for v in vl],
                                                         [v['labels'].to(dev) for v in vl])
                gt_cls, w_cls = torch.stack(gt_cls), torch.stack(w_cls)
                valid = torch.cat(fpn_masks, dim=1)
                pm = torch.logical_and(gt_cls.sum(-1) > 0, valid)                         # meta_archs.py losses: pos_mask
                w = torch.where(pm, w_cls, torch.ones_like(w_cls)) * valid.to(w_cls.dtype)
                x = torch.cat(cls_logits, dim=1).float()
                logits.append(x.reshape(-1, x.shape[-1]))
                bits.append(cls.pack_bits(gt_cls).reshape(-1, 2))
                weight.append(w.float().reshape(-1))
                pos.append(pm.to(torch.uint8).reshape(-1))
                ids.extend((v['video_id'], x.shape[1]) for v in vl)
        finally:
            model.bic_raw_logits = False
            model.train(was_training)
        if not logits:
            raise ValueError("BiC stage 2 needs at least one held-out clip")
        ptr = torch.tensor([0] + [n for _, n in ids], dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
        return cls(torch.cat(logits).contiguous(), torch.cat(bits).contiguous(), torch.cat(weight).contiguous(),
                   torch.cat(pos).contiguous(), ptr, [i for i, _ in ids], model.train_label_smoothing)

    def eval(self, lo, hi, alpha=1.0, beta=0.0):
        """(L, dL/dalpha, dL/dbeta) over all clips of the cache: fp64 [3] on the device"""
        ab = torch.tensor([float(alpha), float(beta)], dtype=torch.float32, device=self.logits.device)
        return ops.bic_eval(self.logits, self.label_bits, self.weight, self.pos, self.clip_ptr, lo, hi, self.smoothing, ab)


def newest_split(model):
    """columns [lo, hi) the newest bias layer corrects (PtTransformer._bic_correct)"""
    if not model.list_bias_layers or len(model.list_bias_layers) != len(model.list_splits):
        raise ValueError("the model has no bias layer to fit (list_bias_layers / list_splits)")
    return (model.list_splits[-2] if len(model.list_splits) > 1 else 0), model.list_splits[-1]


def epoch_orders(n_clips, epochs, batch_clips, seed=0, start_epoch=0):
    """every epoch's shuffle laid end to end: the rule of DistributedBatchLoader._order (seed, epoch), whole batches only"""
    loader = DistributedBatchLoader(range(n_clips), batch_clips, shuffle=True, seed=seed)
    order = []
    for e in range(start_epoch, start_epoch + epochs):
        loader.sampler.set_epoch(e)
        o = loader._order()
        order.extend(o[:len(o) // batch_clips * batch_clips])
    return order


def fit_bias_layer(model, cache, epochs, batch_clips, lr=0.001, seed=0):
    """plain SGD on (alpha, beta) of model.list_bias_layers[-1] over `epochs` shuffled passes of the cache, `batch_clips`
    clips per step -- one `ops.bic_fit` call.  Older bias layers are not touched.  Returns the per-step losses (fp64, on
    the device)."""
    lo, hi = newest_split(model)
    if hi != cache.logits.shape[1]:
        raise ValueError("the cache has %d classes, the newest split ends at %d" % (cache.logits.shape[1], hi))
    dev = cache.logits.device
    layer = model.list_bias_layers[-1]
    order = torch.tensor(epoch_orders(cache.n_clips, epochs, batch_clips, seed), dtype=torch.int32).to(dev)
    ab = torch.cat([layer.alpha.detach().reshape(1), layer.beta.detach().reshape(1)]).to(device=dev, dtype=torch.float32).contiguous()
    losses = ops.bic_fit(cache.logits, cache.label_bits, cache.weight, cache.pos, cache.clip_ptr, order, batch_clips, lo, hi,
                         cache.smoothing, lr, ab)
    with torch.no_grad():
        layer.alpha.copy_(ab[0:1])
        layer.beta.copy_(ab[1:2])
    return losses
