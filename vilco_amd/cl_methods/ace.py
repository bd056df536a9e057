"""ER-ACE (Caccia, Aljundi, Asadi, Tuytelaars, Pineau, Belilovsky: "New Insights on Reducing Abrupt Representation Change in
Online Continual Learning", ICLR 2022): an asymmetric detection loss -- the reference has nothing like it.

A clip of the current task carries labels of the current task's classes only, so under the plain loss every valid point of
it is a focal negative on every OLD class column, and the "al" term pushes every old class's best score down: old actions
that are visible in the new clips are trained as background, and every step lowers every old logit whatever the input.
ER-ACE scores the incoming clips over the current task's classes only and the replayed clips over all classes.

Here that is a class window per clip: `step_table` gives the first class column each clip's classification terms visit --
0 for a clip of the replay memory, `model.n_known` for any other clip -- and the fused loss takes it (`ops.mq_loss_ace`,
csrc/loss.hip with WIN = true: the focal sum, the al softmax, its maximum and its sum run over [lo_b, C); the label
assignment, the regression loss and the normaliser are untouched).  No extra pass, no bank, no state file: the method is the
window.  A stream built with train_enable=True mixes the memory into the task's batches (replay under full supervision); with
train_enable=False no memory clip reaches a batch and the method is the window alone.

What differs from the paper: the head is a sigmoid focal loss, not a softmax cross-entropy (masking a logit out of the focal
sum removes its term and gradient; there is no normaliser over classes to restrict -- the al term, which has one, takes its
softmax over the window); and the window is per clip (the classes of the current task), not the set of classes present in the
incoming batch."""
import torch

from . import hooks      # (which imports this module: both use the other's names in calls only)
from .der import clip_key, labelled


def memory_keys(memory):
    """the keys of the clips in a replay memory ({class: [videos]})"""
    return {clip_key(v) for videos in (memory or {}).values() for v in videos}


def window_rows(video_list, n_known, keys):
    """[lo_b] per labelled clip, on the host: 0 for a memory clip (or while nothing is known), n_known otherwise"""
    n_known = int(n_known)
    return [0 if (n_known == 0 or clip_key(v) in keys) else n_known for v in labelled(video_list)]


def step_table(model, video_list):
    """`ace_lo` of a training step of `model` over `video_list`: int32 [B] on the model's device, built on the host from the
    memory's key set (no device read) -- staged in pinned memory and uploaded without blocking, like the other small tables"""
    n_known = int(getattr(model, 'n_known', 0))
    keys = memory_keys(getattr(model, 'memory', None)) if n_known > 0 else ()
    host = torch.tensor(window_rows(video_list, n_known, keys), dtype=torch.int32)
    device = torch.device(model.device)
    if device.type != 'cuda':
        return host.to(device)
    return host.pin_memory().to(device, non_blocking=True)


def column_mask(cls_lo, n_classes):
    """bool [B, C]: the columns clip b's classification terms visit (tensor-expression path; a value outside [0, C) is 0)"""
    lo = cls_lo.to(torch.int64)
    lo = torch.where((lo < 0) | (lo >= n_classes), torch.zeros_like(lo), lo)
    return torch.arange(n_classes, device=cls_lo.device)[None, :] >= lo[:, None]


def check_supported(cl_name, reducer=None, driver='run_episodes'):
    """the combinations this implementation refuses, by name: the BiC / NLQ drivers (NLQ has one query class: there is no
    window to take) and data parallelism (hooks.SUPPORT_MORE)"""
    if cl_name != 'er_ace':
        return False
    drivers, takes_reducer = hooks.support('er_ace')
    if driver not in drivers:
        raise ValueError("cl_cfg.name 'er_ace' is not supported by %s: only run_episodes trains the class-incremental "
                         "detection loss the window applies to" % driver)
    if reducer is not None and not takes_reducer:
        raise ValueError("cl_cfg.name 'er_ace' does not support data parallelism (reducer is not None): no multi-GPU node has "
                         "run it")
    return True
