"""A-GEM (Chaudhry, Ranzato, Rohrbach, Elhoseiny: "Efficient Lifelong Learning with A-GEM", ICLR 2019) on the replay memory
the episode loop already keeps -- a gradient-projection method, which the reference does not have.

Every iteration takes a reference gradient r on a batch drawn from the memory and the ordinary gradient g on the task's
batch; when the two conflict (g.r < 0) the step goes along g - (g.r / r.r) r, which no longer increases the memory batch's
loss to first order.  The projection is `ops.agem_project` (vilco_agem_project, csrc/optim.hip): three multi-tensor
launches over all gradient tensors, the branch taken on the device, so the step reads no device value and a replayed step
(vilco_amd/graph.py) stays a replayed step.

THE PROJECTED VECTOR.  g and r are the concatenations, in `model.parameters()` order, of the gradients of exactly those
parameters that have a gradient NOW (from the task's batch) AND got one from the reference pass:
  * a parameter without a reference gradient (not reached by the memory batch's loss) is left out: it adds nothing to g.r
    or r.r and keeps its gradient as it is;
  * a parameter without a current gradient (frozen, or not reached by the task batch's loss) is left out of both sums as
    well: there is nothing to project, and its reference gradient is not counted in r.r.
A parameter the optimizer lists twice (the adapter aliases) is one tensor and is projected once.

MEMORY.  The reference gradient is one more gradient-sized set of tensors alive during the task step: about 0.84 GB at
config P (210.7 M fp32 elements).  They are the `p.grad` tensors the reference pass produced, kept without a copy.

What the reference pass shares with a training forward it shares here too: it runs in train mode, so it advances the loss
normaliser's running mean and draws dropout / stochastic-depth masks of its own."""
import random

import torch

from .. import ops
from . import hooks      # (which imports this module: both use the other's names in calls only)


class MemorySampler:
    """An endless iterator of batches (lists of video dicts) over the clips of a replay memory {class: [videos]}.

    The clips are de-duplicated in dataset order (`InMemoryQILStream.flatten`: class by class, the first occurrence of a
    video id wins) and tagged `is_memory = True` when the sampler is built.  Epoch e walks the permutation drawn from
    random.Random(seed * 1000003 + e) -- the loaders' seeding rule -- in batches of `batch_size`; a short tail is dropped
    and the next epoch's permutation is drawn.  A memory smaller than one batch is the batch, whole, every time (in the
    epoch's order).  The same (memory, batch_size, seed) gives the same sequence."""

    def __init__(self, memory, batch_size, seed=0):
        from ..utils.cl_stream import InMemoryQILStream
        self.items = InMemoryQILStream.flatten(memory)
        if not self.items:
            raise ValueError("MemorySampler: the replay memory is empty")
        if int(batch_size) < 1:
            raise ValueError("MemorySampler: batch_size must be at least 1, got %r" % (batch_size,))
        for v in self.items:
            v['is_memory'] = True
        self.batch_size, self.seed = min(int(batch_size), len(self.items)), int(seed)
        self.epoch, self._order, self._pos = 0, None, 0

    def __iter__(self):
        return self

    def __next__(self):
        if self._order is None or self._pos + self.batch_size > len(self._order):
            self._order = list(range(len(self.items)))
            random.Random(self.seed * 1000003 + self.epoch).shuffle(self._order)
            self.epoch += 1
            self._pos = 0
        idx = self._order[self._pos:self._pos + self.batch_size]
        self._pos += self.batch_size
        return [self.items[i] for i in idx]


class AGEM:
    """One task's A-GEM state over `model`: `reference_pass` before the task batch's step, `project` between its backward
    and the clip / update (train_utils.train_one_epoch(agem=...) calls both).  trace: a list that receives every
    iteration's `out` = {g.r, r.r, alpha} (device tensors, not read here), or None."""

    def __init__(self, model, sampler, trace=None):
        self.model, self.sampler, self.trace = model, sampler, trace
        self.ref = {}            # id(param) -> (param, reference gradient)

    def reference_pass(self, task_id):
        """r: forward + backward of the sampler's next batch, eagerly, without distillation targets.  The p.grad tensors
        it leaves ARE r (no copy); p.grad is None before and after."""
        model = self.model
        params = list(model.parameters())
        for p in params:
            p.grad = None
        losses = model(next(self.sampler), task_id=task_id)
        losses['final_loss'].backward()
        self.ref = {}
        for p in params:
            if p.grad is not None:
                self.ref[id(p)] = (p, p.grad)
                p.grad = None
        # this forward packed the weights' operand planes and no update follows it: the task step must not find them cached --
        # a step that is captured now has to record its packs (a replayed graph reads the weights of ITS iteration)
        ops.forget_weight_planes(params)
        return losses

    def project(self):
        """project the gradients that are in p.grad now (see the module docstring for which take part) -> out"""
        grads, refs, dev = [], [], None
        for p in self.model.parameters():
            dev = p.device if dev is None else dev
            ent = self.ref.get(id(p))
            if p.grad is None or ent is None:
                continue
            grads.append(p.grad)
            refs.append(ent[1])
        out = ops.agem_project(grads, refs, device=dev)
        if self.trace is not None:
            self.trace.append(out)
        return out


def check_supported(cl_name, reducer=None, driver='run_episodes'):
    """the combinations this implementation refuses (hooks.SUPPORT), by name: data parallelism (each of the two backward passes of an
    iteration would need a gradient exchange of its own, and no multi-GPU node has run it) and the BiC / NLQ drivers"""
    if cl_name != 'agem':
        return False
    drivers, takes_reducer = hooks.SUPPORT['agem']
    if driver not in drivers:
        raise ValueError("cl_cfg.name 'agem' is not supported by %s: only run_episodes projects gradients" % driver)
    if reducer is not None and not takes_reducer:
        raise ValueError("cl_cfg.name 'agem' does not support data parallelism (reducer is not None): the reference pass "
                         "and the task step would each need their own gradient exchange")
    return True
