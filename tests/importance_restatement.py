"""float64 restatement of the EWC / MAS consolidation arithmetic (vilco_amd/cl_methods/regularizers.py:on_task_update), in
plain torch, for the importance tests.  Its input is what the consolidation pass saw: one {name: gradient} dictionary per
batch of the task's loader.  Nothing here is shared with the code under test."""
import torch


def _f(g, kind):
    g = g.detach().double().cpu()
    return g * g if kind == 'ewc' else g.abs()


def importance(batch_grads, kind, mode):
    """{name: float64 importance} of one task.
    'last': f(gradient of the last batch), for the names that have a gradient there (the reference, EWC.py:24-56 /
            MAS.py:23-57: zero_grad runs before every batch).
    'mean': (1 / n_batches) * sum over the batches of f(gradient); a name missing from a batch contributes zero there."""
    if mode == 'last':
        return {n: _f(g, kind) for n, g in batch_grads[-1].items()}
    assert mode == 'mean', mode
    out = {}
    for grads in batch_grads:
        for n, g in grads.items():
            out[n] = out[n] + _f(g, kind) if n in out else _f(g, kind)
    return {n: v / len(batch_grads) for n, v in out.items()}


def merge(task_importances, task_params, mode, gamma=1.0):
    """(importance list, optpar list) after the tasks in order.  task_importances[k]: `importance(...)` of task k;
    task_params[k]: {name: parameter value when task k was consolidated} for every parameter of the model at that time.
    'per_task': one dictionary per task, anchored at the parameters of the names that have an importance.
    'online':   ONE dictionary: importance = new + gamma * old on the flat prefix the old tensor covers (rows a head gained
                in dim 0 keep the new importance alone); a name without a new importance is carried as gamma * old in the
                parameter's current shape; a name that left the model is dropped; every anchor is the current parameter."""
    assert mode in ('per_task', 'online'), mode
    imps, opts = [], []
    for new, params in zip(task_importances, task_params):
        new = {n: v.clone() for n, v in new.items()}
        if mode == 'online' and imps:
            for n, old in imps[-1].items():
                if n not in params:
                    continue
                if n not in new:
                    new[n] = torch.zeros(params[n].shape, dtype=torch.float64)
                flat = new[n].view(-1)
                flat[:old.numel()] += gamma * old.reshape(-1)
            imps, opts = [], []
        imps.append(new)
        opts.append({n: params[n].detach().double().cpu().clone() for n in new})
    return imps, opts


# ------------------------------------------------------------------------------------------------------------------
# what the tests feed it with
class RecordingSGD(torch.optim.SGD):
    """an optimizer whose zero_grad first keeps clones of the gradients it is about to drop: after a consolidation pass
    `batches()` is exactly the list of per-batch gradients the pass saw (the last batch's are still in p.grad)."""
    def __init__(self, model):
        super().__init__(model.parameters(), lr=0.1)
        self.model, self.seen = model, []

    def _grads(self):
        return {n: p.grad.detach().clone() for n, p in self.model.named_parameters() if p.grad is not None}

    def zero_grad(self, set_to_none=True):
        if self._grads():
            self.seen.append(self._grads())
        super().zero_grad(set_to_none=set_to_none)

    def batches(self):
        return self.seen + [self._grads()]


class GrowToy(torch.nn.Module):
    """`model(batch) -> {'final_loss'}` with a class head that grows in dim 0 between tasks"""
    def __init__(self, rows=4):
        super().__init__()
        self.body = torch.nn.Linear(6, 5)
        self.head = torch.nn.Linear(5, rows)
        self.reg_params = {}

    def grow(self, rows):
        old, new = self.head, torch.nn.Linear(5, rows).to(self.head.weight.device)
        with torch.no_grad():
            new.weight[:old.out_features].copy_(old.weight)
            new.bias[:old.out_features].copy_(old.bias)
        self.head = new

    def forward(self, x):
        return {'final_loss': self.head(torch.tanh(self.body(x))).pow(2).mean()}


def toy_loader(seed, device='cpu', n=3):
    return [torch.randn(4, 6, generator=torch.Generator().manual_seed(seed + i)).to(device) for i in range(n)]
