"""CODA-Prompt (Smith, Karlinsky, Gutta, Cascante-Bonilla, Kim, Arbelle, Panda, Feris, Kira: "CODA-Prompt: COntinual
Decomposed Attention-based Prompting for Rehearsal-Free Continual Learning", CVPR 2023) over the text tokens, where the L2P
pool (cl_methods/prompt.py) sits.  The reference project does not have it.

A pool of M components, each a prompt of `length` tokens with a key K[m] and an attention vector A[m].  The query is the mean
text token xk; component m weighs in with alpha[m] = cos(xk * A[m], K[m]) and the prompt that is prepended is the weighted sum
sum_m alpha[m] prompt[m] -- no top-k, no batch vote, everything differentiable.  Task t of n_tasks owns the components
[s, f) = [t pt, (t + 1) pt), pt = M // n_tasks: components below s are used but frozen (detached), components from f on are
not used yet.  `set_task(t)` re-initialises the task's rows of the three parameters by Gram-Schmidt against all earlier rows
and stores t in the buffer `task_count`, which an eval forward and a reloaded checkpoint take their f from.  The optional
penalty `ortho` (cl_cfg.coda_ortho_mu > 0) holds rows [0, f) of each parameter near an orthonormal set.

On the device the forward and backward are ONE operator, ops.coda_prompt (csrc/coda.hip: two launches forward, three with
the penalty, at most two backward, no host read, so a captured step replays it); VILCO_FUSED_PROMPT=0 (ops.fused_prompt, the
switch of both prompt modules) keeps the tensor-op body below for A/B runs, and CPU tensors always take it."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from . import hooks      # (which imports this module: both use the other's names in calls only)


def check_supported(prompt_type, reducer=None, driver='run_episodes'):
    """-> True when the run uses CODA-Prompt (and may); ValueError by name where it is not wired: the task boundary
    (`set_task`) is called by `run_episodes` only, and no multi-GPU node has run it."""
    if prompt_type != 'coda':
        return False
    drivers, takes_reducer = hooks.SUPPORT['coda']
    if driver not in drivers:
        raise ValueError("cl_cfg.prompt_type 'coda' is not wired into %s: only run_episodes moves the prompt's task window" % driver)
    if reducer is not None and not takes_reducer:
        raise ValueError("cl_cfg.prompt_type 'coda' has not been run with a reducer (data parallel): refused")
    return True


def gram_schmidt_rows(rows, start, stop, generator):
    """rows [M, D] fp32 -> a copy whose rows [start, stop) are redrawn: uniform(-1, 1) from `generator`, orthogonalised in
    float64 against rows [0, row) (two passes of modified Gram-Schmidt), normalised, stored in fp32.  A draw that is linearly
    dependent on the rows before it (or D < row + 1, where no orthogonal direction is left) is redrawn, at most 100 times."""
    out = rows.detach().to('cpu', torch.float64).clone()
    D = out.shape[1]
    for r in range(start, stop):
        for attempt in range(100):
            v = (torch.rand(D, generator=generator, dtype=torch.float64) * 2 - 1)
            n0 = v.norm()
            for _ in range(2):
                for j in range(r):
                    u = out[j]
                    uu = u @ u
                    if uu > 0:                                  # (a task that was skipped left its rows at zero)
                        v = v - (v @ u) / uu * u
            if v.norm() > 1e-6 * n0:
                break
        else:
            raise ValueError("CodaPrompt: no direction orthogonal to rows [0, %d) in %d dimensions" % (r, D))
        out[r] = (v / v.norm()).to(torch.float32).to(torch.float64)       # later rows see the stored value
    return out.to(torch.float32)


class CodaPrompt(nn.Module):
    def __init__(self, pool_size, length, embed_dim, n_tasks, ortho=False, seed=0):
        super().__init__()
        if not n_tasks or int(n_tasks) < 1:
            raise ValueError("CodaPrompt needs cl_cfg.coda_tasks (the number of tasks the pool is divided among), got %r" % (n_tasks,))
        if pool_size % int(n_tasks) != 0 or pool_size < int(n_tasks):
            raise ValueError("CodaPrompt: pool_size %d is not a positive multiple of coda_tasks %d" % (pool_size, n_tasks))
        self.pool_size, self.length, self.embed_dim = int(pool_size), int(length), int(embed_dim)
        self.n_tasks, self.per_task = int(n_tasks), int(pool_size) // int(n_tasks)
        self.want_ortho, self.seed = bool(ortho), int(seed)
        self.prompt = nn.Parameter(torch.zeros(pool_size, length, embed_dim))
        self.prompt_key = nn.Parameter(torch.zeros(pool_size, embed_dim))
        self.prompt_attn = nn.Parameter(torch.zeros(pool_size, embed_dim))
        self.register_buffer('task_count', torch.zeros((), dtype=torch.int64))
        self._task = 0                      # host copy of task_count (set_task, load_state_dict): no device read per forward
        self.set_task_calls = 0
        self.set_task(0)

    def window(self, task_id):
        if not 0 <= int(task_id) < self.n_tasks:
            raise ValueError("CodaPrompt: task %r outside [0, %d)" % (task_id, self.n_tasks))
        return int(task_id) * self.per_task, (int(task_id) + 1) * self.per_task

    @torch.no_grad()
    def set_task(self, t):
        """the task boundary: task_count = t, rows [s, f) of prompt, prompt_key and prompt_attn redrawn by Gram-Schmidt from a
        generator seeded with seed + t (earlier rows keep their bits)"""
        s, f = self.window(t)
        g = torch.Generator().manual_seed(self.seed + int(t))
        for p in (self.prompt, self.prompt_key, self.prompt_attn):
            flat = p.detach().reshape(self.pool_size, -1)
            new = gram_schmidt_rows(flat, s, f, g)
            flat[s:f].copy_(new[s:f].to(p.device))
        self.task_count.fill_(int(t))
        self._task = int(t)
        self.set_task_calls += 1

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + 'task_count' in state_dict:
            self._task = int(state_dict[prefix + 'task_count'])

    def forward(self, x_embed, task_id=-1, train=False):
        if train:
            s, f = self.window(task_id)
        else:
            s = f = (self._task + 1) * self.per_task
        if x_embed.is_cuda and ops.fused_prompt:
            # the op wants 0 <= s < f; with s == f (eval) nothing takes a gradient and any s below f will do
            prompted, ortho, alpha = ops.coda_prompt(x_embed, self.prompt, self.prompt_key, self.prompt_attn, min(s, f - 1), f,
                                                     want_ortho=self.want_ortho and train)
        else:
            prompted, ortho, alpha = self._forward_tensor_ops(x_embed, s, f, self.want_ortho and train)
        return {'prompted_embedding': prompted, 'total_prompt_len': self.length, 'ortho': ortho, 'alpha': alpha}

    @staticmethod
    def _penalty(t):
        # in float64: near an orthonormal set -- where set_task starts every task -- T T^t - I is all cancellation, and an fp32
        # Gram would hand the gradient its own rounding noise
        t64 = t.double()
        g = t64 @ t64.t() - torch.eye(t.shape[0], dtype=torch.float64, device=t.device)
        return (g * g).mean().to(t.dtype)

    def _forward_tensor_ops(self, x_embed, s, f, want_ortho):
        def used(p):                                                # rows [0, s) frozen, [s, f) the task's own
            return torch.cat([p[:s].detach(), p[s:f]], dim=0) if s > 0 else p[:f]
        P, K, A = used(self.prompt), used(self.prompt_key), used(self.prompt_attn)
        xk = x_embed.detach().mean(dim=1)                           # the query is a constant
        u = torch.einsum('bc,mc->bmc', xk, A)
        a = torch.einsum('bmc,mc->bm', F.normalize(u, dim=2), F.normalize(K, dim=1))
        p = torch.einsum('bm,mtc->btc', a, P)
        alpha = torch.zeros(x_embed.shape[0], self.pool_size, dtype=a.dtype, device=a.device)
        alpha[:, :f] = a.detach()
        if want_ortho:
            ortho = self._penalty(K) + self._penalty(A) + self._penalty(P.reshape(f, -1))
        else:
            ortho = torch.zeros((), dtype=x_embed.dtype, device=x_embed.device)
        return torch.cat([p, x_embed], dim=1), ortho, alpha
