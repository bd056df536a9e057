"""EWC / MAS continual-learning regularisers on the HIP path (reference: MQ/libs/cl_methods/EWC.py:6-56,
MAS.py:5-57; called from train_utils.py:337-344 and train_cl.py:381-385).

`model.reg_params` keeps the reference's layout -- {'fisher' | 'importance': [ {name: tensor}, ... one dict per
finished task ], 'optpar': [ {name: tensor}, ... ]} -- so checkpoints ('reg_params' key, train_cl.py:306) interchange.

The penalty  lambda * sum_tasks sum_names sum_elems F (theta* - theta[:len(theta*)])^2  and its gradient are ONE
multi-tensor launch (vilco_cl_penalty, csrc/optim.hip) over a chunk table of every (task, name) pair, instead of
one autograd graph node per pair per step: the value comes back as a device scalar, the gradient
-2 lambda F (theta* - theta) is accumulated straight into p.grad (after backward, before clipping, which is where the
reference's autograd puts it too).

The consolidation pass (`on_task_update`) reproduces the reference by default: the LAST batch's gradient, one more
dictionary per task.  `importance='mean'` estimates the importance over the whole task and `merge='online'` keeps one
dictionary for the whole stream; both do their arithmetic in vilco_cl_accumulate (csrc/optim.hip), one multi-tensor
launch per batch / per merge.

Synaptic Intelligence (kind='si', bottom of the file) shares the penalty and MAS's 'importance' key; its importance is a
path integral the optimizer's update kernel takes at every step, consolidated by one launch at the end of a task.
RWalk (kind='rwalk', below SI) does the same with a Fisher moving average and path scores kept by that kernel."""
import ctypes

import torch

from .. import _lib, ops

CHUNK = ops.CHUNK


def _entries(model, kind):
    """(parameter, importance, optpar) of every consolidated (task, name) pair; kind 'ewc' reads reg_params['fisher'],
    'mas', 'si' and 'rwalk' read reg_params['importance']"""
    if kind not in ('ewc', 'mas', 'si', 'rwalk'):
        raise ValueError("kind must be 'ewc', 'mas', 'si' or 'rwalk', got %r" % (kind,))
    reg = getattr(model, 'reg_params', None) or {}
    key = 'fisher' if kind == 'ewc' else 'importance'
    if key not in reg or 'optpar' not in reg:
        return []
    out = []
    for imp_d, opt_d in zip(reg[key], reg['optpar']):
        for name, p in model.named_parameters():
            if 'scale' not in name and name in imp_d:           # EWC.py:15 / MAS.py:14
                imp, opt = imp_d[name], opt_d[name]
                assert imp.shape == opt.shape and opt.numel() <= p.numel() and opt.shape[1:] == p.shape[1:]
                out.append((p, imp, opt))
    return out


def apply_penalty(model, reg_lambda, kind='ewc'):
    """adds the penalty gradient to p.grad (allocating zeros where a parameter has none) and returns the penalty value
    as a device scalar, or None when no task has been consolidated yet."""
    items = _entries(model, kind)
    if not items:
        return None
    lib = _lib.load()
    dev = items[0][0].device
    for p, imp, opt in items:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        if not (p.is_contiguous() and p.grad.is_contiguous() and imp.is_contiguous() and opt.is_contiguous()
                and imp.is_cuda and opt.is_cuda and imp.dtype == torch.float32):
            raise RuntimeError("vilco_cl_penalty needs contiguous fp32 tensors on the HIP device")
    ptrs = torch.tensor([[p.data_ptr() for p, _, _ in items], [p.grad.data_ptr() for p, _, _ in items],
                         [imp.data_ptr() for _, imp, _ in items], [opt.data_ptr() for _, _, opt in items]],
                        dtype=torch.int64).to(dev, non_blocking=True)
    # numel = optpar's: a prefix of the (possibly grown) parameter.  Rebuilt on every call.
    plan = ops.ChunkPlan([opt.numel() for _, _, opt in items], dev, non_blocking=True)
    partial = torch.empty(max(plan.nchunks, 1), dtype=torch.float32, device=dev)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.check(lib.vilco_cl_penalty(ctypes.byref(plan.table(ptrs, 4)), float(reg_lambda),
                                    int(len({id(p) for p, _, _ in items}) < len(items)), partial.data_ptr(), out.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream))
    return out[0]


def get_regularized_loss(loss, model, reg_lambda, kind='ewc'):
    """reference-shaped entry (EWC.py:6 / MAS.py:5) for callers that want the autograd form: loss + penalty with the
    penalty as ordinary tensor expressions.  train_one_epoch uses `apply_penalty` instead."""
    for p, imp, opt in _entries(model, kind):
        loss = loss + (imp * (opt - p[:opt.size(0)]).pow(2)).sum() * reg_lambda
    return loss


IMPORTANCE_MODES = ('last', 'mean')
MERGE_MODES = ('per_task', 'online')


def check_modes(importance, merge):
    if importance not in IMPORTANCE_MODES:
        raise ValueError("cl_cfg.importance must be one of %s, got %r" % (', '.join(map(repr, IMPORTANCE_MODES)), importance))
    if merge not in MERGE_MODES:
        raise ValueError("cl_cfg.importance_merge must be one of %s, got %r" % (', '.join(map(repr, MERGE_MODES)), merge))


def importance_options(cl_cfg):
    """the keyword arguments of `on_task_update` that a cl_cfg asks for: cl_cfg['importance'] ('last' | 'mean'),
    ['importance_merge'] ('per_task' | 'online'), ['importance_gamma'].  The keys are optional (the reference's config has
    none of them); an unknown value raises ValueError."""
    out = dict(importance=cl_cfg.get('importance', 'last'), merge=cl_cfg.get('importance_merge', 'per_task'),
               gamma=float(cl_cfg.get('importance_gamma', 1.0)))
    check_modes(out['importance'], out['merge'])
    return out


def _mean_importance(loader_task, optimizer, model, kind):
    """{name: mean over the batches of f(batch gradient)}, f = square (EWC) / abs (MAS): after every backward ONE
    cl_accumulate launch adds f(p.grad) of every gradient-bearing parameter to its accumulator, one more launch scales by
    1 / n_batches.  An accumulator is allocated when its parameter first shows a gradient (beta = 0: written, not read)."""
    op = ops.CL_OP_SQUARE if kind == 'ewc' else ops.CL_OP_ABS
    acc, n_batches = {}, 0
    for video_list in loader_task:
        optimizer.zero_grad(set_to_none=True)
        model(video_list)['final_loss'].backward()
        n_batches += 1
        first, later = ([], []), ([], [])
        for name, p in model.named_parameters():
            if p.grad is None:
                continue
            g = p.grad.detach()
            srcs, accs = later if name in acc else first
            if name not in acc:
                acc[name] = torch.empty(p.shape, dtype=p.dtype, device=p.device)
            srcs.append(g if g.is_contiguous() else g.contiguous())
            accs.append(acc[name])
        ops.cl_accumulate(first[0], first[1], op, 1.0, 0.0)
        ops.cl_accumulate(later[0], later[1], op, 1.0, 1.0)
    if n_batches:
        ops.cl_accumulate(list(acc.values()), list(acc.values()), op, 0.0, 1.0 / n_batches)
    return {name: acc[name] for name, _ in model.named_parameters() if name in acc}


def _merge_online(model, old_imp, imp_d, gamma):
    """imp_d[name] += gamma * old_imp[name] on the old tensor's flat prefix (a class head that grew in dim 0 keeps the new
    importance alone on its new rows); a name without a gradient this task is carried as gamma * old in the parameter's
    current shape; a name that left the model is dropped."""
    params = dict(model.named_parameters())
    both, carried = ([], []), ([], [])
    for name, old in old_imp.items():
        if name not in params:
            continue
        if name in imp_d:
            srcs, accs = both
        else:
            srcs, accs = carried
            imp_d[name] = torch.zeros_like(params[name].data, memory_format=torch.contiguous_format)
        new = imp_d[name]
        assert old.numel() <= new.numel() and old.shape[1:] == new.shape[1:], name
        srcs.append(old)
        accs.append(new)
    ops.cl_accumulate(both[0], both[1], ops.CL_OP_COPY, gamma, 1.0, numels=[o.numel() for o in both[0]])
    ops.cl_accumulate(carried[0], carried[1], ops.CL_OP_COPY, gamma, 0.0, numels=[o.numel() for o in carried[0]])


def on_task_update(loader_task, device, optimizer, model, kind='ewc', group=None, data_parallel=False, importance='last',
                   merge='per_task', gamma=1.0):
    """importance of the weights after a task (EWC.py:24-56 / MAS.py:23-57): one pass over the task's loader with
    zero_grad before every batch, plus a copy of the parameters.
    importance='last' (the reference): what is kept is the LAST batch's gradient (squared for EWC, absolute for MAS).
    importance='mean': the mean over ALL batches of the squared / absolute BATCH gradient, accumulated on the device by
      vilco_cl_accumulate (one launch per batch).  The granularity is the reference's -- the gradient of a batch's loss --
      so a loader with batch size 1 gives the per-sample empirical Fisher; larger batches give the Fisher of the batch mean.
    merge='per_task' (the reference): every task appends one dictionary, the penalty walks tasks x tensors entries.
    merge='online': reg[key] and reg['optpar'] hold ONE dictionary: importance = new + gamma * old (the merge the
      commented-out consolidate_reg_params of MAS.py sketches), anchored at the current parameters, so the penalty's cost
      and the importance memory do not grow with the number of tasks.  Dictionaries that are already there (a checkpoint
      of a per-task run) are folded in, each weighted by gamma.
    data_parallel / group: the run is data parallel over `group` (None = the default group).  Every rank sees the last batch of ITS shard, so the importances
    are averaged over the ranks (the reference wraps this pass in no DDP hook and lets them differ; the penalty is
    applied after the gradient exchange, so different importances would pull the replicas apart)."""
    check_modes(importance, merge)
    model.train()
    reg = model.reg_params
    key = 'fisher' if kind == 'ewc' else 'importance'
    if not (key in reg and 'optpar' in reg):
        reg[key], reg['optpar'] = [], []
    if importance == 'mean':
        imp_d = _mean_importance(loader_task, optimizer, model, kind)
    else:
        for video_list in loader_task:
            optimizer.zero_grad(set_to_none=True)
            model(video_list)['final_loss'].backward()
        imp_d = {}
        for name, p in model.named_parameters():
            if p.grad is not None:
                g = p.grad.data.clone()
                imp_d[name] = g.pow(2) if kind == 'ewc' else g.abs()
    if merge == 'online':
        for old_imp in reg[key]:
            _merge_online(model, old_imp, imp_d, float(gamma))
        del reg[key][:], reg['optpar'][:]
    opt_d = {name: p.data.clone() for name, p in model.named_parameters() if name in imp_d}
    if data_parallel and torch.distributed.is_initialized() and torch.distributed.get_world_size(group) > 1:
        ws = float(torch.distributed.get_world_size(group))
        for name in sorted(imp_d):                      # the same order on every rank
            torch.distributed.all_reduce(imp_d[name], group=group)
            imp_d[name].div_(ws)
    reg[key].append(imp_d)
    reg['optpar'].append(opt_d)
    return reg


def on_task_mas_update(loader_task, device, optimizer, model):
    return on_task_update(loader_task, device, optimizer, model, kind='mas')


def get_mas_regularized_loss(loss, model, reg_lambda):
    return get_regularized_loss(loss, model, reg_lambda, kind='mas')


# ------------------------------------------------------------------------------------------------ Synaptic Intelligence
# (Zenke, Poole, Ganguli 2017; the reference has no SI).  Per regularised parameter: `omega`, the path integral of the task so
# far, advanced by the optimizer's update kernel at every step (FusedOptimizer.attach_si -> vilco_optim_desc.si_ptrs):
#     omega <- omega - gr * (p_new - p_old),   gr = the clipped gradient the update consumes (penalty gradient included)
# and `theta_start`, the parameter at the start of the task.  At the end of a task ONE launch (vilco_si_consolidate) makes
#     Omega <- Omega_old + max(omega, 0) / ((theta - theta_start)^2 + xi),  theta* <- theta,  omega <- 0,  theta_start <- theta
# Omega / theta* live in model.reg_params under MAS's keys ('importance' / 'optpar', ONE dictionary for the stream), so
# `_entries(model, 'si')`, the penalty kernel, checkpoints and head growth (optpar a prefix of a grown head) work as for MAS.
SI_XI = 0.1          # Zenke's default; cl_cfg['si_xi'] overrides it


def si_xi(cl_cfg):
    return float(cl_cfg.get('si_xi', SI_XI))


def _si_params(model):
    """the parameters SI regularises: what EWC / MAS regularise (`_entries`: no 'scale' in the name) among the trained ones"""
    return [(name, p) for name, p in model.named_parameters() if p.requires_grad and 'scale' not in name]


def si_begin_task(model, optimizer):
    """Start of a task (after the class head has grown and the task's optimizer exists): a zeroed `omega` and a snapshot
    `theta_start` for every regularised parameter, kept in model.si_state = {name: {'omega', 'theta_start'}}, and the omegas
    attached to the optimizer, whose update kernel advances them from now on -- eagerly or replayed (attaching drops the
    optimizer's cached plans, and a GraphedStep captured over them recaptures).  si_state is per task and is not
    checkpointed.
    Data parallel: nothing is exchanged.  Every rank steps with the averaged gradient and makes the same update, so omega,
    theta_start and the consolidated importance are equal on all ranks by construction."""
    state = {}
    for name, p in _si_params(model):
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
            raise RuntimeError("Synaptic Intelligence needs contiguous fp32 parameters on the HIP device (%s)" % name)
        state[name] = {'omega': torch.zeros_like(p), 'theta_start': p.detach().clone()}
    model.si_state = state
    optimizer.attach_si({p: state[name]['omega'] for name, p in _si_params(model)})
    return state


def on_task_si_update(model, optimizer=None, xi=SI_XI):
    """End of a task: one vilco_si_consolidate launch over all regularised tensors folds the task's path integral into the
    importance (formula above), anchors theta* at the CURRENT parameters, zeroes omega and moves theta_start, all in place;
    model.reg_params then holds one 'importance' / 'optpar' dictionary.  An importance that is already there (an earlier
    task, a checkpoint) is Omega_old on its flat prefix: the rows a class head gained since start from zero, as in
    `_merge_online`; a name SI does not track this task is carried unchanged.
    Ordering (train_cl.run_episodes): SI consolidates from the state at the END of training -- the state its path integral
    led to -- before the task's best checkpoint is reloaded, and needs no pass over the data.  `optimizer` is not stepped;
    it keeps accumulating into the zeroed omegas if training goes on."""
    if not xi > 0:
        raise ValueError("si_xi must be positive, got %r" % (xi,))
    state = getattr(model, 'si_state', None)
    if not state:
        raise RuntimeError("on_task_si_update without si_begin_task: the model carries no si_state")
    reg = model.reg_params
    if not ('importance' in reg and 'optpar' in reg):
        reg['importance'], reg['optpar'] = [], []
    if len(reg['importance']) > 1:
        raise ValueError("Synaptic Intelligence keeps ONE importance dictionary; reg_params holds %d" % len(reg['importance']))
    old_imp = reg['importance'][0] if reg['importance'] else {}
    old_opt = reg['optpar'][0] if reg['optpar'] else {}
    imp_d, opt_d, rows, numel, numel_old = {}, {}, [], [], []
    for name, p in model.named_parameters():
        st = state.get(name)
        if st is None:
            if name in old_imp:
                imp_d[name], opt_d[name] = old_imp[name], old_opt[name]
            continue
        if st['omega'].numel() != p.numel() or not p.is_contiguous():
            raise RuntimeError("si_state of %s does not fit the parameter: call si_begin_task after the head has grown" % name)
        old = old_imp.get(name)
        n_old = 0 if old is None else old.numel()
        if old is not None and old.shape == p.shape and old.is_contiguous() and old.device == p.device:
            imp, opt = old, old_opt[name]                  # updated in place
        else:
            imp, opt = torch.empty_like(p), torch.empty_like(p)          # what lies behind n_old is written, not read
            if old is not None:
                assert n_old <= p.numel() and old.shape[1:] == p.shape[1:], name
                imp.view(-1)[:n_old].copy_(old.reshape(-1))
        imp_d[name], opt_d[name] = imp, opt
        rows.append((p.data_ptr(), st['omega'].data_ptr(), st['theta_start'].data_ptr(), imp.data_ptr(), opt.data_ptr()))
        numel.append(p.numel())
        numel_old.append(n_old)
    if rows:
        dev = next(iter(imp_d.values())).device
        ptrs = torch.tensor([list(col) for col in zip(*rows)], dtype=torch.int64).to(dev)
        plan = ops.ChunkPlan(numel, dev)
        t_old = torch.tensor(numel_old, dtype=torch.int64).to(dev)
        d = _lib.SiDesc(table=plan.table(ptrs, 5), numel_old=t_old.data_ptr(), xi=float(xi))
        _lib.check(_lib.load().vilco_si_consolidate(ctypes.byref(d), torch.cuda.current_stream().cuda_stream))
    reg['importance'], reg['optpar'] = [imp_d], [opt_d]
    return reg


# ------------------------------------------------------------------------------------------------ RWalk
# (Riemannian Walk: Chaudhry, Dokania, Ajanthan, Torr, ECCV 2018; the reference has no RWalk.)  Per element of every parameter
# SI regularises (`_si_params`) four fp32 states, advanced by the optimizer's update kernel (FusedOptimizer.attach_rwalk ->
# vilco_optim_step_rwalk) at every update:
#     F <- F + alpha (gr^2 - F)              the diagonal empirical Fisher as a moving average of the squared gradient;
#     w <- w - gr (p_new - p_old)            SI's path integral, over the interval since the last checkpoint;
#   every delta_t iterations (a checkpoint):  s <- s + max(w, 0) / (0.5 F (p_new - theta_ck)^2 + eps),  w <- 0,  theta_ck <- p_new
# gr = the clipped gradient the update consumes -- as for SI it includes the penalty gradient and excludes the weight decay.
# F and s are kept across tasks, w and theta_ck are per task.  The end of a task needs NO pass over the data
# (`on_task_rwalk_update`): the open interval is closed, importance = F / max F + s / max s goes under MAS's keys, s is halved.
RWALK_ALPHA, RWALK_DELTA_T, RWALK_EPS = 0.9, 10, 1e-8      # alpha, delta_t: the paper's; eps: ours (core/config.py EXTRA_DEFAULTS)


def rwalk_options(cl_cfg):
    """the keyword arguments of `rwalk_begin_task` / `on_task_rwalk_update` that a cl_cfg asks for: cl_cfg['rwalk_alpha'] in
    (0, 1], ['rwalk_delta_t'] an integer >= 1, ['rwalk_eps'] > 0 (all optional); a bad value raises ValueError here, before the
    first task."""
    alpha = float(cl_cfg.get('rwalk_alpha', RWALK_ALPHA))
    delta_t = cl_cfg.get('rwalk_delta_t', RWALK_DELTA_T)
    eps = float(cl_cfg.get('rwalk_eps', RWALK_EPS))
    if not 0.0 < alpha <= 1.0:
        raise ValueError("cl_cfg.rwalk_alpha must lie in (0, 1], got %r" % (alpha,))
    if isinstance(delta_t, bool) or int(delta_t) != delta_t or int(delta_t) < 1:
        raise ValueError("cl_cfg.rwalk_delta_t must be an integer >= 1, got %r" % (delta_t,))
    if not eps > 0.0:
        raise ValueError("cl_cfg.rwalk_eps must be positive, got %r" % (eps,))
    return dict(alpha=alpha, delta_t=int(delta_t), eps=eps)


def rwalk_begin_task(model, optimizer, alpha=RWALK_ALPHA, delta_t=RWALK_DELTA_T, eps=RWALK_EPS):
    """Start of a task (after the class head has grown and the task's optimizer exists): model.rwalk_state = {name: {'fisher',
    'score', 'omega', 'theta_ck'}} for every regularised parameter.  fisher and score of an earlier task (or of
    `load_rwalk_state`) are carried on their flat prefix -- the rows a class head has gained since start from zero -- omega is
    zeroed, theta_ck is a snapshot of the parameter, and the state is attached to the optimizer, which zeroes its iteration
    word `rwalk_tick`.  A name that is no longer regularised is dropped.  A model without any regularised parameter gets an empty
    state and an optimizer with nothing attached (the plain update).
    Data parallel: nothing is exchanged; every rank steps with the averaged gradient and makes the same update (as SI)."""
    old_state = getattr(model, 'rwalk_state', None) or {}
    state = {}
    for name, p in _si_params(model):
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
            raise RuntimeError("RWalk needs contiguous fp32 parameters on the HIP device (%s)" % name)
        st = {'omega': torch.zeros_like(p), 'theta_ck': p.detach().clone()}
        old = old_state.get(name, {})
        for key in ('fisher', 'score'):
            prev = old.get(key)
            if prev is not None and prev.shape == p.shape and prev.device == p.device and prev.is_contiguous():
                st[key] = prev
                continue
            st[key] = torch.zeros_like(p)
            if prev is not None:
                if not (prev.numel() <= p.numel() and prev.shape[1:] == p.shape[1:]):
                    raise RuntimeError("rwalk_state of %s (%s) is no prefix of the parameter (%s)" % (name, tuple(prev.shape), tuple(p.shape)))
                st[key].view(-1)[:prev.numel()].copy_(prev.reshape(-1))
        state[name] = st
    model.rwalk_state = state
    optimizer.attach_rwalk({p: state[name] for name, p in _si_params(model)}, alpha=alpha, delta_t=delta_t, eps=eps)
    return state


def on_task_rwalk_update(model, optimizer=None, eps=RWALK_EPS, return_max=False):
    """End of a task: vilco_rwalk_consolidate -- three launches over all regularised tensors, nothing read by the host -- closes
    the interval the last checkpoint left open, takes max F and max s over ALL tensors on the device and writes
    importance = F / max F + s / max s (each term in [0, 1]; a term whose max is 0 contributes 0) and optpar = the CURRENT
    parameters; then s <- s / 2 (the paper's averaging of old and new scores), theta_ck <- p, w = 0, and F is kept.
    model.reg_params ends up holding ONE 'importance' / 'optpar' dictionary under MAS's keys; it is REPLACED, not accumulated:
    F and s are running quantities that already contain the earlier tasks.  A name RWalk does not track is not carried.
    Ordering (train_cl.run_episodes): as SI, after the task's training and before its best checkpoint is reloaded.
    `optimizer` is not used (the signature mirrors on_task_si_update); an empty rwalk_state (no regularised parameter) leaves
    one empty dictionary and launches nothing.  return_max: also return the device tensor {max F, max s}."""
    if not eps > 0:
        raise ValueError("rwalk_eps must be positive, got %r" % (eps,))
    state = getattr(model, 'rwalk_state', None)
    if state is None or any('omega' not in st for st in state.values()):
        raise RuntimeError("on_task_rwalk_update without rwalk_begin_task: the model carries no rwalk_state of this task")
    if not state:      # rwalk_begin_task found no regularised parameter: nothing was tracked, nothing is penalised
        model.reg_params['importance'], model.reg_params['optpar'] = [{}], [{}]
        return (model.reg_params, None) if return_max else model.reg_params
    imp_d, opt_d, rows, outs, numel = {}, {}, [], [], []
    for name, p in model.named_parameters():
        st = state.get(name)
        if st is None:
            continue
        if st['omega'].numel() != p.numel() or not p.is_contiguous():
            raise RuntimeError("rwalk_state of %s does not fit the parameter: call rwalk_begin_task after the head has grown" % name)
        imp_d[name], opt_d[name] = torch.empty_like(p), torch.empty_like(p)
        rows.append((p.data_ptr(), st['fisher'].data_ptr(), st['score'].data_ptr(), st['omega'].data_ptr(), st['theta_ck'].data_ptr()))
        outs.append((imp_d[name].data_ptr(), opt_d[name].data_ptr()))
        numel.append(p.numel())
    if not rows:
        raise RuntimeError("on_task_rwalk_update: none of the %d names in model.rwalk_state is a parameter of the model"
                           % len(state))
    dev = next(iter(imp_d.values())).device
    ptrs = torch.tensor([list(col) for col in zip(*rows)], dtype=torch.int64).to(dev)
    out_ptrs = torch.tensor([list(col) for col in zip(*outs)], dtype=torch.int64).to(dev)
    plan = ops.ChunkPlan(numel, dev)
    partial = torch.empty(2 * max(plan.nchunks, 1), dtype=torch.float32, device=dev)
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    d = _lib.RwalkDesc(table=plan.table(ptrs, 5), out_ptrs=out_ptrs.data_ptr(), partial=partial.data_ptr(), out=out.data_ptr(),
                       eps=float(eps))
    _lib.check(_lib.load().vilco_rwalk_consolidate(ctypes.byref(d), torch.cuda.current_stream().cuda_stream))
    reg = model.reg_params
    reg['importance'], reg['optpar'] = [imp_d], [opt_d]
    return (reg, out) if return_max else reg


def rwalk_state_dict(model):
    """what outlives a task, on the host: {'fisher': {name: tensor}, 'score': {name: tensor}} (omega and theta_ck are per task)
    and, once a task has been consolidated, its 'importance' / 'optpar' dictionary: the task's checkpoints were written before
    the consolidation and do not hold it."""
    state = getattr(model, 'rwalk_state', None) or {}
    out = {key: {name: st[key].detach().cpu().clone() for name, st in state.items()} for key in ('fisher', 'score')}
    reg = getattr(model, 'reg_params', None) or {}
    if len(reg.get('importance', ())) == 1 and len(reg.get('optpar', ())) == 1:
        for key in ('importance', 'optpar'):
            out[key] = {name: t.detach().cpu().clone() for name, t in reg[key][0].items()}
    return out


def load_rwalk_state(model, sd, device=None):
    """the inverse of `rwalk_state_dict`, for a resume at a task boundary: the next `rwalk_begin_task` carries fisher and score
    on their flat prefix; an 'importance' / 'optpar' dictionary REPLACES model.reg_params -- also one the caller restored from a
    checkpoint before (the file is newer than any checkpoint of the task it closes: those were written before the
    consolidation).  `run_episodes(start_task > 0)` calls this."""
    if not {'fisher', 'score'} <= set(sd) <= {'fisher', 'score', 'importance', 'optpar'} or set(sd['fisher']) != set(sd['score']):
        raise ValueError("not an rwalk_state_dict: keys %s" % sorted(sd))
    model.rwalk_state = {name: {'fisher': sd['fisher'][name].to(device=device).contiguous(),
                                'score': sd['score'][name].to(device=device).contiguous()}
                         for name in sd['fisher']}
    if 'importance' in sd and 'optpar' in sd:
        model.reg_params = {key: [{name: t.to(device=device).contiguous() for name, t in sd[key].items()}]
                            for key in ('importance', 'optpar')}
    return model.rwalk_state
