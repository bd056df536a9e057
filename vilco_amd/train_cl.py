"""Episode (task) loop of query-incremental continual learning on the HIP path -- our counterpart of the
reference driver MQ/train_cl.py:206-389 (+ load_best_checkpoint :31-40), written around the drop-in model:

  for every task j of the stream:
      validate the incoming model                                   (train_cl.py:209-219)
      [type_sampling 'icarl': cache sigmoid(logits) of the task's clips, :226-235]
      for every epoch: sampler.set_epoch, pre_train_epoch (adapters), train_one_epoch, validate after the first
          third of the epochs, keep the best checkpoint             (:237-316)
      replay memory: m = memory_size // #classes per class, add_samples_to_mem, n_known = len(memory), memory
          pickle                                                    (:343-361)
      reload the task's best checkpoint, final validation           (:363-365)
      if another task follows: augment_classification(num_next_classes), EWC / MAS consolidation, NEW optimizer
          and scheduler                                             (:373-389)

A continual-learning method acts at six points of that loop -- begin_run, begin_task, end_training, save_state, after_reload,
before_next_task: cl_methods/hooks.py names them, holds one class per method (EWC / MAS, SI, RWalk, A-GEM, DER, POD, the CODA task
switch) and the table of which method runs in which driver (hooks.SUPPORT).  The drivers call the points and know no method.

What is ours rather than the reference's: the stream is any iterable with QILSetTask's contract
(`(data, loader, num_next_classes)` per task, a `.memory` attribute; utils/cl_stream.py has an in-memory one --
the Ego4D readers are outside the hot path), validation is a callable (the evaluator is outside the hot path;
`train_utils.collect_results` produces its input format), gradients of data-parallel replicas go through
`dist.GradReducer`, and the per-iteration work is `train_utils.train_one_epoch` (fused clip + AdamW, no host sync).
Checkpoints keep the reference's keys: task, epoch, state_dict, scheduler, optimizer, reg_params (:300-307).
"""
import os
import pickle

import numpy as np
import torch

from .cl_methods.hooks import DER_BANK_FILE, RWALK_STATE_FILE, each, make_hooks  # noqa: F401
from .utils.train_utils import make_optimizer, make_scheduler, save_checkpoint, train_one_epoch


def load_best_checkpoint(model, file_folder, file_name, current_task, gpu_id):
    """train_cl.py:31-40: restore state_dict + reg_params when the file exists; the model is returned either way."""
    path = os.path.join(file_folder, file_name)
    if os.path.exists(path):
        ck = torch.load(path, map_location=lambda storage, loc: storage.cuda(gpu_id), weights_only=False)
        model.load_state_dict(ck['state_dict'])
        model.reg_params = ck['reg_params']
        model = model.cuda(gpu_id)
        if 'list_splits' in ck and 'list_bias_layers' in ck:      # BiC checkpoints (train_bic.py:317-326)
            model.list_splits = list(ck['list_splits'])
            model.list_bias_layers = [_bias_layer(model.device, sd) for sd in ck['list_bias_layers']]
    return model


def _bias_layer(device, state=None):
    """a frozen BiasLayer on `device` (train_bic.py:244-248), optionally with a checkpoint's alpha / beta"""
    from .modeling.meta_archs import BiasLayer
    layer = BiasLayer()
    if state is not None:
        layer.load_state_dict(state)
    layer.to(device)
    for p in layer.parameters():
        p.requires_grad = False
    return layer


def memory_quota(memory_size, n_classes):
    """videos kept per class after a task (train_cl.py:343-349)"""
    return 'ALL' if memory_size == 'ALL' else memory_size // n_classes


@torch.no_grad()
def cache_prev_logits(model, loader, task_id, as_numpy=False, kind='sigmoid'):
    """{video_id: [sigmoid(cls logits) per pyramid level]} of the incoming model (train_cl.py:226-235): the distillation
    targets of iCaRL.  They stay ON THE DEVICE (one buffer per clip, its levels views of it; the reference round-trips them
    through numpy and uploads them again in every iteration, meta_archs.py:1492,1508); as_numpy=True gives the
    reference's format.  kind='softmax_T2': softmax(logits[:, :n_known] / 2) instead, the targets of BiC's distillation
    term (train_bic.py:241), which multiplies them with a log-softmax."""
    if kind not in ('sigmoid', 'softmax_T2'):
        raise ValueError("kind must be 'sigmoid' or 'softmax_T2', not %r" % (kind,))
    out = {}
    for video_list in loader:
        cls_logits, _, _ = model(video_list, task_id=task_id, get_emb=True)
        for i, v in enumerate(video_list):
            if kind == 'softmax_T2':
                probs = [torch.softmax(lvl[i][:, :model.n_known] / 2, dim=1) for lvl in cls_logits]
            else:
                probs = [torch.sigmoid(lvl[i]) for lvl in cls_logits]
            # a clip's levels are views of ONE contiguous [sum T_l, .] buffer: the distillation kernel (ops.cl_distill) and a
            # replayed step's input slot (StepInputs.dist_tgt) take it as it is
            buf = torch.cat(probs, dim=0).contiguous()
            probs = list(buf.split([int(t.shape[0]) for t in probs], dim=0))
            out[v['video_id']] = [np.array(t.cpu().numpy()) for t in probs] if as_numpy else probs
    return out


def _barrier(reducer):
    if reducer is not None:
        import torch.distributed as dist
        dist.barrier(group=reducer.group)


def make_mq_validate(cfg, val_stream, evaluator, retrieval_eval=None, idx_classes=None, logger=None, print_freq=100):
    """The `validate(model, epoch, task)` callback of `run_episodes` as the reference's driver validates
    (train_cl.py:210, :291): `valid_one_epoch_cl_single_gpu` over the tasks learnt so far, its mAP as the metric.
    cfg['test_cfg']['ext_score_file'] (external classification scores, utils/postprocessing.py) is passed through."""
    from .utils import train_utils as tu
    ext_score_file = cfg.get('test_cfg', {}).get('ext_score_file')

    def validate(model, epoch, task):
        ret = tu.valid_one_epoch_cl_single_gpu(val_stream, model, epoch, task, ext_score_file=ext_score_file,
                                               evaluator=evaluator, logger=logger, print_freq=print_freq,
                                               dataset_name=cfg.get('dataset_name', 'ego4d_cl'),
                                               retrieval_eval=retrieval_eval, idx_classes=idx_classes)
        model.train()
        return ret[4]

    return validate


def _make_graph(use_graph, cfg, model, optimizer, reducer=None):
    """a fresh GraphedStep for `optimizer` (new parameters, new optimizer: an old task's graphs are dropped), or None"""
    if not use_graph:
        return None
    from .graph import GraphedStep
    return GraphedStep(model, optimizer, clip_grad_l2norm=cfg['train_cfg']['clip_grad_l2norm'], reducer=reducer)


def _save_memory_and_reload(cfg, model, hooks, j, ckpt_folder, ck_name, gpu_id, is_main=True, reducer=None):
    """With a folder: the main rank pickles the replay memory and lets the methods write their state next to it (save_state),
    then EVERY rank reloads the task's best state (train_cl.py:363 runs on every rank): replicas that kept their last-epoch
    weights would never meet the others again -- the gradient average does not re-align weights.  -> the model"""
    if ckpt_folder is None:
        return model
    if is_main:
        os.makedirs(ckpt_folder, exist_ok=True)
        with open(os.path.join(ckpt_folder, cfg['cl_cfg']['path_memory']), 'wb') as h:
            pickle.dump(model.memory, h)
        each(hooks, 'save_state', j, model, ckpt_folder)
    _barrier(reducer)          # the checkpoint rank 0 wrote is complete before anybody reads it
    return load_best_checkpoint(model, ckpt_folder, ck_name, j, gpu_id)


def run_episodes(cfg, model, train_stream, validate=None, ckpt_folder=None, gpu_id=0, start_task=0, start_epoch=0,
                 combine_train=False, reducer=None, logger=None, print_freq=20, on_step_history=None, use_graph=False,
                 keep_history=True):
    """cfg: the merged config dict (opt / train_cfg / cl_cfg as in libs/core/config.py).
    validate(model, epoch, task) -> mAP-like float (higher is better), or None to skip validation (every epoch's
    state then counts as "best", so the last epoch is what gets reloaded).  `validate` must be RANK-LOCAL (no
    collectives): inside the epoch loop only the main rank calls it (train_cl.py:283), the others wait at a barrier.
    use_graph: replay the iterations as hipGraphs (vilco_amd/graph.py; a fresh GraphedStep per optimizer, i.e. per task).
    keep_history: keep every iteration's loss dict (device scalars) in the log; off for long runs.
    cfg['cl_cfg'] names the continual-learning method; what it does and where is in cl_methods/hooks.py (which methods this
    driver runs, and which with a reducer: hooks.SUPPORT).  Every method's options are validated, and resume state read, before
    the model or the stream is used for anything else.
    Returns (model, optimizer, scheduler, log) with log = list of per-task dicts."""
    is_main = int(os.environ.get("LOCAL_RANK", "0")) == 0
    hooks = make_hooks(cfg, 'run_episodes', reducer)
    each(hooks, 'begin_run', model, train_stream, start_task, start_epoch, ckpt_folder)
    optimizer = make_optimizer(model, cfg['opt'])
    graph = _make_graph(use_graph, cfg, model, optimizer, reducer)
    it = iter(train_stream)
    num_tasks = train_stream.num_tasks
    data, loader, num_next = next(it)
    iters_per_epoch = len(loader)
    scheduler = make_scheduler(optimizer, cfg['opt'], iters_per_epoch)
    max_epochs = cfg['opt'].get('early_stop_epochs', cfg['opt']['epochs'] + cfg['opt']['warmup_epochs'])
    memory_size = cfg['cl_cfg']['memory_size']
    log = []
    for j in range(start_task, num_tasks):
        if j != 0:
            data, loader, num_next = next(it)
        entry = {'task': j, 'init_metric': None, 'best_metric': None, 'best_epoch': -1, 'history': []}
        if validate is not None:
            entry['init_metric'] = validate(model, 0, j)
        best, best_epoch = -10000.0, -1
        prev_logits = cache_prev_logits(model, loader, j) if model.type_sampling == 'icarl' else {}
        ck_name = 'best_task_{:03d}_performance.pth.tar'.format(j)
        extra = {}          # what a method adds to train_one_epoch's arguments (A-GEM: agem=)
        for kw in each(hooks, 'begin_task', j, model, optimizer, loader, entry, keep_history):
            extra.update(kw or {})
        for epoch in range(start_epoch, max_epochs):
            sampler = getattr(loader, 'sampler', None)
            if sampler is not None and hasattr(sampler, 'set_epoch'):
                sampler.set_epoch(epoch)
            if model.use_adapt:
                model.pre_train_epoch(task_id=j, current_epoch=epoch)
            hist = train_one_epoch(loader, model, optimizer, scheduler, epoch, 1, model_ema=None,
                                   clip_grad_l2norm=cfg['train_cfg']['clip_grad_l2norm'], print_freq=print_freq,
                                   logger=logger, cl_name=cfg['cl_cfg']['name'], reg_lambda=cfg['cl_cfg']['reg_lambda'],
                                   prev_out_cls_logits_dict=prev_logits, current_task_id=j, reducer=reducer, graph=graph,
                                   keep_history=keep_history or on_step_history is not None, **extra)
            if keep_history:
                entry['history'].append(hist)
            if on_step_history is not None:
                on_step_history(j, epoch, hist)
            if combine_train or epoch < max_epochs // 3:
                continue
            if is_main:
                metric = validate(model, epoch, j) if validate is not None else float(epoch)
                if metric > best:
                    best, best_epoch = metric, epoch
                    if ckpt_folder is not None:
                        save_checkpoint({'task': j, 'epoch': epoch, 'state_dict': model.state_dict(),
                                         'scheduler': scheduler.state_dict(), 'optimizer': optimizer.state_dict(),
                                         'reg_params': model.reg_params}, file_folder=ckpt_folder, file_name=ck_name)
            _barrier(reducer)          # the other ranks do not run ahead into the next epoch's collectives while rank 0
                                       # validates and writes the checkpoint
        entry['best_metric'], entry['best_epoch'] = best, best_epoch
        each(hooks, 'end_training', j, model, optimizer, num_next is not None)

        # replay memory for the next task (train_cl.py:343-361)
        if memory_size != 0:
            model.add_samples_to_mem(train_stream, data, memory_quota(memory_size, model.cls_head.cls_head.conv.out_channels))
        train_stream.memory = model.memory
        model.n_known = len(model.memory)
        model = _save_memory_and_reload(cfg, model, hooks, j, ckpt_folder, ck_name, gpu_id, is_main, reducer)
        each(hooks, 'after_reload', j, model, entry)
        if validate is not None:
            entry['final_metric'] = validate(model, max_epochs - 1, j)
        log.append(entry)

        if num_next is not None:
            model.augment_classification(num_next, torch.device('cuda', gpu_id))
            each(hooks, 'before_next_task', j, model, optimizer, loader, gpu_id)
            optimizer = make_optimizer(model, cfg['opt'])
            scheduler = make_scheduler(optimizer, cfg['opt'], iters_per_epoch)
            if reducer is not None:
                reducer.rebuild()          # the class head and the gaussian parameters are new tensors
            graph = _make_graph(use_graph, cfg, model, optimizer, reducer)
    return model, optimizer, scheduler, log


def run_episodes_bic(cfg, model, train_stream, validate=None, ckpt_folder=None, gpu_id=0, combine_train=False,
                     stage2_epochs=None, stage2_lr=0.001, logger=None, print_freq=20, keep_history=True, use_graph=False):
    """The episode loop of BiC (cl_cfg.name = 'bic'; MQ/train_bic.py:210-760) in its order of events, through the pieces
    of `run_episodes`.  train_stream: `utils.cl_stream.InMemoryBiCStream`'s contract, next() -> (data, stage-1 loader,
    held-out loader or None, num_next_classes).  Per task j:

      a frozen BiasLayer is appended and list_splits grows by num_classes                     (:244-249, :414-419)
      n_known > 0: the distillation targets softmax(logits[:, :n_known] / 2) are cached       (:231-242, :423-435)
      stage 1: train_one_epoch over the stage-1 loader, validation after the first third of the epochs, best
          checkpoint -- with list_splits and every bias layer's alpha / beta                   (:441-549)
      replay memory, n_known, reload of the best checkpoint, final validation                  (:551-576)
      j >= 1, stage 2: the newest layer's alpha, beta are fitted on the held-out clips with everything else frozen --
          `cl_methods.bic.BiCCache.build` once, then `fit_bias_layer` (one device call for all epochs; the reference
          runs a model forward and backward per step and never steps its bias optimizer, :602-649);
          the parameters are printed as `printParam` does (:624-625), the model is validated with the corrected head
          and the checkpoint is written again so that it carries the fitted layer
      if another task follows: augment_classification, a NEW optimizer and scheduler           (:578-599)

    stage2_epochs: epochs of stage 2 (default: as many as stage 1, as in the reference); stage2_lr: its SGD learning rate
    (:622).  use_graph: replay the stage-1 iterations as hipGraphs, as in `run_episodes` (a fresh GraphedStep per optimizer,
    i.e. per task; from the second task on the captured step holds the bias correction, ops.bic_correct, which reads alpha /
    beta from the layers' memory).  Single process (the reference's stage 2 is not data parallel either).  Returns (model, optimizer, scheduler,
    log); a task's log entry has 'bic' = {'alpha', 'beta', 'before', 'after', 'losses'} after a stage 2.
    The methods this driver refuses (ValueError), and those it runs without their hooks: cl_methods/hooks.py, SUPPORT."""
    from .cl_methods.bic import BiCCache, fit_bias_layer, newest_split
    from .utils.cl_stream import DistributedBatchLoader
    hooks = make_hooks(cfg, 'run_episodes_bic')          # refuses what SUPPORT does; no method has hooks in this driver
    optimizer = make_optimizer(model, cfg['opt'])
    graph = _make_graph(use_graph, cfg, model, optimizer)
    it = iter(train_stream)
    num_tasks = train_stream.num_tasks
    max_epochs = cfg['opt'].get('early_stop_epochs', cfg['opt']['epochs'] + cfg['opt']['warmup_epochs'])
    memory_size = cfg['cl_cfg']['memory_size']
    scheduler, log = None, []

    def checkpoint(j, epoch, name):
        save_checkpoint({'task': j, 'epoch': epoch, 'state_dict': model.state_dict(), 'scheduler': scheduler.state_dict(),
                         'optimizer': optimizer.state_dict(), 'reg_params': model.reg_params,
                         'list_splits': list(model.list_splits),
                         'list_bias_layers': [{k: v.detach().cpu() for k, v in b.state_dict().items()}
                                              for b in model.list_bias_layers]}, file_folder=ckpt_folder, file_name=name)

    def every_clip(ld):
        """every clip of a loader once, in dataset order (a training loader shuffles and drops a short last batch)"""
        items = getattr(ld, 'items', None)
        return ld if items is None else DistributedBatchLoader(items, ld.batch_size, shuffle=False, drop_last=False)

    for j in range(num_tasks):
        data, loader, held, num_next = next(it)
        if scheduler is None:
            scheduler = make_scheduler(optimizer, cfg['opt'], len(loader))
        entry = {'task': j, 'init_metric': None, 'best_metric': None, 'best_epoch': -1, 'history': []}
        if validate is not None:
            entry['init_metric'] = validate(model, 0, j)
        model.list_bias_layers.append(_bias_layer(model.device))
        model.list_splits.append(model.num_classes)
        prev_logits = cache_prev_logits(model, every_clip(loader), j, kind='softmax_T2') if model.n_known > 0 else {}
        best, best_epoch = -10000.0, -1
        ck_name = 'best_task_{:03d}_performance.pth.tar'.format(j)
        for epoch in range(max_epochs):
            loader.sampler.set_epoch(epoch)
            hist = train_one_epoch(loader, model, optimizer, scheduler, epoch, 1, model_ema=None,
                                   clip_grad_l2norm=cfg['train_cfg']['clip_grad_l2norm'], print_freq=print_freq,
                                   logger=logger, cl_name=cfg['cl_cfg']['name'], reg_lambda=cfg['cl_cfg']['reg_lambda'],
                                   prev_out_cls_logits_dict=prev_logits, current_task_id=j, graph=graph,
                                   keep_history=keep_history)
            if keep_history:
                entry['history'].append(hist)
            if combine_train or epoch < max_epochs // 3:
                continue
            metric = validate(model, epoch, j) if validate is not None else float(epoch)
            if metric > best:
                best, best_epoch = metric, epoch
                if ckpt_folder is not None:
                    checkpoint(j, epoch, ck_name)
        entry['best_metric'], entry['best_epoch'] = best, best_epoch

        if memory_size != 0:
            model.add_samples_to_mem(train_stream, data, memory_quota(memory_size, model.cls_head.cls_head.conv.out_channels))
        train_stream.memory = model.memory
        model.n_known = len(model.memory)
        model = _save_memory_and_reload(cfg, model, hooks, j, ckpt_folder, ck_name, gpu_id)
        if validate is not None:
            entry['final_metric'] = validate(model, max_epochs - 1, j)

        if held is not None:
            cache = BiCCache.build(model, every_clip(held), j)
            lo, hi = newest_split(model)
            layer = model.list_bias_layers[-1]
            before = cache.eval(lo, hi, float(layer.alpha), float(layer.beta))
            losses = fit_bias_layer(model, cache, max_epochs if stage2_epochs is None else stage2_epochs,
                                    getattr(held, 'batch_size', 1), lr=stage2_lr, seed=getattr(held, 'seed', 0))
            after = cache.eval(lo, hi, float(layer.alpha), float(layer.beta))
            for i, b in enumerate(model.list_bias_layers):
                b.printParam(i)
            entry['bic'] = {'alpha': float(layer.alpha), 'beta': float(layer.beta), 'before': before.tolist(),
                            'after': after.tolist(), 'losses': losses, 'n_clips': cache.n_clips}
            print('BiC stage 2, task %d: held-out focal loss %.6f -> %.6f over %d clips, %d steps'
                  % (j, entry['bic']['before'][0], entry['bic']['after'][0], cache.n_clips, losses.numel()))
            if validate is not None:
                entry['bic_metric'] = validate(model, max_epochs - 1, j)
            if ckpt_folder is not None:
                checkpoint(j, best_epoch, ck_name)
        log.append(entry)

        if num_next is not None:
            model.augment_classification(num_next, torch.device('cuda', gpu_id))
            optimizer = make_optimizer(model, cfg['opt'])
            scheduler = make_scheduler(optimizer, cfg['opt'], len(loader))
            graph = _make_graph(use_graph, cfg, model, optimizer)
    return model, optimizer, scheduler, log


class StickyBest:
    """Which epochs write 'Best_task_XX' in the NLQ driver (NLQ/train_cl.py:216-292).  `is_best = R1 >= best_R1` is assigned
    only at validated epochs (:250) but the save block tests it at EVERY epoch (:283), and nothing resets it between epochs or
    tasks: after a validated epoch that reached the bar every following epoch overwrites the file until a validation misses.
    (The reference leaves is_best undefined before the first validation; epoch 0 validates whenever ckpt_freq > 0.)"""

    def __init__(self):
        self.is_best = False
        self.best = None
        self.best_epoch = -1

    def new_task(self, init_r1):
        self.best, self.best_epoch = init_r1, -1          # (is_best carries over, as in the reference)

    def validated(self, epoch, r1):
        self.is_best = r1 >= self.best
        if self.is_best:
            self.best, self.best_epoch = r1, epoch

    @staticmethod
    def validates(epoch, max_epochs, ckpt_freq):
        return epoch == max_epochs - 1 or (ckpt_freq > 0 and epoch % ckpt_freq == 0)


def run_episodes_nlq(cfg, model, train_stream, val_stream, evaluator, ckpt_folder=None, gpu_id=0, start_task=0,
                     start_epoch=0, ckpt_freq=2, reducer=None, print_freq=100, use_graph=False, keep_history=True,
                     on_validate=None):
    """Episode loop of the NLQ driver (BASELINE configs[3]; NLQ/train_cl.py:113-342), which differs from the MQ loop in
    what surrounds the training iterations:

      optimizer: NLQ's make_optimizer, with the head / backbone learning-rate groups when opt.backbone_lr_weight != 1
          (:115-118), created anew for every task (:331-336); the scheduler keeps the FIRST task's iterations per epoch (:123)
      per task j: R@1 of the incoming model over templates 0..j (:181-183) is the bar the epochs have to reach
          (is_best = R1 >= best_R1, :265); validation after epoch e when e is the last one or e % ckpt_freq == 0 (:216-222);
          the best state goes to 'Best_task_{j:02d}.pth.tar' (keys epoch / state_dict / scheduler / optimizer / current_task /
          reg_params, :269-276)
      replay memory: m = memory_size // 13 queries per template (:293-299 -- 13 is the benchmark's template count,
          hard-wired there), add_samples_to_mem, stream.memory = model.memory, n_known = j + 1 (:303-308), memory pickle
      reload of the task's best checkpoint (:315), final validation over all learnt templates (:317-318), and -- when
          another task follows -- EWC / MAS consolidation (:325-329); no class-head growth (one query class)

    val_stream: `get_valSet_by_taskNum(n)` -> [(loader with batch size 1, #templates), ...] (cl_benchmark.py:60-74);
    evaluator: `.dataset`, `.evaluate(records, verbose) -> (performance[[R@1, ...]], str)` (libs/utils/metrics.py
    ReferringRecall; outside the hot path).  on_validate(kind, task, epoch, r1) is called after every validation.
    The methods this driver runs and those it refuses (ValueError): cl_methods/hooks.py, SUPPORT.
    Returns (model, optimizer, scheduler, log)."""
    from .utils import train_utils_nlq as tu
    is_main = int(os.environ.get("LOCAL_RANK", "0")) == 0
    hooks = make_hooks(cfg, 'run_episodes_nlq', reducer)
    each(hooks, 'begin_run', model, train_stream, start_task, start_epoch, ckpt_folder)

    def new_optimizer():
        return tu.make_optimizer(model, cfg['opt'], head_backbone_group=cfg['opt']["backbone_lr_weight"] != 1)

    optimizer = new_optimizer()
    graph = _make_graph(use_graph, cfg, model, optimizer, reducer)
    it = iter(train_stream)
    num_tasks = train_stream.num_tasks
    data, loader, num_next = next(it)
    iters_per_epoch = len(loader)
    scheduler = tu.make_scheduler(optimizer, cfg['opt'], iters_per_epoch)
    max_epochs = cfg['opt'].get('early_stop_epochs', cfg['opt']['epochs'] + cfg['opt']['warmup_epochs'])
    memory_size = cfg['cl_cfg']['memory_size']
    recalls = {'val': [], 'test': []}
    log = []
    tracker = StickyBest()

    def validate(kind, j, epoch):
        fn = tu.final_validate if kind == 'final' else tu.valid_one_epoch_cl_single_gpu
        kw = dict(list_val_recall_ii=recalls, type_val='val') if kind == 'final' else {}
        r1 = fn(val_stream, model, epoch, j, evaluator=evaluator, print_freq=print_freq, **kw)
        model.train()
        if on_validate is not None:
            on_validate(kind, j, epoch, r1)
        return r1

    for j in range(start_task, num_tasks):
        if j != 0:
            data, loader, num_next = next(it)
        entry = {'task': j, 'history': [], 'R1': []}
        entry['init_R1'] = validate('init', j, 0)
        tracker.new_task(entry['init_R1'])
        prev_logits = cache_prev_logits(model, loader, j, as_numpy=True) if model.type_sampling == 'icarl' else {}
        ck_name = 'Best_task_{:02d}.pth.tar'.format(j)
        each(hooks, 'begin_task', j, model, optimizer, loader, entry, keep_history)      # a new optimizer per task: attached again
        for epoch in range(start_epoch, max_epochs):
            sampler = getattr(loader, 'sampler', None)
            if sampler is not None and hasattr(sampler, 'set_epoch'):
                sampler.set_epoch(epoch)
            if model.use_adapter:
                model.pre_train_epoch(task_id=j, current_epoch=epoch)
            hist = tu.train_one_epoch(loader, model, optimizer, scheduler, epoch, model_ema=None,
                                      clip_grad_l2norm=cfg['train_cfg']['clip_grad_l2norm'], print_freq=print_freq,
                                      cl_name=cfg['cl_cfg']['name'], reg_lambda=cfg['cl_cfg']['reg_lambda'],
                                      prev_out_cls_logits_dict=prev_logits, current_task_id=j, reducer=reducer, graph=graph,
                                      keep_history=keep_history)
            if keep_history:
                entry['history'].append(hist)
            validated = StickyBest.validates(epoch, max_epochs, ckpt_freq)
            if validated:
                r1 = validate('epoch', j, epoch)
                entry['R1'].append((epoch, r1))
                tracker.validated(epoch, r1)
            # The reference's save block sits OUTSIDE the validation `if` and `is_best` is sticky (StickyBest): with ckpt_freq = 2
            # the checkpoint reloaded for final validation, memory selection and the next task is one (unvalidated) epoch newer
            # than the best validated one.  Reproduced here; `saved_epoch` records which epoch the file holds.
            is_best = tracker.is_best
            if is_best:
                entry['saved_epoch'] = epoch
                if is_main and ckpt_folder is not None:
                    save_checkpoint({'epoch': epoch, 'state_dict': model.state_dict(), 'scheduler': scheduler.state_dict(),
                                     'optimizer': optimizer.state_dict(), 'current_task': j, 'reg_params': model.reg_params},
                                    file_folder=ckpt_folder, file_name=ck_name)
            if validated or is_best:
                _barrier(reducer)
        entry['best_R1'], entry['best_epoch'] = tracker.best, tracker.best_epoch
        each(hooks, 'end_training', j, model, optimizer, num_next is not None)
        if memory_size != 0:
            model.add_samples_to_mem(val_stream, data, 'ALL' if memory_size == 'ALL' else memory_size // 13)
        train_stream.memory = model.memory
        model.n_known = j + 1
        model = _save_memory_and_reload(cfg, model, hooks, j, ckpt_folder, ck_name, gpu_id, is_main, reducer)
        each(hooks, 'after_reload', j, model, entry)
        entry['final_R1'] = validate('final', j, max_epochs - 1)
        log.append(entry)
        if num_next is not None:
            each(hooks, 'before_next_task', j, model, optimizer, loader, gpu_id)
            optimizer = new_optimizer()
            scheduler = tu.make_scheduler(optimizer, cfg['opt'], iters_per_epoch)
            graph = _make_graph(use_graph, cfg, model, optimizer, reducer)
    return model, optimizer, scheduler, log
