"""What a continual-learning method does at the six points of an episode at which the drivers of train_cl.py let one act.
The points are the methods of `Hook`, in the order in which a driver reaches them.

A driver calls every point on every member of `make_hooks(cfg, driver, reducer)`: the named method first, CODA second.
SUPPORT says which method runs where."""
import os

import torch

from . import ace as ace_mod, agem as agem_mod, coda as coda_mod, der as der_mod, erd as erd_mod, pod as pod_mod, regularizers

DER_BANK_FILE = 'der_bank.pt'      # cl_cfg.name 'der': DERBank.state_dict(), written next to the memory pickle
RWALK_STATE_FILE = 'rwalk_state.pt'      # cl_cfg.name 'rwalk': regularizers.rwalk_state_dict(), written next to the memory pickle

MQ, NLQ, BIC = 'run_episodes', 'run_episodes_nlq', 'run_episodes_bic'
HOOKS = 'hooks'      # the driver calls the method's hooks
PENALTY_ONLY = 'penalty only'      # no hook is called: train_one_epoch applies the penalty if model.reg_params is populated (by
#                                    a checkpoint, say), and nothing consolidates -- the dictionary never changes
# method -> ({driver: what it gives the method}, whether the method accepts a reducer, i.e. data parallelism).  A driver that is
# not listed refuses the method by name, as does run_episodes with a reducer that is not accepted: agem / der / pod / erd / coda
# .check_supported read their rows and say why, make_hooks reads RWalk's.  'coda' is cl_cfg.prompt_type under cl_cfg.prompt_pool,
# the others are cl_cfg.name; a name that is not here (None, 'icarl', 'bic', ...) has no hooks and runs everywhere.
SUPPORT = {
    'ewc': ({MQ: HOOKS, NLQ: HOOKS, BIC: PENALTY_ONLY}, True),
    'mas': ({MQ: HOOKS, NLQ: HOOKS, BIC: PENALTY_ONLY}, True),
    'si': ({MQ: HOOKS, NLQ: HOOKS, BIC: PENALTY_ONLY}, True),
    'rwalk': ({MQ: HOOKS, NLQ: HOOKS}, True),
    'agem': ({MQ: HOOKS}, False),
    'der': ({MQ: HOOKS}, False),      # (nor with type_sampling 'icarl': der.check_supported)
    'coda': ({MQ: HOOKS}, False),
}
# rows of the same shape for the methods added after tests/test_cl_hooks_cpu.py listed SUPPORT's keys one by one: SUPPORT itself keeps
# that list, `support(name)` reads both tables
SUPPORT_MORE = {
    'pod': ({MQ: HOOKS}, False),      # (nor with type_sampling 'icarl' or start_epoch > 0: pod.check_supported)
    'erd': ({MQ: HOOKS}, False),      # (likewise: erd.check_supported)
    'er_ace': ({MQ: HOOKS}, False),      # (NLQ has one query class, BiC trains its own loss: ace.check_supported)
}


def support(name):
    """the row of `name` in SUPPORT or SUPPORT_MORE (KeyError: the method has no row and runs everywhere)"""
    return SUPPORT[name] if name in SUPPORT else SUPPORT_MORE[name]


def _resume_file(what, start_task, ckpt_folder, name, holds):
    """the path of a method's resume state in `ckpt_folder` -- or ValueError: a resume at a later task cannot do without"""
    path = None if ckpt_folder is None else os.path.join(ckpt_folder, name)
    if path is None or not os.path.exists(path):
        raise ValueError("cl_cfg.name %r resumed at task %d needs %s (%s, written next to the memory pickle after every task): "
                         "none found" % (what, start_task, holds, path or name))
    return path


class Hook:
    """A method that does nothing: the base of the classes below, which override the points at which they act."""

    def __init__(self, cfg, reducer=None):
        self.cl_cfg, self.reducer = cfg['cl_cfg'], reducer

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        """Once, before the first optimizer is built: options are validated, a combination or a resume the method cannot
        serve is refused, resume state is read from ckpt_folder.  Nothing but that touches the model or the stream here."""

    def begin_task(self, j, model, optimizer, loader, entry, keep_history=True):
        """The incoming model's outputs are cached, task j's optimizer exists, its epochs have not started.
        -> None, or keyword arguments this task's train_one_epoch calls get on top of the driver's"""

    def end_training(self, j, model, optimizer, has_next):
        """Right after the epoch loop: the model is where training left it -- the memory is not updated, the best checkpoint
        not reloaded.  has_next: another task follows."""

    def save_state(self, j, model, ckpt_folder):
        """Main rank only, with a folder only: next to the memory pickle, before the barrier and the reload."""

    def after_reload(self, j, model, entry):
        """The memory is final for the task, the best checkpoint is back, the head has not grown; the final validation
        follows."""

    def before_next_task(self, j, model, optimizer, loader, gpu_id):
        """Only when a task follows: the head has grown (MQ; NLQ has one query class), `optimizer` and `loader` are still
        task j's, the next optimizer is built right after."""


class Importance(Hook):
    """cl_cfg.name 'ewc' / 'mas': the importance of the task just learnt, over its loader, from the reloaded best state with the
    head already grown -- reduced over the reducer's group when the run is data parallel.  (make_hooks validated the options.)"""

    def before_next_task(self, j, model, optimizer, loader, gpu_id):
        model.reg_params = regularizers.on_task_update(loader, gpu_id, optimizer, model, kind=self.cl_cfg['name'],
                                                       group=getattr(self.reducer, 'group', None),
                                                       data_parallel=self.reducer is not None,
                                                       **regularizers.importance_options(self.cl_cfg))


class SI(Hook):
    """cl_cfg.name 'si' (Synaptic Intelligence): the path integral is attached to every task's optimizer; the consolidation runs
    where the task's training ends, from the state the integral led to, BEFORE the best checkpoint is reloaded and without a pass
    over the data.  The reload restores the checkpoint's older dictionary, so the new one is held and installed after it.  A
    resume inside a task is refused: the integral of the epochs already trained is per-task state (model.si_state) that
    checkpoints do not carry."""
    held = None

    options = staticmethod(regularizers.si_xi)

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        self.opts = self.options(self.cl_cfg)
        if start_epoch > 0:
            raise ValueError("cl_cfg.name %r cannot resume inside a task (start_epoch = %d): the path integral of the epochs "
                             "already trained is not checkpointed; resume at a task boundary" % (self.cl_cfg['name'], start_epoch))

    def begin_task(self, j, model, optimizer, loader, entry, keep_history=True):
        regularizers.si_begin_task(model, optimizer)      # the head has grown, this task's optimizer exists

    def consolidate(self, model, optimizer):
        return regularizers.on_task_si_update(model, optimizer, xi=self.opts)

    def end_training(self, j, model, optimizer, has_next):
        self.held = {k: list(v) for k, v in self.consolidate(model, optimizer).items()} if has_next else None

    def before_next_task(self, j, model, optimizer, loader, gpu_id):
        model.reg_params = self.held


class RWalk(SI):
    """cl_cfg.name 'rwalk': `rwalk_begin_task` and the consolidation where SI's are.  The Fisher average and the path scores
    outlive a task: with ckpt_folder they are written next to the memory pickle at every task boundary (RWALK_STATE_FILE, with
    the importance dictionary the task's checkpoints predate) and start_task > 0 reads them back -- or raises.  Reading the file
    REPLACES model.reg_params, also a dictionary the caller restored from a checkpoint before the call.  omega and theta_ck are
    per-task state: start_epoch > 0 raises as for SI."""

    options = staticmethod(regularizers.rwalk_options)

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        super().begin_run(model, train_stream, start_task, start_epoch, ckpt_folder)
        if start_task > 0:
            path = _resume_file('rwalk', start_task, ckpt_folder, RWALK_STATE_FILE,
                                "the Fisher average and the path scores of the earlier tasks")
            regularizers.load_rwalk_state(model, torch.load(path, map_location='cpu', weights_only=False), device=model.device)

    def begin_task(self, j, model, optimizer, loader, entry, keep_history=True):
        regularizers.rwalk_begin_task(model, optimizer, **self.opts)      # F and s carried on their prefix, tick = 0

    def consolidate(self, model, optimizer):
        return regularizers.on_task_rwalk_update(model, optimizer, eps=self.opts['eps'])

    def save_state(self, j, model, ckpt_folder):
        if self.held is not None:      # another task follows -- F and the halved s: what it starts from
            torch.save(regularizers.rwalk_state_dict(model), os.path.join(ckpt_folder, RWALK_STATE_FILE))


class AGEM(Hook):
    """cl_cfg.name 'agem' (cl_methods/agem.py): from the first task that finds `train_stream.memory` non-empty, every iteration
    takes a reference gradient on a batch of cl_cfg['agem_batch'] (default: the loader's batch size) memory clips -- drawn by a
    MemorySampler seeded with cl_cfg['agem_seed'] (default: the stream's seed) -- and projects the task batch's gradient against
    it before the clip and the update; before that, training is plain.  A fresh agem.AGEM per task; with keep_history the
    task's log entry gets 'agem' = [out, ...], one device tensor {g.r, r.r, alpha} per iteration.  A-GEM proper wants a stream
    built with train_enable=False, whose task loader does not mix the memory in; with train_enable=True the method is replay
    plus projection.  With use_graph the task batch's step replays as usual and the reference pass stays eager between the
    replays."""

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        agem_mod.check_supported('agem', self.reducer)
        self.stream = train_stream

    def begin_task(self, j, model, optimizer, loader, entry, keep_history=True):
        if not self.stream.memory:
            return None
        sampler = agem_mod.MemorySampler(self.stream.memory, self.cl_cfg.get('agem_batch', loader.batch_size),
                                         self.cl_cfg.get('agem_seed', getattr(self.stream, 'seed', 0)))
        agem = agem_mod.AGEM(model, sampler, trace=[] if keep_history else None)
        if keep_history:
            entry['agem'] = agem.trace
        return {'agem': agem}


class DER(Hook):
    """cl_cfg.name 'der' (cl_methods/der.py): at the end of every task -- memory final, best checkpoint reloaded, head not yet
    grown, so the model is the one the next task starts from -- the clips that entered the memory get their logits recorded in
    `model.der_bank`, evicted clips lose their record and older records stay as they are.  From the next task on every step adds
    cl_cfg['der_alpha'] times the mean squared distance between the memory clips' logits and their records ('der_loss' in the
    loss dict; ops.der_replay, part of a replayed step).  A stream built with train_enable=True gives DER++ (the memory clips'
    labels are in the detection loss); with train_enable=False no memory clip reaches a batch and the term is zero.  With
    ckpt_folder the bank is written next to the memory pickle (DER_BANK_FILE) and start_task > 0 reads it back -- or raises."""

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        der_mod.check_supported('der', self.reducer, type_sampling=self.cl_cfg.get('type_sampling'))
        self.folder = ckpt_folder
        model.der_alpha = float(self.cl_cfg.get('der_alpha', model.der_alpha))
        if getattr(model, 'der_bank', None) is None:
            model.der_bank = der_mod.DERBank()
        if start_task > 0:
            path = _resume_file('der', start_task, ckpt_folder, DER_BANK_FILE, "the recorded logits of the memory")
            model.der_bank.load_state_dict(torch.load(path, map_location='cpu', weights_only=False), device=model.device)

    def after_reload(self, j, model, entry):
        bank = model.der_bank
        entry['der_dropped'] = bank.drop_missing(model.memory)
        entry['der_recorded'] = der_mod.record_memory(model, bank, model.memory, j)
        if self.folder is not None and int(os.environ.get("LOCAL_RANK", "0")) == 0:
            torch.save(bank.state_dict(), os.path.join(self.folder, DER_BANK_FILE))


class POD(Hook):
    """cl_cfg.name 'pod' (cl_methods/pod.py): at the START of every task with known classes -- the incoming model is intact: the
    best checkpoint of the previous task, head grown, no step taken -- `model.pod_bank` is cleared and every clip the task's loader
    yields (the task's own clips and, with train_enable=True, the memory's) gets the pooled, normalised pyramid of that model
    recorded.  Every step of the task then adds PODNet's feature distillation against those records ('pod_loss' in the loss
    dict; ops.pod_distill, part of a replayed step), weighted cl_cfg['pod_lambda'] * sqrt(n_classes / new classes).  The cost
    is ONE inference pass over the task's clips per task (the task's log entry gets 'pod_recorded' = the number of records).
    No state file: a resume at a task boundary rebuilds the records from the reloaded model; a resume inside a task
    (start_epoch > 0) raises, because the incoming model is gone by then.  A loader that re-crops a long clip differently
    from epoch to epoch leaves that clip without a usable record in the epochs whose crop differs (PODBank.skipped)."""

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        pod_mod.check_supported('pod', self.reducer, type_sampling=self.cl_cfg.get('type_sampling'), start_epoch=start_epoch)
        lam = float(self.cl_cfg.get('pod_lambda', model.pod_lambda))
        if not lam >= 0.0 or lam == float('inf'):
            raise ValueError("cl_cfg.pod_lambda must be a finite number >= 0, got %r" % (self.cl_cfg.get('pod_lambda'),))
        model.pod_lambda = lam
        if getattr(model, 'pod_bank', None) is None:
            model.pod_bank = pod_mod.PODBank()

    def begin_task(self, j, model, optimizer, loader, entry, keep_history=True):
        if model.n_known > 0:
            model.pod_bank.clear()
            entry['pod_recorded'] = pod_mod.record_clips(model, model.pod_bank, loader, j)


class ERD(Hook):
    """cl_cfg.name 'erd' (cl_methods/erd.py): at the START of every task with known classes -- where POD records, from the same
    intact incoming model and with the same loader walk -- `model.erd_bank` is cleared and every clip the task's loader yields
    gets the positions selected at which that model answers confidently (per clip, above mean + alpha * std of the clip's
    responses) and their logits over the known classes and finished offsets recorded.  Every step of the task then holds the new
    model's logits and boundaries to the records at those positions ('erd_loss' = 'erd_cls_loss' + 'erd_reg_loss' in the loss
    dict; ops.erd_distill, part of a replayed step).  The cost is ONE inference pass over the task's clips per task; the task's
    log entry gets 'erd_recorded' = the number of records and 'erd_bytes' = what they take.  The records of the previous task
    are released only after the new ones are in place.  No state file: a resume at a task boundary re-records from the
    reloaded model; a resume inside a task (start_epoch > 0) raises, because the incoming model is gone by then."""

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        erd_mod.check_supported('erd', self.reducer, type_sampling=self.cl_cfg.get('type_sampling'), start_epoch=start_epoch)
        self.opts = erd_mod.options(self.cl_cfg)
        for k, v in self.opts.items():
            setattr(model, k, v)
        if getattr(model, 'erd_bank', None) is None:
            model.erd_bank = erd_mod.ERDBank()

    def begin_task(self, j, model, optimizer, loader, entry, keep_history=True):
        if model.n_known > 0:
            bank = model.erd_bank
            bank.clear()
            try:
                entry['erd_recorded'], entry['erd_bytes'] = erd_mod.record_clips(model, bank, loader, j, self.opts)
            finally:
                bank.release()      # the previous task's buffers: no table names them any more


class ERACE(Hook):
    """cl_cfg.name 'er_ace' (cl_methods/ace.py): from the first task with known classes the detection loss itself is asymmetric
    -- a clip of the current task is scored over the current task's classes only, a clip of the replay memory over all classes
    (ops.mq_loss_ace, part of a replayed step; the window table is built per batch from the memory's keys).  A stream built with
    train_enable=True replays the memory under full supervision; with train_enable=False the method is the window alone.  The
    hook refuses what ace.check_supported refuses and keeps no state: a resume works at any task or epoch."""

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        ace_mod.check_supported('er_ace', self.reducer)


class Coda(Hook):
    """cl_cfg.prompt_type 'coda' under cl_cfg.prompt_pool (cl_methods/coda.py), alongside any named method: cl_cfg['coda_tasks']
    None is filled from the stream's task count; a model that holds a CodaPrompt must divide its pool among as many tasks as the
    stream has.  Task j's components are (re)drawn at its start -- after the previous task's reload and head growth, before task
    j's optimizer is built (the rows are new values: their moments start at zero); for task 0 that repeats what construction
    did, bit for bit."""

    def begin_run(self, model, train_stream, start_task=0, start_epoch=0, ckpt_folder=None):
        coda_mod.check_supported('coda', self.reducer)
        if self.cl_cfg.get('coda_tasks') is None:
            self.cl_cfg['coda_tasks'] = int(train_stream.num_tasks)
        prompt = getattr(model, 'prompt', None)
        if not isinstance(prompt, coda_mod.CodaPrompt):
            raise ValueError("cl_cfg.prompt_type 'coda': the model holds no CodaPrompt (build it with cl_cfg.coda_tasks = %d)"
                             % self.cl_cfg['coda_tasks'])
        if prompt.n_tasks < train_stream.num_tasks:
            raise ValueError("cl_cfg.prompt_type 'coda': the pool is divided among %d tasks, the stream has %d"
                             % (prompt.n_tasks, train_stream.num_tasks))
        self.draw(model, start_task)

    def draw(self, model, t):
        model.prompt.set_task(t)      # task t's components, before its optimizer exists

    def before_next_task(self, j, model, optimizer, loader, gpu_id):
        self.draw(model, j + 1)


NAMED = {'ewc': Importance, 'mas': Importance, 'si': SI, 'rwalk': RWalk, 'agem': AGEM, 'der': DER, 'pod': POD, 'erd': ERD,
         'er_ace': ERACE}


def each(hooks, point, *args):
    """calls `point` on every hook, in the list's order -> what they returned"""
    return [getattr(hook, point)(*args) for hook in hooks]


def make_hooks(cfg, driver, reducer=None):
    """-> the hook objects of a run of `driver`: [the named method's] + [Coda()], either of which may be missing.  What SUPPORT
    does not let run in `driver` is refused here -- agem, der, pod, erd, er_ace, coda, rwalk in this order; begin_run refuses the rest.  A driver
    that consolidates validates the importance options whatever the method: a bad value fails here, not after the first task."""
    cl_cfg = cfg['cl_cfg']
    name = cl_cfg['name']
    agem_mod.check_supported(name, driver=driver)
    der_mod.check_supported(name, driver=driver)
    pod_mod.check_supported(name, driver=driver)
    erd_mod.check_supported(name, driver=driver)
    ace_mod.check_supported(name, driver=driver)
    coda = bool(cl_cfg.get('prompt_pool')) and coda_mod.check_supported(cl_cfg.get('prompt_type', 'l2p'), driver=driver)
    if name == 'rwalk' and driver not in SUPPORT['rwalk'][0]:
        raise ValueError("cl_cfg.name 'rwalk' is not supported by %s: only run_episodes and run_episodes_nlq keep its state and "
                         "consolidate it" % driver)
    if SUPPORT['ewc'][0][driver] == HOOKS:
        regularizers.importance_options(cl_cfg)
    named = [NAMED[name](cfg, reducer)] if name in NAMED and support(name)[0][driver] == HOOKS else []
    return named + ([Coda(cfg, reducer)] if coda else [])
