"""cl_methods/hooks.py without a GPU: which hook objects a driver gets for which method -- or which refusal -- against a table
written out from the drivers as they were before the hooks existed (their `use_*` lines, `check_supported(..., driver=...)`
calls and the inline RWalk refusal), and what begin_run validates, in which order, on stubs."""
import types

import pytest
import torch

MQ, NLQ, BIC = 'run_episodes', 'run_episodes_nlq', 'run_episodes_bic'

# refusals, by a fragment of their message
A_DRV, D_DRV, C_DRV, R_DRV = "'agem' is not supported by %s", "'der' is not supported by %s", "'coda' is not wired into %s", \
    "'rwalk' is not supported by %s"
A_RED, D_RED, C_RED = "'agem' does not support data parallelism", "'der' does not support data parallelism", \
    "'coda' has not been run with a reducer"
ICARL = "type_sampling 'icarl'"

# (driver, cl_cfg.name) -> the outcome (plain, with a reducer, with a CODA prompt pool, with both): a list of hook class names
# -- what reaches the first make_optimizer -- or the fragment of the ValueError.  'der+icarl' is 'der' with type_sampling
# 'icarl'.  run_episodes: the named method validates (and refuses a reducer) before CODA does.  run_episodes_nlq /
# run_episodes_bic: agem, der, coda are refused in this order, then (bic) rwalk; run_episodes_bic takes no reducer, so one
# handed to make_hooks changes nothing; it consolidates nothing, so 'ewc' / 'mas' / 'si' get no hook there (the penalty alone).
WANT = {
    (MQ, None): ([], [], ['Coda'], C_RED),
    (MQ, 'icarl'): ([], [], ['Coda'], C_RED),
    (MQ, 'bic'): ([], [], ['Coda'], C_RED),
    (MQ, 'ewc'): (['Importance'], ['Importance'], ['Importance', 'Coda'], C_RED),
    (MQ, 'mas'): (['Importance'], ['Importance'], ['Importance', 'Coda'], C_RED),
    (MQ, 'si'): (['SI'], ['SI'], ['SI', 'Coda'], C_RED),
    (MQ, 'rwalk'): (['RWalk'], ['RWalk'], ['RWalk', 'Coda'], C_RED),
    (MQ, 'agem'): (['AGEM'], A_RED, ['AGEM', 'Coda'], A_RED),
    (MQ, 'der'): (['DER'], D_RED, ['DER', 'Coda'], D_RED),
    (MQ, 'der+icarl'): (ICARL, D_RED, ICARL, D_RED),
    (NLQ, None): ([], [], C_DRV, C_DRV),
    (NLQ, 'icarl'): ([], [], C_DRV, C_DRV),
    (NLQ, 'bic'): ([], [], C_DRV, C_DRV),
    (NLQ, 'ewc'): (['Importance'], ['Importance'], C_DRV, C_DRV),
    (NLQ, 'mas'): (['Importance'], ['Importance'], C_DRV, C_DRV),
    (NLQ, 'si'): (['SI'], ['SI'], C_DRV, C_DRV),
    (NLQ, 'rwalk'): (['RWalk'], ['RWalk'], C_DRV, C_DRV),
    (NLQ, 'agem'): (A_DRV, A_DRV, A_DRV, A_DRV),
    (NLQ, 'der'): (D_DRV, D_DRV, D_DRV, D_DRV),
    (NLQ, 'der+icarl'): (D_DRV, D_DRV, D_DRV, D_DRV),
    (BIC, None): ([], [], C_DRV, C_DRV),
    (BIC, 'icarl'): ([], [], C_DRV, C_DRV),
    (BIC, 'bic'): ([], [], C_DRV, C_DRV),
    (BIC, 'ewc'): ([], [], C_DRV, C_DRV),
    (BIC, 'mas'): ([], [], C_DRV, C_DRV),
    (BIC, 'si'): ([], [], C_DRV, C_DRV),
    (BIC, 'rwalk'): (R_DRV, R_DRV, C_DRV, C_DRV),
    (BIC, 'agem'): (A_DRV, A_DRV, A_DRV, A_DRV),
    (BIC, 'der'): (D_DRV, D_DRV, D_DRV, D_DRV),
    (BIC, 'der+icarl'): (D_DRV, D_DRV, D_DRV, D_DRV),
}


def _model():
    from vilco_amd.cl_methods import CodaPrompt
    return types.SimpleNamespace(der_alpha=0.1, der_bank=None, prompt=CodaPrompt(4, 1, 8, 2), device=torch.device('cpu'),
                                 reg_params={})


def _stream():
    return types.SimpleNamespace(num_tasks=2, memory={}, seed=0)


def _begin(cfg, driver, reducer=None, model=None, stream=None, **kw):
    """what a driver does before its first optimizer: the hooks made, every one through begin_run -> the list"""
    from vilco_amd.cl_methods import hooks
    made = hooks.make_hooks(cfg, driver, reducer)
    hooks.each(made, 'begin_run', model, stream, kw.get('start_task', 0), kw.get('start_epoch', 0), kw.get('ckpt_folder'))
    return made


def _cfg(name, coda=False, **cl):
    cl_cfg = dict(name=name, type_sampling='random', **cl)
    if name == 'der+icarl':
        cl_cfg.update(name='der', type_sampling='icarl')
    if coda:
        cl_cfg.update(prompt_pool=True, prompt_type='coda', coda_tasks=2)
    return {'cl_cfg': cl_cfg}


@pytest.mark.parametrize("driver", [MQ, NLQ, BIC])
def test_support_table_restates_the_drivers(driver):
    from vilco_amd.cl_methods import hooks
    assert {n for d, n in WANT if d == driver} == {None, 'ewc', 'mas', 'si', 'rwalk', 'agem', 'der', 'icarl', 'bic', 'der+icarl'}
    for (d, name), row in WANT.items():
        if d != driver:
            continue
        for want, (reducer, coda) in zip(row, ((None, False), (object(), False), (None, True), (object(), True))):
            case = (driver, name, reducer is not None, coda)
            if isinstance(want, str):
                frag = want % driver if '%s' in want else want
                with pytest.raises(ValueError) as e:
                    _begin(_cfg(name, coda), driver, reducer, _model(), _stream())
                assert frag in str(e.value), (case, str(e.value))
            else:
                made = _begin(_cfg(name, coda), driver, reducer, _model(), _stream())
                assert [type(h).__name__ for h in made] == want, case
                assert all(h.reducer is reducer for h in made), case
    # an L2P pool is no CODA pool, in any driver
    l2p = {'cl_cfg': dict(name='si', prompt_pool=True, prompt_type='l2p')}
    assert [type(h) for h in hooks.make_hooks(l2p, driver, None)] == ([] if driver == BIC else [hooks.SI])
    assert [type(h) for h in hooks.make_hooks({'cl_cfg': dict(name='si', prompt_pool=True)}, driver)] == \
        ([] if driver == BIC else [hooks.SI]), "prompt_type defaults to 'l2p'"


def test_support_table_says_what_the_bic_driver_does_with_the_penalty_methods():
    from vilco_amd.cl_methods import hooks
    for name in ('ewc', 'mas', 'si'):
        drivers, takes_reducer = hooks.SUPPORT[name]
        assert drivers == {MQ: hooks.HOOKS, NLQ: hooks.HOOKS, BIC: hooks.PENALTY_ONLY} and takes_reducer is True
    assert hooks.SUPPORT['rwalk'] == ({MQ: hooks.HOOKS, NLQ: hooks.HOOKS}, True)
    for name in ('agem', 'der', 'coda'):
        assert hooks.SUPPORT[name] == ({MQ: hooks.HOOKS}, False)
    assert sorted(hooks.SUPPORT) == ['agem', 'coda', 'der', 'ewc', 'mas', 'rwalk', 'si']


def test_begin_run_validates_in_the_drivers_order():
    """run_episodes: importance options, SI, RWalk (with its state read), A-GEM, DER (with its bank read), CODA -- each pair of
    neighbours through a configuration that is wrong twice: the earlier complaint is the one raised"""
    bad_imp = dict(importance='sum')
    for name in (None, 'si', 'rwalk', 'agem', 'der', 'icarl'):
        with pytest.raises(ValueError, match="cl_cfg.importance must be"):          # first, whatever the method
            _begin(_cfg(name, coda=True, **bad_imp), MQ, object(), _model(), _stream(), start_epoch=1, start_task=1)
    with pytest.raises(ValueError, match="start_epoch"):                           # SI, then CODA
        _begin(_cfg('si', coda=True), MQ, object(), _model(), _stream(), start_epoch=1)
    with pytest.raises(ValueError, match="rwalk_delta_t"):                         # RWalk's options, then its resumes
        _begin(_cfg('rwalk', coda=True, rwalk_delta_t=0), MQ, object(), _model(), _stream(), start_epoch=1, start_task=1)
    with pytest.raises(ValueError, match="start_epoch"):
        _begin(_cfg('rwalk', coda=True), MQ, object(), _model(), _stream(), start_epoch=1, start_task=1)
    with pytest.raises(ValueError, match="rwalk_state.pt"):                        # RWalk's state read, then CODA
        _begin(_cfg('rwalk', coda=True), MQ, object(), _model(), _stream(), start_task=1)
    with pytest.raises(ValueError, match=A_RED):                                   # A-GEM, then CODA
        _begin(_cfg('agem', coda=True), MQ, object(), _model(), _stream())
    with pytest.raises(ValueError, match=D_RED):                                   # DER: reducer, sampling, bank; then CODA
        _begin(_cfg('der+icarl', coda=True), MQ, object(), _model(), _stream(), start_task=1)
    with pytest.raises(ValueError, match="icarl"):
        _begin(_cfg('der+icarl', coda=True), MQ, None, _model(), _stream(), start_task=1)
    model = _model()
    model.prompt = None
    with pytest.raises(ValueError, match="recorded logits"):
        _begin(_cfg('der', coda=True, der_alpha=0.25), MQ, None, model, _stream(), start_task=1)
    assert model.der_alpha == 0.25 and model.der_bank is not None, "set in begin_run, before the bank is looked for"
    with pytest.raises(ValueError, match="holds no CodaPrompt"):
        _begin(_cfg('der', coda=True), MQ, None, model, _stream())
    # the NLQ driver refuses before it validates
    with pytest.raises(ValueError, match=C_DRV % NLQ):
        _begin(_cfg('rwalk', coda=True, rwalk_delta_t=0, **bad_imp), NLQ, None, _model(), _stream(), start_epoch=1)
    with pytest.raises(ValueError, match="cl_cfg.importance must be"):
        _begin(_cfg('rwalk', rwalk_delta_t=0, **bad_imp), NLQ, None, _model(), _stream(), start_epoch=1)
    # the BiC driver validates nothing of the methods it leaves to the penalty
    assert _begin(_cfg('si', **bad_imp), BIC) == []


def test_all_of_it_runs_before_the_model_or_the_stream_is_touched():
    from vilco_amd import train_cl
    for cfg, frag in ((_cfg('si', coda=True), "start_epoch"), (_cfg('rwalk', rwalk_delta_t=0), "rwalk_delta_t"),
                      (_cfg('mas', importance='sum'), "cl_cfg.importance must be")):
        with pytest.raises(ValueError, match=frag):
            train_cl.run_episodes(cfg, None, None, reducer=object(), start_epoch=1)
        with pytest.raises(ValueError, match=C_DRV % NLQ if cfg['cl_cfg'].get('prompt_pool') else frag):
            train_cl.run_episodes_nlq(cfg, None, None, None, None, reducer=object(), start_epoch=1)
    for cfg, frag in ((_cfg('agem'), A_RED), (_cfg('der'), D_RED), (_cfg(None, coda=True), C_RED)):
        with pytest.raises(ValueError, match=frag):
            train_cl.run_episodes(cfg, None, None, reducer=object())


def test_resumes_without_their_state_raise(tmp_path):
    """DER's bank and RWalk's state: no folder, and a folder that holds neither"""
    from vilco_amd import train_cl
    from vilco_amd.cl_methods import hooks
    assert (train_cl.DER_BANK_FILE, train_cl.RWALK_STATE_FILE) == (hooks.DER_BANK_FILE, hooks.RWALK_STATE_FILE) == \
        ('der_bank.pt', 'rwalk_state.pt')
    for folder in (None, str(tmp_path)):
        with pytest.raises(ValueError, match="recorded logits.*der_bank.pt"):
            hooks.DER(_cfg('der')).begin_run(_model(), _stream(), start_task=1, ckpt_folder=folder)
        with pytest.raises(ValueError, match="Fisher average.*rwalk_state.pt"):
            hooks.RWalk(_cfg('rwalk')).begin_run(_model(), _stream(), start_task=2, ckpt_folder=folder)
        assert _begin(_cfg('der'), MQ, None, _model(), _stream(), start_task=0, ckpt_folder=folder)      # (no resume: no file needed)
    # with the file the bank comes back
    from vilco_amd.cl_methods.der import DERBank
    bank = DERBank()
    bank.record('a', torch.ones(3, 2), 3, (2, 1))
    torch.save(bank.state_dict(), str(tmp_path / 'der_bank.pt'))
    model = _model()
    hooks.DER(_cfg('der')).begin_run(model, _stream(), start_task=1, ckpt_folder=str(tmp_path))
    assert 'a' in model.der_bank and torch.equal(model.der_bank.get('a')[0], torch.ones(3, 2))


def test_coda_begin_run_fills_the_task_count_and_draws_the_first_task():
    from vilco_amd.cl_methods import hooks
    cfg = _cfg(None, coda=True)
    cfg['cl_cfg']['coda_tasks'] = None
    model = _model()
    calls = model.prompt.set_task_calls
    hook, = hooks.make_hooks(cfg, MQ)
    hook.begin_run(model, _stream(), start_task=1)
    assert cfg['cl_cfg']['coda_tasks'] == 2 and model.prompt.set_task_calls == calls + 1 and int(model.prompt.task_count) == 1
    with pytest.raises(ValueError, match="divided among 2 tasks, the stream has 3"):
        hook.begin_run(model, types.SimpleNamespace(num_tasks=3))
