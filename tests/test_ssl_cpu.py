"""CPU: the float64 restatement of the narration-SSL branch (tests/ssl_restatement.py) reproduces the reference golden
(tests/golden/ssl_step.npz: three consecutive steps, the second bank update wraps, the maskless step is skipped), and the
new C-ABI entries (csrc/ssl.hip) refuse bad arguments before anything touches a GPU."""
import ctypes
import os

import numpy as np

import ssl_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 1e-5           # the bar tests/test_cl_parts.py holds this loss to


def gold():
    return np.load(os.path.join(HERE, "golden", "ssl_step.npz"))


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-12)


def golden_steps(g):
    """(step index, inputs of R.step) of the golden's steps, in order"""
    for s in range(len(g['masks'])):
        feats = [g['feats%d_%d' % (s, l)] for l in range(g['feat_lens'].shape[2])]
        yield s, dict(enc_w=g['enc_w'], enc_b=g['enc_b'], tokens_cf=g['tokens%d' % s], tok_lens=g['tok_lens'][s], feats=feats,
                      feat_lens=g['feat_lens'][s], mask=g['masks'][s])


def test_restatement_reproduces_the_reference_golden():
    g = gold()
    bank, ptr = g['bank0'], 0
    assert list(g['skipped']) == [False, True, False]
    for s, kw in golden_steps(g):
        out = R.step(bank=bank, ptr=ptr, **kw)
        bank, ptr = out['bank'], out['ptr']
        assert ptr == int(g['ptr%d' % s]) and rel(bank, g['bank%d' % s]) < BAR, s
        if g['skipped'][s]:
            assert out['n'] == 0 and out['loss'] == 0.0 and not np.any(out['d_tokens_cf'])
            assert all(not np.any(d) for d in out['d_feats'])
            continue
        assert abs(out['loss'] - float(g['loss%d' % s])) <= BAR * float(g['loss%d' % s]), s
        assert rel(out['d_tokens_cf'], g['d_tokens%d' % s]) < BAR, s
        assert rel(out['d_enc_w'], g['d_enc_w%d' % s]) < BAR and rel(out['d_enc_b'], g['d_enc_b%d' % s]) < BAR, s
        for l, d in enumerate(out['d_feats']):
            assert rel(d, g['d_feats%d_%d' % (s, l)]) < BAR, (s, l)
    assert [int(g['ptr%d' % s]) for s in range(3)] == [2, 2, 1]          # the third update wrapped


def test_restatement_gradients_match_finite_differences():
    rng = np.random.default_rng(3)
    B, D, M = 3, 8, 5
    text, video, bank = rng.normal(size=(B, D)), rng.normal(size=(B, D)), rng.normal(size=(M, D))
    mask = np.array([1.0, 0.0, 1.0])
    out = R.nce(text, video, mask, bank, 3)
    for name, x in (('dtext', text), ('dvideo', video)):
        num = np.zeros_like(x)
        for i in range(B):
            for j in range(D):
                hi, lo = x.copy(), x.copy()
                hi[i, j] += 1e-6
                lo[i, j] -= 1e-6
                a = (hi, video) if name == 'dtext' else (text, hi)
                b = (lo, video) if name == 'dtext' else (text, lo)
                # the bank rows written by the update are constants of the loss (no gradient flows into the bank)
                fixed = out['bank']
                num[i, j] = (_loss_fixed_bank(a, mask, fixed) - _loss_fixed_bank(b, mask, fixed)) / 2e-6
        assert rel(out[name], num) < 1e-6, name


def _loss_fixed_bank(tv, mask, bank):
    """the loss over an already updated bank (update switched off by an all-zero mask would change n: evaluate directly)"""
    tn, vn = R.normalize(tv[0])[0], R.normalize(tv[1])[0]
    n, tot = int((mask != 0).sum()), 0.0
    for b in range(len(mask)):
        if mask[b] != 0:
            p = tn[b] @ vn[b] / 0.07
            tot += R._lse(np.concatenate([[p], bank @ tn[b] / 0.07])) + R._lse(np.concatenate([[p], bank @ vn[b] / 0.07])) - 2 * p
    return tot / (2 * n)


def test_new_entries_reject_bad_arguments_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096                                            # dummy, suitably aligned addresses: every check precedes the launch
    ok = dict(B=4, D=64, M=16)

    def nce_fwd(B, D, M, text=x, ring=x, ws=x):
        return lib.vilco_ssl_nce_fwd(text, x, x, B, D, x, M, ring, 0.07, x, x, x, x, ws, 1 << 30, None)

    def nce_bwd(B, D, M, gloss=x):
        return lib.vilco_ssl_nce_bwd(gloss, x, x, x, x, x, B, D, M, 0.07, x, x, x, 1 << 30, None)
    for bad in (dict(ok, D=62), dict(ok, D=4100), dict(ok, B=17), dict(ok, B=0), dict(ok, B=65, M=100)):
        assert nce_fwd(**bad) == -1 and nce_bwd(**bad) == -1, bad
        assert lib.vilco_ssl_ring_update(x, x, bad['B'], bad['D'], x, bad['M'], x, None) == -1, bad
        assert lib.vilco_ssl_nce_workspace(bad['B'], bad['D'], bad['M']) == 0
    assert nce_fwd(text=None, **ok) == -1 and nce_fwd(ring=None, **ok) == -1 and nce_bwd(gloss=None, **ok) == -1
    assert lib.vilco_ssl_ring_update(None, x, 4, 64, x, 16, x, None) == -1
    assert lib.vilco_ssl_nce_workspace(4, 64, 16) > 0
    assert lib.vilco_ssl_nce_fwd(x, x, x, 4, 64, x, 16, x, 0.07, x, x, x, x, x, 16, None) == -4          # short workspace
    # pooling: 1 <= L <= 16 levels, a table of non-null level pointers
    T = (ctypes.c_int32 * 17)(*([8] * 17))
    ptrs = (ctypes.c_void_p * 17)(*([x] * 17))
    assert lib.vilco_ssl_pool_fwd(ptrs, T, 17, x, 2, 32, x, x, 1 << 30, None) == -1
    assert lib.vilco_ssl_pool_bwd(x, ptrs, T, 17, x, 2, 32, None) == -1
    assert lib.vilco_ssl_pool_fwd(ptrs, T, 0, x, 2, 32, x, x, 1 << 30, None) == -1
    assert lib.vilco_ssl_pool_fwd(None, T, 2, x, 2, 32, x, x, 1 << 30, None) == -1
    assert lib.vilco_ssl_pool_fwd(ptrs, T, 2, None, 2, 32, x, x, 1 << 30, None) == -1
    hole = (ctypes.c_void_p * 2)(x, None)
    assert lib.vilco_ssl_pool_fwd(hole, T, 2, x, 2, 32, x, x, 1 << 30, None) == -1
    assert lib.vilco_ssl_pool_bwd(x, hole, T, 2, x, 2, 32, None) == -1
    assert lib.vilco_ssl_pool_workspace(T, 17, 2, 32) == 0 and lib.vilco_ssl_pool_workspace(T, 2, 2, 32) > 0
    assert lib.vilco_ssl_pool_fwd(ptrs, T, 2, x, 2, 32, x, x, 16, None) == -4


def test_ssl_symbols_are_declared_and_bound():
    """the existing ABI test covers the whole table; this names the SSL entries"""
    from vilco_amd import _lib
    text = open(os.path.join(os.path.dirname(HERE), "include", "vilco_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("vilco_ssl_pool_workspace", "vilco_ssl_pool_fwd", "vilco_ssl_pool_bwd", "vilco_ssl_nce_workspace",
              "vilco_ssl_nce_fwd", "vilco_ssl_nce_bwd", "vilco_ssl_ring_update"):
        assert n in _lib.SIGNATURES and n + "(" in text and hasattr(lib, n), n


def test_step_inputs_carry_the_narration_slots():
    import torch
    from vilco_amd.modeling.meta_archs import StepInputs
    inp = StepInputs()
    for k in StepInputs.__slots__:
        setattr(inp, k, None)
    inp.feats_cf, inp.narr_cf = torch.zeros(2, 4, 8), torch.zeros(2, 6, 16)
    inp.narr_lens, inp.narr_mask = torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    names = [k for k, _ in inp.tensors()]
    assert names == ["feats_cf", "narr_cf", "narr_lens", "narr_mask"]
    assert ("narr_cf", (2, 6, 16)) in inp.signature()
