"""CPU: which kernels take an attention call (csrc/attn.hip: attn_route) as the two query entry points report it, and the
return codes of vilco_attn_fwd / vilco_attn_bwd for descriptors that never reach a launch.  Pure host code: no GPU.

The rule is restated below from include/vilco_hip.h: the hd = 64 / fp16 x2 (precision 3) / prefix-mask or no-mask / no-bias /
no-dropout kernels emit output amax partials (one float per workgroup: 128 query rows, or 64 key rows) and o's operand planes;
XLNet's relative attention at hd = 64 (mask mode 3, bias, Tq = Tk, precision 3, any dropout) emits o's planes and -- asked
with has_bias = 2 -- the dS partials of its 128-row dQ workgroups; nobody emits more than 8192 partials.  VILCO_ATTN_FAST=0
sends everything to the general kernels, VILCO_ATTN_XL_FAST=0 the XLNet case; both are read once per process, so the
module also runs itself in a child process with each switch off (python tests/test_attn_routes_cpu.py)."""
import ctypes
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
GENERAL, HD64, HD64XL = "general", "hd64", "hd64-xl"
FAST = os.environ.get("VILCO_ATTN_FAST", "1")[:1] != "0"
XL_FAST = os.environ.get("VILCO_ATTN_XL_FAST", "1")[:1] != "0"
CAP = 8192
TS = (1, 127, 128, 129)


def route(hd, mode, Tq, Tk, precision, has_bias, drop, want_ds=False, bwd=False):
    if not FAST or precision != 3 or hd != 64:
        return GENERAL
    if not has_bias and not want_ds and mode in (0, 2) and not drop:
        return HD64
    if XL_FAST and has_bias and mode == 3 and Tq == Tk and (want_ds or not bwd):
        return HD64XL
    return GENERAL


def amax_parts(B, H, T, hd, mode, precision, has_bias, drop_p, key_side):
    ds = has_bias == 2
    r = route(hd, mode, T, T, precision, has_bias != 0, drop_p > 0, want_ds=ds, bwd=ds)
    if r != (HD64XL if ds else HD64) or (ds and key_side):
        return 0
    rows = 64 if key_side else 128
    n = -(-T // rows) * H * B
    return n if n <= CAP else 0


def _lib():
    from vilco_amd import _lib as L
    return L, L.load()


def check_amax_parts_grid():
    _, lib = _lib()
    n = emitted = capped = 0
    for hd, mode, precision, has_bias, drop_p, key_side, T in itertools.product(
            (32, 64, 128), range(5), range(4), (0, 1, 2), (0.0, 0.1), (0, 1), TS):
        tiles = -(-T // (64 if key_side else 128))
        for B, H in ((2, 4), (1, CAP // tiles), (1, CAP // tiles + 1)):     # a small call, the largest allowed, the first refused
            got = lib.vilco_attn_amax_parts(B, H, T, hd, mode, precision, has_bias, drop_p, key_side)
            want = amax_parts(B, H, T, hd, mode, precision, has_bias, drop_p, key_side)
            assert got == want, (B, H, T, hd, mode, precision, has_bias, drop_p, key_side, got, want)
            n += 1
            emitted += want > 0
            capped += want == 0 and amax_parts(2, 4, T, hd, mode, precision, has_bias, drop_p, key_side) > 0
    for B, H, T in ((0, 4, 128), (2, 0, 128), (2, 4, 0), (-1, 4, 128)):
        assert lib.vilco_attn_amax_parts(B, H, T, 64, 0, 3, 0, 0.0, 0) == 0
    return n, emitted, capped


def check_planes_supported_grid():
    _, lib = _lib()
    n = yes = 0
    for hd, mode, precision, has_bias, drop_p, Tq, Tk in itertools.product(
            (32, 64, 128), range(5), range(4), (0, 1, 2), (0.0, 0.1), TS, TS):     # Tq != Tk: never the XLNet kernels
        got = lib.vilco_attn_planes_supported(Tq, Tk, hd, mode, precision, has_bias, drop_p)
        want = int(route(hd, mode, Tq, Tk, precision, has_bias != 0, drop_p > 0) != GENERAL)
        assert got == want, (Tq, Tk, hd, mode, precision, has_bias, drop_p, got, want)
        n += 1
        yes += want
    return n, yes


P = 1 << 20              # a dummy, 256-byte aligned address: every case below returns before anything is launched
BIG = 1 << 40


def desc(bwd, **kw):
    """a well-formed descriptor (B 1, H 2, T 130, hd 64, prefix mask, fp16 x2) with `kw` on top; None = a null pointer"""
    L, _ = _lib()
    f = dict(q=P, k=P, v=P, kv_len=P, o=P, lse=P, B=1, H=2, Tq=130, Tk=130, hd=64, scale=0.125, mode=0, precision=3,
             workspace=P, workspace_bytes=BIG)
    if bwd:
        f.update(dout=P, dq=P, dk=P, dv=P)
    f.update(kw)
    return L.AttnDesc(**{k: v for k, v in f.items() if v is not None})


XL = dict(mode=3, bias=P)           # XLNet's relative attention (the hd 64 XL route while the switches are on)


def malformed(bwd):
    """(name, descriptor fields, expected return code): both directions share the first block"""
    _, lib = _lib()
    need = (lib.vilco_attn_bwd_workspace if bwd else lib.vilco_attn_fwd_workspace)(1, 2, 130, 130, 64, 3)
    t = [("null " + p, {p: None}, BADARG) for p in ("q", "k", "v", "o", "lse", "kv_len")]
    t += [
        ("no mask needs no kv_len", dict(kv_len=None, mode=2, workspace_bytes=0), WORKSPACE),
        ("drop_p 1", dict(drop_p=1.0), BADARG),
        ("drop_p < 0", dict(drop_p=-0.1), BADARG),
        ("drop_p nan", dict(drop_p=float("nan")), BADARG),
        ("bad drop_p wins over hd 164", dict(drop_p=1.0, hd=164), BADARG),
        ("mode 5", dict(mode=5), BADARG),
        ("mode -1", dict(mode=-1), BADARG),
        ("precision 4", dict(precision=4), BADARG),
        ("precision -1", dict(precision=-1), BADARG),
        ("bad mode wins over hd 164", dict(mode=5, hd=164), BADARG),
        ("window mode, Tq != Tk", dict(mode=4, Tk=131), BADARG),
        ("window < 0", dict(mode=4, window=-1), BADARG),
        ("H 0", dict(H=0), BADARG),
        ("hd 164", dict(hd=164), UNSUPPORTED),
        ("hd 6", dict(hd=6), UNSUPPORTED),
        ("hd 128 in bf16 x3", dict(hd=128, precision=2), UNSUPPORTED),
        ("hd 164 wins over a null q", dict(hd=164, q=None), UNSUPPORTED),
        ("B 0 before the workspace", dict(B=0, workspace=None, workspace_bytes=0), OK),
        ("Tq 0 before Tk 0", dict(Tq=0, Tk=0, workspace=None), OK),
        ("null q wins over B 0", dict(B=0, q=None), BADARG),
        ("Tk 0", dict(Tk=0), BADARG),
        ("Tk 0 wins over the workspace", dict(Tk=0, workspace=None), BADARG),
        ("null workspace", dict(workspace=None), WORKSPACE),
        ("short workspace", dict(workspace_bytes=need - 1), WORKSPACE),
    ]
    hd64 = route(64, 0, 130, 130, 3, False, False) == HD64
    if not bwd:
        xl = route(64, 3, 130, 130, 3, True, False) == HD64XL
        t += [
            ("o_amax, XL route", dict(XL, o_amax=P), UNSUPPORTED),
            ("o_amax, hd 32", dict(hd=32, o_amax=P), UNSUPPORTED),
            ("o_amax, dropout", dict(drop_p=0.1, o_amax=P), UNSUPPORTED),
            ("o_amax, bf16 x2", dict(precision=0, o_amax=P), UNSUPPORTED),
            ("o_planes, hd 128", dict(hd=128, o_planes=P, o_planes_bytes=BIG), UNSUPPORTED),
            ("o_planes, XL route but Tq != Tk", dict(XL, Tk=131, o_planes=P, o_planes_bytes=BIG), UNSUPPORTED),
            ("o_planes unaligned", dict(o_planes=P + 128, o_planes_bytes=BIG), UNSUPPORTED),
            ("o_planes unaligned, XL route", dict(XL, o_planes=P + 16, o_planes_bytes=BIG), UNSUPPORTED),
            ("o_planes short", dict(o_planes=P, o_planes_bytes=64), WORKSPACE if hd64 else UNSUPPORTED),
            ("o_planes short, XL route", dict(XL, drop_p=0.1, o_planes=P, o_planes_bytes=64), WORKSPACE if xl else UNSUPPORTED),
            ("short workspace wins over o_amax on the XL route", dict(XL, o_amax=P, workspace_bytes=need - 1), WORKSPACE),
        ]
    else:
        xl = route(64, 3, 128, 128, 3, True, False, want_ds=True, bwd=True) == HD64XL
        T128 = dict(XL, Tq=128, Tk=128)
        t += [("null " + p, {p: None}, BADARG) for p in ("dout", "dq", "dk", "dv")]
        t += [
            ("null dout wins over B 0", dict(B=0, dout=None), BADARG),
            ("dq_amax, XL route", dict(XL, dbias=P, dq_amax=P), UNSUPPORTED),
            ("dk_amax, XL forward + general backward", dict(XL, dk_amax=P), UNSUPPORTED),
            ("dv_amax, dropout", dict(drop_p=0.1, dv_amax=P), UNSUPPORTED),
            ("dq_amax, hd 32", dict(hd=32, dq_amax=P), UNSUPPORTED),
            ("dbias_amax without dbias", dict(XL, dbias_amax=P), UNSUPPORTED),
            ("dbias_amax, shifted bias (mode 1)", dict(mode=1, bias=P, dbias=P, dbias_amax=P), UNSUPPORTED),
            ("dbias_amax, bf16 x2", dict(XL, precision=0, dbias=P, dbias_amax=P), UNSUPPORTED),
            ("ds_planes with dbias", dict(T128, dbias=P, ds_planes=P, ds_planes_bytes=BIG), UNSUPPORTED),
            ("ds_planes with dbias_amax", dict(T128, dbias_amax=P, ds_planes=P, ds_planes_bytes=BIG), UNSUPPORTED),
            ("ds_planes, Tk % 64", dict(XL, ds_planes=P, ds_planes_bytes=BIG), UNSUPPORTED),
            ("ds_planes, no bias", dict(Tq=128, Tk=128, ds_planes=P, ds_planes_bytes=BIG), UNSUPPORTED),
            ("ds_planes + dq_amax, no bias", dict(Tq=128, Tk=128, dq_amax=P, ds_planes=P, ds_planes_bytes=BIG), UNSUPPORTED),
            ("ds_planes, hd 32", dict(T128, hd=32, ds_planes=P, ds_planes_bytes=BIG), UNSUPPORTED),
            ("ds_planes unaligned", dict(T128, ds_planes=P + 64, ds_planes_bytes=BIG), UNSUPPORTED),
            ("ds_planes short", dict(T128, ds_planes=P, ds_planes_bytes=lib.vilco_attn_dsplanes_bytes(1, 2, 128) - 1),
             WORKSPACE if xl else UNSUPPORTED),
        ]
    return t


def check_malformed():
    _, lib = _lib()
    n = 0
    for bwd in (False, True):
        fn = lib.vilco_attn_bwd if bwd else lib.vilco_attn_fwd
        assert fn(None, None) == BADARG
        for name, kw, want in malformed(bwd):
            got = fn(ctypes.byref(desc(bwd, **kw)), None)
            assert got == want, ("bwd" if bwd else "fwd", name, got, want)
            n += 1
    return n


def test_amax_parts_follow_the_route_rule():
    n, emitted, capped = check_amax_parts_grid()
    print("%d configurations, %d emit partials, %d stopped by the %d cap" % (n, emitted, capped, CAP))
    assert emitted > 0 and capped > 0            # the grid reaches both sides


def test_planes_supported_follows_the_route_rule():
    n, yes = check_planes_supported_grid()
    print("%d configurations, %d with output planes" % (n, yes))
    assert 0 < yes < n


def test_malformed_descriptors_return_codes():
    print("%d descriptors" % check_malformed())


@pytest.mark.parametrize("switch", ["VILCO_ATTN_FAST", "VILCO_ATTN_XL_FAST"])
def test_routes_with_a_switch_off(switch):
    """the same grids and tables in a fresh process that starts with the switch at 0"""
    env = dict(os.environ, **{switch: "0"})
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "routes ok" in r.stdout


if __name__ == "__main__":
    n, emitted, capped = check_amax_parts_grid()
    assert (emitted > 0) == FAST, "with VILCO_ATTN_FAST=0 nobody emits partials"
    m, yes = check_planes_supported_grid()
    assert (yes > 0) == FAST
    print("routes ok: fast %d xl %d: %d + %d configurations (%d emit, %d planes), %d descriptors"
          % (FAST, XL_FAST, n, m, emitted, yes, check_malformed()))
