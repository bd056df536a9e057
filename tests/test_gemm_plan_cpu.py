"""CPU: the GEMM plan (csrc/gemm.hip: operand layout, tile height, split-K, kernel family) as the library shows it without a
launch, pinned to what the library computed BEFORE the host side was split into named rules.  Pure host code: no GPU.

For every descriptor of `grid()` three integers are held against tests/golden/gemm_plan_grid.json:
  vilco_gemm_workspace(d)   -- Kp, both operand layouts (rows, strides, parts) and the split count (the slabs),
  vilco_gemm_amax_parts(d)  -- the tile height / the few-row kernel's rows per workgroup / the split-K finish,
  vilco_gemm(d, NULL)       -- with dummy 256-byte aligned addresses and a NULL workspace: a valid descriptor returns
                               VILCO_ERR_WORKSPACE before anything is launched, an invalid one its own code first.
The golden file was RECORDED from the library of the commit before the refactor (`VILCO_HIP_LIB=<that build> python
tests/test_gemm_plan_cpu.py --record`) and is data: it is never to be recorded from the code under test.  Its "default"
table holds one [workspace, parts, code] row per descriptor; every other configuration -- vilco_gemm_force(bm, ks),
vilco_gemm_set_skinny(0), and one child process per environment switch, which are read once per process -- is held as
[base, rows]: the name of the nearest configuration recorded before it and the rows that differ from that one, each as
[index, workspace, parts, code].

Recorded: 1737 descriptors, 624 distinct (workspace, parts) pairs, 1125 rows differ from the row before them in
workspace or parts (65 %); 22 further configurations with 10083 rows that differ from the default (5433 stored).  VILCO_GEMM_GROUP=0 changes nothing
that is visible without a launch (it is run all the same: the codes must not move)."""
import ctypes
import json
import os
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_grid.json")
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
P = 1 << 20                    # a dummy, 256-byte aligned address: no case below reaches a launch
NN, NT, TN, TT = (1, 0), (1, 1), (0, 0), (0, 1)      # (a_kcontig, b_kcontig): x W, x W^T, dY^T X, and the refused one
FORCES = [(bm, ks) for bm in (0, 128, 192, 256) for ks in (0, 1, 3)]
SWITCHES = [("VILCO_GEMM_KM", "0"), ("VILCO_GEMM_K2", "0"), ("VILCO_GEMM_SUB192", "0"), ("VILCO_GEMM_DW_TALL", "0"),
            ("VILCO_GEMM_SKINNY", "0"), ("VILCO_GEMM_GROUP", "0"), ("VILCO_CONV_DW_KM", "0"), ("VILCO_GEMM_SKINNY_M", "320"),
            ("VILCO_GEMM_SKINNY_BM16", "100"), ("VILCO_GEMM_SKINNY_K", "512")]
ENV_NAMES = [s for s, _ in SWITCHES] + ["VILCO_GEMM_BM", "VILCO_GEMM_KS"]

NAMED = [(4608, 1024, 1024), (4608, 4096, 1024), (4608, 3072, 1024), (1152, 4096, 1024), (2304, 1024, 4096), (1024, 3072, 9082),
         (1024, 6912, 4608), (3072, 1024, 4608), (1024, 1024, 4608), (154, 1024, 768), (512, 512, 512), (288, 1024, 1024),
         (576, 1024, 4096)]


_BINDING = None


def _lib():
    """the ctypes binding; a child process loads vilco_amd/_lib.py alone (ctypes only), not the package, which imports torch"""
    global _BINDING
    if _BINDING is None:
        if __name__ == "__main__":
            import importlib.util
            spec = importlib.util.spec_from_file_location("vilco_lib_binding", os.path.join(ROOT, "vilco_amd", "_lib.py"))
            _BINDING = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(_BINDING)
        else:
            from vilco_amd import _lib as _BINDING
    return _BINDING, _BINDING.load()


def mm(M, N, K, orient=NT, precision=3, **kw):
    """fields of a well-formed, unbatched, dense product on contiguous operands, `kw` on top (None = a null pointer)"""
    akc, bkc = orient
    f = dict(A=P, B=P, C=P, M=M, N=N, K=K, a_kcontig=akc, b_kcontig=bkc, lda=K if akc else M, ldb=K if bkc else N, ldc=N,
             batch_outer=1, batch_inner=1, precision=precision, alpha=1.0)
    f.update(kw)
    return f


def batched(M, N, K, orient, precision, bo, bi, a_var=(1, 1), b_var=(1, 1), **kw):
    """batch z = zo * bi + zi; an operand whose stride is 0 at a level is shared by that level's members"""
    a, b, c = M * K, N * K, M * N
    return mm(M, N, K, orient, precision, batch_outer=bo, batch_inner=bi, sAo=a * bi * a_var[0], sAi=a * a_var[1],
              sBo=b * bi * b_var[0], sBi=b * b_var[1], sCo=c * bi, sCi=c, **kw)


def tap_a(tapC, tapT=192, nseq=4, N=512, precision=3, orient=NT, **kw):
    """k=3 conv forward / dX: A's rows are tokens, K = 3 tapC"""
    f = mm(nseq * tapT, N, 3 * tapC, orient, precision, lda=tapC, tap_operand=1, tapC=tapC, tapT=tapT)
    f.update(kw)
    return f


def tap_b(tapC, M=512, tapT=192, nseq=4, precision=3, **kw):
    """k=3 conv weight gradient: K = the tokens, N = 3 tapC"""
    f = mm(M, 3 * tapC, nseq * tapT, TN, precision, ldb=tapC, tap_operand=2, tapC=tapC, tapT=tapT)
    f.update(kw)
    return f


def malformed():
    """(name, fields, code): one descriptor per check of vilco_gemm's prologue, in its order, then pairs that pin the order"""
    g = dict(M=200, N=136, K=100)
    ok = lambda **kw: mm(**dict(g, **kw))
    planes = dict(a_planes=P, b_planes=P)
    return [
        ("null C", ok(C=None), BADARG),
        ("null A", ok(A=None), BADARG),
        ("null B", ok(B=None), BADARG),
        ("null A with a_planes", ok(A=None, **planes), WORKSPACE),
        ("planes, taps on A and B k-major", tap_a(256, orient=NN, b_planes=P), UNSUPPORTED),
        ("a_planes unaligned", ok(a_planes=P + 128, b_planes=P), BADARG),
        ("b_planes unaligned", ok(a_planes=P, b_planes=P + 16), BADARG),
        ("M < 0", ok(M=-1), BADARG),
        ("N < 0", ok(N=-1), BADARG),
        ("K < 0", ok(K=-1), BADARG),
        ("batch_outer 0", ok(batch_outer=0), BADARG),
        ("batch_inner 0", ok(batch_inner=0), BADARG),
        ("M 0", ok(M=0), OK),
        ("N 0", ok(N=0), OK),
        ("K 0", ok(K=0), WORKSPACE),
        ("precision -1", ok(precision=-1), BADARG),
        ("precision 5", ok(precision=5), BADARG),
        ("act -1", ok(act=-1), BADARG),
        ("act 3", ok(act=3), BADARG),
        ("band -1", ok(band=-1), BADARG),
        ("band 4", ok(band=4, bandT=100), BADARG),
        ("band 2 without bandT", ok(band=2), BADARG),
        ("drop_p < 0", ok(drop_p=-0.1), BADARG),
        ("drop_p 1", ok(drop_p=1.0), BADARG),
        ("drop_p nan", ok(drop_p=float("nan")), BADARG),
        ("dropout, ldc != N", ok(drop_p=0.1, ldc=144), UNSUPPORTED),
        ("dropout, batched", batched(200, 136, 100, NT, 3, 2, 1, drop_p=0.1), UNSUPPORTED),
        ("row_len without rowT", ok(row_len=P), BADARG),
        ("row_mask, batched", batched(200, 136, 100, NT, 3, 1, 2, row_mask=P), UNSUPPORTED),
        ("TT", ok(orient=TT), UNSUPPORTED),
        ("tap, tapC 0", dict(tap_a(256), tapC=0), BADARG),
        ("tap, tapT 0", dict(tap_a(256), tapT=0), BADARG),
        ("tap, batched", tap_a(256, batch_outer=2), UNSUPPORTED),
        ("tap A, K != 3 tapC", tap_a(256, K=512), BADARG),
        ("tap A, lda != tapC", tap_a(256, lda=768), BADARG),
        ("tap A, M % tapT", tap_a(256, M=700), BADARG),
        ("tap A on a k-major A", tap_a(256, orient=TN), BADARG),
        ("tap B, N != 3 tapC", tap_b(256, N=512), BADARG),
        ("tap B, ldb != tapC", tap_b(256, ldb=768), BADARG),
        ("tap B, K % tapT", tap_b(256, K=700), BADARG),
        ("tap B on a k-contiguous B", tap_b(256, a_kcontig=1, b_kcontig=1), BADARG),
        ("tap_operand 3", tap_a(256, tap_operand=3), BADARG),
        ("short workspace", ok(workspace=P, workspace_bytes=4096), WORKSPACE),
        # the order of the checks
        ("null C wins over M 0", ok(C=None, M=0), BADARG),
        ("null C wins over the planes' tap rule", tap_a(256, orient=NN, b_planes=P, C=None), BADARG),
        ("the planes' tap rule wins over M < 0", tap_a(256, orient=NN, b_planes=P, M=-1), UNSUPPORTED),
        ("unaligned planes win over M 0", ok(a_planes=P + 128, b_planes=P, M=0), BADARG),
        ("batch_outer 0 wins over M 0", ok(M=0, batch_outer=0), BADARG),
        ("M 0 wins over precision 5", ok(M=0, precision=5), OK),
        ("N 0 wins over TT", ok(N=0, orient=TT), OK),
        ("precision 5 wins over TT", ok(precision=5, orient=TT), BADARG),
        ("act 3 wins over dropout's ldc", ok(act=3, drop_p=0.1, ldc=144), BADARG),
        ("band 4 wins over dropout's ldc", ok(band=4, bandT=100, drop_p=0.1, ldc=144), BADARG),
        ("dropout's ldc wins over row_len without rowT", ok(drop_p=0.1, ldc=144, row_len=P), UNSUPPORTED),
        ("row_len without rowT wins over a batched row_mask", batched(200, 136, 100, NT, 3, 1, 2, row_mask=P, row_len=P), BADARG),
        ("TT wins over tapC 0", dict(tap_a(256), tapC=0, a_kcontig=0), UNSUPPORTED),
        ("tapC 0 wins over a batched tap", dict(tap_a(256), tapC=0, batch_outer=2), BADARG),
        ("a batched tap wins over K != 3 tapC", tap_a(256, K=512, batch_outer=2), UNSUPPORTED),
        ("tap A's K wins over the seq flag", tap_a(256, K=512, a_planes=P), BADARG),
        ("the seq flag wins over the workspace", ok(a_planes_seq=1, **planes), UNSUPPORTED),
        ("the 2^31 bytes wins over the workspace", mm(32768, 128, 32768), UNSUPPORTED),
    ]


def grid():
    """every descriptor, as a list of field dicts: the order is part of the golden file (its "crc")"""
    g = []
    # the shapes named in the plan's comments: every precision and orientation
    for (M, N, K) in NAMED:
        for precision in range(5):
            for o in (NT, NN, TN, TT):
                g.append(mm(M, N, K, o, precision))
    # both batch levels, operands that vary with neither / one / both
    for (M, N, K) in ((130, 130, 64), (200, 136, 100), (4608, 1024, 64)):
        for precision in (0, 3, 4):
            for bo, bi in ((2, 1), (1, 3), (2, 3), (8, 4)):
                for o in (NT, NN, TN):
                    g.append(batched(M, N, K, o, precision, bo, bi))
                g.append(batched(M, N, K, NT, precision, bo, bi, a_var=(0, 1), b_var=(1, 0)))
                g.append(batched(M, N, K, NN, precision, bo, bi, a_var=(1, 0), b_var=(0, 0)))
    # tile-count edges: tn = 1 (N = 128), M = a count of 128- / 192-row tiles, above M = 2048 ...
    for t in (127, 128, 175, 176, 255, 256, 257):
        for precision in (0, 3, 4):
            for K in (1024, 8192):
                g.append(mm(128 * t, 128, K, NT, precision))
    for t in (176, 256, 257):
        for precision in (0, 3, 4):
            for K in (1024, 8192):
                g.append(mm(192 * t, 128, K, NN, precision))
    # ... and below it: M 2047 / 2048 at 128, 176, 256, 272 tiles of 128 rows; 192-row counts 176 / 256 / 257 with M < 2048
    for M, N in ((2047, 1024), (2048, 1024), (2047, 1408), (2048, 1408), (2047, 2048), (2048, 2048), (2047, 2176), (2048, 2176),
                 (1536, 2816), (1536, 4096), (192, 32896), (1920, 2304), (1920, 3328)):
        for precision in (0, 3, 4):
            for K in (1024, 4096):
                g.append(mm(M, N, K, NT, precision))
    # barrier intervals at the split rules' thresholds: 128..175 tiles (nk / 16 on the fp16 x2 kernel, nk / 32 on the others; (b)
    # of the sub-round rule from nk >= 48), fewer than 128 tiles (nk / 4, nk / 8), one tile, and the 8-interval rule of the tall
    # weight-gradient plan
    for M, N in ((2304, 1024), (2048, 1024), (1024, 1024), (512, 1024), (1000, 1000), (128, 128), (1024, 3072)):
        for precision in (0, 3, 4):
            for K in (96, 224, 256, 480, 512, 992, 1024, 1504, 1536, 2016, 2048, 3040, 3072, 4064, 4096, 6112, 6144, 9082):
                g.append(mm(M, N, K, NN if precision == 3 else TN, precision))
    # the few-row kernel's eligibility edges
    for M in (16, 100, 101, 320, 321, 640, 641):
        for K in (63, 64, 512, 513, 768, 769):
            for N in (1024, 1025):
                g.append(mm(M, N, K, NT, 3))
    for o in (NN, TN):
        g.append(mm(154, 1024, 768, o, 3))
    g.append(mm(154, 1024, 768, NT, 3, band=2, bandT=384))
    g.append(batched(154, 1024, 768, NT, 3, 2, 1))
    # the caps of amax_parts: 2048 blocks of the split-K finish, 8192 tiles
    for M, N in ((512, 1024), (520, 1024), (512, 1025), (724, 724)):
        for precision in (0, 4):
            g.append(mm(M, N, 4608, NT, precision))
    for rows in (128, 192, 256):
        for precision in (0, 3, 4):
            for t in (8192, 8193, 16384, 16385):
                g.append(mm(rows * t, 128, 32, NT, precision))
    g.append(batched(8192, 1024, 64, NT, 0, 16, 4))
    g.append(batched(8192, 1024, 64, NT, 0, 16, 5))
    # one operand matrix of 2^31 - 2^20 bytes is refused, 64 bytes less is not
    lim = ((1 << 31) - (1 << 20)) // 64             # rows of 32 k, 2 bytes each
    for o in (NT, TN):
        for rows in (lim - 32, lim):
            g.append(mm(rows, 128, 32, o, 1))
            g.append(mm(128, rows, 32, o, 1))
    g.append(mm(32768, 128, 32768))
    # M or N = 0 (nothing to do), K = 0 (a bias-only product)
    for M, N, K in ((0, 136, 100), (200, 0, 100), (0, 0, 0), (200, 136, 0), (200, 136, 1)):
        for precision in (0, 3):
            g.append(mm(M, N, K, NT, precision))
    # XLNet's relative-position band: C is the [T, 2T] matrix (1), A is (2), A is its transpose (3)
    for T in (1, 130, 768):
        for precision in range(5):
            for band, (M, N, K) in ((0, (T, 2 * T, 64)), (1, (T, 2 * T, 64)), (2, (T, 64, 2 * T)), (3, (2 * T, 64, T))):
                g.append(mm(M, N, K, NT, precision, band=band, bandT=T))
                g.append(batched(M, N, K, NN, precision, 2, 4, band=band, bandT=T))
    # k=3 convs: taps on A (forward, dX) and on B (the weight gradient), tapC % 8 zero and not, M % 8 zero and not
    for precision in range(5):
        for tapC in (256, 100, 8, 4):
            for o in (NT, NN):
                g.append(tap_a(tapC, precision=precision, orient=o))
            for M in (512, 508):
                g.append(tap_b(tapC, M=M, precision=precision))
        g.append(tap_a(512, tapT=2304, nseq=2, N=512, precision=precision))
        g.append(tap_b(512, M=512, tapT=2304, nseq=2, precision=precision))
        g.append(tap_b(512, M=512, tapT=1, nseq=700, precision=precision))
    # operands that arrive packed: every combination of the two pointers and the two per-sequence flags
    base = [mm(200, 136, 100, NT), mm(200, 136, 100, NN), mm(200, 136, 100, TN), mm(4608, 1024, 1024, NT), tap_a(256), tap_a(256, orient=NN),
            tap_a(100), tap_b(256), tap_b(256, M=508), tap_b(100), batched(200, 136, 100, NT, 3, 2, 3)]
    for f in base:
        for precision in (3, 0):
            for ap, bp, aseq, bseq in [(a, b, s, t) for a in (0, 1) for b in (0, 1) for s in (0, 1) for t in (0, 1)]:
                g.append(dict(f, precision=precision, a_planes=P if ap else None, b_planes=P if bp else None, a_planes_seq=aseq, b_planes_seq=bseq))
    g += [f for _, f, _ in malformed()]
    return g


def make(f):
    L, _ = _lib()
    return L.GemmDesc(**{k: v for k, v in f.items() if v is not None})


def run_grid():
    """[workspace, parts, code] per descriptor, under the process's current configuration"""
    _, lib = _lib()
    rows = []
    for f in grid():
        d = make(f)
        # the two queries plan without validating: a batch count or a tap size of 0 is for vilco_gemm alone, which refuses it first
        q = f["batch_outer"] >= 1 and f["batch_inner"] >= 1 and not (f.get("tap_operand") and (f["tapC"] <= 0 or f["tapT"] <= 0))
        rows.append([int(lib.vilco_gemm_workspace(ctypes.byref(d))) if q else -1, int(lib.vilco_gemm_amax_parts(ctypes.byref(d))) if q else -1,
                     int(lib.vilco_gemm(ctypes.byref(d), None))])
    return rows


def grid_crc():
    return zlib.crc32(repr([sorted((k, repr(v)) for k, v in f.items()) for f in grid()]).encode())


def diff(rows, default):
    return [[i] + r for i, (r, r0) in enumerate(zip(rows, default)) if r != r0]


def expected(t, name):
    """the rows of a configuration: "default" in full, any other as [its nearest earlier configuration, the rows that differ from it]"""
    if name == "default":
        return [list(r) for r in t["default"]]
    base, d = t[name]
    rows = expected(t, base)
    for i, *r in d:
        rows[i] = r
    return rows


def run_in_process():
    """{configuration: rows} for the setters, the defaults restored afterwards; checks that every setter bumps the generation"""
    _, lib = _lib()
    out = {}
    gen = lib.vilco_gemm_config_gen()
    try:
        for bm, ks in FORCES:
            assert lib.vilco_gemm_force(bm, ks) == OK
            gen += 1
            assert lib.vilco_gemm_config_gen() == gen
            out["force %d %d" % (bm, ks)] = run_grid()
        lib.vilco_gemm_force(0, 0)
        gen += 1
        for on in (0, 1):
            assert lib.vilco_gemm_set_skinny(on) == OK
            gen += 1
            assert lib.vilco_gemm_config_gen() == gen
            out["skinny %d" % on] = run_grid()
        assert lib.vilco_gemm_force(-1, 0) == BADARG and lib.vilco_gemm_force(0, -1) == BADARG
        assert lib.vilco_gemm_config_gen() == gen          # a refused call changes nothing
    finally:
        lib.vilco_gemm_force(0, 0)
        lib.vilco_gemm_set_skinny(1)
    return out


def golden():
    with open(GOLDEN) as f:
        t = json.load(f)
    assert t["crc"] == grid_crc() and t["n"] == len(grid()), "grid() no longer yields the descriptors the table was recorded for"
    return t


def compare(name, rows, t):
    want = expected(t, name)
    bad = [(i, r, w) for i, (r, w) in enumerate(zip(rows, want)) if r != w]
    g = grid()
    assert not bad, "%s: %d rows differ from the recorded plan; first: #%d %r got %r want %r" % (
        name, len(bad), bad[0][0], {k: v for k, v in g[bad[0][0]].items() if v != P}, bad[0][1], bad[0][2])


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ENV_NAMES}


@pytest.fixture(scope="module")
def table():
    return golden()


def test_default_plan_matches_the_recorded_table(table):
    rows = run_grid()
    compare("default", rows, table)
    pairs = {(r[0], r[1]) for r in rows}
    moved = sum(1 for a, b in zip(rows, rows[1:]) if a[:2] != b[:2])
    print("%d descriptors, %d distinct (workspace, parts) pairs, %d differ from the row before" % (len(rows), len(pairs), moved))
    assert 2 * moved >= len(rows)               # a flat grid pins nothing


def test_forced_and_skinny_plans_match_the_recorded_table(table):
    for name, rows in run_in_process().items():
        compare("default" if name in ("force 0 0", "skinny 1") else name, rows, table)
    compare("default", run_grid(), table)       # the defaults are back


def test_malformed_descriptors_return_codes():
    _, lib = _lib()
    assert lib.vilco_gemm(None, None) == BADARG
    assert lib.vilco_gemm_workspace(None) == 512 and lib.vilco_gemm_amax_parts(None) == 0
    km = os.environ.get("VILCO_GEMM_KM", "1")[:1] != "0"
    for name, f, want in malformed():
        if not km and (f.get("a_planes") or f.get("b_planes")):
            continue                           # packed operands need the k-major kernels: the recorded table holds those rows
        got = lib.vilco_gemm(ctypes.byref(make(f)), None)
        assert got == want, (name, got, want)
    # a group that cannot be grouped runs its members in order and returns the first failure
    L, _ = _lib()
    two = (L.GemmDesc * 2)(make(mm(200, 136, 128, a_planes=P, b_planes=P)), make(mm(200, 136, 128, a_planes=P, b_planes=P)))
    assert lib.vilco_gemm_group(None, 2, None) == BADARG
    assert lib.vilco_gemm_group(two, 0, None) == BADARG and lib.vilco_gemm_group(two, 5, None) == BADARG
    assert lib.vilco_gemm_group(two, 2, None) == (WORKSPACE if km else UNSUPPORTED)
    assert lib.vilco_gemm_group(two, 1, None) == (WORKSPACE if km else UNSUPPORTED)
    two[1].M = 0
    assert lib.vilco_gemm_group(two, 2, None) == (WORKSPACE if km else UNSUPPORTED)
    two[0].M = 0
    assert lib.vilco_gemm_group(two, 2, None) == (OK if km else UNSUPPORTED)


@pytest.mark.parametrize("switch,value", SWITCHES)
def test_plan_with_a_switch_changed(table, switch, value):
    """the same grid in a fresh process that starts with the switch at `value`"""
    env = dict(clean_env(), **{switch: value})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--check", "%s=%s" % (switch, value)], env=env, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "plan ok" in r.stdout


def record():
    """writes the golden file from the library VILCO_HIP_LIB names: the build of the commit BEFORE the change under test"""
    lib_path = os.environ.get("VILCO_HIP_LIB")
    assert lib_path, "record from a build of the parent commit (VILCO_HIP_LIB), never from the code under test"
    assert not any(k in os.environ for k in ENV_NAMES)
    default = run_grid()
    t = {"n": len(default), "crc": grid_crc(), "default": default}
    full = {"default": default}
    total = stored = 0

    def store(name, rows):
        nonlocal total, stored
        changed = len(diff(rows, default))
        assert changed or name == "VILCO_GEMM_GROUP=0", name + " changes no row: the grid does not reach it"
        base = min(full, key=lambda b: len(diff(rows, full[b])))        # the nearest configuration recorded so far
        t[name] = [base, diff(rows, full[base])]
        full[name] = rows
        total += changed
        stored += len(t[name][1])
        print("%-28s %5d rows differ from the default, %5d from '%s'" % (name, changed, len(t[name][1]), base))

    for name, rows in run_in_process().items():
        if name in ("force 0 0", "skinny 1"):
            assert rows == default
            continue
        store(name, rows)
    for switch, value in SWITCHES:
        env = dict(clean_env(), **{switch: value})
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump"], env=env, capture_output=True, text=True, check=True)
        store("%s=%s" % (switch, value), json.loads(r.stdout))
    with open(GOLDEN, "w") as f:
        f.write("{" + ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in t.items()) + "}\n")
    moved = sum(1 for a, b in zip(default, default[1:]) if a[:2] != b[:2])
    print("recorded from %s: %d descriptors, %d distinct (workspace, parts) pairs, %d differ from the row before, %d configurations, "
          "%d differing rows (%d stored), %d bytes" % (lib_path, len(default), len({(r[0], r[1]) for r in default}), moved, len(t) - 3, total,
                                                        stored, os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
    elif sys.argv[1:] == ["--dump"]:
        print(json.dumps(run_grid()))
    elif len(sys.argv) == 3 and sys.argv[1] == "--check":
        compare(sys.argv[2], run_grid(), golden())
        test_malformed_descriptors_return_codes()
        print("plan ok: %s, %d descriptors" % (sys.argv[2], len(grid())))
    else:
        sys.exit("usage: test_gemm_plan_cpu.py --record | --dump | --check SWITCH=VALUE")
