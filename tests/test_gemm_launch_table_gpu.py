"""Every row of the GEMM launch table (csrc/gemm.hip: launch_plan) once, through ops.gemm, against float64, at the smallest
shape that still has edges: M = 200, N = 136, K = 100 -- ragged tiles in M and N at every tile height, Kp = 128, two
intervals of the 64-wide K loops.  Each case brackets its call with vilco_gemm_profile_begin / _end and asserts from the
record that the intended tile height, split count and k-major flags were taken, so that no case can silently test another row.

Bars (max abs error / max abs reference, as tests/test_ops_gpu.py): two-part bf16 2e-4, plain bf16 2e-2, three-part bf16 2e-6,
fp16 x2 4e-6.  Precision 4 multiplies the leading fp16 parts alone and is held, as there, to 2e-6 against the float64 product of
the operands as the kernel sees them: `lead(x)` = fp16(x s) / s with s the per-tensor power of two that puts max|x| in [2^14, 2^15).

Not reached here: gemm_skinny_kernel<32> -- at the defaults VILCO_GEMM_SKINNY_BM16 = VILCO_GEMM_SKINNY_M = 640, so no M takes
32 rows per workgroup; M = 641 pins that boundary from the other side (the tiled kernel)."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, K = 200, 136, 100
NN, NT, TN = (1, 0), (1, 1), (0, 0)
BAR = {0: 2e-4, 1: 2e-2, 2: 2e-6, 3: 4e-6, 4: 2e-6}
DUMP = os.environ.get("VILCO_GEMM_TABLE_DUMP")          # a file that receives every output of the module (comparing two builds)
_outputs = {}


@pytest.fixture(scope="module")
def data(dev):
    """operands and float64 references, made once"""
    g = torch.Generator().manual_seed(18)
    a = torch.randn(641, 128, generator=g)              # rows: tokens
    b = torch.randn(3, 137, 128, generator=g) / 8       # rows: output features; three weights for the group
    d = dict(a=a.to(dev), b=b.to(dev))
    d["ref"] = a[:M, :K].double() @ b[0, :N, :K].double().t()
    d["ref4"] = lead(a[:M, :K]) @ lead(b[0, :N, :K]).t()
    yield d
    if DUMP:
        torch.save({k: v.cpu() for k, v in _outputs.items()}, DUMP)


@pytest.fixture(autouse=True)
def unforced():
    from vilco_amd import _lib
    try:
        yield
    finally:
        _lib.load().vilco_gemm_force(0, 0)


def lead(t):
    """what a precision-4 product multiplies (tests/test_ops_gpu.py): the leading fp16 part of the per-tensor scaled operand, in float64"""
    s = 2.0 ** (14 - torch.floor(torch.log2(t.abs().max())).item())
    return (t * s).half().double().cpu() / s


def profiled(fn):
    """runs fn between profile_begin / _end; returns the records [M, N, K, batch, BM, ksplit, precision, a_km, b_km, tap]"""
    from vilco_amd import _lib
    lib = _lib.load()
    assert lib.vilco_gemm_profile_begin() == 0
    try:
        fn()
    finally:
        ms, n = C.c_double(), C.c_int64()
        rc = lib.vilco_gemm_profile_end(C.byref(ms), C.byref(n))
    assert rc == 0
    desc = (C.c_int64 * (10 * 8))()
    got = lib.vilco_gemm_profile_records(desc, None, 8)
    assert got == n.value
    return [list(desc[10 * i:10 * i + 10]) for i in range(got)]


def operands(data, orient, m=M, n=N, k=K, w=0):
    """A (m x k) and B (k x n) of the product in the given orientation, as contiguous matrices, and their row strides"""
    a, b = data["a"][:m, :k], data["b"][w, :n, :k]
    A = a.contiguous() if orient[0] else a.t().contiguous()
    B = b.contiguous() if orient[1] else b.t().contiguous()
    return A, B, A.shape[1], B.shape[1]


def product(data, orient, precision, m=M, n=N, k=K, **kw):
    from vilco_amd import ops
    A, B, lda, ldb = operands(data, orient, m, n, k)
    out = torch.full((m, n), float("nan"), device=A.device)
    rec = profiled(lambda: ops.gemm(A, B, out, m, n, k, orient[0], orient[1], lda, ldb, n, precision=precision, **kw))
    torch.cuda.synchronize()
    return out, rec


def check(name, out, ref, bar):
    _outputs[name] = out
    err = ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print("%s: rel err %.3e (bar %.3e)" % (name, err, bar))
    assert err < bar, (name, err, bar)


TABLE = [(p, bm) for p in (0, 1, 2) for bm in (128, 256)] + [(3, 128), (3, 192)] + [(4, 128), (4, 192), (4, 256)]


@pytest.mark.parametrize("orient", [NN, NT, TN], ids=["NN", "NT", "TN"])
@pytest.mark.parametrize("precision,bm", TABLE)
def test_every_tile_height_of_every_kernel_family(dev, data, orient, precision, bm):
    """gemm_pp_kernel on bf16 parts (0 / 1 / 2), gemm_gl_kernel (3), gemm_pp_kernel's K2 loop (4), in all three orientations"""
    from vilco_amd import _lib
    _lib.load().vilco_gemm_force(bm, 1)
    out, rec = product(data, orient, precision)
    assert rec == [[M, N, K, 1, bm, 1, precision, int(not orient[0]), int(not orient[1]), 0]], rec
    check("table p%d bm%d %d%d" % (precision, bm, *orient), out, data["ref4" if precision == 4 else "ref"], BAR[precision])


@pytest.mark.parametrize("m,rows", [(M, 16), (640, 16), (641, 128)])
def test_few_row_kernel_and_its_boundary(dev, data, m, rows):
    """unforced NT at the default precision: gemm_skinny_kernel at 16 rows per workgroup up to M = 640, the tiled kernel from 641"""
    out, rec = product(data, NT, 3, m=m)
    assert rec == [[m, N, K, 1, rows, 1, 3, 0, 0, 0]], rec
    ref = data["ref"] if m == M else data["a"][:m, :K].double().cpu() @ data["b"][0, :N, :K].double().cpu().t()
    check("skinny m%d" % m, out, ref, BAR[3])


@pytest.mark.parametrize("n", [136, 137])
def test_split_k_and_both_finish_kernels(dev, data, n):
    """two splits of the two-interval K loop; N % 4 == 0 takes splitk_reduce_kernel<true>, 137 columns the scalar form"""
    from vilco_amd import _lib
    _lib.load().vilco_gemm_force(128, 2)
    out, rec = product(data, NT, 3, n=n)
    assert rec == [[M, n, K, 1, 128, 2, 3, 0, 0, 0]], rec
    check("splitk n%d" % n, out, data["a"][:M, :K].double().cpu() @ data["b"][0, :n, :K].double().cpu().t(), BAR[3])


@pytest.mark.parametrize("orient", [NT, NN], ids=["NT", "NN"])
def test_grouped_launch_of_three_products(dev, data, orient):
    """the q / k / v projections' shape of launch: forward (x W^T) and dX (dY W) with packed operands, one gemm_gl_group_kernel grid"""
    from vilco_amd import _lib, ops
    k = 128
    _lib.load().vilco_gemm_force(128, 1)
    outs, calls, keep = [], [], []
    for w in range(3):
        A, B, lda, ldb = operands(data, orient, k=k, w=w)
        pa, pb = ops.pack(A, *A.shape), ops.pack(B, *B.shape)
        out = torch.full((M, N), float("nan"), device=dev)
        keep.append((A, B, pa, pb))
        outs.append(out)
        calls.append(((A, B, out, M, N, k, orient[0], orient[1], lda, ldb, N), dict(precision=3, a_planes=pa, b_planes=pb)))
    rec = profiled(lambda: ops.gemm_group(calls))
    torch.cuda.synchronize()
    assert rec == [[M, N, k, 3, 128, 1, 3, 0, int(not orient[1]), 0x100]], rec
    for w, out in enumerate(outs):
        ref = data["a"][:M, :k].double().cpu() @ data["b"][w, :N, :k].double().cpu().t()
        check("group %d%d w%d" % (*orient, w), out, ref, BAR[3])


@pytest.mark.parametrize("T", [1, 100])
def test_single_part_product_under_a_band(dev, data, T):
    """precision 4 with band 2 (A is XLNet's [T, 2T] position-score matrix, zero outside 0 <= p - T + i < T): gemm_pp_kernel on one
    fp16 part, one K-step per interval; bandT = 1 is the smallest the descriptor allows"""
    from vilco_amd import ops
    i, p = torch.arange(T).view(T, 1), torch.arange(2 * T).view(1, 2 * T)
    inband = ((p - T + i >= 0) & (p - T + i < T)).to(dev)
    A = (data["a"][:T, :2 * T] if T == 1 else data["a"][:T, :128].repeat(1, 2)[:, :2 * T]).contiguous() * inband
    B = (data["b"][0, :N, :2 * T] if T == 1 else data["b"][0, :N, :128].repeat(1, 2)[:, :2 * T]).contiguous()
    out = torch.full((T, N), float("nan"), device=dev)
    rec = profiled(lambda: ops.gemm(A, B, out, T, N, 2 * T, 1, 1, 2 * T, 2 * T, N, precision=4, band=2, bandT=T))
    torch.cuda.synchronize()
    assert rec == [[T, N, 2 * T, 1, 128, 1, 4, 0, 0, 0]], rec
    check("band T%d" % T, out, lead(A) @ lead(B).t(), BAR[4])      # (A is masked already: the zeros outside the band do not move its scale)
