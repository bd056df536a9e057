"""Torch-facing operators backed by libvilco_hip.so (hand-written HIP for gfx950).

Every operator here is a `torch.autograd.Function` whose forward AND backward launch kernels
through the C ABI (include/vilco_hip.h) on the current HIP stream.  PyTorch only provides device
memory, the stream and the autograd tape.  Activations are token-major fp32 `[B, T, C]`.

There is deliberately no CPU / ATen fallback: a non-CUDA tensor raises.
"""
import ctypes as C
import math

import torch

from . import _lib, switches
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, TAP_A, TAP_B, TAP_NONE, GemmDesc

# 0 = split-bf16 (hi+lo, 3 MFMAs), 1 = single bf16 pass, 2 = three-part bf16 split (6 MFMAs, ~2^-25),
# 3 = two fp16 parts of per-tensor scaled operands (3 MFMAs, ~2^-22; attention keeps the three bf16 parts)
_PRECISIONS = {"split": 0, 0: 0, "bf16": 1, 1: 1, "split3": 2, "fp32": 2, 2: 2, "f16x2": 3, 3: 3}
DEFAULT_PRECISION = _PRECISIONS[switches.text("VILCO_PRECISION")]
_precision = DEFAULT_PRECISION


# Weight-gradient products dW = dZ^T X (one third of the GEMM flops).  Their operands are already packed as fp16 x2
# planes for the forward / dX products; "f16x1" multiplies only the leading parts (1 MFMA instead of 3).  Unlike the
# forward (where a LayerNorm -> ReLU pre-activation within 1e-5 of zero flips its derivative below ~20 operand bits)
# and the dX chain (whose errors travel on through every earlier layer), a dW error is a zero-mean 2^-11 rounding per
# product and ends in that one gradient tensor; relative to the tensor's largest entries (the parity metric) it shrinks
# with the contraction length K = B*T: measured 5e-4 .. 1e-3 at K = 128 (the golden size: too close to the 1e-3 bar),
# 2e-4 .. 3.5e-4 at K = 4608 (config P, tests/test_fullsize_gpu.py).  So it is used for LONG contractions only (K >= DW_FAST_MIN_K), where
# the time is; short ones keep three MFMAs.  VILCO_DW_PRECISION=f16x2 restores three MFMAs everywhere.
_DW = {"f16x1": 4, "f16x2": None}
dw_precision = _DW[switches.text("VILCO_DW_PRECISION")]
DW_FAST_MIN_K = 2048


def _dw_prec(prec, K=0):
    """precision code of a weight-gradient product with contraction length K whose planes were packed in `prec`"""
    return dw_precision if (dw_precision is not None and prec == 3 and K >= DW_FAST_MIN_K) else prec


def set_precision(p=None):
    """'split' / 0: two-part split-bf16 MFMA (~2^-17);  'bf16' / 1: single bf16 pass;
    'split3' / 'fp32' / 2: three-part bf16 split, numerically an fp32 GEMM (~2^-25);
    'f16x2' / 3: two fp16 parts of power-of-two scaled operands (~2^-22, half the MFMAs of split3).
    None restores the default (env VILCO_PRECISION, else f16x2)."""
    global _precision
    _precision = DEFAULT_PRECISION if p is None else _PRECISIONS[p]


def arithmetic_key():
    """Everything that decides WHICH arithmetic a step's kernels run with and is a module-level switch rather than an input:
    a captured hipGraph replays the kernels it recorded, so graph.GraphedStep keys its graphs on this tuple (VERDICT r04,
    weak 2: flipping set_precision / dw_precision between replays used to replay the old arithmetic silently).  The switches
    come from switches.TABLE (every row marked KEYED that names an attribute of this module); no variable sets the other
    three: the active precision, DW_FAST_MIN_K and the library's own configuration generation (vilco_gemm_force /
    vilco_gemm_set_skinny).  Only ever compared for equality inside one process."""
    g = globals()
    return (_precision, DW_FAST_MIN_K, _lib.load().vilco_gemm_config_gen(),
            *[frozenset(v) if type(v) is set else v for v in map(g.__getitem__, switches.KEYED_OPS)])


def get_precision():
    return _precision


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """raw handle of the CURRENT stream of the current device (honours `torch.cuda.stream(...)` contexts).  Asked ~330
    times per step: the private accessor is 10x cheaper than building a torch.cuda.Stream object each time (3 ms of host
    time per P step, tools/cpu_overhead.py)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# Where a weight gradient is written.  Under data parallelism dist.GradReducer keeps one flat buffer per bucket; the kernels
# that produce the large gradients (the dW products) write straight into the parameter's slot of that buffer, so the
# collective finds its input in place (no gather copy) and p.grad ends up a view of the bucket.  None = ordinary memory.
grad_slot_provider = None


def _grad_out(w):
    if grad_slot_provider is not None:
        slot = grad_slot_provider(w)
        if slot is not None and slot.shape == w.shape and slot.is_contiguous():
            return slot
    return torch.empty_like(w)


# ---- concurrency inside a captured step (vilco_amd/graph.py).  A replayed hipGraph has no host in the loop, so independent
# chains can be forked onto side streams at capture time and the runtime overlaps them: the 77-token text branch under the
# video stem, the regression head beside the classification head, and the weight-gradient products (nothing in backward
# waits for them) beside the dX chain -- they fill the CUs that the 75 %-full GEMM rounds of this model's shapes leave
# idle.  VILCO_GRAPH_STREAMS lists what is forked ("text,heads,dw"; "" = nothing); only active while a stream is capturing
# (in eager mode a second queue made the step time erratic, DESIGN_LOG.md 3.6).
_FORKS = set(x for x in switches.text("VILCO_GRAPH_STREAMS").split(",") if x)
_side_streams = {}
_dw_seen = set()


def fork_enabled(what):
    if not (what in _FORKS and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        return False
    cur = torch.cuda.current_stream()               # no nested forks: a chain already on a side stream stays on it
    return all(st != cur for st in _side_streams.values())


def side_stream(name, device=None):
    dev = torch.cuda.current_device() if device is None else (device.index if device.index is not None else torch.cuda.current_device())
    key = (name, dev)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=dev)
    return _side_streams[key]


def join_side_streams():
    """make the current stream wait for everything forked so far (end of a captured backward)"""
    cur = torch.cuda.current_stream()
    capturing = torch.cuda.is_current_stream_capturing()
    for (name, dev), st in _side_streams.items():
        if dev == cur.device_index:
            if capturing:                       # a backward captured in stages: only the streams this capture forked into
                with torch.cuda.stream(st):     # (an event of a stream outside the capture cannot be waited for inside it)
                    live = torch.cuda.is_current_stream_capturing()
                if not live:
                    continue
            cur.wait_stream(st)
    _dw_seen.clear()


# "dw" forks only the weight-gradient products whose contraction runs over at most this many token rows (0: all of them): the
# products of the small pyramid levels, which sit on a chain that leaves most of the chip idle anyway
_dw_fork_rows = switches.number("VILCO_DW_FORK_ROWS")


class _DwFork:
    """context for one weight-gradient product: on the "dw" side stream when forking is on and this weight has not been
    seen in the current backward (a weight used twice accumulates its gradients on the main stream: keep those ordered)"""

    def __init__(self, w, rows=0):
        key = w.data_ptr()          # inside autograd the weight arrives as a fresh saved-tensor alias per use: id() never repeats
        self.on = fork_enabled("dw") and key not in _dw_seen and (_dw_fork_rows <= 0 or 0 < rows <= _dw_fork_rows)
        if fork_enabled("dw"):
            _dw_seen.add(key)
        self.ctx = None

    def __enter__(self):
        if self.on:
            cur = torch.cuda.current_stream()
            st = side_stream("dw")
            st.wait_stream(cur)
            self.ctx = torch.cuda.stream(st)
            self.ctx.__enter__()
        return self

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)
        return False


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); "
                               "there is no CPU fallback" % t.device)
        if t.dtype != torch.float32:
            raise RuntimeError("expected scalar type Float, got %s" % t.dtype)
        if not t.is_contiguous():
            raise RuntimeError("tensor must be contiguous")


def _ws(nbytes, device):
    t = torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=device)
    if _defer["on"]:
        _defer["keep"].append(t)          # partials a recorded second stage will read at the flush
    return t


# ---- deferred finishing of the backward pass's two-stage reductions (csrc/defer.hip, include/vilco_hip.h).
# Column sums into PARAMETER gradients (LayerNorm affine, biases, scales, depthwise taps) and the slab sums of split-K
# weight-gradient products end in small second launches -- ~350 dependent graph nodes per step that nothing in backward
# waits for.  Inside `with _Deferring(param, ...)` the library records them; one autograd end-of-backward callback issues
# them all as a few batched launches (bitwise the same sums).  Two things make that safe:
#   * a parameter used twice in the forward: autograd sums its gradients the moment the second one arrives -- so only the
#     FIRST gradient a backward produces for a storage is deferred; a later one flushes what is still recorded (when the
#     first is among it) and is finished in place;
#   * nothing may read gradients during backward: dist.GradReducer's autograd hooks do (they launch the all-reduce of a
#     complete bucket), so it blocks deferral while they are live (`defer_blocked`).
# Tensors a recorded item reads or writes are held until the flush (a gradient autograd drops would otherwise hand its
# memory to the next allocation).  VILCO_DEFER_FINISH=0 switches the whole thing off (tested equal).
defer_finish = switches.on("VILCO_DEFER_FINISH")
defer_blocked = False
_defer = {"on": False, "armed": False, "task": -1, "keep": [], "pending": set(), "seen": set()}


def _defer_flush(final=True):
    """issue what is recorded.  final: the end-of-backward callback (or a reset) -- also forgets which parameters this
    backward has already produced a gradient for"""
    st = _defer
    _dw_group_flush()
    if _lib.load().vilco_defer_pending():
        if torch.cuda.is_current_stream_capturing():
            # recorded items may have been produced on a forked side stream (VILCO_GRAPH_STREAMS "dw": split-K slabs written
            # there); autograd's leaf-stream sync does not cover it, so the captured flush needs its own edge
            cur = torch.cuda.current_stream()
            for (name, dev), side in _side_streams.items():
                if dev == cur.device_index and side != cur:
                    with torch.cuda.stream(side):       # only streams THIS capture forked into (a stage graph forks none):
                        live = torch.cuda.is_current_stream_capturing()      # an event from outside a capture cannot be
                    if live:                                                 # waited for inside it (join_side_streams)
                        cur.wait_stream(side)
        _lib.check(_lib.load().vilco_defer_flush(_stream()))
    else:
        _lib.load().vilco_defer_set(0)
    st["on"] = False
    st["keep"].clear()
    st["pending"].clear()
    if final:
        st["armed"] = False
        st["seen"].clear()


# ---- debug-mode dynamic-range check of the backward operands.  The fp16 x2 planes carry ONE power-of-two
# scale per tensor: 22 bits for every element within ~2^16 of the tensor's maximum, fewer below, nothing below 2^-40 of it.
# A gradient tensor whose ROWS span more than that (the mask-ignoring channel attention of a twice-applied stem block: the
# first padded row at ~1e10 x the rest) needs the bf16 x3 format (8 exponent bits per element).  The model marks
# the one site it knows statically (ChannelAttention.wide_range); this check finds such tensors wherever they arise:
#   VILCO_RANGE_CHECK=warn   every Linear backward measures max-row / median-row amax of dZ (a host sync: debug mode only),
#                            records (M, N, K, spread) in ops.range_events and warns once per shape above 2^20;
#   VILCO_RANGE_CHECK=auto   ... and runs that call's two backward products in bf16 x3.
range_check = switches.text("VILCO_RANGE_CHECK")
RANGE_SPREAD_LIMIT = float(2 ** 20)
range_events = []
_range_warned = set()


def _row_spread(t2d):
    """max row amax / median of the non-zero row amaxes of a [rows, cols] tensor (1.0 for an all-zero tensor)"""
    ra = t2d.abs().amax(dim=1)
    nz = ra[ra > 0]
    if nz.numel() == 0:
        return 1.0
    return float(ra.max() / nz.median())


def _range_wide(dz, M, N, K):
    if range_check not in ("warn", "auto") or _precision != 3 or torch.cuda.is_current_stream_capturing():
        return False
    spread = _row_spread(dz.reshape(M, N))
    if spread <= RANGE_SPREAD_LIMIT:
        return False
    range_events.append((int(M), int(N), int(K), spread))
    if (M, N, K) not in _range_warned:
        _range_warned.add((M, N, K))
        import warnings
        warnings.warn("vilco_amd: the output gradient of a Linear [%d x %d] <- [%d x %d] spans a row-amax spread of %.3g (> 2^20): "
                      "one fp16 x2 scale per tensor cannot carry it; %s" %
                      (M, N, M, K, spread, "running its backward products in bf16 x3" if range_check == "auto"
                       else "mark the call site (bwd_precision=2) or run with VILCO_RANGE_CHECK=auto"))
    return range_check == "auto"


class _Deferring:
    def __init__(self, *params):
        self.ptrs = [p.data_ptr() for p in params if p is not None]
        # A deferred gradient holds UNFINISHED values until the end-of-backward flush.  That is only safe where autograd's
        # AccumulateGrad ADOPTS the tensor: the owner must be a leaf whose .grad is still None.  With a gradient already in
        # place (micro-batch accumulation, zero_grad(set_to_none=False), a second backward over a retained graph) autograd
        # does `p.grad += new` in the middle of backward and would read the partial sums; a non-leaf owner's backward reads
        # the value too.  Those cases finish in place (round 5; tests/test_model_gpu.py::test_deferred_finish_with_existing_grads).
        self.adoptable = all(p.is_leaf and p.grad is None for p in params if p is not None)
        self.on = False

    def __enter__(self):
        if not (defer_finish and not defer_blocked and self.ptrs and torch._C._current_graph_task_id() != -1):
            return self
        if not self.adoptable:
            st = _defer
            if st["armed"] and any(p in st["pending"] for p in self.ptrs):
                _defer_flush(final=False)
            return self
        st = _defer
        task = torch._C._current_graph_task_id()
        if st["armed"] and st["task"] != task:
            _defer_flush()                 # left over from a backward that ended in an exception: its callback never ran
        if any(p in st["seen"] for p in self.ptrs):
            # a further use of a parameter: autograd sums its gradients the moment this one arrives, so the earlier one
            # must be complete by then (flush if it is still recorded) and this one is finished in place
            if any(p in st["pending"] for p in self.ptrs):
                _defer_flush(final=False)
            return self
        if not st["armed"]:
            torch.autograd.Variable._execution_engine.queue_callback(_defer_flush)
            st["armed"], st["task"] = True, task
        st["pending"].update(self.ptrs)
        st["seen"].update(self.ptrs)
        _lib.load().vilco_defer_set(1)
        st["on"] = self.on = True
        return self

    def hold(self, *tensors):
        # an ALIAS of each tensor: holding the tensor object itself would raise its reference count, and AccumulateGrad
        # only adopts a gradient it holds the sole reference to (otherwise it copies -- here: the unfinished values)
        if self.on:
            _defer["keep"].extend(t.detach() for t in tensors if t is not None)

    def __exit__(self, *a):
        if self.on:
            _lib.load().vilco_defer_set(0)
            _defer["on"] = False
        return False


# ---------------------------------------------------------------------------------------- dropout
# Counter-based masks (vilco_dropout): a mask is identified by (p, seed); seeds come from torch's seed and a per-process
# call counter, so a run is reproducible under torch.manual_seed.  `dropout_log` (when a list) records
# (site, p, seed, shape) of every mask drawn: the parity tests rebuild the masks from it for the oracle.
_drop_counter = [0]
dropout_log = None


def _rank():
    """data-parallel replicas seeded alike must still draw different masks"""
    import torch.distributed as dist
    return dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0


def _new_drop(site, p, shape):
    if p <= 0.0:
        return (0.0, 0)
    _drop_counter[0] += 1
    seed = ((torch.initial_seed() + 0x632BE5AB * _rank()) * 0x9E3779B1 + _drop_counter[0] * 0x85EBCA6B) & 0xFFFFFFFF
    if dropout_log is not None:
        dropout_log.append((site, float(p), int(seed), tuple(int(x) for x in shape)))
    return (float(p), int(seed))


def dropout_mask(p, seed, shape, device, site=None):
    """the mask factors (0 or 1/(1-p)) of the stream (p, seed), as the kernels apply them.  `site` = the site name the
    dropout log recorded: the attention probabilities ("attn_prob", shape [B, H, Tq, Tk]) have a mask function of their
    own (csrc/common.h: vilco_attn_drop_*)"""
    m = torch.empty(shape, dtype=torch.float32, device=device)
    if site == "attn_prob":
        cols = int(shape[-1])
        _lib.check(_lib.load().vilco_attn_dropout_mask(m.data_ptr(), m.numel() // max(cols, 1), cols, float(p), int(seed), _stream()))
    else:
        _lib.check(_lib.load().vilco_dropout(None, m.data_ptr(), m.numel(), float(p), int(seed), 0, _stream()))
    return m


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, site):
        _chk(x)
        ctx.drop = _new_drop(site, p, x.shape)
        y = torch.empty_like(x)
        _lib.check(_lib.load().vilco_dropout(x.data_ptr(), y.data_ptr(), x.numel(), ctx.drop[0], ctx.drop[1], 0, _stream()))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        _lib.check(_lib.load().vilco_dropout(dy.data_ptr(), dx.data_ptr(), dy.numel(), ctx.drop[0], ctx.drop[1], 0, _stream()))
        return dx, None, None


def dropout(x, p, training, site="dropout"):
    """nn.Dropout(p) on the HIP path (inverted dropout, fresh counter-based mask per call)."""
    if not training or p <= 0.0:
        return x
    return _Dropout.apply(x.contiguous(), float(p), site)


# ---------------------------------------------------------------------------------------- GEMM
def gemm(A, B, Cc, M, N, K, a_kc, b_kc, lda, ldb, ldc, batch=(1, 1), sA=(0, 0), sB=(0, 0),
         sC=(0, 0), offA=0, offB=0, offC=0, tap=TAP_NONE, tapC=0, tapT=0, alpha=1.0, beta=0.0,
         bias=None, preact=None, act=ACT_NONE, row_len=None, rowT=0, colscale=None, residual=None,
         res_masked=0, precision=None, a_planes=None, b_planes=None, band=0, bandT=0, drop=(0.0, 0), want_amax=False,
         a_amax=None, b_amax=None, planes_seq=(False, False), row_mask=None, _into=None, _group_n=0):
    """Raw launch of vilco_gemm; A/B/Cc are fp32 CUDA tensors, offsets in elements.  a_planes / b_planes: operands
    already packed by `pack` (the fp32 tensor may then be None).  want_amax: the call writes ALL of Cc, which goes on
    into another product -- the kernel leaves max|C| partials and Cc is tagged with them (`_tag_amax`).
    _into: (internal, gemm_group) a GemmDesc to fill instead of launching; returns what must stay alive + the amax tag;
    _group_n: ... as a member of a group of that many products (sizes the workspace)."""
    lib = _lib.load()
    d = GemmDesc() if _into is None else _into
    d.A = None if A is None else A.data_ptr() + 4 * offA
    d.B = None if B is None else B.data_ptr() + 4 * offB
    d.a_planes, d.b_planes = _p(a_planes), _p(b_planes)
    d.a_planes_seq, d.b_planes_seq = int(bool(planes_seq[0])), int(bool(planes_seq[1]))     # pack_tap images (k=3 convs)
    d.band, d.bandT = int(band), int(bandT)
    d.drop_p, d.drop_seed = float(drop[0]), int(drop[1])
    d.C = Cc.data_ptr() + 4 * offC
    d.M, d.N, d.K = int(M), int(N), int(K)
    d.a_kcontig, d.b_kcontig = int(a_kc), int(b_kc)
    d.lda, d.ldb, d.ldc = int(lda), int(ldb), int(ldc)
    d.batch_outer, d.batch_inner = int(batch[0]), int(batch[1])
    d.sAo, d.sAi = int(sA[0]), int(sA[1])
    d.sBo, d.sBi = int(sB[0]), int(sB[1])
    d.sCo, d.sCi = int(sC[0]), int(sC[1])
    d.tap_operand, d.tapC, d.tapT = int(tap), int(tapC), int(tapT)
    d.precision = _precision if precision is None else int(precision)
    d.alpha, d.beta = float(alpha), float(beta)
    d.bias = _p(bias)
    d.preact = None if preact is None else preact.data_ptr() + 4 * offC
    d.act = int(act)
    d.row_len = _p(row_len)
    d.row_mask = _p(row_mask)            # one float per output row: rows with 0 are zeroed like rows beyond row_len
    d.rowT = int(rowT)
    d.colscale = _p(colscale)
    d.residual = None if residual is None else residual.data_ptr() + 4 * offC
    d.res_masked = int(res_masked)
    # bf16 operand planes + split-K partials
    nbytes = lib.vilco_gemm_group_workspace(C.byref(d), int(_group_n)) if _group_n else lib.vilco_gemm_workspace(C.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Cc.device)
    if _defer["on"]:
        _defer["keep"].extend((ws, Cc.detach()))    # split-K slabs of a recorded weight-gradient product, and (an alias of) its output
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    for pre, am in (("a", a_amax), ("b", b_amax)):          # (partials, count) of an operand this call packs itself
        if am is not None and am[0] is not None and d.precision in (3, 4):
            setattr(d, pre + "_amax", am[0].data_ptr())
            setattr(d, pre + "_namax", int(am[1]))
    parts, n = None, 0
    if want_amax and produce_amax and d.precision == 3:
        n = int(lib.vilco_gemm_amax_parts(C.byref(d)))
        if n > 0:
            parts = torch.empty(n, dtype=torch.float32, device=Cc.device)
            d.amax_out = parts.data_ptr()
    if _into is not None:
        return (ws, Cc, parts, n)
    _lib.check(lib.vilco_gemm(C.byref(d), _stream()))
    if parts is not None:
        _tag_amax(Cc, parts, n)


def gemm_group(calls):
    """calls: [(args, kwargs) of `gemm`, ...]: independent products of one shape with packed operands (2..4 of the ambient
    two-part format, or any number of single-part ones, precision=4) as ONE launch (vilco_gemm_group; whatever does not
    qualify runs one by one inside the library -- same results)."""
    lib = _lib.load()
    arr = (GemmDesc * len(calls))()
    keep = [gemm(*a, _into=arr[i], _group_n=len(calls), **k) for i, (a, k) in enumerate(calls)]
    _lib.check(lib.vilco_gemm_group(arr, len(calls), _stream()))
    for ws, Cc, parts, n in keep:
        if parts is not None:
            _tag_amax(Cc, parts, n)


# ---- the single-part weight gradients of a backward, grouped.  dW = dZ^T X of one 1024 x 1024 layer is 64 tiles: alone it is split
# four ways over K to fill the chip, writes four fp32 slabs and needs a pass that sums them.  Nothing in backward reads a weight
# gradient (what `_Deferring` already relies on), and both operand images are complete when backward reaches the layer -- so a
# product that `_Deferring` would record a slab sum for is itself recorded here, keyed by shape and orientation, and the
# end-of-backward flush (`_defer_flush`: also every mid-backward flush and, with a staged data-parallel replay, every stage's)
# issues ONE grouped launch per key (vilco_gemm_group, precision 4: no split where the group fills the chip).  The operand planes
# are held until then (2 x 9.4 MB per product at 1024 x 1024 x 4608); the fp32 tensors are not.  A key with one member is a plain
# launch.  vilco_gemm_set_group_dw(0) / VILCO_GEMM_GROUP_DW=0: every product where backward meets it.
_dw_pending = {}


def _dw_gemm(dfr, A, B, Cc, M, N, K, a_kc, b_kc, lda, ldb, ldc, precision=None, a_planes=None, b_planes=None):
    """a Linear layer's weight-gradient product, inside `with _Deferring(w) as dfr`: launched, or -- single-part, operands
    packed, its gradient one that may stay unfinished until backward ends -- recorded for the grouped launch"""
    if not (dfr.on and precision == 4 and a_planes is not None and b_planes is not None and _lib.load().vilco_gemm_group_dw()):
        return gemm(A, B, Cc, M, N, K, a_kc, b_kc, lda, ldb, ldc, precision=precision, a_planes=a_planes, b_planes=b_planes)
    key = (int(M), int(N), int(K), int(a_kc), int(b_kc), int(ldc), Cc.data_ptr() % 16 == 0)
    _dw_pending.setdefault(key, []).append(((None, None, Cc.detach(), M, N, K, a_kc, b_kc, lda, ldb, ldc),
                                            dict(precision=4, a_planes=a_planes, b_planes=b_planes)))


def _dw_group_flush():
    """issue what `_dw_gemm` recorded: one grouped launch per key, on the "dw" side stream where that is forked"""
    if not _dw_pending:
        return
    items = list(_dw_pending.values())
    _dw_pending.clear()
    lib = _lib.load()
    fork = fork_enabled("dw")
    if fork:
        cur, side = torch.cuda.current_stream(), side_stream("dw")
        side.wait_stream(cur)
        ctx = torch.cuda.stream(side)
        ctx.__enter__()
    lib.vilco_defer_set(1)            # a small group still splits K: its slab sums join the deferred ones, and
    _defer["on"] = True               # every workspace is held until those have been issued
    try:
        for calls in items:
            if len(calls) == 1:
                gemm(*calls[0][0], **calls[0][1])
            else:
                gemm_group(calls)
    finally:
        lib.vilco_defer_set(0)
        _defer["on"] = False
        if fork:
            ctx.__exit__(None, None, None)
            cur.wait_stream(side)


# ---- what a producer already knows about its output.  The fp16 x2 planes need max|x| of the whole tensor before anything can be
# packed; kernels whose output goes (mostly) straight into a matrix product -- LayerNorm forward, the fused q/k/v
# pre-projection, the activation backward, the GEMM epilogues -- leave per-block partial maxima next to their output ("amax":
# `pack` hands them to vilco_pack_many, which then skips its amax launch), and some write the output's fp16 operand planes
# themselves ("planes": the consumer's `pack` / `pack_tap` is then a lookup, like for a tensor that was packed before).
# Both hang on the tensor as ONE record (`_Hints`), read and written through the accessors below and nowhere else.
# amax is ignored once the tensor's version counter moved (in-place edits) or another precision is active.
produce_amax = switches.on("VILCO_PRODUCER_AMAX")
AMAX_PARTS = 2048
_pack_cache = switches.on("VILCO_PACK_CACHE")


class _Hints:
    """The record of one tensor.  All of it describes the tensor's values at `version` (torch's in-place counter): once the
    counter has moved the whole record is dead, amax and planes alike.
    amax: (partials, count) of max|x|, or None;  planes: {layout: (plane buffer, `_plane_key`, `_cache_mark`)}, or None.
    (No __init__: some 500 of these are made per eager step, and a Python-level constructor doubles their cost.)"""
    __slots__ = ("version", "amax", "planes")


def _hints(t, create=False):
    """the record on t if it still describes t, else None -- create: else a fresh one, hung on t"""
    rec = getattr(t, "_vilco_hints", None)
    if rec is not None and rec.version == t._version:
        return rec
    if not create:
        return None
    rec = t._vilco_hints = _Hints()
    rec.version, rec.amax, rec.planes = t._version, None, None
    return rec


def _tag_amax(t, parts, n):
    if n > 0:
        _hints(t, True).amax = (parts, int(n))
    return t


def _amax_of(x):
    rec = _hints(x) if produce_amax else None
    return (None, 0) if rec is None or rec.amax is None else rec.amax


def _cache_mark(x):
    """the stream the planes remembered on x were written on, while capturing.  Inside a stream capture independent chains run on side
    streams (fork_enabled), and a chain that finds another chain's planes in this Python-level cache has no edge to the pack
    that writes them: `_cache_ok` treats such a hit as a miss and the chain packs its own (an event behind every pack would
    order it, at the price of ~290 extra event records per captured step).  Eager steps run on one stream."""
    return torch.cuda.current_stream() if x.is_cuda and torch.cuda.is_current_stream_capturing() else None


def _cache_ok(mark):
    return mark is None or not torch.cuda.is_current_stream_capturing() or mark == torch.cuda.current_stream()


def _plane_key(layout, shape, prec):
    """what remembered planes are valid for.  layout "nat": the row-major matrix shape = (rows, cols) that `pack` reads;
    "seq": the k=3 convs' zero-padded per-sequence image of shape = (B, T, C), `pack_tap`."""
    return (layout, tuple(shape), prec)


def _planes_of(x, layout, shape, prec, any_stream=False):
    """the planes remembered on x for this layout, shape and precision, or None.  any_stream: also those a capture wrote on
    another stream (which a consumer must not read: see `_cache_mark`)."""
    rec = _hints(x) if _pack_cache else None
    ent = rec.planes.get(layout) if rec is not None and rec.planes is not None else None
    if ent is None or ent[1] != _plane_key(layout, shape, prec) or not (any_stream or _cache_ok(ent[2])):
        return None
    return ent[0]


def _remember_planes(x, layout, shape, prec, buf):
    if _pack_cache:
        rec = _hints(x, True)
        if rec.planes is None:
            rec.planes = {}
        rec.planes[layout] = (buf, _plane_key(layout, shape, prec), _cache_mark(x))
    return buf


# ---- hints across Function.apply.  Attributes set on a tensor inside `forward` do not survive apply() (autograd hands back
# other Python objects), so a producer LEAVES its hints (`_leave`) and its public wrapper calls the Function through `_apply`,
# which hangs them on the tensors apply() returned, by output position.  One frame per `_apply` in flight: a wrapper called
# from inside another Function's forward has its own, and the outer one is on top again when it returns.
_handover = []


def _leave(fn, i, amax=None, planes=None, layout="nat"):
    """from fn.forward: output i of this call carries `amax` = (partials, count) of max|x| and / or `planes`, its fp16 x2
    operand planes in `layout` (producers write no other format).  Kept only when fn was called through `_apply`."""
    if _handover and _handover[-1][0] is fn:
        _handover[-1].append((i, amax, planes, layout))


def _apply(fn, *args):
    """fn.apply(*args), with what fn.forward left hung on the outputs"""
    frame = [fn]                         # then what `_leave` adds
    _handover.append(frame)
    try:
        out = fn.apply(*args)
    finally:
        _handover.pop()                  # (also when forward raises: nothing of this call can land on the next one's output)
    for i, amax, planes, layout in frame[1:]:
        t = out[i] if isinstance(out, tuple) else out
        if planes is not None:
            Cn = t.shape[-1]
            _remember_planes(t, layout, t.shape if layout == "seq" else (t.numel() // Cn, Cn), 3, planes)
        if amax is not None and amax[0] is not None:
            _tag_amax(t, *amax)
    return out


# ---- cuts of the autograd graph (vilco_amd.graph.GraphedStep, data-parallel replays).  With a tape active the
# backbone hands every pyramid level on as a detached LEAF (`seg_cut`): the backward of the step then runs as one
# torch.autograd.backward call per stage -- heads + losses first, then block by block -- each stops at the previous stage's
# leaves, whose accumulated .grad seeds the next call.  The stages are captured as separate hipGraphs, and between their
# replays the gradient buckets that are already complete go out on the collective's stream under the rest of backward.
class SegTape:
    def __init__(self):
        self.records = []          # (root tensor, leaf that continued the forward, stage that produced the root)
        self.stage = 0


seg_tape = None


def seg_cut(x, next_stage=False):
    """x -> the tensor the forward continues with: x itself, or (tape active) a leaf sharing its memory.
    next_stage: what follows belongs to the next stage."""
    tape = seg_tape
    if tape is None or not torch.is_tensor(x) or not x.requires_grad:
        return x
    leaf = x.detach().requires_grad_(True)
    rec = _hints(x)
    if rec is not None:                    # producer-written operand planes / maxima travel along (the leaf shares x's version counter)
        mine = _hints(leaf, True)
        mine.amax, mine.planes = rec.amax, None if rec.planes is None else dict(rec.planes)
    tape.records.append((x, leaf, tape.stage))
    if next_stage:
        tape.stage += 1
    return leaf


def _pack_item(it, x, rows, cols, prec, nbatch=1, relshift=False, seq_len=0, nbytes=None):
    """fill the vilco_pack_item `it` for the fp32 source x (`nbatch` contiguous [rows, cols] matrices), with the max|x|
    partials x's producer left and a fresh plane buffer of `nbytes` (None: as many as the item asks for) -> that buffer"""
    it.src, it.rows, it.cols, it.ld = x.data_ptr(), int(rows), int(cols), int(cols)
    it.nbatch, it.batch_stride = int(nbatch), int(rows) * int(cols) if nbatch > 1 else 0
    it.relshift, it.seq_len = int(bool(relshift)), int(seq_len)
    parts, n = _amax_of(x) if prec == 3 else (None, 0)       # max|x| partials left by the producer of the whole tensor
    if parts is not None:
        it.amax, it.namax = parts.data_ptr(), n
    if nbytes is None:
        nbytes = _lib.load().vilco_pack_item_bytes(C.byref(it), prec)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    it.planes, it.planes_bytes = buf.data_ptr(), nbytes
    return buf


def pack(x, rows, cols, precision=None):
    """One pass over the fp32 row-major matrix x[rows][cols] -> 16-bit operand planes (a uint8 tensor) that every
    product the tensor appears in consumes, in either orientation (vilco_pack, include/vilco_hip.h).  The planes are
    remembered on the tensor: an activation that feeds several layers (XLNet's h -> q, k, v) is packed once."""
    lib = _lib.load()
    prec = _precision if precision is None else int(precision)
    buf = _planes_of(x, "nat", (rows, cols), prec)
    if buf is not None:
        return buf
    nbytes = lib.vilco_pack_bytes(int(rows), int(cols), prec)
    if prec != 3 or _amax_of(x)[0] is None:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.vilco_pack(x.data_ptr(), int(rows), int(cols), int(cols), prec, buf.data_ptr(), nbytes, _stream()))
    else:
        it = _lib.PackItem()
        buf = _pack_item(it, x, rows, cols, prec, nbytes=nbytes)
        _lib.check(lib.vilco_pack_many(C.byref(it), 1, prec, _stream()))
    return _remember_planes(x, "nat", (rows, cols), prec, buf)


def pack_tap(x, precision=None):
    """x [B, T, C] (C % 8 == 0) -> the operand planes the k=3 convs read: every sequence with a zero row before and after it
    (vilco_pack_item.seq_len).  One pack of a conv's input serves its forward product and its weight gradient; one pack of
    the output gradient serves dX and the weight gradient.  Remembered on the tensor like `pack`."""
    prec = _precision if precision is None else int(precision)
    buf = _planes_of(x, "seq", x.shape, prec)
    if buf is not None:
        return buf
    B, T, Cn = x.shape
    it = _lib.PackItem()
    buf = _pack_item(it, x, B * T, Cn, prec, seq_len=T)
    _lib.check(_lib.load().vilco_pack_many(C.byref(it), 1, prec, _stream()))
    return _remember_planes(x, "seq", x.shape, prec, buf)


def pack_many(items, precision=None, nbatch=1, relshift=False):
    """[(x, rows, cols), ...] (at most four) packed by the same two launches -> list of plane buffers.
    nbatch > 1: every x holds `nbatch` contiguous [rows, cols] matrices (planes for batched GEMMs);
    relshift: pack XLNet's unshifted [rows, rows + cols] view of each matrix (vilco_pack_item.relshift)."""
    prec = _precision if precision is None else int(precision)
    arr = (_lib.PackItem * len(items))()
    bufs = [_pack_item(it, x, rows, cols, prec, nbatch, relshift) for it, (x, rows, cols) in zip(arr, items)]
    _lib.check(_lib.load().vilco_pack_many(arr, len(items), prec, _stream()))
    return bufs


pack_group_enabled = switches.on("VILCO_PACK_GROUP")
ln_bwd_amax = switches.on("VILCO_LN_BWD_AMAX")            # LayerNorm backward leaves max|dx| partials
conv_dz_planes = switches.on("VILCO_CONV_DZ_PLANES")      # masked k=3 convs: dZ's operand image from the mask kernel itself


def pack_group(xs, rows, cols, precision=None):
    """`[pack(x, rows, cols) for x in xs]` for 2..4 tensors of ONE shape that are packed back to back on one chain (the q / k / v
    inputs of an attention block's projections, their three output gradients): one launch (vilco_pack_many) instead of len(xs),
    the same planes bit for bit, remembered on the tensors like `pack`.  Falls back to per-tensor packs when any of them already
    carries its planes (a cache hit must stay a hit), when the tensors repeat, or VILCO_PACK_GROUP=0."""
    prec = _precision if precision is None else int(precision)
    n = len(xs)
    fresh = all(_planes_of(x, "nat", (rows, cols), prec, any_stream=True) is None for x in xs)
    if (not pack_group_enabled or not (2 <= n <= 4) or not fresh or len({x.data_ptr() for x in xs}) != n
            or any(not x.is_contiguous() for x in xs)):
        return [pack(x, rows, cols, precision) for x in xs]
    bufs = pack_many([(x, rows, cols) for x in xs], precision=prec)
    return [_remember_planes(x, "nat", (rows, cols), prec, buf) for x, buf in zip(xs, bufs)]


# packed operands are shared between forward, dX and dW (env VILCO_PACK_REUSE=0: every GEMM packs its own operands)
_reuse_packs = switches.on("VILCO_PACK_REUSE")
# k=3 convs: x and dZ packed once each in the zero-padded per-sequence image, for all three products (VILCO_CONV_TAP_PLANES=0,
# or VILCO_CONV_DW_KM=0 which also takes the weight gradient back to its transposing packs)
conv_tap_planes = switches.on("VILCO_CONV_TAP_PLANES") and switches.on("VILCO_CONV_DW_KM")

# ---- weight planes are packed ONCE per parameter version, not once per step.  A weight's planes (and the re-laid
# [Cout][tap][Cin] images of k=3 conv weights) are cached on the parameter object, keyed by torch's in-place version
# counter plus a generation number that everything writing parameters behind autograd's back must bump
# (`weights_changed()`: FusedOptimizer.step does).  VILCO_WEIGHT_CACHE=0 re-packs on every call.
_weight_cache = switches.on("VILCO_WEIGHT_CACHE")
_weight_gen = [0]


def weights_changed():
    """call after writing parameter memory through raw pointers (the fused optimizer kernels)"""
    _weight_gen[0] += 1


def _cached(w, tag, build):
    """`build()` result cached on w's owning tensor under (tag, storage offset, shape, precision), valid while the
    owner's version counter and the global weight generation stand still."""
    if not _weight_cache:
        return build()
    owner = w._base if w._base is not None else w
    if owner.requires_grad and not owner.is_leaf:
        return build()                                      # an activation, not a stored weight
    store = owner.__dict__.setdefault("_vilco_cache", {})
    key = (tag, w.data_ptr(), tuple(w.shape), _precision)
    ver = (owner._version, _weight_gen[0])
    ent = store.get(key)
    if ent is not None and ent[0] == ver:
        return ent[1]
    val = build()
    store[key] = (ver, val)
    return val


def forget_weight_planes(params):
    """drop the cached planes / images of these parameters, keeping their max|w| tags.  For a forward that is NOT followed by
    an update (A-GEM's reference pass): the next step would otherwise find the planes valid and, when it is being captured,
    record no pack -- a replayed graph must pack the weights it reads inside itself (vilco_amd/graph.py)."""
    for p in params:
        p.__dict__.pop("_vilco_cache", None)


def tag_weight_amax(p, parts, n):
    """max|p| partials of parameter p left by whoever wrote it (FusedOptimizer.step: vilco_optim_desc.chunk_amax); valid until
    p's version counter or the weight generation moves.  Call after weights_changed()."""
    p._vilco_wamax = (parts, int(n), p._version, _weight_gen[0])


def _weight_amax(w):
    """(partials, count) for the pack of the stored weight w -- only when w is its whole owning parameter"""
    owner = w._base if w._base is not None else w
    tag = getattr(owner, "_vilco_wamax", None)
    if (tag is None or not produce_amax or _precision != 3 or tag[2] != owner._version or tag[3] != _weight_gen[0]
            or w.numel() != owner.numel()):
        return None, 0
    return tag[0], tag[1]


def _weight_src(w, src):
    """`src` (w.detach() or a permuted image of it: the same multiset of values) carrying w's amax tag"""
    parts, n = _weight_amax(w)
    return src if parts is None else _tag_amax(src, parts, n)


def weight_planes(w, rows, cols):
    """operand planes of the stored matrix w [rows][cols] (a Linear / 1x1-conv weight, an XLNet projection)"""
    return _cached(w, ("planes", rows, cols), lambda: pack(_weight_src(w, w.detach()), rows, cols))


# dz of a layer goes nowhere but into its two backward products: `_act_bwd(planes=True)` has the kernel write dz as operand planes
# (vilco_act_bwd_desc.planes: scale from a bound on max|dz|, no pack launch, no fp32 dz) when dy carries its producer's amax partials.
# VILCO_PRODUCER_PLANES=0: fp32 dz + pack, as before.
producer_planes = switches.on("VILCO_PRODUCER_PLANES")
ln_planes = switches.on("VILCO_LN_PLANES")          # the LayerNorm half of it (ops.layernorm(planes=...))
attn_planes = switches.on("VILCO_ATTN_PLANES")      # the attention-output part (hd = 64 forward kernels)


def _act_bwd(dy, aux, act, lens, T, want_bias, drop=(0.0, 0), bias_param=None, planes=False, row_mask=None):
    """dz = dropmask(dy) * act'(aux) * rowmask, optional column sums -> (dz, dbias).  bias_param: the parameter dbias is the
    gradient of (its column sum may then finish with the other deferred reductions, see _Deferring).
    planes=True -> (dz or None, dbias, operand planes of dz or None): when the planes come back, dz was never written."""
    lib = _lib.load()
    rows, Cn = dy.numel() // dy.shape[-1], dy.shape[-1]
    # planes == "seq" (round 6, the masked k=3 convs): the planes in the convs' zero-padded per-sequence image of T-row sequences
    seq = int(T) if planes == "seq" else 0
    fits = (Cn % 8 == 0 and seq > 0 and rows % seq == 0 and conv_tap_planes) if planes == "seq" else Cn % 32 == 0
    dy_parts, dy_n = _amax_of(dy) if (planes and producer_planes and _precision == 3 and fits and rows > 0) else (None, 0)
    pz = None
    if dy_parts is not None:
        nbytes = lib.vilco_act_bwd_planes_bytes(rows, Cn, seq)
        pz = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    dz = torch.empty_like(dy) if pz is None else None
    db = torch.empty(Cn, dtype=torch.float32, device=dy.device) if want_bias else None
    with _Deferring(bias_param if want_bias else None) as dfr:
        ws = _ws(lib.vilco_colsum_workspace(rows, Cn), dy.device) if want_bias else None
        parts = torch.empty(AMAX_PARTS, dtype=torch.float32, device=dy.device) if (produce_amax and _precision == 3 and pz is None) else None
        n = C.c_int32(0)
        d = _lib.ActBwdDesc(dy=dy.data_ptr(), aux=_p(aux), dz=_p(dz), dbias=_p(db), act=act, len=_p(lens), T=int(T or 0), rows=rows,
                            C=Cn, drop_p=float(drop[0]), drop_seed=int(drop[1]), workspace=_p(ws),
                            workspace_bytes=ws.numel() if ws is not None else 0, amax_parts=_p(parts), n_parts=C.addressof(n),
                            dy_amax=_p(dy_parts), n_dy_amax=int(dy_n), planes=_p(pz),
                            planes_bytes=pz.numel() if pz is not None else 0, seq_len=seq, row_mask=_p(row_mask))
        _lib.check(lib.vilco_act_bwd(C.byref(d), _stream()))
        dfr.hold(db)
    if parts is not None:
        _tag_amax(dz, parts, n.value)
    return (dz, db, pz) if planes else (dz, db)


def colsum(x2d, param=None):
    """column sums of x2d; param: the parameter the result is the gradient of (deferred finish, see _Deferring)"""
    lib = _lib.load()
    rows, Cn = x2d.shape
    out = torch.empty(Cn, dtype=torch.float32, device=x2d.device)
    with _Deferring(param) as dfr:
        ws = _ws(lib.vilco_colsum_workspace(rows, Cn), x2d.device)
        _lib.check(lib.vilco_colsum(x2d.data_ptr(), out.data_ptr(), rows, Cn, ws.data_ptr(), ws.numel(),
                                    _stream()))
        dfr.hold(out, x2d)
    return out


class _BiasAdd(torch.autograd.Function):
    """x [..., C] + b (C elements, any shape).  The backward of the plain expression `x + b.view(1, 1, -1)` is ATen's `sum` over
    all rows -- a multi-block reduction whose semaphores are cleared by a memset INSIDE the op; on torch 2.10 + ROCm 7 that kernel
    writes its result on the first replay of a captured hipGraph only and leaves the output untouched afterwards
    (tools/lab/sum_graph_probe.py, profiles/r06_sum_graph_probe.txt: every later replay returns the first one's sum) -- the cause
    of round 5's "null-stream hazard": XLNet's r_w_bias / r_r_bias gradients stood still in replayed steps at full size.  Here the
    bias gradient is a column sum by this library's own kernels (vilco_colsum; deferred finish like every other bias gradient)."""

    @staticmethod
    def forward(ctx, x, b):
        _chk(x, b)
        ctx.bshape = b.shape
        ctx.save_for_backward(b)
        return x + b.reshape(*([1] * (x.dim() - 1)), -1)

    @staticmethod
    def backward(ctx, dy):
        (b,) = ctx.saved_tensors
        dy = dy.contiguous()
        Cn = dy.shape[-1]
        db = colsum(dy.view(-1, Cn), param=b).view(ctx.bshape) if ctx.needs_input_grad[1] else None
        return (dy if ctx.needs_input_grad[0] else None), db


def bias_add(x, b):
    """x + b broadcast over the rows, with the bias gradient summed by vilco_colsum instead of ATen (see _BiasAdd)"""
    return _BiasAdd.apply(x, b)


class _Linear(torch.autograd.Function):
    """y = act(x W^T + b) * rowmask.  x [..., K] token-major, W [N, K] (conv1x1 / nn.Linear weight)."""

    @staticmethod
    def forward(ctx, x, w, b, act, lens, T, drop_p=0.0, drop_site="dropout", bwd_precision=None):
        _chk(x, w, b)
        K = x.shape[-1]
        N = w.shape[0]
        ctx.bwd_precision = bwd_precision
        assert w.numel() == N * K, "weight shape %s does not match input dim %d" % (tuple(w.shape), K)
        M = x.numel() // K
        y = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
        pre = torch.empty_like(y) if act == ACT_GELU else None
        px = pw = None
        if _reuse_packs:
            ctx.prec = _precision
            if _weight_cache:
                px, pw = pack(x, M, K), weight_planes(w, N, K)
            else:
                px, pw = pack_many([(x, M, K), (w, N, K)])
        ctx.drop = _new_drop(drop_site, drop_p, y.shape)      # nn.Dropout after the layer, fused into the epilogue
        gemm(x, w, y, M, N, K, 1, 1, K, K, N, bias=b, preact=pre, act=act, row_len=lens,
             rowT=T or 0, a_planes=px, b_planes=pw, drop=ctx.drop, want_amax=True)
        _leave(_Linear, 0, amax=_amax_of(y))             # max|y| partials left by the GEMM epilogue
        ctx.act, ctx.T = act, T
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, w, pre if act == ACT_GELU else (y if act == ACT_RELU else None), lens, px, pw, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, aux, lens, px, pw, b = ctx.saved_tensors
        dy = dy.contiguous()
        K, N = x.shape[-1], w.shape[0]
        M = x.numel() // K
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        pz = None
        if ctx.act != ACT_NONE or lens is not None or ctx.drop[0] > 0.0:
            # (the planes of dz straight from the kernel when both products below take planes in the ambient format)
            want_planes = ctx.bwd_precision is None and px is not None and ctx.prec == 3 and _precision == 3
            r = _act_bwd(dy, aux, ctx.act, lens, ctx.T, need_db, ctx.drop, bias_param=b, planes=want_planes)
            dz, db, pz = r if want_planes else (r[0], r[1], None)
        else:
            dz, db = dy, (colsum(dy.view(M, N), param=b) if need_db else None)
        dx = dw = None
        prec = None
        if ctx.bwd_precision is None and range_check != "0" and _range_wide(dz if dz is not None else dy, M, N, K):
            if dz is None:                 # (the producer wrote planes only: this call needs the fp32 tensor after all)
                dz = _act_bwd(dy, aux, ctx.act, lens, ctx.T, False, ctx.drop)[0]
            ctx.bwd_precision = 2
        if ctx.bwd_precision is not None:
            # a call site whose gradient tensors span more exponent range than one scale per tensor can carry (see
            # `wide_range` in modeling/blocks.py: ChannelAttention): both backward products from the fp32 tensors, in the
            # requested format (bf16 x3: 8 exponent bits per element)
            bp = int(ctx.bwd_precision)
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                gemm(dz, w, dx, M, K, N, 1, 0, N, K, K, precision=bp)
            if ctx.needs_input_grad[1]:
                dw = _grad_out(w)
                gemm(dz, x, dw, N, K, M, 0, 0, N, K, K, precision=bp)
            return dx, dw, db, None, None, None, None, None, None
        if px is not None:                       # one pack of dZ feeds dX and dW; X and W planes come from forward
            prec = ctx.prec
            if pz is None:
                pz = pack(dz, M, N, prec)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gemm(dz, w, dx, M, K, N, 1, 0, N, K, K, precision=prec, a_planes=pz, b_planes=pw, want_amax=True)   # dX = dZ W     (NN)
        if ctx.needs_input_grad[1]:
            with _DwFork(w, M), _Deferring(w) as dfr:     # (may finish, or run as a whole, with the deferred ones: _dw_gemm)
                dw = _grad_out(w)
                _dw_gemm(dfr, dz, x, dw, N, K, M, 0, 0, N, K, K, precision=_dw_prec(prec, M), a_planes=pz, b_planes=px)   # dW = dZ^T X   (TN)
        return dx, dw, db, None, None, None, None, None, None


class _LinearGroup(torch.autograd.Function):
    """(y_i = x_i W_i^T + b_i) for n independent plain Linear layers of ONE shape -- an attention block's q / k / v projections
    (MQ/libs/modeling/blocks.py:332-344) -- with the n forward products and the n dX products each as one grouped launch
    (vilco_gemm_group).  Per layer it is _Linear without activation / mask / dropout: same packs, same kernels, same sums."""

    @staticmethod
    def forward(ctx, n, *args):
        xs, ws, bs = args[:n], args[n:2 * n], args[2 * n:3 * n]
        _chk(*xs, *ws, *bs)
        K, N = xs[0].shape[-1], ws[0].shape[0]
        M = xs[0].numel() // K
        ys = [torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device) for x in xs]
        pxs = pack_group(xs, M, K)
        pws = [weight_planes(w, N, K) for w in ws]
        gemm_group([((x, w, y, M, N, K, 1, 1, K, K, N), dict(bias=b, a_planes=px, b_planes=pw, want_amax=True))
                    for x, w, b, y, px, pw in zip(xs, ws, bs, ys, pxs, pws)])
        ctx.n, ctx.prec = n, _precision
        for i, y in enumerate(ys):
            _leave(_LinearGroup, i, amax=_amax_of(y))            # max|y| partials left by the GEMM epilogue
        ctx.save_for_backward(*xs, *ws, *bs, *pxs, *pws)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        n = ctx.n
        sv = ctx.saved_tensors
        xs, ws, bs, pxs, pws = sv[:n], sv[n:2 * n], sv[2 * n:3 * n], sv[3 * n:4 * n], sv[4 * n:5 * n]
        K, N = xs[0].shape[-1], ws[0].shape[0]
        M = xs[0].numel() // K
        dys = [dy.contiguous() for dy in dys]
        dbs = [colsum(dy.view(M, N), param=b) if ctx.needs_input_grad[1 + 2 * n + i] else None for i, (dy, b) in enumerate(zip(dys, bs))]
        pzs = pack_group(dys, M, N, ctx.prec)
        need_dx = [ctx.needs_input_grad[1 + i] for i in range(n)]
        dxs = [torch.empty_like(x) if nd else None for x, nd in zip(xs, need_dx)]
        calls = [((dy, w, dx, M, K, N, 1, 0, N, K, K), dict(precision=ctx.prec, a_planes=pz, b_planes=pw, want_amax=True))
                 for dy, w, dx, pz, pw in zip(dys, ws, dxs, pzs, pws) if dx is not None]
        if len(calls) > 1:
            gemm_group(calls)                                     # dX_i = dY_i W_i   (NN), one launch
        else:
            for a, k in calls:
                gemm(*a, **k)
        dws = []
        for i, (dy, x, w, pz, px) in enumerate(zip(dys, xs, ws, pzs, pxs)):
            if ctx.needs_input_grad[1 + n + i]:
                with _DwFork(w, M), _Deferring(w) as dfr:
                    dw = _grad_out(w)
                    _dw_gemm(dfr, dy, x, dw, N, K, M, 0, 0, N, K, K, precision=_dw_prec(ctx.prec, M), a_planes=pz, b_planes=px)   # dW = dY^T X
                dws.append(dw)
            else:
                dws.append(None)
        return (None, *dxs, *dws, *dbs)


linear_group_enabled = switches.on("VILCO_LINEAR_GROUP")


def linear_group(xs, ws, bs):
    """[x_i W_i^T + b_i]: independent Linear layers of one shape as grouped launches (falls back to `linear` per layer when the
    shapes differ, a bias is missing, the ambient format is not fp16 x2, or VILCO_LINEAR_GROUP=0)."""
    n = len(xs)
    same = (linear_group_enabled and 2 <= n <= 4 and _precision == 3 and _reuse_packs and _weight_cache and range_check == "0"
            and all(b is not None for b in bs)
            and all(x.shape == xs[0].shape and w.shape == ws[0].shape for x, w in zip(xs, ws)))
    if not same:
        return [linear(x, w, b) for x, w, b in zip(xs, ws, bs)]
    return list(_apply(_LinearGroup, n, *xs, *ws, *bs))


def linear(x, w, b=None, act=ACT_NONE, lens=None, T=None, drop_p=0.0, drop_site="dropout", bwd_precision=None):
    """drop_p: nn.Dropout(drop_p) applied to the layer's output (pass 0 outside training), fused into the GEMM epilogue.
    With a ReLU (output saved as the activation witness) the dropout stays a separate op.
    bwd_precision: operand format of this layer's two backward products when not the ambient one (2 = bf16 x3)."""
    if drop_p > 0.0 and act == ACT_RELU:
        return dropout(_apply(_Linear, x, w, b, act, lens, T, 0.0, drop_site, bwd_precision), drop_p, True, drop_site)
    return _apply(_Linear, x, w, b, act, lens, T, float(drop_p), drop_site, bwd_precision)


class _LinearKN(torch.autograd.Function):
    """y = x W + b with W stored [K, N] (XLNet's einsum("ibh,hnd->ibnd") projections,
    modeling_xlnet_x.py:437-443, viewed as [D, H*hd])."""

    @staticmethod
    def forward(ctx, x, w, b):
        _chk(x, w, b)
        K = x.shape[-1]
        N = w.numel() // K
        M = x.numel() // K
        y = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
        px = pw = None
        if _reuse_packs:
            ctx.prec = _precision
            if _weight_cache:
                px, pw = pack(x, M, K), weight_planes(w, K, N)
            else:
                px, pw = pack_many([(x, M, K), (w, K, N)])
        gemm(x, w, y, M, N, K, 1, 0, K, N, N, bias=b, a_planes=px, b_planes=pw)                 # NN
        ctx.has_bias = b is not None
        ctx.bshape = None if b is None else b.shape
        ctx.save_for_backward(x, w, px, pw)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, px, pw = ctx.saved_tensors
        dy = dy.contiguous()
        K = x.shape[-1]
        N = w.numel() // K
        M = x.numel() // K
        dx = dw = db = pz = None
        prec = None
        if px is not None:
            prec = ctx.prec
            pz = pack(dy, M, N, prec)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gemm(dy, w, dx, M, K, N, 1, 1, N, N, K, precision=prec, a_planes=pz, b_planes=pw)   # dX = dY W^T   (NT)
        if ctx.needs_input_grad[1]:
            with _DwFork(w, M), _Deferring(w) as dfr:
                dw = _grad_out(w)
                _dw_gemm(dfr, x, dy, dw, K, N, M, 0, 0, K, N, N, precision=_dw_prec(prec, M), a_planes=px, b_planes=pz)   # dW = X^T dY   (TN)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = colsum(dy.view(M, N)).view(ctx.bshape)
        return dx, dw, db


def linear_kn(x, w, b=None):
    return _LinearKN.apply(x, w, b)


def permute3(src, dims, off, strides, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty(dims, dtype=torch.float32, device=src.device)
    assert tuple(out.shape) == tuple(dims) and out.is_contiguous()
    _lib.check(lib.vilco_permute3(src.data_ptr(), out.data_ptr(), dims[0], dims[1], dims[2], off,
                                  strides[0], strides[1], strides[2], _stream()))
    return out


def _conv3_weight(w, dims, off, strides, rows, cols):
    """(re-laid conv weight, its operand planes or None when the conv's GEMM packs for itself)"""
    wp = _weight_src(w, permute3(w.detach(), dims, off, strides))
    planes = pack(wp, rows, cols) if _reuse_packs else None
    return wp, planes


class _Conv3(torch.autograd.Function):
    """k=3 'same' conv over time + bias, output rows masked (MaskedConv1D, blocks.py:106-130).
    x [B,T,Cin], w [Cout,Cin,3] (reference layout) -> y [B,T,Cout].  Implicit GEMM over overlapped
    token rows (K = 3*Cin), no im2col buffer."""

    @staticmethod
    def forward(ctx, x, w, b, lens, row_mask=None):
        _chk(x, w, b, row_mask)
        assert row_mask is None or row_mask.numel() == x.shape[0] * x.shape[1]
        B, T, Cin = x.shape
        Cout = w.shape[0]
        assert w.shape[1] == Cin and w.shape[2] == 3
        # [Cout][tap][Cin] image of the weight and its planes: built once per weight version
        wp, pwp = _cached(w, "conv3_fwd", lambda: _conv3_weight(w, (Cout, 3, Cin), 0, (Cin * 3, 1, 3), Cout, 3 * Cin))
        y = torch.empty(B, T, Cout, dtype=torch.float32, device=x.device)
        # x in the convs' zero-padded image: packed once, read by this product and by the weight gradient in backward
        px = pack_tap(x) if (_reuse_packs and conv_tap_planes and pwp is not None and Cin % 8 == 0) else None
        gemm(x, wp, y, B * T, Cout, 3 * Cin, 1, 1, Cin, 3 * Cin, Cout, tap=TAP_A, tapC=Cin, tapT=T,
             bias=b, row_len=lens, rowT=T, a_planes=px, b_planes=pwp, a_amax=_amax_of(x), planes_seq=(px is not None, False),
             row_mask=row_mask)
        ctx.has_bias = b is not None
        ctx.prec = _precision
        ctx.save_for_backward(x, w, lens, b, px, row_mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, lens, b, px, row_mask = ctx.saved_tensors
        B, T, Cin = x.shape
        Cout = w.shape[0]
        dy = dy.contiguous()
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        want_planes = px is not None and Cout % 8 == 0 and ctx.prec == _precision
        pz = None
        if lens is not None or row_mask is not None:
            # (round 6) the mask multiply writes dZ straight into the convs' operand image when both backward products will read
            # planes: no fp32 dz, no pack_tap launch (conv_dz_planes; needs dy's amax partials -- LayerNorm backward leaves them)
            direct = (want_planes and conv_dz_planes and ctx.prec == 3 and range_check == "0" and _weight_cache
                      and (not ctx.needs_input_grad[0] or _cached(w, "conv3_dx", lambda: _conv3_weight(w, (Cin, 3, Cout), 2, (3, -1, Cin * 3), Cin, 3 * Cout))[1] is not None))
            if direct:
                dz, db, pz = _act_bwd(dy, None, ACT_NONE, lens, T, need_db, bias_param=b, planes="seq", row_mask=row_mask)
            else:
                dz, db = _act_bwd(dy, None, ACT_NONE, lens, T, need_db, bias_param=b, row_mask=row_mask)
        else:
            dz, db = dy, (colsum(dy.view(B * T, Cout), param=b) if need_db else None)
        dx = dw = None
        # dZ in the convs' image: one pack for dX and the weight gradient (needs the format the forward planes were made in)
        if pz is None:
            pz = pack_tap(dz, ctx.prec) if want_planes else None
        if ctx.needs_input_grad[0]:
            # wt[ci][j'][co] = w[co][ci][2-j']: dX is the k=3 conv of dZ with flipped taps
            wt, pwt = _cached(w, "conv3_dx", lambda: _conv3_weight(w, (Cin, 3, Cout), 2, (3, -1, Cin * 3), Cin, 3 * Cout))
            dx = torch.empty_like(x)
            gemm(dz, wt, dx, B * T, Cin, 3 * Cout, 1, 1, Cout, 3 * Cout, Cin, tap=TAP_A, tapC=Cout,
                 tapT=T, a_planes=pz if pwt is not None else None, b_planes=pwt, a_amax=_amax_of(dz) if dz is not None else None,
                 planes_seq=(pz is not None and pwt is not None, False))
        if ctx.needs_input_grad[1]:
            with _DwFork(w, B * T):
                dwp = torch.empty(Cout, 3 * Cin, dtype=torch.float32, device=x.device)
                if pz is not None:          # k-major x k-major over the padded token rows: no operand pack at all (gemm.hip: make_plan)
                    gemm(dz, x, dwp, Cout, 3 * Cin, B * T, 0, 0, Cout, Cin, 3 * Cin, tap=TAP_B, tapC=Cin,
                         tapT=T, precision=_dw_prec(ctx.prec, B * T), a_planes=pz, b_planes=px, planes_seq=(True, True))
                else:
                    gemm(dz, x, dwp, Cout, 3 * Cin, B * T, 0, 0, Cout, Cin, 3 * Cin, tap=TAP_B, tapC=Cin,
                         tapT=T, precision=_dw_prec(_precision, B * T), a_amax=_amax_of(dz), b_amax=_amax_of(x))
                dw = permute3(dwp, (Cout, Cin, 3), 0, (3 * Cin, 1, Cin), out=_grad_out(w))
        return dx, dw, db, None, None


def conv3(x, w, b=None, lens=None, row_mask=None):
    """row_mask: one float per token row ([B, T] or [B, T, 1], contiguous); output rows whose entry is 0 are zeroed (and take no
    gradient) -- the validity pattern of the heads over the concatenated pyramid levels, which `lens` cannot express"""
    return _Conv3.apply(x, w, b, lens, row_mask)


# ---------------------------------------------------------------------------------------- LayerNorm
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, planes=None, row_mask=None, skip=False):
        _chk(x, gamma, beta, row_mask)
        assert row_mask is None or relu, "row_mask: the backward kernel drops masked rows through the ReLU test on the saved output"
        ctx.skip = bool(skip)
        ctx.set_materialize_grads(False)
        lib = _lib.load()
        Cn = x.shape[-1]
        rows = x.numel() // Cn
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        parts = torch.empty(AMAX_PARTS, dtype=torch.float32, device=x.device) if (produce_amax and _precision == 3) else None
        n = C.c_int32(0)
        # planes: "nat" / "seq" -- the caller knows y goes into a Linear / a k=3 conv: the kernel writes its operand planes too
        seq = int(x.shape[-2]) if planes == "seq" else 0
        ok = (planes in ("nat", "seq") and producer_planes and ln_planes and _pack_cache and _reuse_packs and _precision == 3 and rows > 0 and
              (Cn % 8 == 0 and x.dim() == 3 and conv_tap_planes if seq else Cn % 32 == 0))
        buf = None
        if ok:
            nbytes = lib.vilco_layernorm_planes_bytes(rows, Cn, seq)
            buf = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        d = _lib.LnFwdDesc(x=x.data_ptr(), gamma=_p(gamma), beta=_p(beta), y=y.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(),
                           rows=rows, C=Cn, eps=eps, relu=int(relu), amax_parts=_p(parts), n_parts=C.addressof(n), planes=_p(buf),
                           planes_bytes=buf.numel() if buf is not None else 0, seq_len=seq, row_mask=_p(row_mask),
                           mask_rows=row_mask.numel() if row_mask is not None else 0)
        _lib.check(lib.vilco_layernorm_fwd(C.byref(d), _stream()))
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, gamma, mean, rstd, y if relu else None)
        _leave(_LayerNorm, 0, amax=(parts, n.value), planes=buf, layout="seq" if seq else "nat")
        # skip: x is returned as a second output (autograd makes it a view of x).  A block that opens a residual branch with
        # this LayerNorm takes its skip connection from THAT tensor: the gradient over the skip then arrives here, and the
        # backward kernel adds it to dx itself instead of autograd summing the two with a launch of its own (55 per P step).
        return (y, x) if skip else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, gamma, mean, rstd, y = ctx.saved_tensors
        lib = _lib.load()
        if dy is None:                           # only the skip output was used
            return dskip, None, None, None, None, None, None, None
        dy = dy.contiguous()
        if dskip is not None:
            dskip = dskip.contiguous()
        Cn = x.shape[-1]
        rows = x.numel() // Cn
        dx = torch.empty_like(x)
        dg = torch.empty(Cn, dtype=torch.float32, device=x.device)
        db = torch.empty(Cn, dtype=torch.float32, device=x.device)
        with _Deferring(gamma) as dfr:           # the d-gamma / d-beta column sums may finish with the other deferred ones
            ws = _ws(lib.vilco_layernorm_bwd_workspace(rows, Cn), x.device)
            # (round 6) max|dx| partials ride along: dx is the output gradient of the layer in front (a masked k=3 conv of the heads /
            # the embedding: its mask kernel then writes the operand image itself, _act_bwd(planes="seq"))
            parts = (torch.empty(AMAX_PARTS, dtype=torch.float32, device=x.device)
                     if (ln_bwd_amax and produce_amax and producer_planes and _precision == 3) else None)
            n = C.c_int32(0)
            d = _lib.LnBwdDesc(dy=dy.data_ptr(), x=x.data_ptr(), y=_p(y), gamma=_p(gamma), mean=mean.data_ptr(), rstd=rstd.data_ptr(),
                               dres=_p(dskip), dx=dx.data_ptr(), dgamma=dg.data_ptr(), dbeta=db.data_ptr(), rows=rows, C=Cn,
                               relu=int(ctx.relu), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                               dx_amax_parts=_p(parts), n_parts=C.addressof(n))
            _lib.check(lib.vilco_layernorm_bwd(C.byref(d), _stream()))
            dfr.hold(dg, db)
            if parts is not None and n.value > 0:
                _tag_amax(dx, parts, n.value)
        return dx, dg.view_as(gamma), db.view_as(gamma), None, None, None, None, None


# parity tooling (tests/test_fullsize_gpu.py): a list -> every LayerNorm -> ReLU call appends (site, y > 0), the derivative mask the
# backward kernel will use, so that an oracle run can be handed exactly the sign decisions this step took
relu_log = None
relu_log_values = False      # True: the entries also carry y itself (site, y > 0, y) -- which side of zero, and by how much


def layernorm(x, gamma, beta, eps=1e-5, relu=False, planes=None, row_mask=None, skip=False, site=None):
    """gamma/beta may have the reference's [1,C,1] shape (blocks.py:152-155) or [C].
    skip: return (y, x_skip) -- x_skip is x as an output of this op; use it for the residual connection around the branch
    that y feeds, and the backward kernel adds the skip gradient to dx itself (see _LayerNorm.forward).
    planes: "nat" when y feeds a Linear, "seq" when it feeds a k=3 conv -- the kernel then writes y's operand planes as well
    (vilco_ln_fwd_desc.planes) and the consumer's `pack` / `pack_tap` finds them on the tensor.
    row_mask (relu only): a contiguous 0 / 1 float mask over the token rows, repeated over the batch -- y[b, t] *= row_mask[t]."""
    y = _apply(_LayerNorm, x, gamma, beta, float(eps), bool(relu), planes, row_mask, bool(skip and fold_skip_grads and x.requires_grad))
    xs = x
    if isinstance(y, tuple):
        y, xs = y
    if relu and relu_log is not None:
        relu_log.append((site, y.detach() > 0, y.detach().clone()) if relu_log_values else (site, y.detach() > 0))
    return (y, xs) if skip else y


# ---------------------------------------------------------------------------------------- dwconv / pool
class _DwConv3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, lens, stride):
        _chk(x, w)
        lib = _lib.load()
        B, T, Cn = x.shape
        y = torch.empty(B, T // stride, Cn, dtype=torch.float32, device=x.device)
        _lib.check(lib.vilco_dwconv3_fwd(x.data_ptr(), w.data_ptr(), lens.data_ptr(), y.data_ptr(), B,
                                         T, Cn, stride, _stream()))
        ctx.stride = stride
        ctx.save_for_backward(x, w, lens)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, lens = ctx.saved_tensors
        lib = _lib.load()
        dy = dy.contiguous()
        B, T, Cn = x.shape
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        with _Deferring(w if dw is not None else None) as dfr:
            ws = _ws(lib.vilco_dwconv3_bwd_workspace(B, T, Cn, ctx.stride), x.device)
            _lib.check(lib.vilco_dwconv3_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), lens.data_ptr(),
                                             _p(dx), _p(dw), B, T, Cn, ctx.stride, ws.data_ptr(),
                                             ws.numel(), _stream()))
            dfr.hold(dw)
        return dx, dw, None, None


def dwconv3(x, w, lens, stride):
    """w: [C,1,3] (reference depthwise conv weight, blocks.py:315-318)."""
    return _DwConv3.apply(x, w, lens, int(stride))


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lens):
        _chk(x)
        lib = _lib.load()
        B, T, Cn = x.shape
        y = torch.empty(B, T // 2, Cn, dtype=torch.float32, device=x.device)
        _lib.check(lib.vilco_maxpool3s2_fwd(x.data_ptr(), lens.data_ptr(), y.data_ptr(), B, T, Cn,
                                            _stream()))
        ctx.save_for_backward(x, lens)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, lens = ctx.saved_tensors
        lib = _lib.load()
        dy = dy.contiguous()
        B, T, Cn = x.shape
        dx = torch.empty_like(x)
        _lib.check(lib.vilco_maxpool3s2_bwd(dy.data_ptr(), x.data_ptr(), lens.data_ptr(),
                                            dx.data_ptr(), B, T, Cn, _stream()))
        return dx, None


def maxpool3s2(x, lens):
    return _MaxPool.apply(x, lens)


# ---------------------------------------------------------------------------------------- glue
class _ScaleAdd(torch.autograd.Function):
    """out = a*(mask_a ? m : 1) + colscale (.) rowscale (.) b   (blocks.py:567,573,576)."""

    @staticmethod
    def forward(ctx, a, b, colscale, rowscale, lens, mask_a):
        _chk(a, b, colscale, rowscale)
        lib = _lib.load()
        B, T, Cn = b.shape
        out = torch.empty_like(b)
        _lib.check(lib.vilco_scale_add_fwd(out.data_ptr(), _p(a), b.data_ptr(), _p(colscale),
                                           _p(rowscale), _p(lens), int(mask_a), B, T, Cn, _stream()))
        ctx.mask_a = int(mask_a)
        ctx.has_a = a is not None
        ctx.save_for_backward(b, colscale, rowscale, lens)
        return out

    @staticmethod
    def backward(ctx, dout):
        b, colscale, rowscale, lens = ctx.saved_tensors
        lib = _lib.load()
        dout = dout.contiguous()
        B, T, Cn = b.shape
        need_a = ctx.has_a and ctx.needs_input_grad[0]
        need_b = ctx.needs_input_grad[1]
        need_cs = colscale is not None and ctx.needs_input_grad[2]
        plain_a = need_a and not (ctx.mask_a and lens is not None)
        da = dout if plain_a else (torch.empty_like(b) if need_a else None)
        plain_b = need_b and colscale is None and rowscale is None
        db = dout if plain_b else (torch.empty_like(b) if need_b else None)
        dcs = torch.empty(Cn, dtype=torch.float32, device=b.device) if need_cs else None
        if (need_a and not plain_a) or (need_b and not plain_b) or need_cs:
            # (db goes up the residual branch into its last layer's backward: its max|db| partials ride along, see _act_bwd)
            parts = (torch.empty(AMAX_PARTS, dtype=torch.float32, device=b.device)
                     if (need_b and not plain_b and produce_amax and producer_planes and _precision == 3) else None)
            n = C.c_int32(0)
            with _Deferring(colscale if need_cs else None) as dfr:
                ws = _ws(lib.vilco_colsum_workspace(B * T, Cn), b.device) if need_cs else None
                d = _lib.ScaleAddBwdDesc(dout=dout.data_ptr(), bval=b.data_ptr(), colscale=_p(colscale), rowscale=_p(rowscale),
                                         len=_p(lens), mask_a=ctx.mask_a, da=None if plain_a else _p(da),
                                         db=None if plain_b else _p(db), dcolscale=_p(dcs), B=B, T=T, C=Cn, workspace=_p(ws),
                                         workspace_bytes=ws.numel() if ws is not None else 0, db_amax_parts=_p(parts),
                                         n_parts=C.addressof(n))
                _lib.check(lib.vilco_scale_add_bwd(C.byref(d), _stream()))
                dfr.hold(dcs)
            if parts is not None:
                _tag_amax(db, parts, n.value)
        return da, db, (dcs.view_as(colscale) if need_cs else None), None, None, None


def scale_add(a, b, colscale=None, rowscale=None, lens=None, mask_a=False):
    return _ScaleAdd.apply(a, b, colscale, rowscale, lens, bool(mask_a))


class _Axpby(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, alpha, beta):
        _chk(a, b)
        lib = _lib.load()
        out = torch.empty_like(a)
        _lib.check(lib.vilco_axpby(out.data_ptr(), a.data_ptr(), _p(b), alpha, beta, a.numel(),
                                   _stream()))
        ctx.alpha, ctx.beta = alpha, beta
        ctx.has_b = b is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        dout = dout.contiguous()

        def scaled(s):
            if s == 1.0:
                return dout
            o = torch.empty_like(dout)
            _lib.check(lib.vilco_axpby(o.data_ptr(), dout.data_ptr(), None, s, 0.0, dout.numel(),
                                       _stream()))
            return o
        da = scaled(ctx.alpha) if ctx.needs_input_grad[0] else None
        db = scaled(ctx.beta) if (ctx.has_b and ctx.needs_input_grad[1]) else None
        return da, db, None, None


def axpby(a, b, alpha, beta):
    return _Axpby.apply(a, b, float(alpha), float(beta))


class _AddPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pe, lens):
        _chk(x, pe)
        lib = _lib.load()
        B, T, Cn = x.shape
        out = torch.empty_like(x)
        _lib.check(lib.vilco_add_pe(out.data_ptr(), x.data_ptr(), pe.data_ptr(), lens.data_ptr(), B, T,
                                    Cn, _stream()))
        return out

    @staticmethod
    def backward(ctx, dout):
        return dout, None, None


def add_pe(x, pe_tm, lens):
    """x + pe[t] * mask; pe_tm is the [T, C] token-major slice of the sinusoid table."""
    return _AddPE.apply(x, pe_tm, lens)


class _Transpose(torch.autograd.Function):
    """[Z, R, S] -> [Z, S, R] (the channel-first <-> token-major boundary)."""

    @staticmethod
    def forward(ctx, x):
        _chk(x)
        lib = _lib.load()
        Z, R, S = x.shape
        out = torch.empty(Z, S, R, dtype=torch.float32, device=x.device)
        _lib.check(lib.vilco_transpose2d(x.data_ptr(), out.data_ptr(), Z, R, S, _stream()))
        return out

    @staticmethod
    def backward(ctx, dout):
        return _Transpose.apply(dout.contiguous())


def transpose(x):
    return _Transpose.apply(x)


def mask_rows_(x, lens):
    """in place x[b,t,:] = 0 for t >= lens[b] (no autograd; used on inputs)."""
    lib = _lib.load()
    B, T, Cn = x.shape
    _lib.check(lib.vilco_mask_rows(x.data_ptr(), lens.data_ptr(), B, T, Cn, _stream()))
    return x


# ---------------------------------------------------------------------------------------- attention
MASK_KEYS, MASK_XLNET, MASK_NONE = 0, 1, 2
MASK_XLNET_REL = 3      # XLNet mask + bias given as UNSHIFTED position scores [B,H,Tq,Tq+Tk] (attn.hip: bias_at)
MASK_LOCAL = 4          # sliding window |i - j| <= window below kv_len (NLQ LocalMaskedMHCA)
use_flash = True     # fused attention kernels when the head dim is supported; False = materialised scores


def _softmax_(s, kv_len, B, H, Tq, Tk, mode):
    lib = _lib.load()
    _lib.check(lib.vilco_softmax_fwd(s.data_ptr(), _p(kv_len), B, H, Tq, Tk, mode, _stream()))


class _Attention(torch.autograd.Function):
    """softmax(scale * q k^T + mask) v per head; q [B,Tq,C], k/v [B,Tk,C], heads = channel slices
    (blocks.py:383-400 / 251-265).  Round 1: scores are materialised ([B,H,Tq,Tk] fp32) and the
    contractions run on the batched MFMA GEMM; P is kept for backward."""

    @staticmethod
    def forward(ctx, q, k, v, kv_len, H, scale, mode):
        _chk(q, k, v)
        B, Tq, Cn = q.shape
        Tk = k.shape[1]
        hd = Cn // H
        P = torch.empty(B, H, Tq, Tk, dtype=torch.float32, device=q.device)
        gemm(q, k, P, Tq, Tk, hd, 1, 1, Cn, Cn, Tk, batch=(B, H), sA=(Tq * Cn, hd), sB=(Tk * Cn, hd),
             sC=(H * Tq * Tk, Tq * Tk), alpha=scale)
        _softmax_(P, kv_len, B, H, Tq, Tk, mode)
        o = torch.empty_like(q)
        gemm(P, v, o, Tq, hd, Tk, 1, 0, Tk, Cn, Cn, batch=(B, H), sA=(H * Tq * Tk, Tq * Tk),
             sB=(Tk * Cn, hd), sC=(Tq * Cn, hd))
        ctx.H, ctx.scale = H, scale
        ctx.save_for_backward(q, k, v, P)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, P = ctx.saved_tensors
        lib = _lib.load()
        do = do.contiguous()
        H, scale = ctx.H, ctx.scale
        B, Tq, Cn = q.shape
        Tk = k.shape[1]
        hd = Cn // H
        sP = (H * Tq * Tk, Tq * Tk)
        dv = torch.empty_like(v)
        gemm(P, do, dv, Tk, hd, Tq, 0, 0, Tk, Cn, Cn, batch=(B, H), sA=sP, sB=(Tq * Cn, hd),
             sC=(Tk * Cn, hd))                                                 # dV = P^T dO
        dP = torch.empty_like(P)
        gemm(do, v, dP, Tq, Tk, hd, 1, 1, Cn, Cn, Tk, batch=(B, H), sA=(Tq * Cn, hd),
             sB=(Tk * Cn, hd), sC=sP)                                          # dP = dO V^T
        _lib.check(lib.vilco_softmax_bwd(dP.data_ptr(), P.data_ptr(), B, H, Tq, Tk, _stream()))
        dq = torch.empty_like(q)
        gemm(dP, k, dq, Tq, hd, Tk, 1, 0, Tk, Cn, Cn, batch=(B, H), sA=sP, sB=(Tk * Cn, hd),
             sC=(Tq * Cn, hd), alpha=scale)                                    # dQ = dS K
        dk = torch.empty_like(k)
        gemm(dP, q, dk, Tk, hd, Tq, 0, 0, Tk, Cn, Cn, batch=(B, H), sA=sP, sB=(Tq * Cn, hd),
             sC=(Tk * Cn, hd), alpha=scale)                                    # dK = dS^T Q
        return dq, dk, dv, None, None, None, None


def flash_supported(hd):
    """head dims 4..128 in steps of 4; above 64 not in bf16x3 (three planes of a 128-wide tile exceed the LDS)"""
    return bool(_lib.load().vilco_attn_supported(int(hd))) and (hd <= 64 or _precision != 2)


def _attn_amax_parts(B, H, T, hd, mode, bias, drop, key_side):
    """partials the fused kernels leave for the packs of their outputs (0: this configuration does not emit them)"""
    if not produce_amax:
        return 0
    return int(_lib.load().vilco_attn_amax_parts(B, H, T, hd, int(mode), _precision, int(bias is not None), float(drop[0]), key_side))


def _attn_amax_in(q, k, v, do=None):
    """partials the producers of q / k / v / dO left (GEMM epilogues): the attention call then skips its amax pass"""
    if _precision != 3:
        return None
    a = _lib.AttnAmaxIn()
    keep = []
    for name, t in (("q", q), ("k", k), ("v", v), ("dout", do)):
        if t is None:
            continue
        parts, n = _amax_of(t)
        if parts is not None:
            setattr(a, name, parts.data_ptr())
            setattr(a, "n" + ("do" if name == "dout" else name), n)
            keep.append(parts)
    return (a, keep) if keep else None


def _flash_fwd(q, k, v, bias, kv_len, H, scale, mode, drop=(0.0, 0), window=0, hints_to=None, hint_amax=True):
    """-> (o, lse).  hints_to: the Function this call is the forward of -- its output 0 is o, and carries what the kernel
    leaves for the output projection: o's operand planes, and (hint_amax) its max|o| partials."""
    lib = _lib.load()
    B, Tq, Cn = q.shape
    Tk = k.shape[1]
    o = torch.empty_like(q)
    lse = torch.empty(B, H, Tq, dtype=torch.float32, device=q.device)
    nws = lib.vilco_attn_fwd_workspace(B, H, Tq, Tk, Cn // H, _precision)
    ws = _ws(nws, q.device)
    na = _attn_amax_parts(B, H, Tq, Cn // H, mode, bias, drop, 0)
    am = torch.empty(na, dtype=torch.float32, device=q.device) if na else None
    ain = _attn_amax_in(q, k, v)
    # the output goes into the output projection: the hd = 64 kernels write its operand planes themselves (|o| <= max|v| / keep)
    planes = None
    if (producer_planes and attn_planes and _pack_cache and _reuse_packs and _precision == 3 and B * Tq > 0 and
            lib.vilco_attn_planes_supported(Tq, Tk, Cn // H, int(mode), _precision, int(bias is not None), float(drop[0]))):
        planes = torch.empty(lib.vilco_pack_bytes(B * Tq, Cn, 3), dtype=torch.uint8, device=q.device)
    d = _lib.AttnDesc(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), bias=_p(bias), kv_len=_p(kv_len), o=o.data_ptr(),
                      lse=lse.data_ptr(), B=B, H=H, Tq=Tq, Tk=Tk, hd=Cn // H, scale=scale, mode=mode, window=int(window),
                      precision=_precision, drop_p=float(drop[0]), drop_seed=int(drop[1]), amax_in=C.addressof(ain[0]) if ain else None,
                      workspace=ws.data_ptr(), workspace_bytes=nws, o_amax=_p(am), o_planes=_p(planes),
                      o_planes_bytes=planes.numel() if planes is not None else 0)
    _lib.check(lib.vilco_attn_fwd(C.byref(d), _stream()))
    if hints_to is not None:
        _leave(hints_to, 0, amax=(am, na) if hint_amax else None, planes=planes)
    return o, lse


# XLNet backward: dS as operand planes of the unshifted view straight from the dQ kernel (vilco_attn_desc.ds_planes) instead of
# fp32 dS + a pack of it.  The kernel writes the band only; everything else in the buffer must be zero and stays zero, so ONE
# buffer per (device, B*H, T) is zeroed when first needed and reused by every later backward (1.36 GB at config P; a step
# captured as a hipGraph has met it in the eager iterations before the capture).  VILCO_XL_DS_PLANES=0: the fp32 dS + pack path.
# residual joins: the skip gradient is added inside the LayerNorm backward kernel (VILCO_FOLD_SKIP=0: autograd's own add_)
fold_skip_grads = switches.on("VILCO_FOLD_SKIP")
xl_ds_planes = switches.on("VILCO_XL_DS_PLANES")
# XLNet forward: the position scores by vilco_xl_scores (dedicated kernel) instead of the band-limited K = 64 GEMM (VILCO_XL_SCORES=0)
xl_scores_kernel = switches.on("VILCO_XL_SCORES")
_ds_plane_bufs = {}


_capture_pins = None       # while graph.GraphedStep captures: the persistent buffers the recorded kernels address by raw pointer


def _xl_ds_planes_buf(B, H, T, device):
    """The persistent, zero-outside-the-band plane buffer of XLNet's dS (~1.4 GB at config P), one per (device, B, H, T).  At
    most two stay cached; an evicted one is only DROPPED from this table -- a captured hipGraph that recorded its address holds
    its own reference (`_capture_pins`, kept in the graph's entry by GraphedStep), so the memory stays the graph's until the
    graph goes (a third shape used to free a buffer a live graph still wrote through)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), B, H, T)
    buf = _ds_plane_bufs.get(key)
    if buf is None:
        if torch.cuda.is_current_stream_capturing():
            return None                                      # never allocate-and-zero inside a capture: fall back for this call
        if len(_ds_plane_bufs) >= 2:
            _ds_plane_bufs.clear()                           # shapes that keep changing: keep at most two buffers cached
        buf = torch.zeros(int(_lib.load().vilco_attn_dsplanes_bytes(B, H, T)), dtype=torch.uint8, device=device)
        _ds_plane_bufs[key] = buf
    if _capture_pins is not None and all(b is not buf for b in _capture_pins):
        _capture_pins.append(buf)
    return buf


def _flash_bwd(q, k, v, bias, kv_len, o, lse, do, H, scale, mode, want_dbias, drop=(0.0, 0), window=0, ds_planes=None):
    """ds_planes: (XLNet fast path) buffer the dQ kernel writes dS' operand planes into; the returned dbias is then None"""
    lib = _lib.load()
    B, Tq, Cn = q.shape
    Tk = k.shape[1]
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    want_dbias = bool(want_dbias) and ds_planes is None
    dbias = torch.empty(B, H, Tq, Tk, dtype=torch.float32, device=q.device) if want_dbias else None
    nws = lib.vilco_attn_bwd_workspace(B, H, Tq, Tk, Cn // H, _precision)
    ws = _ws(nws, q.device)
    nq = nk = nds = 0
    if ds_planes is None and not want_dbias:
        nq = _attn_amax_parts(B, H, Tq, Cn // H, mode, bias, drop, 0)
        nk = _attn_amax_parts(B, H, Tk, Cn // H, mode, bias, drop, 1)
    am = torch.empty(nq + 2 * nk, dtype=torch.float32, device=q.device) if nq and nk else None
    aq, ak, av = (am[:nq], am[nq:nq + nk], am[nq + nk:]) if am is not None else (None, None, None)
    ain = _attn_amax_in(q, k, v, do)
    if want_dbias and bias is not None and produce_amax and _precision == 3 and mode == MASK_XLNET_REL and Tq == Tk:
        nds = int(lib.vilco_attn_amax_parts(B, H, Tq, Cn // H, int(mode), _precision, 2, float(drop[0]), 0))
    ads = torch.empty(nds, dtype=torch.float32, device=q.device) if nds else None
    d = _lib.AttnDesc(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), bias=_p(bias), kv_len=_p(kv_len), o=o.data_ptr(),
                      lse=lse.data_ptr(), B=B, H=H, Tq=Tq, Tk=Tk, hd=Cn // H, scale=scale, mode=mode, window=int(window),
                      precision=_precision, drop_p=float(drop[0]), drop_seed=int(drop[1]), amax_in=C.addressof(ain[0]) if ain else None,
                      workspace=ws.data_ptr(), workspace_bytes=nws, dout=do.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(),
                      dv=dv.data_ptr(), dbias=_p(dbias), dq_amax=_p(aq), dk_amax=_p(ak), dv_amax=_p(av), dbias_amax=_p(ads),
                      ds_planes=_p(ds_planes), ds_planes_bytes=ds_planes.numel() if ds_planes is not None else 0)
    _lib.check(lib.vilco_attn_bwd(C.byref(d), _stream()))
    if ads is not None:
        _tag_amax(dbias, ads, nds)
    if am is not None:
        _tag_amax(dq, aq, nq)
        _tag_amax(dk, ak, nk)
        _tag_amax(dv, av, nk)
    return dq, dk, dv, dbias


class _FlashAttention(torch.autograd.Function):
    """fused attention (vilco_attn_fwd / vilco_attn_bwd): scores never reach HBM; backward recomputes P
    from (q, k, lse)."""

    @staticmethod
    def forward(ctx, q, k, v, kv_len, H, scale, mode, drop_p=0.0, window=0):
        _chk(q, k, v)
        ctx.drop = _new_drop("attn_prob", drop_p, (q.shape[0], H, q.shape[1], k.shape[1]))
        o, lse = _flash_fwd(q, k, v, None, kv_len, H, scale, mode, ctx.drop, window, hints_to=_FlashAttention)
        ctx.H, ctx.scale, ctx.mode, ctx.window = H, scale, mode, window
        ctx.save_for_backward(q, k, v, kv_len, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, kv_len, o, lse = ctx.saved_tensors
        dq, dk, dv, _ = _flash_bwd(q, k, v, None, kv_len, o, lse, do.contiguous(), ctx.H, ctx.scale, ctx.mode, False,
                                   ctx.drop, ctx.window)
        return dq, dk, dv, None, None, None, None, None, None


def attention(q, k, v, kv_len, n_head, scale=None, mode=MASK_KEYS, drop_p=0.0, window=0):
    """drop_p: dropout on the attention probabilities (training only; the caller passes 0 in eval).
    mode MASK_LOCAL: sliding-window self-attention, keys |i - j| <= window (fused kernels only)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1] // n_head)
    if use_flash and flash_supported(q.shape[-1] // n_head):
        return _apply(_FlashAttention, q, k, v, kv_len, int(n_head), float(scale), int(mode), float(drop_p), int(window))
    if mode == MASK_LOCAL:
        raise NotImplementedError("local-window attention needs the fused kernels (head dim <= 160, multiple of 4)")
    if drop_p > 0.0:
        raise NotImplementedError("attention dropout needs the fused kernels (head dim <= 160, multiple of 4)")
    return _Attention.apply(q, k, v, kv_len, int(n_head), float(scale), int(mode))


class _RelAttention(torch.autograd.Function):
    """XLNet relative attention core (modeling_xlnet_x.py:270-320, bi / no mems / no segments):
    score = scale * ((q + r_w_bias) k^T + rel_shift((q + r_r_bias) k_r^T)) - 1e30 * mask, softmax, @ v.
    qw = q + r_w_bias and qr = q + r_r_bias are formed by the caller.  kr: [2T, C] (no batch)."""

    @staticmethod
    def forward(ctx, qw, qr, k, v, kr, kv_len, H, scale):
        _chk(qw, qr, k, v, kr)
        lib = _lib.load()
        B, T, Cn = qw.shape
        hd = Cn // H
        sP = (H * T * T, T * T)
        P = torch.empty(B, H, T, T, dtype=torch.float32, device=qw.device)
        gemm(qw, k, P, T, T, hd, 1, 1, Cn, Cn, T, batch=(B, H), sA=(T * Cn, hd), sB=(T * Cn, hd), sC=sP,
             alpha=scale)
        bd = torch.empty(B, H, T, 2 * T, dtype=torch.float32, device=qw.device)
        gemm(qr, kr, bd, T, 2 * T, hd, 1, 1, Cn, Cn, 2 * T, batch=(B, H), sA=(T * Cn, hd), sB=(0, hd),
             sC=(H * T * 2 * T, T * 2 * T))
        _lib.check(lib.vilco_relshift_add(P.data_ptr(), bd.data_ptr(), scale, B, H, T, _stream()))
        del bd
        _softmax_(P, kv_len, B, H, T, T, MASK_XLNET)
        o = torch.empty_like(qw)
        gemm(P, v, o, T, hd, T, 1, 0, T, Cn, Cn, batch=(B, H), sA=sP, sB=(T * Cn, hd), sC=(T * Cn, hd))
        ctx.H, ctx.scale = H, scale
        ctx.save_for_backward(qw, qr, k, v, kr, P)
        return o

    @staticmethod
    def backward(ctx, do):
        qw, qr, k, v, kr, P = ctx.saved_tensors
        lib = _lib.load()
        do = do.contiguous()
        H, scale = ctx.H, ctx.scale
        B, T, Cn = qw.shape
        hd = Cn // H
        sP = (H * T * T, T * T)
        sX = (T * Cn, hd)
        dv = torch.empty_like(v)
        gemm(P, do, dv, T, hd, T, 0, 0, T, Cn, Cn, batch=(B, H), sA=sP, sB=sX, sC=sX)
        dS = torch.empty_like(P)
        gemm(do, v, dS, T, T, hd, 1, 1, Cn, Cn, T, batch=(B, H), sA=sX, sB=sX, sC=sP)
        _lib.check(lib.vilco_softmax_bwd(dS.data_ptr(), P.data_ptr(), B, H, T, T, _stream()))
        dqw = torch.empty_like(qw)
        gemm(dS, k, dqw, T, hd, T, 1, 0, T, Cn, Cn, batch=(B, H), sA=sP, sB=sX, sC=sX, alpha=scale)
        dk = torch.empty_like(k)
        gemm(dS, qw, dk, T, hd, T, 0, 0, T, Cn, Cn, batch=(B, H), sA=sP, sB=sX, sC=sX, alpha=scale)
        # position term: d(bd) = scale * unshift(dS)
        dbd = torch.empty(B, H, T, 2 * T, dtype=torch.float32, device=qw.device)
        _lib.check(lib.vilco_relshift_bwd(dS.data_ptr(), dbd.data_ptr(), scale, B, H, T, _stream()))
        sB2 = (H * T * 2 * T, T * 2 * T)
        dqr = torch.empty_like(qr)
        gemm(dbd, kr, dqr, T, hd, 2 * T, 1, 0, 2 * T, Cn, Cn, batch=(B, H), sA=sB2, sB=(0, hd), sC=sX)
        # d(kr)[2T, hd] per head = sum_b dbd[b]^T qr[b]: accumulate over the batch with beta = 1
        dkr = torch.zeros_like(kr)
        for b in range(B):
            gemm(dbd, qr, dkr, 2 * T, hd, T, 0, 0, 2 * T, Cn, Cn, batch=(1, H), sA=(0, T * 2 * T),
                 sB=(0, hd), sC=(0, hd), offA=b * H * T * 2 * T, offB=b * T * Cn, beta=1.0)
        return dqw, dqr, dk, dv, dkr, None, None, None


class _FlashRelAttention(torch.autograd.Function):
    """XLNet relative attention (modeling_xlnet_x.py:270-325) with the content term fused: the position scores
    bd = qr kr^T are one band-limited batched GEMM that the flash kernels read unshifted (mask mode 3); backward
    gets dS and derives the position-term gradients from one batched pack of it.  kr is [2T, C] (shared by the
    batch) or [B, 2T, C] (per clip: the reference drops out the expanded position embedding per batch element)."""

    @staticmethod
    def forward(ctx, qw, qr, k, v, kr, kv_len, H, scale, drop_p=0.0):
        _chk(qw, qr, k, v, kr)
        B, T, Cn = qw.shape
        hd = Cn // H
        sKr = (2 * T * Cn if kr.dim() == 3 else 0, hd)
        bd = torch.empty(B, H, T, 2 * T, dtype=torch.float32, device=qw.device)
        if xl_scores_kernel and hd == 64 and _precision == 3 and qr.is_contiguous() and kr.is_contiguous():
            lib = _lib.load()        # the attention kernels' first product on (qr, kr): only the band p in [T-i, 2T-i) is written
            nws = lib.vilco_xl_scores_workspace(B, H, T, int(kr.dim() == 3))
            ws = _ws(nws, qw.device)
            _lib.check(lib.vilco_xl_scores(qr.data_ptr(), kr.data_ptr(), bd.data_ptr(), B, H, T, hd, int(kr.dim() == 3), _precision,
                                           ws.data_ptr(), nws, _stream()))
        else:
            gemm(qr, kr, bd, T, 2 * T, hd, 1, 1, Cn, Cn, 2 * T, batch=(B, H), sA=(T * Cn, hd), sB=sKr,
                 sC=(H * T * 2 * T, T * 2 * T), band=1, bandT=T)      # only the band p in [T-i, 2T-i) is ever read
        ctx.drop = _new_drop("attn_prob", drop_p, (B, H, T, T))
        # the flash kernel reads the unshifted scores in place (mask mode 3): no [T,T] bias tensor, no shift pass
        # (the planes only: this output has never carried its max|o| partials, and where the kernel writes no planes they
        # would send the output projection's pack through another library entry)
        o, lse = _flash_fwd(qw, k, v, bd, kv_len, H, scale, MASK_XLNET_REL, ctx.drop, hints_to=_FlashRelAttention, hint_amax=False)
        ctx.H, ctx.scale = H, scale
        ctx.save_for_backward(qw, qr, k, v, kr, kv_len, bd, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        qw, qr, k, v, kr, kv_len, bd, o, lse = ctx.saved_tensors
        lib = _lib.load()
        H, scale = ctx.H, ctx.scale
        B, T, Cn = qw.shape
        hd = Cn // H
        per_clip = kr.dim() == 3
        sKr = (2 * T * Cn if per_clip else 0, hd)
        pd = None
        if (xl_ds_planes and _reuse_packs and _precision == 3 and hd == 64 and T % 64 == 0
                and lib.vilco_attn_planes_supported(T, T, hd, MASK_XLNET_REL, _precision, 1, float(ctx.drop[0]))):
            pd = _xl_ds_planes_buf(B, H, T, qw.device)
        dqw, dk, dv, dS = _flash_bwd(qw, k, v, bd, kv_len, o, lse, do.contiguous(), H, scale, MASK_XLNET_REL, True,
                                     ctx.drop, ds_planes=pd)
        del bd
        sX, sB2 = (T * Cn, hd), (H * T * 2 * T, T * 2 * T)
        dqr = torch.empty_like(qr)
        if _reuse_packs:
            # d(bd) = scale * unshift(dS) is never materialised: dS in the unshifted [T, 2T] view (per b, h) as operand planes --
            # written by the dQ kernel itself (pd), or ONE pack of the fp32 dS -- feeds dqr = d(bd) kr (k-contiguous) and
            # dkr = [sum_b] d(bd)^T qr (k-major)
            if pd is None:
                (pd,) = pack_many([(dS, T, T)], nbatch=B * H, relshift=True)
            del dS
            gemm(None, kr, dqr, T, hd, 2 * T, 1, 0, 2 * T, Cn, Cn, batch=(B, H), sA=sB2, sB=sKr, sC=sX,
                 alpha=scale, a_planes=pd, band=2, bandT=T)
            dkr_b = torch.empty(B, 2 * T, Cn, dtype=torch.float32, device=kr.device)
            gemm(None, qr, dkr_b, 2 * T, hd, T, 0, 0, 2 * T, Cn, Cn, batch=(B, H), sA=sB2, sB=sX,
                 sC=(2 * T * Cn, hd), alpha=scale, a_planes=pd, band=3, bandT=T)
            dkr = dkr_b if per_clip else (dkr_b.sum(0) if B > 1 else dkr_b[0])
        else:
            dbd = torch.empty(B, H, T, 2 * T, dtype=torch.float32, device=qw.device)
            _lib.check(lib.vilco_relshift_bwd(dS.data_ptr(), dbd.data_ptr(), scale, B, H, T, _stream()))
            del dS
            gemm(dbd, kr, dqr, T, hd, 2 * T, 1, 0, 2 * T, Cn, Cn, batch=(B, H), sA=sB2, sB=sKr, sC=sX)
            dkr = torch.zeros_like(kr)
            for b in range(B):
                gemm(dbd, qr, dkr, 2 * T, hd, T, 0, 0, 2 * T, Cn, Cn, batch=(1, H), sA=(0, T * 2 * T),
                     sB=(0, hd), sC=(0, hd), offA=b * H * T * 2 * T, offB=b * T * Cn,
                     offC=b * 2 * T * Cn if per_clip else 0, beta=0.0 if per_clip else 1.0)
        return dqw, dqr, dk, dv, dkr, None, None, None, None


def rel_attention(qw, qr, k, v, kr, kv_len, n_head, scale, drop_p=0.0):
    """kr [2T, C] or [B, 2T, C]; drop_p: dropout on the attention probabilities (training only)."""
    if use_flash and flash_supported(qw.shape[-1] // n_head):
        return _apply(_FlashRelAttention, qw, qr, k, v, kr, kv_len, int(n_head), float(scale), float(drop_p))
    if drop_p > 0.0 or kr.dim() == 3:
        raise NotImplementedError("XLNet dropout needs the fused attention kernels (head dim <= 160, multiple of 4)")
    return _RelAttention.apply(qw, qr, k, v, kr, kv_len, int(n_head), float(scale))


_unit = {}


def _unit_bound(device):
    """(partials, count) saying max|x| <= 1: the scale bound of a softmax output"""
    t = _unit.get(device)
    if t is None:
        if torch.cuda.is_current_stream_capturing():      # (never allocate a cached constant from a graph's private pool)
            return (None, 0)
        t = _unit[device] = torch.ones(1, dtype=torch.float32, device=device)
    return (t, 1)


class _ChannelAttn(torch.autograd.Function):
    """ChannelAttention core (blocks.py:426-434) on a fused qkv [B,T,3C]:
    A_h = softmax_rows(scale * k_h^T v_h)  [hd,hd];  out_h[t,:] = q_h[t,:] A_h^T."""

    @staticmethod
    def forward(ctx, qkv, H, scale, bwd_precision=None):
        _chk(qkv)
        ctx.bp = bwd_precision
        B, T, C3 = qkv.shape
        Cn = C3 // 3
        hd = Cn // H
        sQ = (T * C3, hd)
        A = torch.empty(B, H, hd, hd, dtype=torch.float32, device=qkv.device)
        # operand scales without a pass over the operands: max|qkv| (left by the qkv projection's epilogue) bounds each of its
        # three slices, a softmax output is bounded by 1
        qa, one = _amax_of(qkv), _unit_bound(qkv.device)
        gemm(qkv, qkv, A, hd, hd, T, 0, 0, C3, C3, hd, batch=(B, H), sA=sQ, sB=sQ, sC=(H * hd * hd, hd * hd),
             offA=Cn, offB=2 * Cn, alpha=scale, a_amax=qa, b_amax=qa)            # (k*scale)^T v
        _softmax_(A, None, B, H, hd, hd, MASK_NONE)
        out = torch.empty(B, T, Cn, dtype=torch.float32, device=qkv.device)
        gemm(qkv, A, out, T, hd, hd, 1, 1, C3, hd, Cn, batch=(B, H), sA=sQ, sB=(H * hd * hd, hd * hd),
             sC=(T * Cn, hd), want_amax=True, a_amax=qa, b_amax=one)             # q A^T (its output goes straight into proj)
        _leave(_ChannelAttn, 0, amax=_amax_of(out))
        ctx.H, ctx.scale = H, scale
        ctx.save_for_backward(qkv, A)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, A = ctx.saved_tensors
        lib = _lib.load()
        dout = dout.contiguous()
        H, scale = ctx.H, ctx.scale
        B, T, C3 = qkv.shape
        Cn = C3 // 3
        hd = Cn // H
        sQ = (T * C3, hd)
        sA_ = (H * hd * hd, hd * hd)
        sO = (T * Cn, hd)
        dqkv = torch.empty_like(qkv)
        # dq[t,e] = sum_d dout[t,d] A[d,e]                                   (NN)
        bp = ctx.bp                            # None: the ambient format (see _Linear.backward on bwd_precision)
        qa, da, one = _amax_of(qkv), _amax_of(dout), _unit_bound(qkv.device)      # (scales from bounds, as in forward)
        gemm(dout, A, dqkv, T, hd, hd, 1, 0, Cn, hd, C3, batch=(B, H), sA=sO, sB=sA_, sC=sQ, precision=bp, a_amax=da, b_amax=one)
        # dA[d,e] = sum_t dout[t,d] q[t,e]                                   (TN)
        dA = torch.empty_like(A)
        gemm(dout, qkv, dA, hd, hd, T, 0, 0, Cn, C3, hd, batch=(B, H), sA=sO, sB=sQ, sC=sA_, precision=bp, a_amax=da, b_amax=qa)
        _lib.check(lib.vilco_softmax_bwd(dA.data_ptr(), A.data_ptr(), B, H, hd, hd, _stream()))
        # S[d,e] = scale * sum_t k[t,d] v[t,e]:  dk[t,d] = scale * sum_e v[t,e] dS[d,e]   (NT)
        gemm(qkv, dA, dqkv, T, hd, hd, 1, 1, C3, hd, C3, batch=(B, H), sA=sQ, sB=sA_, sC=sQ,
             offA=2 * Cn, offC=Cn, alpha=scale, precision=bp, a_amax=qa)
        # dv[t,e] = scale * sum_d k[t,d] dS[d,e]                                          (NN)
        gemm(qkv, dA, dqkv, T, hd, hd, 1, 0, C3, hd, C3, batch=(B, H), sA=sQ, sB=sA_, sC=sQ, offA=Cn,
             offC=2 * Cn, alpha=scale, precision=bp, a_amax=qa)
        return dqkv, None, None, None


def channel_attention(qkv, n_head, scale, bwd_precision=None):
    return _apply(_ChannelAttn, qkv, int(n_head), float(scale), bwd_precision)


# ---------------------------------------------------------------------------------------- labels + losses
_almax_state = {}


class _MQLoss(torch.autograd.Function):
    """label_points + losses of the heads (meta_archs.py:1253-1344, 1374-1447) as two launches each way
    (vilco_mq_loss_fwd / _bwd).  Returns (cls_loss, reg_loss, al_loss, final_loss); `loss_norm` (device float[1]) is the
    loss_normalizer EMA, updated in place."""

    @staticmethod
    def forward(ctx, logits, offsets, level_scale, gauss, tables, level_len, gt, loss_norm, cfg):
        _chk(logits, offsets, level_scale, gauss)
        lib = _lib.load()
        B, R, Cn = logits.shape
        points, row_level, row_pos = tables
        d = _lib.LossDesc()
        d.logits, d.offsets, d.level_scale = logits.data_ptr(), offsets.data_ptr(), _p(level_scale)
        d.points, d.row_level, d.row_pos = points.data_ptr(), row_level.data_ptr(), row_pos.data_ptr()
        d.level_len, d.gt, d.gauss, d.loss_norm = level_len.data_ptr(), gt.data_ptr(), gauss.data_ptr(), loss_norm.data_ptr()
        d.B, d.R, d.C, d.L, d.Nmax = B, R, Cn, level_len.shape[1], (gt.shape[1] - 1) // 3
        d.center_radius, d.label_smoothing, d.momentum = cfg['radius'], cfg['smoothing'], cfg['momentum']
        d.loss_weight, d.al_weight, d.use_al = cfg['loss_weight'], cfg['al_weight'], int(cfg['use_al'])
        key = (logits.device.index, B * Cn)
        st = _almax_state.get(key)
        if st is None:
            st = _almax_state[key] = torch.zeros(B * Cn, dtype=torch.int64, device=logits.device)
        nws = lib.vilco_mq_loss_workspace(B, R, Cn)
        ws = _ws(nws, logits.device)
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        saved = torch.empty(1, dtype=torch.float32, device=logits.device)
        _lib.check(lib.vilco_mq_loss_fwd(C.byref(d), out.data_ptr(), saved.data_ptr(), st.data_ptr(), ws.data_ptr(), nws,
                                         _stream()))
        ctx.desc, ctx.keep = d, (points, row_level, row_pos, level_len, gt, loss_norm)
        ctx.save_for_backward(logits, offsets, level_scale, gauss, saved, ws)
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def backward(ctx, g_cls, g_reg, g_al, g_final):
        logits, offsets, level_scale, gauss, saved, ws = ctx.saved_tensors
        lib = _lib.load()
        d = ctx.desc
        dl, do = torch.empty_like(logits), torch.empty_like(offsets)
        dsc = torch.empty_like(level_scale) if level_scale is not None else None
        dg = torch.empty_like(gauss)
        gs = [None if g is None else g.contiguous().float() for g in (g_cls, g_reg, g_al, g_final)]
        _lib.check(lib.vilco_mq_loss_bwd(C.byref(d), _p(gs[0]), _p(gs[1]), _p(gs[2]), _p(gs[3]), saved.data_ptr(),
                                         ws.data_ptr(), dl.data_ptr(), do.data_ptr(), _p(dsc), dg.data_ptr(), _stream()))
        return dl, do, dsc, dg, None, None, None, None, None


def mq_loss(logits, offsets, level_scale, gauss, tables, level_len, gt, loss_norm, radius, smoothing, momentum, loss_weight,
            al_weight, use_al):
    """logits [B,R,C], offsets [B,R,2] (raw when level_scale [L] is given), gauss [6,C], tables = (points [R,4],
    row_level [R] int32, row_pos [R] int32), level_len [B,L] int32, gt float [B, 3*Nmax+1] (include/vilco_hip.h).
    loss_weight must be positive: loss_weight <= 0 means cls / max(reg, 0.01) as the weight (meta_archs.py:1076-1079), which the
    kernels do not compute -- the model keeps that configuration on the tensor expressions."""
    if not float(loss_weight) > 0:
        raise ValueError("mq_loss: loss_weight must be > 0 (got %r): the adaptive weight is not implemented by the fused op" % (loss_weight,))
    cfg = dict(radius=float(radius), smoothing=float(smoothing), momentum=float(momentum), loss_weight=float(loss_weight),
               al_weight=float(al_weight), use_al=bool(use_al))
    return _MQLoss.apply(logits.contiguous(), offsets.contiguous(), level_scale, gauss.contiguous(), tables, level_len, gt,
                         loss_norm, cfg)


class _MQLossAce(torch.autograd.Function):
    """_MQLoss with ER-ACE's class window per clip (vilco_mq_loss_ace_fwd / _bwd): `cls_lo` is read by the kernels when they run,
    forward and backward alike, so a captured step follows the table its replay wrote"""

    @staticmethod
    def forward(ctx, logits, offsets, level_scale, gauss, tables, level_len, gt, loss_norm, cfg, cls_lo):
        _chk(logits, offsets, level_scale, gauss)
        lib = _lib.load()
        B, R, Cn = logits.shape
        points, row_level, row_pos = tables
        d = _lib.LossDesc()
        d.logits, d.offsets, d.level_scale = logits.data_ptr(), offsets.data_ptr(), _p(level_scale)
        d.points, d.row_level, d.row_pos = points.data_ptr(), row_level.data_ptr(), row_pos.data_ptr()
        d.level_len, d.gt, d.gauss, d.loss_norm = level_len.data_ptr(), gt.data_ptr(), gauss.data_ptr(), loss_norm.data_ptr()
        d.B, d.R, d.C, d.L, d.Nmax = B, R, Cn, level_len.shape[1], (gt.shape[1] - 1) // 3
        d.center_radius, d.label_smoothing, d.momentum = cfg['radius'], cfg['smoothing'], cfg['momentum']
        d.loss_weight, d.al_weight, d.use_al = cfg['loss_weight'], cfg['al_weight'], int(cfg['use_al'])
        key = (logits.device.index, B * Cn)         # the plain op's state: both leave it zero
        st = _almax_state.get(key)
        if st is None:
            st = _almax_state[key] = torch.zeros(B * Cn, dtype=torch.int64, device=logits.device)
        nws = lib.vilco_mq_loss_workspace(B, R, Cn)
        ws = _ws(nws, logits.device)
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        saved = torch.empty(1, dtype=torch.float32, device=logits.device)
        _lib.check(lib.vilco_mq_loss_ace_fwd(C.byref(d), cls_lo.data_ptr(), out.data_ptr(), saved.data_ptr(), st.data_ptr(),
                                             ws.data_ptr(), nws, _stream()))
        ctx.desc, ctx.keep = d, (points, row_level, row_pos, level_len, gt, loss_norm)
        ctx.save_for_backward(logits, offsets, level_scale, gauss, saved, ws, cls_lo)
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def backward(ctx, g_cls, g_reg, g_al, g_final):
        logits, offsets, level_scale, gauss, saved, ws, cls_lo = ctx.saved_tensors
        lib = _lib.load()
        d = ctx.desc
        dl, do = torch.empty_like(logits), torch.empty_like(offsets)
        dsc = torch.empty_like(level_scale) if level_scale is not None else None
        dg = torch.empty_like(gauss)
        gs = [None if g is None else g.contiguous().float() for g in (g_cls, g_reg, g_al, g_final)]
        _lib.check(lib.vilco_mq_loss_ace_bwd(C.byref(d), cls_lo.data_ptr(), _p(gs[0]), _p(gs[1]), _p(gs[2]), _p(gs[3]),
                                             saved.data_ptr(), ws.data_ptr(), dl.data_ptr(), do.data_ptr(), _p(dsc),
                                             dg.data_ptr(), _stream()))
        return dl, do, dsc, dg, None, None, None, None, None, None


def mq_loss_ace(logits, offsets, level_scale, gauss, tables, level_len, gt, loss_norm, radius, smoothing, momentum, loss_weight,
                al_weight, use_al, cls_lo):
    """ops.mq_loss under ER-ACE's asymmetric window (cl_methods/ace.py; include/vilco_hip.h: vilco_mq_loss_ace_fwd): cls_lo int32
    [B] on the logits' device, contiguous -- clip b's classification and al terms visit the classes [cls_lo[b], C) only (a value
    outside [0, C): all of them).  The kernels read the table when they run: rewrite it in place before a replay."""
    if not float(loss_weight) > 0:
        raise ValueError("mq_loss_ace: loss_weight must be > 0 (got %r): the adaptive weight is not implemented by the fused op" % (loss_weight,))
    if not torch.is_tensor(cls_lo) or cls_lo.dtype != torch.int32 or cls_lo.dim() != 1 or logits.dim() != 3 or \
            cls_lo.shape[0] != logits.shape[0]:
        raise ValueError("mq_loss_ace: cls_lo must be an int32 tensor [%s], got %s" % (
            logits.shape[0] if logits.dim() == 3 else 'B',
            "%s %s" % (cls_lo.dtype, tuple(cls_lo.shape)) if torch.is_tensor(cls_lo) else type(cls_lo).__name__))
    if cls_lo.device != logits.device:
        raise RuntimeError("mq_loss_ace: cls_lo lives on %s, the logits on %s" % (cls_lo.device, logits.device))
    if not cls_lo.is_contiguous():
        raise ValueError("mq_loss_ace: cls_lo must be contiguous (the kernels read the caller's table, not a copy)")
    cfg = dict(radius=float(radius), smoothing=float(smoothing), momentum=float(momentum), loss_weight=float(loss_weight),
               al_weight=float(al_weight), use_al=bool(use_al))
    return _MQLossAce.apply(logits.contiguous(), offsets.contiguous(), level_scale, gauss.contiguous(), tables, level_len, gt,
                            loss_norm, cfg, cls_lo)


# ---------------------------------------------------------------------------------------- iCaRL / BiC distillation
DISTILL_ICARL, DISTILL_BIC = 0, 1
_distill_tabs = {}


def _distill_levels(level_row, level_T, device):
    """(host rows, host lengths, device int32 [2, L]) of a level layout; the device copy is made once per layout and kept (a
    captured step addresses it)"""
    rows, lens = tuple(int(r) for r in level_row), tuple(int(t) for t in level_T)
    if len(rows) != len(lens) or not rows:
        raise ValueError("cl_distill: level_row and level_T must list the same, non-zero number of levels")
    key = (rows, lens, str(device))
    tab = _distill_tabs.get(key)
    if tab is None:
        L = len(rows)
        tab = _distill_tabs[key] = ((C.c_int32 * L)(*rows), (C.c_int32 * L)(*lens),
                                    torch.tensor([rows, lens], dtype=torch.int32, device=device))
    return tab


def distill_targets(levels, device):
    """The cached outputs of one clip (a list over pyramid levels of [T_l, ldt] device tensors or NumPy arrays, as
    train_cl.cache_prev_logits hands them out) -> (fp32 device buffer [sum T_l, ldt], (T_l, ...)).  Views of one
    contiguous buffer, level after level, are taken as they are; anything else is concatenated once (NumPy: on the host,
    then one upload)."""
    lens = tuple(int(t.shape[0]) for t in levels)
    if all(torch.is_tensor(t) for t in levels):
        t0 = levels[0]
        if t0.dim() == 2 and t0.is_cuda and t0.dtype == torch.float32 and t0.device == torch.device(device):
            ldt, off, ok = t0.shape[1], t0.storage_offset(), True
            for t in levels:
                ok = ok and (t.dim() == 2 and t.shape[1] == ldt and t.dtype == t0.dtype and t.is_contiguous() and
                             t.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr() and t.storage_offset() == off)
                off += t.shape[0] * ldt
            if ok:
                return t0.as_strided((sum(lens), ldt), (ldt, 1), t0.storage_offset()), lens
        return torch.cat([t.to(device=device, dtype=torch.float32) for t in levels], dim=0).contiguous(), lens
    import numpy as np
    host = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.float32) for t in levels], axis=0))
    return torch.from_numpy(host).to(device), lens


def _distill_desc(logits, targets, tab, n_known, mode, scale, clip):
    d = _lib.DistillDesc()
    d.logits, d.targets = logits.data_ptr(), targets.data_ptr()
    d.level_row, d.level_T, d.level_dev = C.addressof(tab[0]), C.addressof(tab[1]), tab[2].data_ptr()
    d.B, d.R, d.C, d.L = logits.shape[0], logits.shape[1], logits.shape[2], len(tab[0])
    d.clip, d.ldt, d.n_known, d.mode, d.scale = int(clip), targets.shape[1], int(n_known), int(mode), float(scale)
    return d


class _ClDistill(torch.autograd.Function):
    """the distillation term of iCaRL / BiC (meta_archs.py:1482-1519) over the concatenated head output: two launches
    forward, one backward (vilco_cl_distill_fwd / _bwd); the gradient is non-zero on [clip, level rows, :n_known] only"""

    @staticmethod
    def forward(ctx, logits, targets, tab, cfg):
        _chk(logits, targets)
        lib = _lib.load()
        d = _distill_desc(logits, targets, tab, *cfg)
        nws = lib.vilco_cl_distill_workspace(targets.shape[0])
        ws = _ws(nws, logits.device)
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        _lib.check(lib.vilco_cl_distill_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws, _stream()))
        ctx.desc, ctx.tab = d, tab
        ctx.save_for_backward(logits, targets)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        logits, targets = ctx.saved_tensors
        g = g.contiguous().float()
        dl = torch.zeros_like(logits)          # the kernel assigns its footprint; autograd adds this to mq_loss' gradient
        _lib.check(_lib.load().vilco_cl_distill_bwd(C.byref(ctx.desc), g.data_ptr(), dl.data_ptr(), _stream()))
        return dl, None, None, None


def cl_distill(logits, level_row, level_T, targets, n_known, mode, scale, clip=0):
    """iCaRL (mode DISTILL_ICARL) / BiC (DISTILL_BIC) distillation of batch row `clip` against the previous model's cached
    outputs (include/vilco_hip.h: vilco_distill_desc) -> scalar.
    logits: [B, R, C] with level l in rows level_row[l] .. level_row[l] + level_T[l], or the list of per-level [B, T_l, C]
    tensors (concatenated here; level_row may then be None).  targets: [sum T_l, ldt], or the per-level list (device
    tensors or NumPy arrays: distill_targets).  BiC: scale = 0.01 * n_known / n_classes; iCaRL's 0.01 is fixed."""
    if isinstance(logits, (list, tuple)):
        level_T = [int(x.shape[1]) for x in logits]
        level_row = [sum(level_T[:i]) for i in range(len(level_T))]
        logits = torch.cat(list(logits), dim=1)
    if not torch.is_tensor(targets):
        targets, lens = distill_targets(targets, logits.device)
        if lens != tuple(int(t) for t in level_T):
            raise ValueError("cl_distill: the targets' level lengths %s differ from the logits' %s" % (lens, tuple(level_T)))
    if targets.dim() != 2 or targets.shape[0] != sum(int(t) for t in level_T):
        raise ValueError("cl_distill: targets %s do not hold the %d rows of the levels %s" %
                         (tuple(targets.shape), sum(int(t) for t in level_T), tuple(level_T)))
    if not torch.is_tensor(logits) or logits.dim() != 3:
        raise ValueError("cl_distill: logits must be [B, R, C] or a list of [B, T_l, C]")
    tab =_distill_levels(level_row, level_T, logits.device)
    return _ClDistill.apply(logits.contiguous(), targets.contiguous(), tab,
                            (int(n_known), int(mode), float(scale), int(clip)))


# ---------------------------------------------------------------------------------------- Dark Experience Replay
def der_pairs_per_round():
    """(batch row, pyramid row) pairs the capped grid of csrc/der.hip covers in one round (4 waves per block); beyond it
    the waves walk further pairs.  Read off vilco_der_workspace, which holds one partial per block."""
    lib = _lib.load()
    return 4 * ((lib.vilco_der_workspace(1 << 40) - 256) // 8 - 1)


class _DerReplay(torch.autograd.Function):
    """the logit-replay term of DER / DER++ over the concatenated head output: two launches forward, one backward
    (vilco_der_fwd / _bwd); the gradient is non-zero on the compared elements only"""

    @staticmethod
    def forward(ctx, logits, tab, level_len, der_tab, alpha):
        _chk(logits)
        lib = _lib.load()
        d = _lib.DerDesc()
        d.logits, d.level_len, d.der_tab = logits.data_ptr(), level_len.data_ptr(), der_tab.data_ptr()
        d.level_row, d.level_T, d.level_dev = C.addressof(tab[0]), C.addressof(tab[1]), tab[2].data_ptr()
        d.B, d.R, d.C, d.L = logits.shape[0], logits.shape[1], logits.shape[2], len(tab[0])
        d.alpha = float(alpha)
        nws = lib.vilco_der_workspace(logits.shape[0] * sum(tab[1]))
        # the workspace is this call's own: backward reads N from it (not ops._ws, whose buffers deferred stages may share)
        ws = torch.empty(int(nws), dtype=torch.uint8, device=logits.device)
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        _lib.check(lib.vilco_der_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws, _stream()))
        ctx.desc, ctx.tab, ctx.nws = d, tab, nws
        ctx.save_for_backward(logits, level_len, der_tab, ws)
        off = (-ws.data_ptr()) % 256
        count = ws[off:off + 8].view(torch.int64)[0]
        ctx.mark_non_differentiable(count)
        return out[0], count

    @staticmethod
    def backward(ctx, g, _g_count):
        logits, level_len, der_tab, ws = ctx.saved_tensors
        g = g.contiguous().float()
        dl = torch.zeros_like(logits)          # the kernel assigns its footprint; autograd adds this to mq_loss' gradient
        _lib.check(_lib.load().vilco_der_bwd(C.byref(ctx.desc), g.data_ptr(), dl.data_ptr(), ws.data_ptr(), ctx.nws, _stream()))
        return dl, None, None, None, None


def der_replay(logits, level_row, level_T, valid_lens, der_tab, alpha, return_count=False):
    """Dark Experience Replay's term (include/vilco_hip.h: vilco_der_desc) -> scalar alpha * S / N, 0 when nothing is compared.
    logits: [B, R, C] with level l in rows level_row[l] .. level_row[l] + level_T[l]; valid_lens: device int32 [B, L], the
    valid length of every level of every row (what ops.mq_loss is given); der_tab: device int64 [B, 2] = (address of the row's
    record [sum T_l, n_b] or 0, n_b) -- cl_methods.der.DERBank.table_for builds it and keeps the records alive.
    return_count: also the device int64 scalar N (compared elements)."""
    for t in (logits, valid_lens, der_tab):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback"
                               % (t.device if torch.is_tensor(t) else type(t).__name__))
    if logits.dim() != 3:
        raise ValueError("der_replay: logits must be [B, R, C]")
    tab = _distill_levels(level_row, level_T, logits.device)
    B, L = logits.shape[0], len(tab[0])
    if valid_lens.dtype != torch.int32 or tuple(valid_lens.shape) != (B, L):
        raise ValueError("der_replay: valid_lens must be int32 [%d, %d], got %s %s" % (B, L, valid_lens.dtype, tuple(valid_lens.shape)))
    if der_tab.dtype != torch.int64 or tuple(der_tab.shape) != (B, 2):
        raise ValueError("der_replay: der_tab must be int64 [%d, 2], got %s %s" % (B, der_tab.dtype, tuple(der_tab.shape)))
    if valid_lens.device != logits.device or der_tab.device != logits.device:
        raise RuntimeError("der_replay: all tensors must live on one device")
    loss, count = _DerReplay.apply(logits.contiguous(), tab, valid_lens.contiguous(), der_tab.contiguous(), float(alpha))
    return (loss, count) if return_count else loss


# ---------------------------------------------------------------------------------------- pooled feature distillation (PODNet)
def pod_tile_rows():
    """rows of a level one workgroup of csrc/pod.hip covers (a longer level takes several, whose column partials are added in
    block order)"""
    return int(_lib.load().vilco_pod_tile_rows())


def pod_record_width(level_T, C):
    """floats of one clip's record: every level's [p (C) ; q (T_l)], levels end to end"""
    return sum(int(C) + int(t) for t in level_T)


def _pod_desc(feats, level_len, pod_tab, scale):
    """-> (descriptor, workspace bytes, what the descriptor points into on the host: keep it alive across the call)"""
    L = len(feats)
    T = (_lib.i32 * L)(*[int(f.shape[1]) for f in feats])
    ptrs = _ptr_table(feats)
    d = _lib.PodDesc()
    d.feats, d.level_T = C.addressof(ptrs), C.addressof(T)
    d.level_len, d.pod_tab = level_len.data_ptr(), (pod_tab.data_ptr() if pod_tab is not None else None)
    d.B, d.C, d.L, d.scale = feats[0].shape[0], feats[0].shape[2], L, float(scale)
    nws = _lib.load().vilco_pod_workspace(T, L, d.B, d.C)
    if nws == 0:
        raise ValueError("pod: levels %s x C = %d are not a pyramid the op takes" % ([int(t) for t in T], d.C))
    return d, nws, (ptrs, T)


class _PodDistill(torch.autograd.Function):
    """the pooled-feature distillation term over every level of the pyramid: three launches forward, one backward
    (vilco_pod_fwd / _bwd); the backward assigns every element of every level's gradient"""

    @staticmethod
    def forward(ctx, level_len, pod_tab, scale, *feats):
        _chk(*feats)
        d, nws, keep = _pod_desc(feats, level_len, pod_tab, scale)
        # the workspace is this call's own: backward reads N_rec and g_v / w from it
        ws = torch.empty(int(nws), dtype=torch.uint8, device=feats[0].device)
        out = torch.empty(1, dtype=torch.float32, device=feats[0].device)
        _lib.check(_lib.load().vilco_pod_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws, _stream()))
        ctx.scale, ctx.nws = float(scale), nws
        ctx.save_for_backward(level_len, pod_tab, ws, *feats)
        off = (-ws.data_ptr()) % 256
        count = ws[off:off + 8].view(torch.int64)[0]
        ctx.mark_non_differentiable(count)
        return out[0], count

    @staticmethod
    def backward(ctx, g, _g_count):
        level_len, pod_tab, ws = ctx.saved_tensors[:3]
        feats = ctx.saved_tensors[3:]
        g = g.contiguous().float()
        grads = [torch.empty_like(f) for f in feats]             # the kernel assigns every element
        d, nws, keep = _pod_desc(feats, level_len, pod_tab, ctx.scale)
        _lib.check(_lib.load().vilco_pod_bwd(C.byref(d), g.data_ptr(), _ptr_table(grads), ws.data_ptr(), ctx.nws, _stream()))
        return (None, None, None) + tuple(grads)


def _pod_args(name, feats, level_len):
    feats = list(feats)
    if not 1 <= len(feats) <= 16:
        raise ValueError("%s takes 1 to 16 levels, got %d" % (name, len(feats)))
    for t in feats + [level_len]:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback"
                               % (t.device if torch.is_tensor(t) else type(t).__name__))
    if any(f.dim() != 3 for f in feats):
        raise ValueError("%s: every level must be [B, T_l, C]" % name)
    B, Cn = feats[0].shape[0], feats[0].shape[2]
    if any(f.shape[0] != B or f.shape[2] != Cn or f.shape[1] < 1 or f.dtype != torch.float32 for f in feats) or B < 1 or Cn < 1:
        raise ValueError("%s: every level must be fp32 [B, T_l, C] with the same B >= 1 and C >= 1 and T_l >= 1" % name)
    if level_len.dtype != torch.int32 or tuple(level_len.shape) != (B, len(feats)):
        raise ValueError("%s: level_len must be int32 [%d, %d], got %s %s"
                         % (name, B, len(feats), level_len.dtype, tuple(level_len.shape)))
    if any(f.device != feats[0].device for f in feats) or level_len.device != feats[0].device:
        raise RuntimeError("%s: all tensors must live on one device" % name)
    return [f.contiguous() for f in feats], level_len.contiguous()


def pod_distill(feats, level_len, pod_tab, scale, return_count=False):
    """PODNet's pooled feature distillation over the pyramid (include/vilco_hip.h: vilco_pod_desc) -> the scalar
    scale / (L N_rec) * sum_b sum_l ||u_bl - r_bl||, an exact 0 when no row has a record.  feats: list of L <= 16 token-major
    fp32 [B, T_l, C]; level_len: device int32 [B, L] valid lengths; pod_tab: device int64 [B] = the address of the row's record
    (fp32 [sum_l (C + T_l)], ops.pod_record's layout) or 0 -- cl_methods.pod.PODBank.table_for builds it and keeps the records
    alive.  return_count: also the device int64 scalar N_rec."""
    feats, level_len = _pod_args("pod_distill", feats, level_len)
    B = feats[0].shape[0]
    if not (torch.is_tensor(pod_tab) and pod_tab.is_cuda):
        raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback"
                           % (pod_tab.device if torch.is_tensor(pod_tab) else type(pod_tab).__name__))
    if pod_tab.dtype != torch.int64 or tuple(pod_tab.shape) != (B,):
        raise ValueError("pod_distill: pod_tab must be int64 [%d], got %s %s" % (B, pod_tab.dtype, tuple(pod_tab.shape)))
    if pod_tab.device != feats[0].device:
        raise RuntimeError("pod_distill: all tensors must live on one device")
    loss, count = _PodDistill.apply(level_len, pod_tab.contiguous(), float(scale), *feats)
    return (loss, count) if return_count else loss


def pod_record(feats, level_len):
    """-> fp32 [B, L * C + sum T_l]: every row's pooled, normalised vectors u_bl = [p ; q] / max(||[p ; q]||, 1e-12), levels
    end to end, entries at t >= level_len[b][l] zero (vilco_pod_record: two launches) -- what pod_distill compares against"""
    feats, level_len = _pod_args("pod_record", feats, level_len)
    with torch.no_grad():
        d, nws, keep = _pod_desc(feats, level_len, None, 1.0)
        ws = torch.empty(int(nws), dtype=torch.uint8, device=feats[0].device)
        rec = torch.empty(feats[0].shape[0], pod_record_width([f.shape[1] for f in feats], feats[0].shape[2]),
                          dtype=torch.float32, device=feats[0].device)
        _lib.check(_lib.load().vilco_pod_record(C.byref(d), rec.data_ptr(), ws.data_ptr(), nws, _stream()))
    return rec


# ---------------------------------------------------------------------------------------- Elastic Response Distillation
ERD_TAB_COLS = 5      # erd_tab columns: map_cls, map_reg, val_cls, val_reg (addresses), n_b


def erd_pairs_per_round():
    """(batch row, pyramid row) pairs the capped forward grid of csrc/erd.hip covers in one round; beyond it the waves walk
    further pairs"""
    return int(_lib.load().vilco_erd_pairs_per_round())


class _ErdDistill(torch.autograd.Function):
    """the response-distillation term over the concatenated head output: two launches forward, one backward (vilco_erd_fwd /
    _bwd); the backward assigns every element of the logits' and the offsets' gradient (and d scale on the raw-offset route)"""

    @staticmethod
    def forward(ctx, logits, offsets, scale, tab, level_len, erd_tab, lambda_cls, lambda_reg):
        _chk(logits, offsets)
        lib = _lib.load()
        d = _lib.ErdDesc()
        d.logits, d.offsets, d.scale = logits.data_ptr(), offsets.data_ptr(), (scale.data_ptr() if scale is not None else None)
        d.level_len, d.erd_tab = level_len.data_ptr(), erd_tab.data_ptr()
        d.level_row, d.level_T, d.level_dev = C.addressof(tab[0]), C.addressof(tab[1]), tab[2].data_ptr()
        d.B, d.R, d.C, d.L = logits.shape[0], logits.shape[1], logits.shape[2], len(tab[0])
        d.lambda_cls, d.lambda_reg = float(lambda_cls), float(lambda_reg)
        nws = lib.vilco_erd_workspace(logits.shape[0] * sum(tab[1]))
        # the workspace is this call's own: backward reads N_c, N_r and the unweighted d scale from it
        ws = torch.empty(int(nws), dtype=torch.uint8, device=logits.device)
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        _lib.check(lib.vilco_erd_fwd(C.byref(d), out.data_ptr(), ws.data_ptr(), nws, _stream()))
        ctx.desc, ctx.tab, ctx.nws, ctx.has_scale = d, tab, nws, scale is not None
        ctx.save_for_backward(logits, offsets, scale, level_len, erd_tab, ws)
        off = (-ws.data_ptr()) % 256
        counts = ws[off:off + 16].view(torch.int64)
        parts = out[1:3]
        ctx.mark_non_differentiable(parts, counts)
        return out[0], parts, counts

    @staticmethod
    def backward(ctx, g, _g_parts, _g_counts):
        logits, offsets, scale, level_len, erd_tab, ws = ctx.saved_tensors
        g = g.contiguous().float()
        dl, do = torch.empty_like(logits), torch.empty_like(offsets)          # the kernel assigns every element
        ds = torch.empty_like(scale) if ctx.has_scale else None
        _lib.check(_lib.load().vilco_erd_bwd(C.byref(ctx.desc), g.data_ptr(), dl.data_ptr(), do.data_ptr(),
                                             ds.data_ptr() if ds is not None else None, ws.data_ptr(), ctx.nws, _stream()))
        return dl, do, ds, None, None, None, None, None


def erd_distill(logits, offsets, scale, level_row, level_T, level_len, erd_tab, lambda_cls, lambda_reg, return_counts=False):
    """Elastic Response Distillation's term (include/vilco_hip.h: vilco_erd_desc) -> (erd_loss, erd_cls_loss, erd_reg_loss):
    lambda_cls A / N_c + lambda_reg D / N_r and its two parts (detached), a part whose count is 0 an exact 0.
    logits: [B, R, C] with level l in rows level_row[l] .. level_row[l] + level_T[l]; offsets: [B, R, 2] in the same rows --
    finished, or, with `scale` (fp32 [L], the per-level Scale of the fused loss route), raw: the op takes relu(scale_l raw)
    itself and returns the gradients of raw and scale; level_len: device int32 [B, L] valid lengths; erd_tab: device int64
    [B, 5] = the addresses of the row's two maps and two value buffers and n_b, or zeros -- cl_methods.erd.ERDBank.table_for
    builds it and keeps the records alive.  return_counts: also the device int64 [2] (N_c, N_r)."""
    for t in (logits, offsets, level_len, erd_tab) + ((scale,) if scale is not None else ()):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback"
                               % (t.device if torch.is_tensor(t) else type(t).__name__))
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError("erd_distill: logits must be fp32 [B, R, C]")
    tab = _distill_levels(level_row, level_T, logits.device)
    B, R, L = logits.shape[0], logits.shape[1], len(tab[0])
    if L > 16:
        raise ValueError("erd_distill takes 1 to 16 levels, got %d" % L)
    if tuple(offsets.shape) != (B, R, 2) or offsets.dtype != torch.float32:
        raise ValueError("erd_distill: offsets must be fp32 [%d, %d, 2], got %s %s" % (B, R, offsets.dtype, tuple(offsets.shape)))
    if scale is not None and (tuple(scale.shape) != (L,) or scale.dtype != torch.float32):
        raise ValueError("erd_distill: scale must be fp32 [%d], got %s %s" % (L, scale.dtype, tuple(scale.shape)))
    if level_len.dtype != torch.int32 or tuple(level_len.shape) != (B, L):
        raise ValueError("erd_distill: level_len must be int32 [%d, %d], got %s %s" % (B, L, level_len.dtype, tuple(level_len.shape)))
    if erd_tab.dtype != torch.int64 or tuple(erd_tab.shape) != (B, ERD_TAB_COLS):
        raise ValueError("erd_distill: erd_tab must be int64 [%d, %d], got %s %s"
                         % (B, ERD_TAB_COLS, erd_tab.dtype, tuple(erd_tab.shape)))
    if any(t.device != logits.device for t in (offsets, level_len, erd_tab)) or (scale is not None and scale.device != logits.device):
        raise RuntimeError("erd_distill: all tensors must live on one device")
    loss, parts, counts = _ErdDistill.apply(logits.contiguous(), offsets.contiguous(),
                                            scale.contiguous() if scale is not None else None, tab, level_len.contiguous(),
                                            erd_tab.contiguous(), float(lambda_cls), float(lambda_reg))
    out = (loss, parts[0], parts[1])
    return out + (counts,) if return_counts else out


def erd_select(logits, offsets, level_T, level_len, n_old, alpha_cls, alpha_reg):
    """The record-time selection of Elastic Response Distillation (vilco_erd_select, vilco_erd_select_fill: three launches and
    one host read of the counts in between).  logits: fp32 [B, P, C], the incoming model's logits, levels end to end; offsets:
    fp32 [B, P, 2], its finished offsets; level_len: device int32 [B, L].  -> per clip (map_cls int32 [P], map_reg int32 [P],
    val_cls fp32 [max(K_c, 1), n_old], val_reg fp32 [max(K_r, 1), 2], K_c, K_r): position -> slot (-1: not selected) and the
    selected rows in ascending position; a set that is empty keeps one unused row, so that every buffer has an address."""
    for t in (logits, offsets, level_len):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback"
                               % (t.device if torch.is_tensor(t) else type(t).__name__))
    level_T = [int(t) for t in level_T]
    L = len(level_T)
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError("erd_select: logits must be fp32 [B, P, C]")
    B, P, Cn = logits.shape
    if P != sum(level_T) or not 1 <= L <= 16 or min(level_T) < 1:
        raise ValueError("erd_select: %d rows do not hold the levels %s" % (P, level_T))
    if tuple(offsets.shape) != (B, P, 2) or offsets.dtype != torch.float32:
        raise ValueError("erd_select: offsets must be fp32 [%d, %d, 2], got %s %s" % (B, P, offsets.dtype, tuple(offsets.shape)))
    if level_len.dtype != torch.int32 or tuple(level_len.shape) != (B, L):
        raise ValueError("erd_select: level_len must be int32 [%d, %d], got %s %s" % (B, L, level_len.dtype, tuple(level_len.shape)))
    if not 1 <= int(n_old) <= Cn:
        raise ValueError("erd_select: n_old = %d outside 1 .. %d" % (n_old, Cn))
    dev = logits.device
    with torch.no_grad():
        logits, offsets, level_len = logits.contiguous(), offsets.contiguous(), level_len.contiguous()
        lib = _lib.load()
        T = (_lib.i32 * L)(*level_T)
        conf = torch.empty(B, P, dtype=torch.float32, device=dev)
        flags = torch.empty(B, P, dtype=torch.int32, device=dev)
        counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
        d = _lib.ErdSelectDesc()
        d.logits, d.offsets, d.level_T, d.level_len = logits.data_ptr(), offsets.data_ptr(), C.addressof(T), level_len.data_ptr()
        d.conf, d.flags, d.counts, d.out_tab = conf.data_ptr(), flags.data_ptr(), counts.data_ptr(), None
        d.B, d.P, d.C, d.n_old, d.L = B, P, Cn, int(n_old), L
        d.alpha_cls, d.alpha_reg = float(alpha_cls), float(alpha_reg)
        _lib.check(lib.vilco_erd_select(C.byref(d), _stream()))
        K = counts.tolist()                                      # the one host read: the buffers' sizes
        recs = []
        for kc, kr in K:
            recs.append((torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                         torch.zeros(max(kc, 1), int(n_old), dtype=torch.float32, device=dev),
                         torch.zeros(max(kr, 1), 2, dtype=torch.float32, device=dev), int(kc), int(kr)))
        out_tab = torch.tensor([[r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), r[3].data_ptr()] for r in recs],
                               dtype=torch.int64).to(dev)
        d.out_tab = out_tab.data_ptr()
        _lib.check(lib.vilco_erd_select_fill(C.byref(d), _stream()))
    return recs


# ---------------------------------------------------------------------------------------- BiC bias correction
_bic_tabs = {}


def bic_split_table(splits, n_classes, n_layers):
    """list_splits of a BiC model -> the validated tuple of cumulative column ends: non-empty, strictly increasing from above
    0, ending at n_classes <= 128, one bias layer per split.  Anything else raises (the C launcher checks the same again,
    before any device work)."""
    ends = tuple(int(v) for v in splits)
    if not ends:
        raise ValueError("bic_correct: the split table is empty")
    if int(n_layers) != len(ends):
        raise ValueError("bic_correct: %d bias layers for %d splits" % (int(n_layers), len(ends)))
    if int(n_classes) > 128:
        raise ValueError("bic_correct: %d classes, the kernels take at most 128" % int(n_classes))
    if ends[0] <= 0 or any(b <= a for a, b in zip(ends, ends[1:])):
        raise ValueError("bic_correct: the splits %s are not strictly increasing cumulative ends" % (ends,))
    if ends[-1] != int(n_classes):
        raise ValueError("bic_correct: the last split ends at column %d, the logits have %d" % (ends[-1], int(n_classes)))
    return ends


def _bic_table(ends, params, device):
    """(host int32 [S] ends, device int64 [3][S]: the addresses of every alpha and beta, the ends) -- the `_ptr_table` of this op,
    on the device because the kernel walks it.  Made once per (splits, parameter addresses) and kept: a captured step
    addresses it, and the VALUES behind the addresses are read when the kernel runs."""
    ptrs = tuple(p.data_ptr() for p in params)
    key = (ends, ptrs, str(device))
    tab = _bic_tabs.get(key)
    if tab is None:
        S = len(ends)
        tab = _bic_tabs[key] = ((C.c_int32 * S)(*ends),
                                torch.tensor([ptrs[0::2], ptrs[1::2], ends], dtype=torch.int64, device=device))
    return tab


def _bic_rows(t, inplace=False):
    """[..., C] float tensor -> (tensor, rows, row stride): rows laid out at one constant stride are taken as they are (the
    columns C .. stride of such a buffer are neither read nor written), anything else is made contiguous first"""
    Cn = t.shape[-1]
    rows = t.numel() // max(Cn, 1)
    ok = t.stride(-1) == 1 and t.dim() >= 2 and t.stride(-2) >= Cn
    if ok:
        ld = t.stride(-2)
        exp = ld * t.shape[-2]
        for k in range(t.dim() - 3, -1, -1):
            ok = ok and (t.shape[k] == 1 or t.stride(k) == exp)
            exp *= t.shape[k]
    if not ok or rows == 0:
        if inplace:
            raise ValueError("bic_correct: an in-place call needs rows at one constant stride, got strides %s" % (tuple(t.stride()),))
        t = t.contiguous()
        ld = Cn
    if ld >= 1 << 31:
        raise ValueError("bic_correct: row stride %d" % ld)
    return t, rows, ld


class _BicCorrect(torch.autograd.Function):
    """y = alpha[s(c)] x + beta[s(c)] over the concatenated head output (vilco_bic_correct_fwd / _bwd): one launch each way; the
    parameter gradients (two more launches, fixed-order sums) only when a layer requires one"""

    @staticmethod
    def forward(ctx, x, tab, inplace, *params):
        lib = _lib.load()
        ctx.want = any(ctx.needs_input_grad[3:])
        if ctx.want and inplace:
            raise RuntimeError("bic_correct: in place the input is gone, and a layer that requires a gradient needs it")
        x, rows, ldx = _bic_rows(x, inplace)
        if inplace:
            y, ldy = x, ldx
            ctx.mark_dirty(x)
        else:
            y, ldy = torch.empty(x.shape, dtype=torch.float32, device=x.device), x.shape[-1]
        d = _lib.BicCorrectDesc()
        d.x, d.y, d.splits, d.table = x.data_ptr(), y.data_ptr(), C.addressof(tab[0]), tab[1].data_ptr()
        d.rows, d.C, d.S, d.ldx, d.ldy, d.n_layers = rows, x.shape[-1], len(tab[0]), ldx, ldy, len(params) // 2
        _lib.check(lib.vilco_bic_correct_fwd(C.byref(d), _stream()))
        ctx.tab, ctx.geom = tab, (rows, x.shape[-1], ldx)
        ctx.save_for_backward(*((x,) if ctx.want else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        tab, (rows, Cn, ldx) = ctx.tab, ctx.geom
        S = len(tab[0])
        dy = dy.contiguous().float()
        dx = torch.empty_like(dy)
        d = _lib.BicCorrectDesc()
        d.x, d.y, d.splits, d.table = dy.data_ptr(), dx.data_ptr(), C.addressof(tab[0]), tab[1].data_ptr()
        d.rows, d.C, d.S, d.ldx, d.ldy, d.n_layers = rows, Cn, S, Cn, Cn, S
        dpar = ws = x = None
        nws = 0
        if ctx.want:
            x, = ctx.saved_tensors
            dpar = torch.empty(2, S, dtype=torch.float32, device=dy.device)
            nws = lib.vilco_bic_correct_bwd_workspace(rows)
            ws = _ws(nws, dy.device)
        _lib.check(lib.vilco_bic_correct_bwd(C.byref(d), _p(x), ldx, _p(dpar), _p(ws), nws, _stream()))
        grads = [None] * (2 * S)
        for i in range(2 * S):
            if ctx.needs_input_grad[3 + i]:
                grads[i] = dpar[i % 2, i // 2:i // 2 + 1]
        return (dx, None, None) + tuple(grads)


def bic_correct(logits, splits, layers, inplace=False):
    """BiC's bias layers over their column ranges of the head output (include/vilco_hip.h: vilco_bic_correct_desc):
    logits [..., C] fp32 on the device, rows at one constant stride >= C (the LevelCat / loss-table layout, separator rows
    included: every row gets the affine); splits = list_splits; layers = list_bias_layers (each .alpha, .beta: float32 [1] on
    the logits' device).  alpha and beta are read on the device when the kernel runs.  inplace=True writes into `logits`
    (frozen layers only).  A bad split table, a CPU tensor or a layer elsewhere raises."""
    if not torch.is_tensor(logits) or not logits.is_cuda:
        raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback"
                           % (logits.device if torch.is_tensor(logits) else type(logits).__name__))
    if logits.dtype != torch.float32:
        raise RuntimeError("expected scalar type Float, got %s" % logits.dtype)
    if logits.dim() < 2:
        raise ValueError("bic_correct: logits must be [..., rows, C]")
    ends = bic_split_table(splits, logits.shape[-1], len(layers))
    params = []
    for l in layers:
        for p in (l.alpha, l.beta):
            if p.device != logits.device:
                raise RuntimeError("bic_correct: a bias layer lives on %s, the logits on %s" % (p.device, logits.device))
            if p.dtype != torch.float32 or p.numel() != 1:
                raise RuntimeError("bic_correct: alpha / beta must be float32 [1], got %s %s" % (p.dtype, tuple(p.shape)))
            params.append(p)
    tab = _bic_table(ends, params, logits.device)
    return _BicCorrect.apply(logits, tab, bool(inplace), *params)


# ---------------------------------------------------------------------------------------- L2P prompt pool
# VILCO_FUSED_PROMPT=0: cl_methods.Prompt keeps its tensor-op body on the device too (A/B runs).  Part of arithmetic_key():
# a captured step replays the path it recorded.
fused_prompt = switches.on("VILCO_FUSED_PROMPT")
PROMPT_KEY_MODES = {'mean': 0, 'max': 1, 'mean_max': 2, 'cls': 3}
_prompt_windows = {}


def prompt_window(start, k, B, device):
    """the fixed per-task window [start, start + k) for every row of the batch as a device int64 [B, k], made once per
    (start, k, B, device) and kept: a captured step addresses it"""
    key = (int(start), int(k), int(B), str(device))
    w = _prompt_windows.get(key)
    if w is None:
        w = _prompt_windows[key] = torch.arange(int(start), int(start) + int(k), device=device).unsqueeze(0).repeat(int(B), 1)
    return w


def status_word_take():
    """the library's device status word, read and cleared (synchronises the device).  Bit 0: a prompt index outside the pool."""
    v = C.c_int32(0)
    _lib.check(_lib.load().vilco_status_word_take(C.byref(v)))
    return v.value


def _prompt_desc(x, prompt, key, idx_in, cls, cfg):
    k, mode, vote = cfg
    d = _lib.PromptDesc()
    d.x, d.prompt, d.key, d.cls, d.idx_in = x.data_ptr(), prompt.data_ptr(), key.data_ptr(), _p(cls), _p(idx_in)
    d.B, d.L, d.C = x.shape
    d.P, d.len = prompt.shape[0], prompt.shape[1]
    d.k, d.key_mode, d.vote = int(k), int(mode), int(bool(vote))
    return d


class _PromptPool(torch.autograd.Function):
    """vilco_prompt_fwd / _bwd: two launches forward, at most two backward, no host read, no data-dependent allocation"""

    @staticmethod
    def forward(ctx, x, prompt, key, idx_in, cls, cfg):
        _chk(x, prompt, key, cls)
        lib = _lib.load()
        dev, (B, L, Cn), k = x.device, x.shape, int(cfg[0])
        P, length = prompt.shape[0], prompt.shape[1]
        d = _prompt_desc(x, prompt, key, idx_in, cls, cfg)
        f32 = dict(dtype=torch.float32, device=dev)
        kk, ll = max(k, 0), max(length, 0)               # a bad k / len is the launcher's to refuse
        idx = torch.empty(B, kk, dtype=torch.int64, device=dev)
        sim, pn, xn = torch.empty(B, P, **f32), torch.empty(P, Cn, **f32), torch.empty(B, Cn, **f32)
        selkey, prompted = torch.empty(B, kk, Cn, **f32), torch.empty(B, kk * ll + L, Cn, **f32)
        rs = torch.empty((), **f32)
        nws = lib.vilco_prompt_workspace(C.byref(d))
        ws = torch.empty(max(int(nws), 4), dtype=torch.uint8, device=dev)      # written forward, read backward: kept on ctx
        d.idx, d.sim, d.pn, d.xn, d.selkey = idx.data_ptr(), sim.data_ptr(), pn.data_ptr(), xn.data_ptr(), selkey.data_ptr()
        d.prompted, d.reduce_sim, d.workspace, d.workspace_bytes = prompted.data_ptr(), rs.data_ptr(), ws.data_ptr(), nws
        _lib.check(lib.vilco_prompt_fwd(C.byref(d), _stream()))
        ctx.desc, ctx.keep = d, (x, prompt, key, idx_in, cls, ws)      # the backward reads these through the descriptor
        ctx.save_for_backward(idx, pn, xn)
        ctx.mark_non_differentiable(idx, sim, pn, xn, selkey)
        return prompted, rs, idx, sim, pn, xn, selkey

    @staticmethod
    def backward(ctx, g_prompted, g_rs, *unused):
        idx, pn, xn = ctx.saved_tensors
        x, prompt, key = ctx.keep[:3]
        d = ctx.desc
        d.idx, d.pn, d.xn = idx.data_ptr(), pn.data_ptr(), xn.data_ptr()
        dev = x.device
        g_prompted = (torch.zeros(x.shape[0], d.k * d.len + d.L, d.C, dtype=torch.float32, device=dev) if g_prompted is None
                      else g_prompted.contiguous().float())
        g_rs = torch.zeros((), dtype=torch.float32, device=dev) if g_rs is None else g_rs.contiguous().float()
        want_x, want_p, want_k = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if want_x else None
        dp = torch.empty_like(prompt) if want_p else None
        dk = torch.empty_like(key) if want_k else None
        _lib.check(_lib.load().vilco_prompt_bwd(C.byref(d), g_prompted.data_ptr(), g_rs.data_ptr(), _p(dp), _p(dk), _p(dx),
                                                _stream()))
        return dx, dp, dk, None, None, None


def prompt_pool(x, prompt, key, idx=None, top_k=None, batchwise=False, embedding_key='mean', cls_features=None):
    """The L2P prompt pool as one operator (include/vilco_hip.h: vilco_prompt_desc; reference MQ/libs/cl_methods/prompt.py:47-117).
    x [B, L, C], prompt [P, len, C], key [P, C]: fp32 on the device.  idx [B, k] int64 on the device = the fixed window; None:
    the k = top_k prompts of largest cosine similarity are chosen on the device by counting rank (larger similarity first,
    equal similarities by smaller index), with `batchwise` the k most-picked ids of the batch (larger count first, equal
    counts by smaller id) for every row.  -> (prompted [B, k len + L, C], reduce_sim (0-dim), idx [B, k] int64, sim [B, P],
    pn [P, C], xn [B, C], selected_key [B, k, C]).
    Gradients reach prompt, key and x (each only if it requires one) from prompted and reduce_sim.  The other five outputs
    are marked non-differentiable -- nothing in the project or the reference differentiates them -- and cls_features gets
    no gradient.  An idx entry outside [0, P) sets bit 0 of the status word (status_word_take) and is clamped."""
    for t in (x, prompt, key):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback"
                               % (t.device if torch.is_tensor(t) else type(t).__name__))
    if embedding_key not in PROMPT_KEY_MODES:
        raise NotImplementedError("Not supported way of calculating embedding keys!")
    if x.dim() != 3 or prompt.dim() != 3 or key.dim() != 2 or prompt.shape[2] != x.shape[2] or key.shape != (prompt.shape[0], x.shape[2]):
        raise ValueError("prompt_pool: x [B, L, C], prompt [P, len, C], key [P, C]; got %s %s %s" %
                         (tuple(x.shape), tuple(prompt.shape), tuple(key.shape)))
    mode = PROMPT_KEY_MODES[embedding_key]
    if mode == 3 and cls_features is None:
        mode = 1                                             # the reference: the maximum stands in
    cls = None
    if mode == 3:
        if cls_features.shape != (x.shape[0], x.shape[2]) or cls_features.device != x.device:
            raise ValueError("prompt_pool: cls_features must be [B, C] on the device of x")
        cls = cls_features.detach().contiguous()
    if idx is not None:
        if idx.dim() != 2 or idx.shape[0] != x.shape[0] or idx.dtype != torch.int64 or idx.device != x.device:
            raise ValueError("prompt_pool: idx must be int64 [B, k] on the device of x")
        idx, k = idx.contiguous(), idx.shape[1]
    else:
        if top_k is None:
            raise ValueError("prompt_pool: top_k is needed when no idx is given")
        k = int(top_k)
    return _PromptPool.apply(x.contiguous(), prompt.contiguous(), key.contiguous(), idx, cls, (k, mode, bool(batchwise)))


# ---------------------------------------------------------------------------------------- CODA-Prompt
def _coda_desc(x, prompt, key, attn, s, f, want_ortho):
    d = _lib.CodaDesc()
    d.x, d.prompt, d.key, d.attn = x.data_ptr(), prompt.data_ptr(), key.data_ptr(), attn.data_ptr()
    d.B, d.L, d.C = x.shape
    d.M, d.len = prompt.shape[0], prompt.shape[1]
    d.s, d.f, d.want_ortho = int(s), int(f), int(bool(want_ortho))
    return d


class _CodaPrompt(torch.autograd.Function):
    """vilco_coda_fwd / _bwd: two launches forward (three with the penalty), at most two backward, no host read"""

    @staticmethod
    def forward(ctx, x, prompt, key, attn, cfg):
        _chk(x, prompt, key, attn)
        lib = _lib.load()
        dev, (B, L, Cn) = x.device, x.shape
        M, length = prompt.shape[0], prompt.shape[1]
        d = _coda_desc(x, prompt, key, attn, *cfg)
        f32 = dict(dtype=torch.float32, device=dev)
        alpha, prompted, ortho = torch.empty(B, M, **f32), torch.empty(B, max(length, 0) + L, Cn, **f32), torch.empty((), **f32)
        nws = lib.vilco_coda_workspace(C.byref(d))
        ws = torch.empty(max(int(nws), 4), dtype=torch.uint8, device=dev)      # written forward, read backward: kept on ctx
        d.alpha, d.prompted, d.ortho, d.workspace, d.workspace_bytes = alpha.data_ptr(), prompted.data_ptr(), ortho.data_ptr(), ws.data_ptr(), nws
        _lib.check(lib.vilco_coda_fwd(C.byref(d), _stream()))
        # the backward reads the operands and the workspace through the descriptor (never the three outputs it also names)
        ctx.desc, ctx.keep = d, (x, prompt, key, attn, ws)
        ctx.mark_non_differentiable(alpha)
        return prompted, ortho, alpha

    @staticmethod
    def backward(ctx, g_prompted, g_ortho, *unused):
        x, prompt, key, attn = ctx.keep[:4]
        d, dev = ctx.desc, x.device
        g_prompted = (torch.zeros(d.B, d.len + d.L, d.C, dtype=torch.float32, device=dev) if g_prompted is None
                      else g_prompted.contiguous().float())
        g_ortho = torch.zeros((), dtype=torch.float32, device=dev) if g_ortho is None else g_ortho.contiguous().float()
        want_x, want_p, want_k, want_a = ctx.needs_input_grad[:4]
        dp = torch.empty_like(prompt) if want_p else None
        dk = torch.empty_like(key) if want_k else None
        da = torch.empty_like(attn) if want_a else None
        _lib.check(_lib.load().vilco_coda_bwd(C.byref(d), g_prompted.data_ptr(), g_ortho.data_ptr(), _p(dp), _p(dk), _p(da),
                                              _stream()))
        dx = g_prompted[:, d.len:] if want_x else None              # the query is a constant: the slice, no launch
        return dx, dp, dk, da, None


def coda_prompt(x, prompt, key, attn, s, f, want_ortho=False):
    """CODA-Prompt as one operator (include/vilco_hip.h: vilco_coda_desc; Smith et al., CVPR 2023).  x [B, L, C], prompt
    [M, len, C], key [M, C], attn [M, C]: fp32 on the device.  Components [0, f) are mixed, [s, f) are the task's own: with
    xk = mean_l x, alpha[b][m] = cos(xk[b] * attn[m], key[m]) (F.normalize semantics) and p[b] = sum_{m < f} alpha[b][m]
    prompt[m]  -> (prompted [B, len + L, C] = [p ; x], ortho (0-dim; the orthogonality penalty over rows [0, f) of the three
    tensors when want_ortho, else an exact 0 and no Gram launch), alpha [B, M] with zeros in columns >= f).
    Gradients reach prompt, key and attn (each only if it requires one; rows outside [s, f) are exact zeros) from prompted and
    ortho, and x as the slice g_prompted[:, len:] (the query is a constant, as in the paper).  alpha is non-differentiable."""
    for t in (x, prompt, key, attn):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback"
                               % (t.device if torch.is_tensor(t) else type(t).__name__))
    if (x.dim() != 3 or prompt.dim() != 3 or key.dim() != 2 or prompt.shape[2] != x.shape[2]
            or key.shape != (prompt.shape[0], x.shape[2]) or attn.shape != key.shape):
        raise ValueError("coda_prompt: x [B, L, C], prompt [M, len, C], key [M, C], attn [M, C]; got %s %s %s %s" %
                         (tuple(x.shape), tuple(prompt.shape), tuple(key.shape), tuple(attn.shape)))
    return _CodaPrompt.apply(x.contiguous(), prompt.contiguous(), key.contiguous(), attn.contiguous(),
                             (int(s), int(f), bool(want_ortho)))


# ---------------------------------------------------------------------------------------- inference decode
def decode(logits, offsets, points, level_row0, level_len, topk, pre_nms_thresh, duration_thresh):
    """vilco_decode: threshold -> exact top-k -> segment decode -> duration filter of one clip's pyramid (all levels, one
    launch) -> (segments [n, 2], scores [n], labels [n] int64); ONE host read (n)."""
    lib = _lib.load()
    R, Cn = logits.shape
    L = int(level_row0.numel())
    cap = L * int(topk)
    dev = logits.device
    segs = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    scores = torch.empty(cap, dtype=torch.float32, device=dev)
    labels = torch.empty(cap, dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    nws = lib.vilco_decode_workspace(L, int(topk))
    ws = _ws(nws, dev)
    _lib.check(lib.vilco_decode(logits.data_ptr(), offsets.data_ptr(), points.data_ptr(), level_row0.data_ptr(),
                                level_len.data_ptr(), int(Cn), L, int(topk), float(pre_nms_thresh), float(duration_thresh),
                                segs.data_ptr(), scores.data_ptr(), labels.data_ptr(), total.data_ptr(), ws.data_ptr(), nws,
                                _stream()))
    n = int(total.item())
    return segs[:n], scores[:n], labels[:n]


# ---------------------------------------------------------------------------------------- herding exemplar selection
def frob_scale(x):
    """vilco_frob_scale: 1 / ||row||_2 of every row of fp32 x [N, D] -> [N] fp32."""
    _chk(x)
    lib = _lib.load()
    N, D = x.shape
    inv = torch.empty(N, dtype=torch.float32, device=x.device)
    nws = lib.vilco_frob_scale_workspace(N, D)
    ws = _ws(nws, x.device)
    _lib.check(lib.vilco_frob_scale(x.data_ptr(), N, D, D, inv.data_ptr(), ws.data_ptr(), nws, _stream()))
    return inv


def gram(x, row_scale=None, out_dtype=torch.float32):
    """vilco_gram: G = diag(row_scale) x x^T diag(row_scale) for fp32 x [N, D] -> [N, N] fp32 or fp64 (exact fp32
    products, fp32 accumulation per K slab, slabs added in fp64 in a fixed order; exactly symmetric)."""
    _chk(x, row_scale)
    if out_dtype not in (torch.float32, torch.float64):
        raise RuntimeError("gram writes fp32 or fp64, not %s" % out_dtype)
    lib = _lib.load()
    N, D = x.shape
    if row_scale is not None and tuple(row_scale.shape) != (N,):
        raise RuntimeError("row_scale must have one entry per row")
    g = torch.empty(N, N, dtype=out_dtype, device=x.device)
    nws = lib.vilco_gram_workspace(N, D)
    ws = _ws(nws, x.device)
    _lib.check(lib.vilco_gram(x.data_ptr(), N, D, D, _p(row_scale), g.data_ptr(), int(out_dtype == torch.float64),
                              ws.data_ptr(), nws, _stream()))
    return g


def herd_select(grams, m):
    """vilco_herd_select: the greedy herding order of one class from its per-level Gram matrices.  grams: [L, N, N] (a
    tensor or a list of L [N, N] tensors; fp32 is widened), m: how many to pick -> int32 [min(m, N)] on the device."""
    if not torch.is_tensor(grams):
        grams = torch.stack([g.to(torch.float64) for g in grams], dim=0)
    if not grams.is_cuda:
        raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback" % grams.device)
    if grams.dim() != 3 or grams.shape[1] != grams.shape[2]:
        raise RuntimeError("grams must be [L, N, N]")
    grams = grams.to(torch.float64).contiguous()
    lib = _lib.load()
    L, N = int(grams.shape[0]), int(grams.shape[1])
    m = max(int(m), 0)
    sel = torch.empty(min(m, N), dtype=torch.int32, device=grams.device)
    nws = lib.vilco_herd_select_workspace(1, L, N)
    ws = _ws(nws, grams.device)
    _lib.check(lib.vilco_herd_select(grams.data_ptr(), 1, L, N, m, sel.data_ptr(), ws.data_ptr(), nws, _stream()))
    return sel


# ---------------------------------------------------------------------------------------- multi-tensor chunk tables
CHUNK = 16384           # elements one block of a multi-tensor kernel walks (csrc/optim.hip)


class ChunkPlan:
    """The host half of a vilco_chunk_table (include/vilco_hip.h) over tensors of `numels` elements: the device tensors `numel`,
    `chunk_tensor`, `chunk_off` (uploaded in this order; an empty one is padded to one element, so its address is not null),
    `nchunks`, and the host list `first` -- first[i] .. first[i + 1] are the chunks of tensor i.  `table(ptrs, rows)` adds the
    [rows, n] pointer tensor of a call."""

    def __init__(self, numels, device, chunk=CHUNK, non_blocking=False):
        self.n, self.chunk = len(numels), chunk
        ct, co, self.first = [], [], []
        for i, n in enumerate(numels):
            self.first.append(len(ct))
            for off in range(0, n, chunk):
                ct.append(i)
                co.append(off)
        self.first.append(len(ct))
        self.nchunks = len(ct)
        self.numel, self.chunk_tensor, self.chunk_off = (
            torch.tensor(v or [0], dtype=dt).to(device, non_blocking=non_blocking)
            for v, dt in ((list(numels), torch.int64), (ct, torch.int32), (co, torch.int64)))

    def table(self, ptrs, rows):
        return _lib.ChunkTable(ptrs=ptrs.data_ptr(), numel=self.numel.data_ptr(), chunk_tensor=self.chunk_tensor.data_ptr(),
                               chunk_off=self.chunk_off.data_ptr(), rows=rows, n=self.n, nchunks=self.nchunks, chunk=self.chunk)


# ---------------------------------------------------------------------------------------- EWC / MAS importance accumulation
CL_CHUNK = CHUNK
CL_OP_COPY, CL_OP_SQUARE, CL_OP_ABS = 0, 1, 2
_cl_plan = {}           # the last ChunkPlan, by (numels, device): a consolidation pass asks for the same one every batch


def cl_accumulate(srcs, accs, op, alpha, beta, numels=None):
    """vilco_cl_accumulate: accs[t][:n_t] = beta * accs[t][:n_t] + alpha * f(srcs[t][:n_t]) over the flat elements of every
    pair, in place, as ONE multi-tensor launch.  op: 0 f(x) = x, 1 x * x, 2 |x|.  numels: n_t per pair (default: all of
    accs[t]); elements past it are not touched.  beta == 0: accs is not read; alpha == 0: srcs is not read.
    Pairs that live in HOST memory get the same expression, in the same order, as tensor ops (the consolidation pass of a
    model that lives on the host); device tensors always go through the kernel."""
    if op not in (CL_OP_COPY, CL_OP_SQUARE, CL_OP_ABS):
        raise ValueError("cl_accumulate: op must be 0 (x), 1 (x * x) or 2 (|x|), got %r" % (op,))
    srcs, accs = list(srcs), list(accs)
    if len(srcs) != len(accs):
        raise RuntimeError("cl_accumulate: %d sources for %d accumulators" % (len(srcs), len(accs)))
    numels = [a.numel() for a in accs] if numels is None else [int(n) for n in numels]
    if len(numels) != len(accs) or any(n < 0 or n > a.numel() or n > s.numel() for n, s, a in zip(numels, srcs, accs)):
        raise RuntimeError("cl_accumulate: numels must give a prefix of every source and accumulator")
    if not accs:
        return
    alpha, beta = float(alpha), float(beta)
    if not any(t.is_cuda for t in srcs + accs):
        for s, a, n in zip(srcs, accs, numels):
            if s.dtype != torch.float32 or a.dtype != torch.float32 or not (s.is_contiguous() and a.is_contiguous()):
                raise RuntimeError("cl_accumulate needs contiguous fp32 tensors")
            av = a.detach().view(-1)[:n]
            if alpha == 0.0:
                av.mul_(beta) if beta != 0.0 else av.zero_()
                continue
            x = s.detach().view(-1)[:n]
            f = x * x if op == CL_OP_SQUARE else x.abs() if op == CL_OP_ABS else x
            if beta == 0.0:
                av.copy_(f * alpha)
            else:
                av.mul_(beta).add_(f * alpha)
        return
    _chk(*srcs)
    _chk(*accs)
    dev = accs[0].device
    key = (tuple(numels), dev)
    if key not in _cl_plan:
        _cl_plan.clear()
        _cl_plan[key] = ChunkPlan(numels, dev)
    ptrs = torch.tensor([[s.data_ptr() for s in srcs], [a.data_ptr() for a in accs]], dtype=torch.int64).to(dev, non_blocking=True)
    _lib.check(_lib.load().vilco_cl_accumulate(C.byref(_cl_plan[key].table(ptrs, 2)), int(op), alpha, beta, _stream()))


# ---------------------------------------------------------------------------------------- A-GEM gradient projection
_agem_plan = {}         # the last (ChunkPlan, partials), by (numels, device): a task asks for the same one every iteration


def agem_project(grads, refs, device=None):
    """vilco_agem_project (Chaudhry et al., ICLR 2019): with g = all of `grads` and r = all of `refs` taken as one vector each,
    grads[t] -= (g.r / r.r) * refs[t] in place when g.r < 0 and r.r > 0; otherwise nothing is written.  Three launches, the
    branch is taken on the device.  grads / refs: lists of contiguous fp32 device tensors with pairwise equal numel.
    -> out, a device tensor [3] = {g.r, r.r, alpha} (alpha = 0: no projection), not synchronised.  Empty lists give zeros
    (on `device`, default the current one)."""
    grads, refs = list(grads), list(refs)
    if len(grads) != len(refs):
        raise RuntimeError("agem_project: %d gradients for %d reference gradients" % (len(grads), len(refs)))
    _chk(*grads)
    _chk(*refs)
    numels = tuple(g.numel() for g in grads)
    if any(r.numel() != n for r, n in zip(refs, numels)):
        raise RuntimeError("agem_project: a gradient and its reference gradient differ in their element count")
    dev = grads[0].device if grads else torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if any(t.device != dev for t in grads + refs):
        raise RuntimeError("agem_project: all tensors must live on one device")
    key = (numels, dev)
    if key not in _agem_plan:
        _agem_plan.clear()
        plan = ChunkPlan(numels, dev)
        _agem_plan[key] = (plan, torch.empty(2 * max(plan.nchunks, 1), dtype=torch.float32, device=dev))
    plan, partial = _agem_plan[key]
    ptrs = torch.tensor([[g.data_ptr() for g in grads], [r.data_ptr() for r in refs]] if grads else [[0], [0]],
                        dtype=torch.int64).to(dev, non_blocking=True)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().vilco_agem_project(C.byref(plan.table(ptrs, 2)), partial.data_ptr(), out.data_ptr(), _stream()))
    return out


# ---------------------------------------------------------------------------------------- BiC stage 2 over cached logits
def _bic_cache_args(logits, label_bits, weight, pos, clip_ptr):
    for t, dt, name in ((logits, torch.float32, 'logits'), (label_bits, torch.int64, 'label_bits'),
                        (weight, torch.float32, 'weight'), (pos, torch.uint8, 'pos'), (clip_ptr, torch.int32, 'clip_ptr')):
        if not t.is_cuda:
            raise RuntimeError("vilco_amd ops run on the HIP device only (got a %s tensor); there is no CPU fallback" % t.device)
        if t.dtype != dt or not t.is_contiguous():
            raise RuntimeError("%s must be a contiguous %s tensor" % (name, dt))
    N, Cn = logits.shape
    if tuple(label_bits.shape) != (N, 2) or tuple(weight.shape) != (N,) or tuple(pos.shape) != (N,) or clip_ptr.dim() != 1 \
            or clip_ptr.numel() < 1:
        raise RuntimeError("BiC cache arrays do not agree: logits [N, C], label_bits [N, 2], weight [N], pos [N], clip_ptr [n + 1]")
    return int(N), int(Cn), int(clip_ptr.numel()) - 1


def bic_eval(logits, label_bits, weight, pos, clip_ptr, lo, hi, smoothing, ab):
    """vilco_bic_eval: (L, dL/dalpha, dL/dbeta) of the stage-2 objective over ALL clips of the cache at ab = (alpha, beta)
    (fp32 [2] on the device) -> fp64 [3] on the device.  label_bits: int64 [N, 2] holding the uint64 bit patterns."""
    N, Cn, n_clips = _bic_cache_args(logits, label_bits, weight, pos, clip_ptr)
    _chk(ab)
    lib = _lib.load()
    out = torch.empty(3, dtype=torch.float64, device=logits.device)
    nws = lib.vilco_bic_eval_ws_bytes(N, n_clips, int(lo), int(hi))
    ws = _ws(nws, logits.device)
    _lib.check(lib.vilco_bic_eval(logits.data_ptr(), label_bits.data_ptr(), weight.data_ptr(), pos.data_ptr(), clip_ptr.data_ptr(),
                                  N, n_clips, Cn, int(lo), int(hi), float(smoothing), ab.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                  nws, _stream()))
    return out


def bic_fit(logits, label_bits, weight, pos, clip_ptr, order, batch_clips, lo, hi, smoothing, lr, ab):
    """vilco_bic_fit: order.numel() // batch_clips plain-SGD steps on ab = (alpha, beta) (fp32 [2] on the device, updated in
    place), step k over the clips order[k * batch_clips : (k + 1) * batch_clips] (int32 on the device).  Returns the steps'
    losses, fp64 [n_steps] on the device.  Nothing waits for the host."""
    N, Cn, n_clips = _bic_cache_args(logits, label_bits, weight, pos, clip_ptr)
    _chk(ab)
    if not order.is_cuda or order.dtype != torch.int32 or not order.is_contiguous():
        raise RuntimeError("order must be a contiguous int32 tensor on the device")
    lib = _lib.load()
    batch_clips = int(batch_clips)
    n_steps = int(order.numel()) // batch_clips if batch_clips > 0 else 0
    losses = torch.empty(n_steps, dtype=torch.float64, device=logits.device)
    nws = lib.vilco_bic_fit_ws_bytes(N, n_clips, batch_clips, int(lo), int(hi))
    ws = _ws(nws, logits.device)
    _lib.check(lib.vilco_bic_fit(logits.data_ptr(), label_bits.data_ptr(), weight.data_ptr(), pos.data_ptr(), clip_ptr.data_ptr(),
                                 N, n_clips, order.data_ptr(), n_steps, batch_clips, Cn, int(lo), int(hi), float(smoothing),
                                 float(lr), ab.data_ptr(), losses.data_ptr(), ws.data_ptr(), nws, _stream()))
    return losses


# ---------------------------------------------------------------------------------------- fused ln1 -> q/k/v pre-projection
def qkv_pre_supported(Cn):
    return bool(_lib.load().vilco_qkv_pre_supported(int(Cn)))


use_qkv_pre = switches.on("VILCO_QKV_PRE")


def _ptr3(ts):
    return (_lib.c_fp * 3)(*[_p(t) for t in ts])


class _QkvPre(torch.autograd.Function):
    """h = LN1(x); y_j = LN_j(dwconv3_stride(h; w_j) * mask), j = q, k, v   (blocks.py:561-563, 363-369) in one launch
    (vilco_qkv_pre_fwd); backward = vilco_qkv_pre_bwd (conv outputs recomputed from h) + LN1's ordinary backward."""

    @staticmethod
    def forward(ctx, x, g1, b1, wq, wk, wv, gq, bq, gk, bk, gv, bv, lens, stride, eps1, eps, want_h, skip=False):
        _chk(x, g1, b1, wq, wk, wv, gq, bq, gk, bk, gv, bv)
        ctx.skip = bool(skip)            # x returned as a last output: the block's skip connection (see _LayerNorm.forward)
        ctx.set_materialize_grads(False)
        lib = _lib.load()
        B, T, Cn = x.shape
        To = T // stride
        dev = x.device
        ys = [torch.empty(B, To, Cn, dtype=torch.float32, device=dev) for _ in range(3)]
        h = torch.empty_like(x) if want_h else None
        stats1 = torch.empty(2, B * T, dtype=torch.float32, device=dev)
        stats = torch.empty(6, B * To, dtype=torch.float32, device=dev)
        means, rstds = [stats[2 * j] for j in range(3)], [stats[2 * j + 1] for j in range(3)]
        npart = lib.vilco_qkv_pre_amax_parts(B, T, int(stride)) if (produce_amax and _precision == 3) else 0
        parts = torch.empty(3, npart, dtype=torch.float32, device=dev) if npart > 0 else None
        _lib.check(lib.vilco_qkv_pre_fwd(x.data_ptr(), _p(g1), _p(b1), _ptr3([wq, wk, wv]), _ptr3([gq, gk, gv]),
                                         _ptr3([bq, bk, bv]), lens.data_ptr(), _p(h), _ptr3(ys), stats1[0].data_ptr(),
                                         stats1[1].data_ptr(), _ptr3(means), _ptr3(rstds),
                                         _ptr3([parts[0], parts[1], parts[2]]) if parts is not None else None, B, T, Cn,
                                         int(stride), float(eps1), float(eps), _stream()))
        if parts is not None:
            for j in range(3):
                _leave(_QkvPre, j, amax=(parts[j], npart))
        ctx.stride, ctx.eps1, ctx.want_h = int(stride), float(eps1), bool(want_h)
        ctx.save_for_backward(x, g1, b1, wq, wk, wv, gq, gk, gv, lens, stats1, stats, h)
        outs = (ys[0], ys[1], ys[2], h) if want_h else (ys[0], ys[1], ys[2])
        return outs + (x,) if skip else outs

    @staticmethod
    def backward(ctx, dq, dk, dv, *more):
        x, g1, b1, wq, wk, wv, gq, gk, gv, lens, stats1, stats, h = ctx.saved_tensors
        more = list(more)
        dh_ext = more.pop(0) if ctx.want_h and more else None
        dskip = more.pop(0) if ctx.skip and more else None
        dskip = None if dskip is None else dskip.contiguous()
        lib = _lib.load()
        B, T, Cn = x.shape
        To = T // ctx.stride
        dev = x.device
        if h is None:        # nobody else needed h in forward: rebuild it (one LayerNorm pass) for the conv recomputation
            h = torch.empty_like(x)
            d = _lib.LnFwdDesc(x=x.data_ptr(), gamma=_p(g1), beta=_p(b1), y=h.data_ptr(), rows=B * T, C=Cn, eps=ctx.eps1)
            _lib.check(lib.vilco_layernorm_fwd(C.byref(d), _stream()))
        dys = [torch.zeros(B, To, Cn, dtype=torch.float32, device=dev) if g is None else g.contiguous() for g in (dq, dk, dv)]
        dcs = [torch.empty(B, To, Cn, dtype=torch.float32, device=dev) for _ in range(3)]
        dh = torch.empty_like(x)
        dpar = torch.empty(15, Cn, dtype=torch.float32, device=dev)
        nws = lib.vilco_qkv_pre_bwd_workspace(B, T, Cn, ctx.stride)
        means, rstds = [stats[2 * j] for j in range(3)], [stats[2 * j + 1] for j in range(3)]
        dh_ext = None if dh_ext is None else dh_ext.contiguous()
        dx = torch.empty_like(x)
        dg1 = torch.empty(Cn, dtype=torch.float32, device=dev)
        db1 = torch.empty(Cn, dtype=torch.float32, device=dev)
        with _Deferring(g1, wq, wk, wv, gq, gk, gv) as dfr:      # 15 parameter-gradient rows + LN1's affine gradients
            ws = _ws(nws, dev)
            _lib.check(lib.vilco_qkv_pre_bwd(h.data_ptr(), _ptr3([wq, wk, wv]), _ptr3([gq, gk, gv]), _ptr3(dys), _ptr3(means),
                                             _ptr3(rstds), lens.data_ptr(), _p(dh_ext), _ptr3(dcs), dh.data_ptr(), dpar.data_ptr(),
                                             B, T, Cn, ctx.stride, ws.data_ptr(), nws, _stream()))
            del dcs
            ws1 = _ws(lib.vilco_layernorm_bwd_workspace(B * T, Cn), dev)
            d = _lib.LnBwdDesc(dy=dh.data_ptr(), x=x.data_ptr(), gamma=_p(g1), mean=stats1[0].data_ptr(), rstd=stats1[1].data_ptr(),
                               dres=_p(dskip), dx=dx.data_ptr(), dgamma=dg1.data_ptr(), dbeta=db1.data_ptr(), rows=B * T, C=Cn,
                               workspace=ws1.data_ptr(), workspace_bytes=ws1.numel())
            _lib.check(lib.vilco_layernorm_bwd(C.byref(d), _stream()))
            dfr.hold(dpar, dg1, db1)
        dws = [dpar[6 + 3 * j:9 + 3 * j].view_as(w) for j, w in enumerate((wq, wk, wv))]      # already [C][1][3] (qkvpre.hip)
        dgs = [dpar[2 * j].view_as(g) for j, g in enumerate((gq, gk, gv))]
        dbs = [dpar[2 * j + 1].view_as(g) for j, g in enumerate((gq, gk, gv))]
        return (dx, dg1.view_as(g1), db1.view_as(g1), dws[0], dws[1], dws[2], dgs[0], dbs[0], dgs[1], dbs[1], dgs[2], dbs[2],
                None, None, None, None, None, None)


def qkv_pre(x, ln1, convs, norms, lens, stride, want_h, skip=False):
    """x [B,T,C]; ln1 = (weight, bias, eps) of the block's first LayerNorm; convs = three depthwise [C,1,3] weights
    (query, key, value); norms = three (weight, bias) pairs + one eps -> (q, k, v[, h][, x_skip]).
    skip: x comes back as the last output, for the block's skip connection (ops.layernorm's `skip`)."""
    (g1, b1, eps1), (wq, wk, wv), ((gq, bq), (gk, bk), (gv, bv), eps) = ln1, convs, norms
    x = x.contiguous()
    fold = bool(skip and fold_skip_grads and x.requires_grad)
    outs = _apply(_QkvPre, x, g1, b1, wq, wk, wv, gq, bq, gk, bk, gv, bv, lens, int(stride), float(eps1),
                  float(eps), bool(want_h), fold)
    return tuple(outs) + (x,) if skip and not fold else outs


# ---------------------------------------------------------------------------------------- narration SSL (csrc/ssl.hip)
def _ptr_table(ts):
    return (_lib.c_fp * len(ts))(*[t.data_ptr() for t in ts])


class _SslPool(torch.autograd.Function):
    """masked mean over time of every level, averaged over the levels (vilco_ssl_pool_fwd / _bwd)"""

    @staticmethod
    def forward(ctx, lens, *feats):
        _chk(*feats)
        lib = _lib.load()
        B, _, Cn = feats[0].shape
        L = len(feats)
        T = (_lib.i32 * L)(*[int(f.shape[1]) for f in feats])
        out = torch.empty(B, Cn, dtype=torch.float32, device=feats[0].device)
        nws = lib.vilco_ssl_pool_workspace(T, L, B, Cn)
        ws = _ws(nws, out.device)
        _lib.check(lib.vilco_ssl_pool_fwd(_ptr_table(feats), T, L, lens.data_ptr(), B, Cn, out.data_ptr(), ws.data_ptr(), nws,
                                          _stream()))
        ctx.T, ctx.shapes, ctx.lens = T, [f.shape for f in feats], lens
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        grads = [torch.empty(s, dtype=torch.float32, device=dout.device) for s in ctx.shapes]
        B, _, Cn = ctx.shapes[0]
        _lib.check(_lib.load().vilco_ssl_pool_bwd(dout.data_ptr(), _ptr_table(grads), ctx.T, len(grads), ctx.lens.data_ptr(),
                                                  B, Cn, _stream()))
        return (None,) + tuple(grads)


def ssl_pool(feats, lens):
    """feats: list of L <= 16 token-major fp32 [B, T_l, C]; lens: int32 [B, L] prefix lengths on the device ->
    [B, C] = mean over levels of the mean over the rows below the length (0 for an empty level).  meta_archs.py:794-811."""
    if not 1 <= len(feats) <= 16:
        raise RuntimeError("ssl_pool takes 1 to 16 levels, got %d" % len(feats))
    B, Cn = feats[0].shape[0], feats[0].shape[2]
    if any(f.dim() != 3 or f.shape[0] != B or f.shape[2] != Cn for f in feats):
        raise RuntimeError("ssl_pool: every level must be [B, T_l, C] with the same B and C")
    if lens.dtype != torch.int32 or tuple(lens.shape) != (B, len(feats)) or not lens.is_cuda or not lens.is_contiguous():
        raise RuntimeError("ssl_pool: lens must be a contiguous int32 [B, L] device tensor")
    return _SslPool.apply(lens, *[f.contiguous() for f in feats])


class _SslNce(torch.autograd.Function):
    """normalise -> ring update of the memory bank -> InfoNCE (vilco_ssl_nce_fwd / _bwd)"""

    @staticmethod
    def forward(ctx, text, video, mask, bank, ring, temperature):
        _chk(text, video, mask, bank)
        lib = _lib.load()
        B, D = text.shape
        M = bank.shape[0]
        dev = text.device
        xn = torch.empty(2, B, D, dtype=torch.float32, device=dev)
        stats = torch.empty(7 * B, dtype=torch.float32, device=dev)
        logits = torch.empty(2 * B, M, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nws = lib.vilco_ssl_nce_workspace(B, D, M)
        ws = _ws(nws, dev)
        _lib.check(lib.vilco_ssl_nce_fwd(text.data_ptr(), video.data_ptr(), mask.data_ptr(), B, D, bank.data_ptr(), M,
                                         ring.data_ptr(), temperature, xn.data_ptr(), stats.data_ptr(), logits.data_ptr(),
                                         loss.data_ptr(), ws.data_ptr(), nws, _stream()))
        ctx.temperature, ctx.bank = temperature, bank           # (the bank is not an autograd input's value: no version check)
        ctx.save_for_backward(mask, xn, stats, logits)
        ctx.mark_non_differentiable(xn)
        return loss[0], xn

    @staticmethod
    def backward(ctx, gloss, _gxn):
        mask, xn, stats, logits = ctx.saved_tensors
        lib = _lib.load()
        _, B, D = xn.shape
        bank = ctx.bank
        M = bank.shape[0]
        gloss = gloss.contiguous().float().reshape(1)
        dt = torch.empty(B, D, dtype=torch.float32, device=xn.device)
        dv = torch.empty(B, D, dtype=torch.float32, device=xn.device)
        nws = lib.vilco_ssl_nce_workspace(B, D, M)
        ws = _ws(nws, xn.device)
        _lib.check(lib.vilco_ssl_nce_bwd(gloss.data_ptr(), mask.data_ptr(), xn.data_ptr(), stats.data_ptr(), logits.data_ptr(),
                                         bank.data_ptr(), B, D, M, ctx.temperature, dt.data_ptr(), dv.data_ptr(), ws.data_ptr(),
                                         nws, _stream()))
        return dt, dv, None, None, None, None


def _ssl_bank_args(rows, mask, bank, ring):
    B, D = rows.shape
    if tuple(mask.shape) != (B,) or bank.dim() != 2 or bank.shape[1] != D:
        raise RuntimeError("narration SSL: rows [B, D], mask [B] and bank [M, D] do not fit together")
    if D % 4 or D > 4096 or not 1 <= B <= 64 or B > bank.shape[0]:
        raise RuntimeError("narration SSL: need D %% 4 == 0, D <= 4096, 1 <= B <= 64 and B <= the bank's size "
                           "(B = %d, D = %d, M = %d)" % (B, D, bank.shape[0]))
    if ring.dtype != torch.int32 or ring.numel() != 1 or not ring.is_cuda:
        raise RuntimeError("narration SSL: the ring word is a device int32[1]")


def ssl_nce(text, video, mask, bank, ring, temperature=0.07):
    """raw pooled text / video [B, D], mask float [B], bank [M, D] and ring word int32[1] (both updated in place) ->
    (loss, normalised rows [2, B, D]).  meta_archs.py:38-60, 939-945, 1351-1372; include/vilco_hip.h has the definition.
    The backward reads the bank as the forward left it (its rows are constants of the loss and are not saved a second time):
    run each call's backward before the next call that writes the same bank, as a training step does.  The bank is not an
    autograd input, so autograd does not police this -- two forwards followed by two backwards give the first one the
    second one's negatives."""
    text, video, mask = text.contiguous(), video.contiguous(), mask.contiguous()
    if text.shape != video.shape or text.dim() != 2:
        raise RuntimeError("ssl_nce: text and video must both be [B, D]")
    _chk(text, mask, bank)
    _ssl_bank_args(text, mask, bank, ring)
    return _SslNce.apply(text, video, mask, bank, ring, float(temperature))


def ssl_ring_update(rows, mask, bank, ring):
    """the bank's masked ring update alone: rows [B, D] (already normalised) with mask != 0 go to (ring + rank) mod M"""
    rows, mask = rows.contiguous(), mask.contiguous()
    _chk(rows, mask, bank)
    _ssl_bank_args(rows, mask, bank, ring)
    _lib.check(_lib.load().vilco_ssl_ring_update(rows.data_ptr(), mask.data_ptr(), rows.shape[0], rows.shape[1],
                                                 bank.data_ptr(), bank.shape[0], ring.data_ptr(), _stream()))
