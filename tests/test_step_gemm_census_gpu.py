"""Every GEMM launch of a full-size training step against float64.

`ops.gemm` / `ops.gemm_group` are the only way into vilco_gemm / vilco_gemm_group.  Wrapped here, every launch of one eager
forward + backward of the benchmarked config P, of config W (D = 2304, hd = 144) and of cfg1 (BASELINE configs[0]) is checked
on its own: the device is synchronised, the fp32 inputs are snapshotted, the real call runs, and C (and the pre-activation,
when one is written) is compared with a float64 product built from the descriptor's documented semantics
(include/vilco_hip.h, vilco_gemm_desc): batch strides and offsets, operand orientation, the k = 3 conv taps, the XLNet band,
alpha, bias, activation, row length / row mask, column scale, fused dropout, residual and beta.

Bars (max|got - want| / max|want|, as tests/test_ops_gpu.py): 2e-5 for precision 3 (fp16 x2) and 2 (bf16 x3), 2e-4 for 0
(bf16 x2), 2e-2 for 1 (bf16), 2e-6 for 4 (single-part weight gradients) against the product of the lead-rounded operands.
Entries zeroed by the row mask or by dropout must be exactly zero (or exactly the residual).

Contracts checked on every launch that uses them:
  * max|x| partials handed in (a_amax / b_amax): when they are the producer's tag of the operand tensor, their maximum IS
    max|x| of that tensor, exactly; any other partials (a bound, e.g. the unit bound of a softmax output) must bound it;
  * partials written (amax_out): their maximum is max|C|, exactly;
  * operand planes handed in (a_planes / b_planes): they decode (vilco_pack's layout, csrc/pack.h) to the fp32 operand to
    the format's precision; where the call gets no fp32 operand (planes written by a producer kernel; XLNet's band products
    on the relshift-packed dS) the decoded planes are the reference operand."""
import inspect
import math
import traceback

import pytest
import torch
import torch.nn.functional as F

from fullsize_steps import STEPS, build_step, run_step

pytestmark = pytest.mark.gpu

BARS = {3: 2e-5, 2: 2e-5, 0: 2e-4, 1: 2e-2, 4: 2e-6}
NPARTS = {0: 2, 1: 1, 2: 3, 3: 2, 4: 2}            # 16-bit planes per operand (precision 4 reads the precision-3 planes)
PACK_HDR = 4096 + 512                              # vilco_pack buffers: amax partials, {1/s, s}, pad (csrc/common.h)
MIN_LAUNCHES = {"P": 300}


def _decode_tol(prec, x, s):
    """how far decoded planes may be from the fp32 operand x (pack.h: fp16 x2 of x*s to 22 bits, floor 2^-25 / s; bf16 parts)"""
    if prec in (3, 4):
        return x.abs() * 2.0 ** -21 + 2.0 ** -24 / s
    return x.abs() * {2: 2.0 ** -22, 0: 2.0 ** -15, 1: 2.0 ** -8}[prec] + 1e-37


def _strided(t, off, shape, strides):
    base = t.storage_offset() + int(off)
    last = base + sum((n - 1) * st for n, st in zip(shape, strides))
    assert last < t.untyped_storage().nbytes() // t.element_size(), "operand view beyond its tensor's storage"
    return t.detach().as_strided(shape, strides, base)


def _taps(S, T):
    """k = 3 'same' conv rows: [nb, R, W] token rows (sequences of T) -> [nb, R, 3W] = [x[t-1] | x[t] | x[t+1]], zero outside
    the sequence (the gather form of the tapped operand; no convolution call)"""
    nb, R, W = S.shape
    p = F.pad(S.reshape(nb, R // T, T, W), (0, 0, 1, 1))
    return torch.cat([p[:, :, 0:T], p[:, :, 1:T + 1], p[:, :, 2:T + 2]], -1).reshape(nb, R, 3 * W)


def _tap_plane_rows(nseq, T):
    return (nseq * (T + 2) + 31) // 32 * 32 + 64          # csrc/common.h: vilco_tap_plane_rows


class _Census:
    def __init__(self, ops, lib, real_gemm):
        self.ops, self.lib = ops, lib
        self.sig = inspect.signature(real_gemm)
        self.launches, self.groups = 0, 0
        self.descs = set()
        self.worst = {}
        self.contracts = {"a_amax exact": 0, "amax bound": 0, "amax_out": 0, "planes decoded": 0, "planes as operand": 0}
        self.failures = []

    # ------------------------------------------------------------------------------------------ snapshot
    def _site(self):
        fr = [f for f in traceback.extract_stack()[:-3] if "vilco_amd" in f.filename or "modeling" in f.filename]
        return " <- ".join("%s:%d %s" % (f.filename.split("vilco_amd/")[-1], f.lineno, f.name) for f in fr[::-1][:5])

    def _geom(self, b, which):
        """(rows, width, ld, tapped) of the matrix an operand lives in (the matrix vilco_pack packs)"""
        M, N, K = b["M"], b["N"], b["K"]
        if which == "a":
            kc, ld, tapped = b["a_kc"], b["lda"], b["tap"] == self.ops.TAP_A
            R, W = (M, b["tapC"]) if tapped else ((M, K) if kc else (K, M))
        else:
            kc, ld, tapped = b["b_kc"], b["ldb"], b["tap"] == self.ops.TAP_B
            R, W = (K, b["tapC"]) if tapped else ((N, K) if kc else (K, N))
        if tapped:
            assert ld == b["tapC"] and kc == (1 if which == "a" else 0), "unexpected tapped operand layout %s" % (b,)
        return R, W, ld, tapped

    def _decode(self, planes, prec, R, W, seq_T, lead_only=False):
        """planes -> (fp64 [nb, R, W] matrix, scale s) ; seq_T > 0: the k = 3 convs' per-sequence image"""
        np_ = NPARTS[prec]
        dt = torch.float16 if prec in (3, 4) else torch.bfloat16
        s = float(planes[:PACK_HDR].view(torch.float32)[1025]) if prec in (3, 4) else 1.0
        body = planes[PACK_HDR:]
        if seq_T:
            nseq = R // seq_T
            tr = _tap_plane_rows(nseq, seq_T)
            stride = (tr * W + 7) // 8 * 8
            img = body[:np_ * stride * 2].view(dt).view(np_, stride)[:, :tr * W].reshape(np_, tr, W)
            img = img[:, :nseq * (seq_T + 2)].reshape(np_, nseq, seq_T + 2, W)
            pad = torch.stack([img[:, :, 0], img[:, :, seq_T + 1]])
            assert not bool(pad.any()), "per-sequence plane image: a sequence's pad row is not zero"
            parts = img[:, :, 1:seq_T + 1].reshape(np_, 1, R, W)
        else:
            r32, c32 = (R + 31) // 32 * 32, (W + 31) // 32 * 32
            per = np_ * r32 * c32 * 2
            nb = (planes.numel() - PACK_HDR) // per
            assert nb >= 1 and planes.numel() - PACK_HDR == nb * per, "planes of %d bytes are not [%d][%d] x %d" % (planes.numel(), R, W, nb)
            parts = body.view(dt).view(np_, nb, r32, c32)[:, :, :R, :W]
        parts = parts.double()
        dec = parts[0] if lead_only else parts.sum(0)
        return dec / s, s

    def snapshot(self, args, kwargs, desc=None):
        ops = self.ops
        b = self.sig.bind(*args, **kwargs)
        b.apply_defaults()
        b = dict(b.arguments)
        prec = ops.get_precision() if b["precision"] is None else int(b["precision"])
        bo, bi = int(b["batch"][0]), int(b["batch"][1])
        snap = dict(b=b, prec=prec, site=self._site(), nb=bo * bi)
        checks = []
        for w, X, off, st, pl, seq in (("a", b["A"], b["offA"], b["sA"], b["a_planes"], b["planes_seq"][0]),
                                       ("b", b["B"], b["offB"], b["sB"], b["b_planes"], b["planes_seq"][1])):
            R, W, ld, tapped = self._geom(b, w)
            S = None
            if X is not None:
                S = _strided(X, off, (bo, bi, R, W), (int(st[0]), int(st[1]), int(ld), 1)).clone().reshape(bo * bi, R, W)
            Sp, s = None, None
            if pl is not None:
                Sp, s = self._decode(pl, prec, R, W, int(b["tapT"]) if seq else 0, lead_only=False)
                if S is not None:
                    Sd = S.double()
                    if Sp.shape[0] == 1 and Sd.shape[0] > 1:
                        Sp = Sp.expand_as(Sd)
                    bad = (Sp - Sd).abs() > _decode_tol(prec, Sd, s)
                    if bool(bad.any()):
                        i = bad.nonzero()[0].tolist()
                        checks.append("%s_planes do not decode to the fp32 operand: %d entries, first %s: %r vs %r (scale %g)"
                                      % (w, int(bad.sum()), i, float(Sp[tuple(i)]), float(Sd[tuple(i)]), s))
                    self.contracts["planes decoded"] += 1
                    del Sd
                else:
                    self.contracts["planes as operand"] += 1
            # max|x| partials handed in: only read by a call that packs the operand itself, at precision 3 / 4
            am = b[w + "_amax"]
            if am is not None and am[0] is not None and prec in (3, 4) and pl is None and X is not None:
                mx = float(am[0][:int(am[1])].max())
                if ops._amax_of(X)[0] is am[0]:
                    whole = float(X.detach().abs().max())
                    if mx != whole:
                        checks.append("%s_amax: the producer's partials give max %r, max|x| of the operand tensor is %r" % (w, mx, whole))
                    self.contracts["a_amax exact"] += 1
                else:
                    seen = float(S.abs().max())
                    if not seen <= mx:
                        checks.append("%s_amax: the bound %r is below max|x| = %r of the operand" % (w, mx, seen))
                    self.contracts["amax bound"] += 1
            snap["op_" + w] = (S, Sp, s, tapped)
        M, N = b["M"], b["N"]
        Cc = b["Cc"]
        cshape, cstr = (bo, bi, M, N), (int(b["sC"][0]), int(b["sC"][1]), int(b["ldc"]), 1)
        snap["cview"] = (cshape, cstr)
        snap["c_old"] = _strided(Cc, b["offC"], cshape, cstr).clone() if float(b["beta"]) != 0.0 else None
        snap["residual"] = (_strided(b["residual"], b["offC"], cshape, cstr).clone() if b["residual"] is not None else None)
        snap["bias"] = None if b["bias"] is None else b["bias"].detach().clone()
        snap["colscale"] = None if b["colscale"] is None else b["colscale"].detach().clone()
        snap["row_len"] = None if b["row_len"] is None else b["row_len"].detach().cpu().tolist()
        snap["row_mask"] = None if b["row_mask"] is None else b["row_mask"].detach().clone()
        snap["amax_tag_before"] = ops._amax_of(Cc)[0]
        snap["checks"] = checks
        return snap

    # ------------------------------------------------------------------------------------------ reference + compare
    def _operand(self, snap, w):
        S, Sp, s, tapped = snap["op_" + w]
        b, prec = snap["b"], snap["prec"]
        if prec == 4:           # what the kernel multiplies: the leading fp16 parts (of the planes; else of the call's own pack)
            R, W, _, _ = self._geom(b, w)
            pl = b[w + "_planes"]
            if pl is not None:
                X, _ = self._decode(pl, prec, R, W, int(b["tapT"]) if b["planes_seq"][0 if w == "a" else 1] else 0, lead_only=True)
            else:
                am = b[w + "_amax"]
                mx = float(am[0][:int(am[1])].max()) if am is not None and am[0] is not None else float(S.abs().max())
                sc = 2.0 ** (14 - math.floor(math.log2(mx))) if mx > 0 else 1.0
                X = (S.double() * sc).half().double() / sc
        else:
            X = S.double() if S is not None else Sp
        if X.shape[0] == 1 and snap["nb"] > 1:
            X = X.expand(snap["nb"], -1, -1)
        T = int(b["tapT"])
        if tapped:
            X = _taps(X, T)
            return X if w == "a" else X          # A: [M][3 tapC] (k = tap * tapC + c);  B: [K rows = tokens][N = 3 tapC]
        a_kc, b_kc = b["a_kc"], b["b_kc"]
        if w == "a":
            X = X if a_kc else X.transpose(1, 2)
            band, bT = int(b["band"]), int(b["bandT"])
            if band in (2, 3):          # only the band 0 <= p - T + i < T of XLNet's [T, 2T] position matrix exists
                r = torch.arange(X.shape[1], device=X.device)[:, None]
                c = torch.arange(X.shape[2], device=X.device)[None, :]
                i, p = (r, c) if band == 2 else (c, r)
                X = X * ((p - bT + i >= 0) & (p - bT + i < bT)).to(X.dtype)
            return X
        return X.transpose(1, 2) if b_kc else X

    def verify(self, snap, plan):
        ops, b, prec = self.ops, snap["b"], snap["prec"]
        self.launches += 1
        M, N, K = b["M"], b["N"], b["K"]
        dev = b["Cc"].device
        key = (M, N, K, b["a_kc"], b["b_kc"], tuple(b["batch"]), int(b["tap"]), prec, int(b["band"]), b["bias"] is not None,
               int(b["act"]), b["row_len"] is not None or b["row_mask"] is not None, b["colscale"] is not None,
               b["residual"] is not None, float(b["drop"][0]) > 0, float(b["beta"]) != 0, b["a_planes"] is not None,
               b["b_planes"] is not None)
        self.descs.add(key)
        msgs = list(snap["checks"])
        A = self._operand(snap, "a")
        Bm = self._operand(snap, "b")
        acc = torch.matmul(A, Bm)                               # [nb, M, N] float64
        want = float(b["alpha"]) * acc
        if snap["bias"] is not None:
            want += snap["bias"].double()
        pre_want = want.clone() if b["preact"] is not None else None
        if int(b["act"]) == ops.ACT_RELU:
            want = want.clamp_min(0.0)
        elif int(b["act"]) == ops.ACT_GELU:
            want = 0.5 * want * (1.0 + torch.erf(want / math.sqrt(2.0)))
        valid = torch.ones(M, dtype=torch.bool, device=dev)
        if snap["row_len"] is not None:
            m = torch.arange(M, device=dev)
            lens = torch.tensor(snap["row_len"], device=dev)
            valid &= (m % int(b["rowT"])) < lens[m // int(b["rowT"])]
        if snap["row_mask"] is not None:
            valid &= snap["row_mask"].reshape(-1)[:M] != 0
        want = want * valid[None, :, None].to(want.dtype)
        if snap["colscale"] is not None:
            want = want * snap["colscale"].double()
        dropped = None
        p, seed = float(b["drop"][0]), int(b["drop"][1])
        if p > 0:
            assert snap["nb"] == 1 and int(b["ldc"]) == N, "fused dropout needs batch 1, ldc == N"
            fac = ops.dropout_mask(p, seed, (M, N), dev).double()
            dropped = (fac == 0)[None]
            want = want * fac
        res = snap["residual"]
        if res is not None:
            keep = torch.ones_like(valid) if not int(b["res_masked"]) else valid
            want = want + res.reshape(snap["nb"], M, N).double() * keep[None, :, None].to(torch.float64)
        if snap["c_old"] is not None:
            want = want + float(b["beta"]) * snap["c_old"].reshape(snap["nb"], M, N).double()
        got32 = _strided(b["Cc"], b["offC"], *snap["cview"]).reshape(snap["nb"], M, N)
        got = got32.double()
        cmp = None
        if int(b["band"]) == 1:          # C is the [T, 2T] band matrix: tiles outside the band are left unwritten
            bT = int(b["bandT"])
            i = torch.arange(M, device=dev)[:, None]
            pp = torch.arange(N, device=dev)[None, :]
            cmp = ((pp - bT + i >= 0) & (pp - bT + i < bT))[None]
        diff = (got - want).abs()
        ref = want.abs()
        if cmp is not None:
            diff, ref = diff * cmp, ref * cmp
        err = float(diff.max() / ref.max().clamp_min(1e-30))
        self.worst[prec] = max(self.worst.get(prec, 0.0), err)
        bar = BARS[prec]
        if not err < bar:
            cond = float(torch.matmul(A.abs(), Bm.abs()).max() * abs(float(b["alpha"])) / ref.max().clamp_min(1e-30))
            msgs.append("C: max|got - want| / max|want| = %.3e >= %.0e (precision %d; conditioning max(|A||B|) / max|C64| = %.3g)"
                        % (err, bar, prec, cond))
        if pre_want is not None:
            gp = _strided(b["preact"], b["offC"], *snap["cview"]).reshape(snap["nb"], M, N).double()
            e2 = float((gp - pre_want).abs().max() / pre_want.abs().max().clamp_min(1e-30))
            self.worst[prec] = max(self.worst[prec], e2)
            if not e2 < bar:
                msgs.append("preact: rel err %.3e >= %.0e" % (e2, bar))
        # entries the row mask or dropout zeroed: exactly zero, or exactly the residual
        if float(b["beta"]) == 0.0:
            zero = (~valid)[None, :, None].expand(snap["nb"], M, N)
            if dropped is not None:
                zero = zero | dropped
            if cmp is not None:
                zero = zero & cmp
            if bool(zero.any()):
                exact = torch.zeros_like(got32)
                if res is not None:
                    r32 = res.reshape(snap["nb"], M, N)
                    keep = torch.ones_like(valid) if not int(b["res_masked"]) else valid
                    exact = torch.where(keep[None, :, None], r32, exact)
                nbad = int((zero & (got32 != exact)).sum())
                if nbad:
                    msgs.append("%d masked / dropped entries are not exactly %s" % (nbad, "the residual" if res is not None else "zero"))
        # partials of max|C| written by the call
        tag = ops._amax_of(b["Cc"])
        if tag[0] is not None and tag[0] is not snap["amax_tag_before"]:
            mx, whole = float(tag[0][:tag[1]].max()), float(b["Cc"].detach().abs().max())
            if mx != whole:
                msgs.append("amax_out: partials give max %r, max|C| = %r" % (mx, whole))
            self.contracts["amax_out"] += 1
        del A, Bm, acc, want, got, diff, ref, pre_want
        if msgs:
            desc = {k: v for k, v in b.items() if not torch.is_tensor(v) and k not in ("a_amax", "b_amax", "_into")}
            desc.update({k: tuple(v.shape) for k, v in b.items() if torch.is_tensor(v)})
            self.failures.append("call site: %s\n  descriptor: %s\n  precision %d, plan (M, N, K, batch, tile rows, split-K, ...): %s\n  %s"
                                 % (snap["site"], desc, prec, plan, "\n  ".join(msgs)))

    # ------------------------------------------------------------------------------------------ the wrappers
    def _plan_begin(self):
        from vilco_amd import _lib
        _lib.check(self.lib.vilco_gemm_profile_begin())

    def _plan_end(self):
        import ctypes
        from vilco_amd import _lib
        ms, cnt = ctypes.c_double(), ctypes.c_int64()
        _lib.check(self.lib.vilco_gemm_profile_end(ctypes.byref(ms), ctypes.byref(cnt)))
        n = int(self.lib.vilco_gemm_profile_records(None, None, 0))
        desc = (ctypes.c_int64 * (10 * max(n, 1)))()
        self.lib.vilco_gemm_profile_records(desc, None, n)
        return [tuple(desc[i * 10:i * 10 + 6]) for i in range(n)]

    def wrap(self, real_gemm, real_group):
        pending = []

        def gemm(*args, **kwargs):
            if kwargs.get("_into") is not None:           # a descriptor of a group: snapshot now, verify after the group launch
                pending.append(self.snapshot(args, kwargs))
                return real_gemm(*args, **kwargs)
            torch.cuda.synchronize()
            snap = self.snapshot(args, kwargs)
            self._plan_begin()
            real_gemm(*args, **kwargs)
            plan = self._plan_end()
            torch.cuda.synchronize()
            self.verify(snap, plan)

        def gemm_group(calls):
            torch.cuda.synchronize()
            del pending[:]
            self._plan_begin()
            real_group(calls)
            plan = self._plan_end()
            torch.cuda.synchronize()
            self.groups += 1
            snaps = list(pending)
            del pending[:]
            assert len(snaps) == len(calls), "gemm_group filled %d descriptors through gemm(_into=...), expected %d" % (len(snaps), len(calls))
            for s in snaps:
                self.verify(s, plan)
        return gemm, gemm_group


@pytest.mark.parametrize("name", STEPS)
def test_every_gemm_of_the_step_vs_float64(dev, name, monkeypatch):
    from vilco_amd import ops, _lib
    monkeypatch.setattr(ops, "defer_finish", False)
    assert ops.get_precision() == 3
    if name == "P":
        assert ops.dw_precision == 4          # single-part weight gradients, as benchmarked
    model, batch = build_step(name, dev)
    census = _Census(ops, _lib.load(), ops.gemm)
    g, gg = census.wrap(ops.gemm, ops.gemm_group)
    monkeypatch.setattr(ops, "gemm", g)
    monkeypatch.setattr(ops, "gemm_group", gg)
    try:
        losses = run_step(model, batch)
    finally:
        monkeypatch.undo()
        del model
        torch.cuda.empty_cache()
    worst = ", ".join("precision %d: %.2e" % (p, e) for p, e in sorted(census.worst.items()))
    print("\n[gemm census %s] %d launches (%d group launches), %d distinct descriptors; worst error %s; contracts %s; losses %s"
          % (name, census.launches, census.groups, len(census.descs), worst, census.contracts,
             {k: round(v, 5) for k, v in losses.items()}))
    assert not census.failures, "%d of %d GEMM launches missed:\n%s" % (len(census.failures), census.launches,
                                                                          "\n".join(census.failures[:12]))
    assert census.launches >= MIN_LAUNCHES.get(name, 1), (name, census.launches)
    for p, e in census.worst.items():
        assert e < BARS[p]
