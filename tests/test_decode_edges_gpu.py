"""vilco_decode (csrc/decode.hip) against the float64 restatement of tests/decode_restatement.py where such a kernel goes
wrong: levels on both sides of every multiple of the 1024 threads (per = ceil(n / 1024) from 1 to 248, second trips of the
grid-stride loops), cuts at total - 1 / total / total + 1, tie groups that straddle the cut over several threads and waves,
a cut the last radix pass decides, saturated and non-finite logits, the duration filter after the cut, row layouts with
gaps and over-long allotments whose rows would win every cut if read, L = 1 and L = 64, the C ABI's error returns, a
workspace that is not aligned, the write footprint, and the recipe's own shape.

Calls go through the C ABI with raw pointers.  Outputs of capacity L * topk sit in NaN-filled (labels: poison-filled) buffers
between canaries; the workspace is the test's, between guard bytes.  The comparison is level by level in index order
(decode_restatement.compare): counts, labels and order exactly, scores within BAR_P relative (4 x the measured error of the
fp32 formula), segment ends within 2 2^-24 (|t| + |off stride|).  Every element of every case is compared, rows past
out_total must still hold their poison.  Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import decode_restatement as R
from glue_restatement import CANARY, guarded

pytestmark = pytest.mark.gpu

OK, BADARG, ERR_WORKSPACE = 0, -1, -4
POISON = -0x0123456789ABCDEF            # no class index
WS_PAD = 512


def _lib():
    import vilco_amd._lib as L
    return L.load()


def _stream():
    from vilco_amd import ops
    return ops._stream()


def guarded_i64(n, device):
    """glue_restatement.guarded for int64: [64 canary | n poison | 64 canary] -> (payload view, check)"""
    buf = torch.full((n + 2 * CANARY,), POISON, dtype=torch.int64, device=device)
    pat = (torch.arange(2 * CANARY, dtype=torch.int64) * 0x9E3779B97F4A7C + 0x5A5A00000000).to(device)
    buf[:CANARY] = pat[:CANARY]
    buf[CANARY + n:] = pat[CANARY:]

    def check():
        assert torch.equal(buf[:CANARY], pat[:CANARY]), "write in front of the labels"
        assert torch.equal(buf[CANARY + n:], pat[CANARY:]), "write past the end of the labels"
    return buf[CANARY:CANARY + n], check


class Call:
    """the device copies of a case and the guarded outputs of ONE vilco_decode call of capacity L * topk"""

    def __init__(self, dev, case, topk, misalign=0, short=0):
        self.case, self.topk = case, topk
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.d = {k: up(case[k]) for k in ("logits", "offsets", "points", "row0", "lens")}
        self.L = len(case["row0"])
        self.cap = self.L * topk
        self.segs, self.c_segs = guarded(2 * self.cap, dev)
        self.scores, self.c_scores = guarded(self.cap, dev)
        self.labels, self.c_labels = guarded_i64(self.cap, dev)
        self.total = torch.tensor([-77, -78, -79], dtype=torch.int32, device=dev)
        lib = _lib()
        self.nws = int(lib.vilco_decode_workspace(self.L, topk))
        self.ws = torch.full((self.nws + 2 * WS_PAD,), 0xA5, dtype=torch.uint8, device=dev)
        self.ws_off = (-self.ws.data_ptr()) % 256 + 256 + misalign          # the workspace starts `misalign` past a 256-byte line
        self.ws_bytes = self.nws - short
        self.ptrs = dict(logits=self.d["logits"].data_ptr(), offsets=self.d["offsets"].data_ptr(), points=self.d["points"].data_ptr(),
                         row0=self.d["row0"].data_ptr(), lens=self.d["lens"].data_ptr(), segs=self.segs.data_ptr(),
                         scores=self.scores.data_ptr(), labels=self.labels.data_ptr(), total=self.total[1:].data_ptr(),
                         ws=self.ws.data_ptr() + self.ws_off)

    def launch(self, C=None, **null):
        p = dict(self.ptrs, **{k: None for k in null})
        c = self.case
        rc = _lib().vilco_decode(p["logits"], p["offsets"], p["points"], p["row0"], p["lens"], c["C"] if C is None else C, self.L,
                                 self.topk, float(c["thresh"]), float(c["dur"]), p["segs"], p["scores"], p["labels"], p["total"],
                                 p["ws"], self.ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc

    def guards(self):
        for c in (self.c_segs, self.c_scores, self.c_labels):
            c()
        assert self.total[0].item() == -77 and self.total[2].item() == -79, "write next to out_total"
        w = self.ws.cpu()
        assert bool((w[:self.ws_off] == 0xA5).all()), "write in front of the workspace"
        assert bool((w[self.ws_off + self.nws:] == 0xA5).all()), "write past the end of the workspace"

    def untouched(self):
        """an error return writes nothing at all"""
        self.guards()
        assert bool(torch.isnan(self.segs).all()) and bool(torch.isnan(self.scores).all()) and bool((self.labels == POISON).all())
        assert self.total[1].item() == -78
        assert bool((self.ws == 0xA5).all())

    def result(self):
        """a successful call -> (segs [n, 2], scores [n], labels [n]) as numpy; rows >= n and all guards still hold"""
        self.guards()
        n = int(self.total[1].item())
        assert 0 <= n <= self.cap, n
        assert bool(torch.isnan(self.segs[2 * n:]).all()) and bool(torch.isnan(self.scores[n:]).all()), "write past out_total rows"
        assert bool((self.labels[n:] == POISON).all()), "label written past out_total rows"
        return self.segs[:2 * n].view(n, 2).cpu().numpy(), self.scores[:n].cpu().numpy(), self.labels[:n].cpu().numpy()


def run(dev, case, topk, **kw):
    c = Call(dev, case, topk, **kw)
    assert c.launch() == OK
    return c.result()


def held(name, dev, case, topk, **kw):
    """one call compared with the restatement; prints, then asserts the two figures"""
    out = run(dev, case, topk, **kw)
    fig = R.compare(case, topk, *out)
    print("%-34s topk %6d  count %6d  score %.3e (bar %.3e)  segment %.3f of its bound"
          % (name, topk, fig["count"], fig["score"], R.BAR_P, fig["seg"]))
    assert fig["score"] <= R.BAR_P, (name, fig)
    assert fig["seg"] <= 1.0, (name, fig)
    return out, fig


# ------------------------------------------------------------------------------------------------ chunk edges
@pytest.mark.parametrize("C,n", R.CHUNK_CASES)
def test_chunk_edges(dev, C, n):
    """single level, grid inputs without repetition, n on both sides of every multiple of 1024 up to 5 x 1024 + 1; without a
    cut (topk >= n) and with the cut at n // 3"""
    case = R.chunk_case(C, n)
    for topk in R.chunk_topks(n):
        held("chunk C %d n %d" % (C, n), dev, case, topk)


def test_cut_boundary(dev):
    """total candidates above the threshold, total < n = 4400: topk = 1, total - 1, total, total + 1, n + 5"""
    case, topks = R.cut_case()
    total = R.totals(case)[0]
    for topk in topks:
        _, fig = held("cut total %d" % total, dev, case, topk)
        assert fig["count"] == min(topk, total)


def test_ties_across_the_cut(dev):
    """the cut value stands at 40 places over threads 0 .. 879 of 14 waves; need_eq = 1, 20, 39, 40: exactly the lowest-index
    duplicates are admitted (compare asserts the labels in index order; the count here)"""
    case, places, topks = R.tie_case()
    for need, topk in zip(R.TIE_NEED, topks):
        (segs, scores, labels), fig = held("ties need_eq %d" % need, dev, case, topk)
        assert fig["count"] == topk
        assert places[0] == 0
        v = scores[0]                      # flat index 0 holds the cut value and is the first duplicate admitted
        assert int((scores == v).sum()) == need and int((scores < v).sum()) == 0


def test_all_equal(dev):
    """4400 logits of 0 (all 0.5): topk = 1500 admits flat indices 0 .. 1499; with thresh = 0.5 nothing is admitted"""
    case = R.zeros_case(R.THRESH)
    (segs, scores, labels), fig = held("all equal", dev, case, 1500)
    assert fig["count"] == 1500 and bool((scores == 0.5).all())
    assert np.array_equal(labels, np.arange(1500) % R.CUT_C)
    (segs, scores, labels), fig = held("all equal, thresh 0.5", dev, R.zeros_case(0.5), 1500)
    assert fig["count"] == 0


@pytest.mark.parametrize("topk", R.LOWBYTE_TOPK)
def test_low_byte_cut(dev, topk):
    """the cut falls between cluster values that share the top 24 bits of their probability"""
    _, fig = held("low byte", dev, R.lowbyte_case(), topk)
    assert fig["count"] == topk


@pytest.mark.parametrize("topk", R.SAT_TOPK)
def test_saturated_and_non_finite(dev, topk):
    """60 logits in {18, 20, 25, 30, +inf} (all 1.0f), 30 in {-100, -inf, NaN}, NaN offsets on rows of the first ties: topk
    below, at and above the number of ties; a NaN offset drops its candidate and keeps its slot"""
    case = R.saturated_case()
    (segs, scores, labels), fig = held("saturated", dev, case, topk)
    assert fig["count"] < topk
    assert topk > R.SAT_N_ONE or bool((scores == 1.0).all())


def test_duration_filter_after_the_cut(dev):
    """every other member of the top-1000 has zero offsets: 500 remain and nobody ranked below the cut moves up"""
    case, ranked = R.duration_case()
    (segs, scores, labels), fig = held("duration after cut", dev, case, R.DURCUT_TOPK)
    assert fig["count"] == R.DURCUT_TOPK // 2
    floor = R.sigmoid64(case["logits"].reshape(-1)[ranked[R.DURCUT_TOPK - 1]])
    assert float(scores.min()) >= floor * (1 - R.BAR_P), "a candidate ranked below the cut appears"


@pytest.mark.parametrize("topk", [700, 5000])
def test_length_equal_to_the_threshold_is_dropped(dev, topk):
    """t integer, offsets 0.25 / 0.25, stride 1, dur 0.5: right - left == dur exactly, not longer"""
    case = R.exact_duration_case()
    (segs, scores, labels), fig = held("length == dur", dev, case, topk)
    assert 0 < fig["count"] < topk and bool(((segs[:, 1] - segs[:, 0]) == 0.75).all())


# ------------------------------------------------------------------------------------------------ row layout
@pytest.mark.parametrize("topk", R.LAYOUT_TOPK)
def test_row_layout_with_gaps(dev, topk):
    """L = 6; gap rows and rows at or beyond level_len hold logit +30 and finite offsets: none may appear.  Levels 1 and 5
    are empty."""
    (segs, scores, labels), fig = held("layout", dev, R.layout_case(), topk)
    assert fig["count"] > 0 and float(scores.max()) < 0.999


def test_sixty_four_levels(dev):
    """L = 64, the limit of the concatenation's table; lengths cycle 0 .. 3"""
    (segs, scores, labels), fig = held("64 levels", dev, R.many_levels_case(), 5)
    assert fig["count"] > 0 and float(scores.max()) < 0.999


# ------------------------------------------------------------------------------------------------ ABI
def test_bad_arguments_write_nothing(dev):
    case = R.chunk_case(7, 1029)
    for L in (0, 65):
        c = Call(dev, case, 50)
        c.L = L
        rc = c.launch()
        print("%-12s -> %d" % ("L = %d" % L, rc))
        assert rc == BADARG
        c.untouched()
    c = Call(dev, case, 50)
    rc = c.launch(C=0)
    print("%-12s -> %d" % ("C = 0", rc))
    assert rc == BADARG
    c.untouched()
    c = Call(dev, case, 50)
    c.topk = 0
    rc = c.launch()
    print("%-12s -> %d" % ("topk = 0", rc))
    assert rc == BADARG
    c.untouched()
    for ptr in ("logits", "offsets", "points", "row0", "lens", "segs", "scores", "labels", "total"):
        c = Call(dev, case, 50)
        rc = c.launch(**{ptr: True})
        print("%-12s -> %d" % ("null " + ptr, rc))
        assert rc == BADARG
        c.untouched()
    lib = _lib()
    assert lib.vilco_decode_workspace(0, 5) == 0 and lib.vilco_decode_workspace(65, 5) == 0 and lib.vilco_decode_workspace(3, 0) == 0


def test_short_workspace_writes_nothing(dev):
    case = R.chunk_case(7, 1029)
    c = Call(dev, case, 50, short=1)
    rc = c.launch()
    print("one byte short -> %d" % rc)
    assert rc == ERR_WORKSPACE
    c.untouched()
    c = Call(dev, case, 50)
    rc = c.launch(ws=True)
    print("null workspace -> %d" % rc)
    assert rc == ERR_WORKSPACE
    c.untouched()


@pytest.mark.parametrize("which", ["layout", "ties"])
def test_unaligned_workspace(dev, which):
    """exactly vilco_decode_workspace bytes starting 4 past a 256-byte line: the same bits as from an aligned one, and not
    a byte outside the workspace"""
    case, topk = (R.layout_case(), 50) if which == "layout" else (R.tie_case()[0], R.TIE_ABOVE + 20)
    a = run(dev, case, topk)
    c = Call(dev, case, topk, misalign=4)
    assert c.ptrs["ws"] % 256 == 4
    assert c.launch() == OK
    b = c.result()
    fig = R.compare(case, topk, *b)
    print("unaligned workspace (%s): count %d, score %.3e" % (which, fig["count"], fig["score"]))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_repeatable(dev):
    """two calls on the cut-and-ties input: bit-equal outputs"""
    case, places, topks = R.tie_case()
    a, b = run(dev, case, topks[1]), run(dev, case, topks[1])
    print("repeat: %d candidates" % a[1].shape[0])
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ recipe shape
@pytest.mark.parametrize("clip_len", R.RECIPE_CLIPS)
def test_recipe_shape(dev, clip_len):
    """T = 2304, C = 110, six levels (level 0: 253 440 elements, per = 248), topk 5000, thresh 0.001, dur 0.05, grid with
    repetition (ties everywhere, at the cuts too); a full clip and one of 1500 rows whose tail rows hold logit +30"""
    case = R.recipe_case(clip_len)
    (segs, scores, labels), fig = held("recipe clip %d" % clip_len, dev, case, R.RECIPE_TOPK)
    assert fig["count"] == sum(min(t, R.RECIPE_TOPK) for t in R.totals(case)) and float(scores.max()) < 0.999


# ------------------------------------------------------------------------------------------------ through the model
def test_through_the_model_with_an_active_cut(dev, monkeypatch):
    """the `noxl` golden model in eval mode, test_pre_nms_topk lowered to half of what passes the threshold on level 0: the
    device decode and the tensor-expression path give the same detections after postprocessing"""
    from parity_util import build_hip_model, golden_inputs, load_golden
    gold = load_golden("noxl")
    model = build_hip_model(gold, dev)
    vl = golden_inputs(gold)[:1]
    with torch.no_grad():
        cls, off, masks = model(vl, is_training=False, get_emb=True)
    passing = int(((cls[0][0].float().sigmoid() * masks[0][0].unsqueeze(-1)) > model.test_pre_nms_thresh).sum())
    model.test_pre_nms_topk = max(1, passing // 2)
    print("level 0: %d of %d pass the threshold, topk %d" % (passing, cls[0][0].numel(), model.test_pre_nms_topk))
    assert passing > model.test_pre_nms_topk, "the cut is not active on level 0"
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("VILCO_DEVICE_DECODE", flag)
        with torch.no_grad():
            res[flag] = model(vl, is_training=False)[0]
    a, b = res["1"], res["0"]
    print("detections: %d (device decode), %d (tensor expressions)" % (a["scores"].shape[0], b["scores"].shape[0]))
    assert a["scores"].shape[0] == b["scores"].shape[0] > 0
    ds = float(((a["scores"] - b["scores"]).abs() / b["scores"].abs()).max())
    print("worst relative score difference %.3e" % ds)
    assert torch.equal(a["labels"], b["labels"])
    np.testing.assert_allclose(a["scores"].numpy(), b["scores"].numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(a["segments"].numpy(), b["segments"].numpy(), rtol=2e-5, atol=0)
