"""Shared builder of the ops.mq_loss parity tests (tests/test_loss_gpu.py, tests/test_loss_edges_gpu.py,
tests/test_loss_cases_cpu.py).  A plain module, not a conftest.

A `Case` describes one call: pyramid, clips, GT, seed, overrides.  Three views of it:

  expected(case)        CPU, float64: oracle.mq_oracle.losses + autograd -> losses, new normaliser, every gradient
  run_device(case, dev) what ops.mq_loss and its backward produce for the same numbers (float32 copies)
  audit(case)           CPU, float64, numbers only: how far every decision of the assignment and of the "al" maximum lies from
                        its threshold, so that a case can show that float32 takes the same decisions as float64 -- or sits on a
                        threshold exactly, where both do too

check(case, want, got) holds the assertions every case shares; CASES is the table of the edge cases."""
import dataclasses
from typing import Optional

import torch

from parity_util import rel_err

L = 6
GAUSS_KEYS = ('mu', 'sigma', 'mu_reg_left', 'sigma_reg_left', 'mu_reg_right', 'sigma_reg_right')
LOSS_KEYS = ('cls_loss', 'reg_loss', 'al_loss', 'final_loss')
INIT_NORM = 100.0


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    ncls: int
    Ts: tuple                          # length of every pyramid level (need not be powers of two)
    gts: tuple                         # per clip: (segments [[s0, s1], ...], labels [...]); ([], []) = a clip without GT
    lens: tuple                        # valid length of every clip at level 0
    gaps: bool = True                  # LevelCat layout: one separator row between levels
    radius: float = 1.5                # <= 0: center_sample = 'none'
    smoothing: float = 0.0
    seed: int = 0
    al: float = 0.2
    loss_weight: float = 1.0
    use_al: Optional[bool] = None      # None: ncls != 1 (what the model passes)
    scale: bool = True                 # False: level_scale=None, offsets arrive as non-negative predictions
    gw: tuple = (0.3, -0.2, 0.5, 1.0)  # upstream gradient of (cls, reg, al, final); None = that output carries none
    nmax: Optional[int] = None         # GT slots per clip in the device table (None: the largest count)
    logit_std: float = 2.0
    logit_mean: float = -2.0
    # overrides, applied in order after the seeded draw:
    #   ('logits', b, level, q, values[C])     ('logit_shift', b, c, delta): every row of clip b
    #   ('raw', b, level, q, (l, r)): the head's raw offsets     ('pred', b, level, q, (l, r)): raw = pred / level_scale
    edits: tuple = ()
    # audit: (kind, b, level, q, j) entries that must sit exactly on their threshold and decide the label there
    named: tuple = ()
    # (b, j) of GT deliberately off the 1/4 grid (the ...0005 near-ties): their distances need 1e-4, not 1e-2 -- float32 places a
    # bound near 25 within 2e-6 and the centre-sampling window within 4e-6, so 1e-4 still leaves a factor 25
    off_grid: tuple = ()
    loss_tol: float = 2e-5             # the bars of test_loss_gpu.py unless a case states a measured one
    grad_tol: float = 1e-4

    @property
    def al_on(self):
        return self.ncls != 1 if self.use_al is None else self.use_al


def _cfg(ncls, T, radius=1.5, smoothing=0.0, loss_weight=1.0, al=0.2):
    from vilco_amd.core.config import make_config
    return make_config(dataset=dict(input_dim=8, num_classes=ncls, max_seq_len=T),
                       model=dict(embd_dim=8, fpn_dim=8, head_dim=8, n_head=2, backbone_arch=(2, 2, 5), use_xl=False),
                       train_cfg=dict(init_loss_norm=100, loss_weight=loss_weight, al_loss_weight=al, label_smoothing=smoothing,
                                      center_sample='radius' if radius > 0 else 'none', center_sample_radius=max(radius, 0.1)))['model']


def point_index(case, level, q):
    """index of point q of `level` among the concatenated points (no separator rows)"""
    return sum(case.Ts[:level]) + q


def device_row(case, level, q):
    return point_index(case, level, q) + (level if case.gaps else 0)


def build(case):
    """the float64 numbers of a case, drawn from its seed in the order tests/test_loss_gpu.py always drew them"""
    from oracle import mq_oracle
    torch.manual_seed(case.seed)
    ncls, Ts, B = case.ncls, list(case.Ts), len(case.gts)
    cfg = _cfg(ncls, Ts[0], case.radius, case.smoothing, case.loss_weight, case.al)
    pts = mq_oracle.points(cfg, Ts, torch.float64)
    assert [p.shape[0] for p in pts] == Ts
    # per-level validity from the clip lengths (stride-2 pyramid: ceil)
    lvl_len = torch.tensor([[min(-(-ln // (1 << l)), Ts[l]) for l in range(L)] for ln in case.lens], dtype=torch.int32)
    masks = [(torch.arange(Ts[l])[None, :] < lvl_len[:, l:l + 1]).unsqueeze(1) for l in range(L)]
    logits = [case.logit_std * torch.randn(B, Ts[l], ncls, dtype=torch.float64) + case.logit_mean for l in range(L)]
    raw = [torch.randn(B, Ts[l], 2, dtype=torch.float64) * 3 for l in range(L)]
    scales = torch.rand(L, dtype=torch.float64) + 0.5
    p = {'mu': 0.2 * torch.randn(ncls, 1, dtype=torch.float64), 'sigma': 1 + 0.2 * torch.rand(ncls, 1, dtype=torch.float64),
         'mu_reg_left': -0.5 + 0.1 * torch.randn(ncls, 1, dtype=torch.float64), 'sigma_reg_left': 1 + 0.2 * torch.rand(ncls, 1, dtype=torch.float64),
         'mu_reg_right': 0.5 + 0.1 * torch.randn(ncls, 1, dtype=torch.float64), 'sigma_reg_right': 1 + 0.2 * torch.rand(ncls, 1, dtype=torch.float64)}
    if not case.scale:                 # the heads already applied relu(scale * raw): the offsets are the leaf
        raw = [torch.relu(r * scales[l]) for l, r in enumerate(raw)]
    for e in case.edits:
        if e[0] == 'logits':
            logits[e[2]][e[1], e[3]] = torch.tensor(e[4], dtype=torch.float64)
        elif e[0] == 'logit_shift':
            for t in logits:
                t[e[1], :, e[2]] += e[3]
        elif e[0] == 'raw':
            assert case.scale
            raw[e[2]][e[1], e[3]] = torch.tensor(e[4], dtype=torch.float64)
        elif e[0] == 'pred':
            v = torch.tensor(e[4], dtype=torch.float64)
            raw[e[2]][e[1], e[3]] = v / scales[e[2]] if case.scale else v
        else:
            raise ValueError(e[0])
    max_len = cfg['max_seq_len'] * cfg['max_buffer_len_factor']
    segs, labs = [], []
    for g in case.gts:
        if len(g[1]):
            segs.append(torch.tensor(g[0], dtype=torch.float64).reshape(-1, 2)); labs.append(torch.tensor(g[1], dtype=torch.long))
        else:                          # the oracle cannot label an empty list: one segment past every point matches none
            segs.append(torch.tensor([[max_len + 8.0, max_len + 16.0]], dtype=torch.float64)); labs.append(torch.tensor([0]))
    return dict(cfg=cfg, pts=pts, lvl_len=lvl_len, masks=masks, logits=logits, raw=raw, scales=scales, p=p, segs=segs, labs=labs)


_expected = {}


def expected(case, dtype=torch.float64):
    """oracle losses + autograd in `dtype` on the CPU (float64: the reference; float32: how far plain float32 arithmetic of the
    same expressions lands from it, the yardstick of a measured bar).  Cached: one evaluation per case, never modified."""
    key = (case.name, dtype)
    if key not in _expected:
        _expected[key] = _evaluate(case, dtype)
    return _expected[key]


def _evaluate(case, dtype):
    from oracle import mq_oracle
    d = build(case)
    logits = [t.to(dtype).requires_grad_(True) for t in d['logits']]
    raw = [t.to(dtype).requires_grad_(True) for t in d['raw']]
    scales = d['scales'].to(dtype).requires_grad_(True)
    p = {k: v.to(dtype).requires_grad_(True) for k, v in d['p'].items()}
    offs = [torch.relu(r * scales[l]) for l, r in enumerate(raw)] if case.scale else raw
    segs = [s.to(dtype) for s in d['segs']]
    want, want_norm = mq_oracle.losses(p, d['cfg'], d['masks'], logits, offs, segs, d['labs'], INIT_NORM)
    want, want_norm = {k: want[k].sum() for k in LOSS_KEYS}, float(want_norm)
    if not case.al_on:                 # the kernel is told to leave the "al" term out
        want['al_loss'] = torch.zeros((), dtype=dtype)
        want['final_loss'] = want['cls_loss'] + want['reg_loss'] * case.loss_weight
    total = sum(g * want[k] for g, k in zip(case.gw, LOSS_KEYS) if g is not None)
    total.backward()

    def grad(t):
        return t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(losses={k: float(v.detach()) for k, v in want.items()}, norm=want_norm, dlogits=[grad(t) for t in logits],
                doffsets=[grad(t) for t in raw], dscale=grad(scales) if case.scale else None,
                dgauss=torch.cat([grad(p[k]) for k in GAUSS_KEYS], dim=1).t())


def device_inputs(case, dev):
    """float32 device tensors of a case in the layout ops.mq_loss takes (LevelCat rows with separator rows when `gaps`)"""
    d = build(case)
    ncls, Ts, B = case.ncls, list(case.Ts), len(case.gts)
    rows_l, rows_o, tab_p, tab_l, tab_q = [], [], [], [], []
    for l in range(L):
        if l and case.gaps:
            rows_l.append(torch.zeros(B, 1, ncls, dtype=torch.float64)); rows_o.append(torch.zeros(B, 1, 2, dtype=torch.float64))
            tab_p.append(torch.zeros(1, 4, dtype=torch.float64)); tab_l.append(l); tab_q.append(1 << 30)
        rows_l.append(d['logits'][l]); rows_o.append(d['raw'][l]); tab_p.append(d['pts'][l])
        tab_l += [l] * Ts[l]; tab_q += list(range(Ts[l]))
    lg = torch.cat(rows_l, 1).float().to(dev).requires_grad_(True)
    of = torch.cat(rows_o, 1).float().to(dev).requires_grad_(True)
    sc = d['scales'].float().to(dev).requires_grad_(True) if case.scale else None
    gauss = torch.cat([d['p'][k] for k in GAUSS_KEYS], dim=1).t().contiguous().float().to(dev).requires_grad_(True)
    tables = (torch.cat(tab_p).float().contiguous().to(dev), torch.tensor(tab_l, dtype=torch.int32, device=dev),
              torch.tensor(tab_q, dtype=torch.int32, device=dev))
    counts = [len(g[1]) for g in case.gts]
    nmax = max(counts) if case.nmax is None else case.nmax
    assert nmax >= max(counts)
    gt = torch.zeros(B, 3 * nmax + 1)
    for b, g in enumerate(case.gts):
        n = counts[b]
        if n:
            gt[b, :2 * n] = torch.tensor(g[0], dtype=torch.float32).reshape(-1)
            gt[b, 2 * nmax:2 * nmax + n] = torch.tensor(g[1], dtype=torch.float32)
        gt[b, 3 * nmax] = n
    return dict(lg=lg, of=of, sc=sc, gauss=gauss, tables=tables, lvl_len=d['lvl_len'].to(dev), gt=gt.to(dev))


def call(case, x, norm):
    from vilco_amd import ops
    return ops.mq_loss(x['lg'], x['of'], x['sc'], x['gauss'], x['tables'], x['lvl_len'], x['gt'], norm, case.radius, case.smoothing,
                       0.9, case.loss_weight, case.al, case.al_on)


def run_device(case, dev):
    """ops.mq_loss forward + backward; the gradients come back per level, separator rows split off"""
    from vilco_amd import ops
    x = device_inputs(case, dev)
    norm = torch.full((1,), INIT_NORM, device=dev)
    got = call(case, x, norm)
    sum(g * got[i] for i, g in enumerate(case.gw) if g is not None).backward()
    Ts, B = list(case.Ts), len(case.gts)

    def uncat(t):
        out, sep, o = [], 0.0, 0
        for l in range(L):
            if l and case.gaps:
                sep = max(sep, float(t[:, o].abs().max()))
                o += 1
            out.append(t[:, o:o + Ts[l]].detach().cpu())
            o += Ts[l]
        return out, sep
    dlogits, sep_l = uncat(x['lg'].grad)
    doffsets, sep_o = uncat(x['of'].grad)
    # the packed-maximum workspace is left clean: a second call gives the same value
    x2 = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in x.items()}
    again = call(case, x2, torch.full((1,), INIT_NORM, device=dev))
    state = ops._almax_state[(dev.index, B * case.ncls)]
    return dict(losses={k: float(got[i]) for i, k in enumerate(LOSS_KEYS)}, norm=float(norm), dlogits=dlogits, doffsets=doffsets,
                dscale=x['sc'].grad.detach().cpu() if case.scale else None, dgauss=x['gauss'].grad.detach().cpu(),
                separator=max(sep_l, sep_o), final_again=float(again[3]), almax_clean=bool((state == 0).all()))


def check(case, want, got):
    assert abs(got['norm'] - want['norm']) <= 1e-5 * want['norm']
    for k in LOSS_KEYS:
        w, g = want['losses'][k], got['losses'][k]
        assert abs(g - w) <= case.loss_tol * max(abs(w), 1e-3), (k, g, w)
    assert got['separator'] == 0.0                                   # separator rows get zero gradient
    for l, (a, b_) in enumerate(zip(got['dlogits'], want['dlogits'])):
        assert rel_err(a, b_, 1e-9) < case.grad_tol, ("dlogits", l, rel_err(a, b_, 1e-9))
    for l, (a, b_) in enumerate(zip(got['doffsets'], want['doffsets'])):
        assert rel_err(a, b_, 1e-9) < case.grad_tol, ("doffsets", l, rel_err(a, b_, 1e-9))
    if case.scale:
        assert rel_err(got['dscale'], want['dscale'], 1e-9) < case.grad_tol, ("dscale", rel_err(got['dscale'], want['dscale'], 1e-9))
    assert rel_err(got['dgauss'], want['dgauss'], 1e-9) < case.grad_tol, ("dgauss", rel_err(got['dgauss'], want['dgauss'], 1e-9))
    assert got['final_again'] == got['losses']['final_loss']
    assert got['almax_clean']                                        # the cached packed-maximum state went back to zero


def _case(dev, ncls, T, gts, lens, gaps, radius=1.5, smoothing=0.0, seed=0, al=0.2, loss_weight=1.0):
    """the call tests/test_loss_gpu.py has always made: power-of-two pyramid, level_scale given, all four outputs carry gradient"""
    case = Case('legacy/%d/%d/%d/%s' % (ncls, T, seed, gaps), ncls, tuple(T >> l for l in range(L)), tuple(gts), tuple(lens), gaps,
                radius, smoothing, seed, al, loss_weight)
    check(case, _evaluate(case, torch.float64), run_device(case, dev))


# ------------------------------------------------------------------------------------------------------------------- audit
def audit(case):
    """Signed float64 distance of every decision from its threshold.

    per clip with GT, as [points, GT] lists (points concatenated level after level, no separator rows):
      inside   min(lo, hi) with centre sampling, min(left, right) without        (positive: inside)
      far_lo   far - range_lo                                                   (>= 0: in range)
      far_hi   range_hi - far                                                   (>= 0: in range)
      len      len - (min_len + 1e-3) for the GT that match the point, nan otherwise   (<= 0: in the multi-hot target)
    per (clip, class), over the rows of the clip with masked rows at the uniform score 1/C as the loss has them:
      al_best, al_second  the two largest scores among distinct rows;  al_gap = (best - second) / best
      al_row              the first row holding the best;  al_row_valid = 0 when that row is masked"""
    d = build(case)
    pts = torch.cat(d['pts'])
    t, lo_r, hi_r, stride = (pts[:, i, None] for i in range(4))
    out = dict(inside=[], far_lo=[], far_hi=[], len=[])
    for g, seg in zip(case.gts, d['segs']):
        if not len(g[1]):
            for k in out:
                out[k].append(None)
            continue
        s0, s1 = seg[None, :, 0], seg[None, :, 1]
        left, right = t - s0, s1 - t
        if case.radius > 0:
            ctr = 0.5 * (s0 + s1)
            ins = torch.minimum(t - torch.maximum(ctr - stride * case.radius, s0), torch.minimum(ctr + stride * case.radius, s1) - t)
        else:
            ins = torch.minimum(left, right)
        far = torch.maximum(left, right)
        ok = (ins > 0) & (far >= lo_r) & (far <= hi_r)
        lens = (s1 - s0).expand_as(far).masked_fill(~ok, float('inf'))
        min_len = lens.min(dim=1, keepdim=True)[0]
        dist = lens - (min_len + 1e-3)
        dist[~ok] = float('nan')
        out['inside'].append(ins.tolist()); out['far_lo'].append((far - lo_r).tolist()); out['far_hi'].append((hi_r - far).tolist())
        out['len'].append(dist.tolist())
    valid = torch.cat([m.squeeze(1) for m in d['masks']], dim=1)
    sc = torch.cat(d['logits'], dim=1).masked_fill(~valid.unsqueeze(-1), -1e7).softmax(-1)           # [B, P, C]
    top = sc.topk(min(2, sc.shape[1]), dim=1)[0]
    best, second = top[:, 0], top[:, -1]
    idx = torch.arange(sc.shape[1])[None, :, None].expand_as(sc)
    row = idx.masked_fill(sc != best[:, None, :], sc.shape[1]).min(dim=1)[0]                          # first row holding the maximum
    out.update(al_best=best.tolist(), al_second=second.tolist(), al_gap=((best - second) / best).tolist(), al_row=row.tolist(),
               al_row_valid=torch.gather(valid, 1, row).to(torch.int64).tolist(), valid=valid.to(torch.int64).tolist())
    return out


# ------------------------------------------------------------------------------------------------------------------- table
def _pow2(T):
    return tuple(T >> l for l in range(L))


def _spread(labels, shift=0.0):
    """one GT per label, 8 apart, lengths cycling through four values: every bound a multiple of 1/4"""
    widths = (3.0, 5.5, 7.0, 12.25)
    return ([[8.0 * i + 2.0 + shift, 8.0 * i + 2.0 + shift + widths[i % 4]] for i in range(len(labels))], list(labels))


def _seeded_gts(seed, B, T, ncls):
    """one or two GT per clip from the seed, bounds on multiples of 1/4 inside [0, T)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        n = int(torch.randint(1, 3, (1,), generator=g))
        segs = []
        for _ in range(n):
            s0 = int(torch.randint(0, 4 * (T - 130), (1,), generator=g)) / 4.0
            segs.append([s0, s0 + int(torch.randint(4, 4 * 128, (1,), generator=g)) / 4.0])
        out.append((segs, [int(v) for v in torch.randint(0, ncls, (n,), generator=g)]))
    return tuple(out)


def _class_case(C, seed):
    """GT labels on C-1 and on each side of every 32-bit word boundary of the kernel's class bitset"""
    labs = sorted({c for c in (0, 31, 32, 63, 64, 95, 96, 127, C - 1) if c < C})
    std, mean = (0.5, 0.0) if C <= 2 else (2.0, -2.0)      # two classes: a spread of 2 would saturate the best softmax score
    return Case('classes_%d' % C, C, _pow2(64), (_spread(labs), _spread(labs[::-1], 1.25)), (64, 51), seed=seed, logit_std=std,
                logit_mean=mean)


# four classes: a logit spread of 2 would push the best softmax score of a clip past 1 - 1e-2
_C4 = dict(logit_std=0.7, logit_mean=-1.0)

# GT of the threshold cases: integers, so that points (integers too) land on the bounds exactly.
#   clip 0  [8, 16]  ctr 12: far == 4 at t = 12 is the upper bound of level 0 and the lower bound of level 1: the same GT labels
#                    both; at level 2 (stride 4) the window is the segment itself: t = 8 has left == 0, t = 16 has right == 0
#   clip 1  [9, 17]  ctr 13, level 1 (stride 2, radius 1.5 -> 3): t = 10 and t = 16 sit on ctr -/+ 1.5 stride, t = 12, 14 inside
#   clip 2  [4, 14]  without centre sampling t = 12 has far == 8: upper bound of level 1, lower bound of level 2
_EDGE_GTS = (([[8.0, 16.0]], [0]), ([[9.0, 17.0]], [1]), ([[4.0, 14.0]], [2]))
_EDGE_RADIUS = (('far_hi', 0, 0, 12, 0), ('far_lo', 0, 1, 6, 0), ('inside', 0, 2, 2, 0), ('inside', 0, 2, 4, 0),
                ('inside', 1, 1, 5, 0), ('inside', 1, 1, 8, 0))
_EDGE_NONE = (('far_hi', 0, 0, 12, 0), ('far_lo', 0, 1, 6, 0), ('inside', 0, 2, 2, 0), ('inside', 0, 2, 4, 0),
              ('far_hi', 2, 1, 6, 0), ('far_lo', 2, 2, 3, 0))


def _live_offsets(named):
    """positive predictions on the named rows: a row labelled positive there has a non-zero offsets gradient"""
    return tuple(('pred', b, level, q, (1.5, 2.5)) for _, b, level, q, _ in named)


# a row of C = 10 logits whose class-`c` score is 0.943: above every seeded row, below the 1 - 1e-2 the al term needs
def _TOP(c):
    return tuple(3.0 if i == c else -2.0 for i in range(10))


_SAT = (('logits', 0, 1, 5, (100.0, -100.0, 30.0, -30.0)),        # rows positive for class 1 (GT [8, 16]: level 1 q 5..7, level 0 q 12)
        ('logits', 0, 1, 6, (17.0, -17.0, 0.0, 30.0)),
        ('logits', 0, 1, 7, (-100.0, 100.0, -17.0, 0.0)),
        ('logits', 0, 0, 12, (-30.0, 100.0, -17.0, 17.0)),
        ('logits', 0, 0, 0, (100.0, -100.0, 30.0, -30.0)),        # negative rows
        ('logits', 0, 0, 1, (17.0, -17.0, 0.0, -100.0)),
        ('logits', 0, 2, 1, (-30.0, 17.0, 100.0, 0.0)),
        ('logits', 0, 0, 50, (100.0, -100.0, 17.0, -17.0)),       # masked row (clip length 40)
        ('logits', 1, 0, 3, (0.0, 100.0, -100.0, 30.0)),          # clip 1, GT class 2 at [30, 36]: a negative row, two positive rows
        ('logits', 1, 1, 16, (30.0, -30.0, 100.0, -100.0)),
        ('logits', 1, 1, 17, (-17.0, 17.0, -100.0, 100.0)))
_SAT_GTS = (([[8.0, 16.0]], [1]), ([[30.0, 36.0]], [2]))

# positive rows of GT [8, 16] (targets in strides): level 1 q 5, 6, 7 -> (1, 3), (2, 2), (3, 1); level 0 q 12 -> (4, 4)
_DIOU_GTS = (([[8.0, 16.0]], [1]), ([[20.0, 41.5]], [3]))

CASES = [
    # ---- strided loops of loss_finish_kernel
    Case('finish_BC_330', 110, _pow2(64), (_spread((109, 64, 33, 0)), _spread((5, 31, 32), 0.5), _spread((63, 96, 108), 2.25)),
         (64, 64, 40), seed=11),
    # 65 clips x 4 workgroups = 260 partial sums; C = 2 (logit spread 0.5, see _class_case).  The float32 oracle lies 7e-8 (losses) and
    # 5e-7 (gradients) from the float64 one: the bars of test_loss_gpu.py hold as they are
    Case('finish_nparts_260', 2, (512, 256, 128, 64, 32, 16), _seeded_gts(21, 65, 512, 2), tuple(512 - 7 * (b % 9) for b in range(65)),
         seed=21, logit_std=0.5, logit_mean=0.0),
    # ---- row counts around one workgroup
    Case('rows_256', 10, (127, 64, 32, 16, 8, 4), (_spread((1, 5, 9, 0, 3)), _spread((2, 2, 7), 3.5)), (127, 90), seed=31),
    Case('rows_257', 10, _pow2(128), (_spread((1, 5, 9, 0, 3)), _spread((2, 2, 7), 3.5)), (128, 90), seed=34),
    Case('rows_131', 10, _pow2(64), (_spread((1, 5, 9, 0, 3)), _spread((2, 2, 7), 3.5)), (64, 45), seed=35),
    # ---- class counts at the bitset word boundaries
    Case('classes_1', 1, _pow2(64), (_spread((0, 0, 0)), _spread((0,), 1.25)), (64, 51), seed=40, use_al=False),
    _class_case(2, 41), _class_case(32, 42), _class_case(33, 43), _class_case(64, 44), _class_case(65, 45), _class_case(128, 46),
    # ---- thresholds
    Case('thresholds_radius', 4, _pow2(64), _EDGE_GTS, (64, 64, 64), seed=50, **_C4,
         named=_EDGE_RADIUS, edits=_live_offsets(_EDGE_RADIUS)),
    Case('thresholds_none', 4, _pow2(64), _EDGE_GTS, (64, 64, 64), radius=0.0, seed=51, **_C4,
         named=_EDGE_NONE, edits=_live_offsets(_EDGE_NONE)),
    # ---- near-ties of the GT length.  clip 0: the shorter GT is listed second, `best` is 1 (class 3) and both bits are set;
    # clip 1: three GT of one length, two classes: the first wins, the doubled class clamps at 1; clip 2: 0.25 apart, no tie
    Case('near_ties', 10, _pow2(64), (([[5.0, 25.0005], [5.0, 25.0]], [7, 3]),
                                      ([[10.0, 30.0], [11.0, 31.0], [10.0, 30.0]], [2, 5, 2]),
                                      ([[40.0, 60.0], [40.0, 60.25]], [1, 4])), (64, 64, 64), seed=60, off_grid=((0, 0),)),
    # ---- "al" maximum ties: rows (level 0, q 10) and (level 0, q 200) share a workgroup; (level 0, q 10) and (level 1, q 9) are
    # device rows 10 and 266: they meet only in the global atomicMax.  torch.max sends the gradient to the first.
    Case('al_tie_one_workgroup', 10, _pow2(256), (_spread((1, 5, 9, 0, 3)), _spread((2, 2, 7), 3.5)), (256, 239), seed=70,
         edits=(('logits', 0, 0, 10, _TOP(6)), ('logits', 0, 0, 200, _TOP(6)), ('logits', 1, 0, 10, _TOP(2)), ('logits', 1, 0, 200, _TOP(2)))),
    Case('al_tie_two_workgroups', 10, _pow2(256), (_spread((1, 5, 9, 0, 3)), _spread((2, 2, 7), 3.5)), (256, 239), seed=70,
         edits=(('logits', 0, 0, 10, _TOP(6)), ('logits', 0, 1, 9, _TOP(6)), ('logits', 1, 0, 10, _TOP(2)), ('logits', 1, 1, 9, _TOP(2)))),
    # ---- clip 1 is valid for 21 of 64 points and class 4 is pushed below the uniform 1/C on every valid row: a masked row wins
    Case('masked_winner', 10, _pow2(64), (_spread((1, 5, 9)), _spread((4, 2), 1.0)), (64, 21), seed=80, edits=(('logit_shift', 1, 4, -12.0),)),
    # ---- level_scale = None; which outputs carry gradient
    Case('no_level_scale', 10, _pow2(64), (_spread((1, 5, 9, 0, 3)), _spread((2, 2, 7), 3.5)), (64, 45), seed=90, scale=False),
    Case('grad_final_only', 10, _pow2(64), (_spread((1, 5, 9, 0, 3)), _spread((2, 2, 7), 3.5)), (64, 45), seed=91, gw=(None, None, None, 1.0)),
    Case('grad_reg_only', 10, _pow2(64), (_spread((1, 5, 9, 0, 3)), _spread((2, 2, 7), 3.5)), (64, 45), seed=92, gw=(None, 1.0, None, None)),
    # ---- saturated logits (use_al = False: the scores of such rows are 0 or 1).  float32 oracle vs float64: 1.3e-7 (losses), 1.2e-6
    # (gradients): the bars of test_loss_gpu.py hold as they are
    Case('saturation_smooth_0', 4, _pow2(64), _SAT_GTS, (40, 64), seed=100, use_al=False, edits=_SAT),
    Case('saturation_smooth_0.1', 4, _pow2(64), _SAT_GTS, (40, 64), seed=100, use_al=False, smoothing=0.1, edits=_SAT),
    # ---- DIoU corners: prediction (0, 0) behind the relu, predictions of 1e4, one of each
    Case('diou_zero_and_huge', 4, _pow2(64), _DIOU_GTS, (64, 64), seed=110, **_C4,
         edits=(('raw', 0, 1, 5, (-1.0, -2.5)), ('pred', 0, 1, 6, (1e4, 1e4)), ('raw', 0, 1, 7, (-0.5, 1e4)), ('pred', 0, 0, 12, (1e4, 0.25)))),
    # prediction == target (float32-exact: integers over a power-of-two stride): both sides, left only, right only, both
    Case('diou_tie', 4, _pow2(64), _DIOU_GTS, (64, 64), seed=111, scale=False, **_C4,
         edits=(('pred', 0, 1, 6, (2.0, 2.0)), ('pred', 0, 1, 5, (1.0, 2.5)), ('pred', 0, 1, 7, (3.5, 1.0)), ('pred', 0, 0, 12, (4.0, 4.0)))),
    # ---- a clip without GT, table padded to 4 slots.  The oracle labels that clip with one segment past every point (build()); the
    # al term is left out (use_al = False) and only cls_loss and reg_loss carry gradient.
    Case('empty_clip', 5, _pow2(64), (_spread((1, 4)), ([], []), _spread((0, 2, 3), 2.5)), (64, 64, 30), seed=120, use_al=False,
         gw=(0.3, -0.2, None, None), nmax=4),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# audit(case): entries exactly on the ('inside', 'far_lo', 'far_hi') thresholds, counted once from the float64 audit: a case whose
# GT or pyramid drifts cannot lose its on-threshold points unnoticed (tests/test_loss_cases_cpu.py)
ON_EDGE = {
    'finish_BC_330': (10, 6, 12),
    'finish_nparts_260': (46, 4, 12),
    'rows_256': (11, 4, 13),
    'rows_257': (11, 4, 13),
    'rows_131': (11, 4, 13),
    'classes_1': (6, 3, 8),
    'classes_2': (4, 2, 5),
    'classes_32': (4, 2, 5),
    'classes_33': (6, 3, 8),
    'classes_64': (6, 3, 9),
    'classes_65': (9, 4, 12),
    'classes_128': (12, 6, 17),
    'thresholds_radius': (10, 6, 10),
    'thresholds_none': (16, 6, 10),
    'near_ties': (8, 2, 3),
    'al_tie_one_workgroup': (11, 4, 13),
    'al_tie_two_workgroups': (11, 4, 13),
    'masked_winner': (9, 4, 11),
    'no_level_scale': (11, 4, 13),
    'grad_final_only': (11, 4, 13),
    'grad_reg_only': (11, 4, 13),
    'saturation_smooth_0': (8, 8, 11),
    'saturation_smooth_0.1': (8, 8, 11),
    'diou_zero_and_huge': (5, 5, 7),
    'diou_tie': (5, 5, 7),
    'empty_clip': (5, 3, 7),
}
