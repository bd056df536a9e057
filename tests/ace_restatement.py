"""The ER-ACE windowed MQ loss (vilco_amd/cl_methods/ace.py, ops.mq_loss_ace, PtTransformer.losses' 'er_ace' branch) restated in
float64 with the plain tensor ops of the CPU path: oracle.mq_oracle's label assignment, focal map times a column mask, -inf on
the masked columns before the al softmax, the masked al sum.  A plain module, not a conftest; shares the `Case` of
tests/loss_cases.py and its three views, for any number of pyramid levels:

  expected(case, cls_lo)              CPU, float64 + autograd -> losses, new normaliser, every gradient, the al scores
  run_device(case, dev, cls_lo, ...)  what ops.mq_loss_ace (or ops.mq_loss) and its backward produce for the same numbers
  loss_cases.check(case, want, got)   the assertions and tolerances every case shares

cls_lo: one int per clip; a value outside [0, C) means 0, as in the kernels."""
import torch

import loss_cases as LC
from oracle import mq_oracle as O

LOSS_KEYS, GAUSS_KEYS, INIT_NORM = LC.LOSS_KEYS, LC.GAUSS_KEYS, LC.INIT_NORM


def windows(cls_lo, B, C):
    lo = [int(v) for v in (cls_lo if cls_lo is not None else [0] * B)]
    assert len(lo) == B
    return [v if 0 <= v < C else 0 for v in lo]


def column_mask(cls_lo, B, C):
    """bool [B, C]: the columns clip b's classification terms visit"""
    return torch.arange(C)[None, :] >= torch.tensor(windows(cls_lo, B, C))[:, None]


def losses(p, cfg, masks, cls_logits, offsets, segments, labels, al_labels, loss_normalizer, cls_lo, al_on=True):
    """oracle.mq_oracle.losses under the window.  labels: what the points are assigned with (a clip without GT: one segment
    past every point); al_labels: the classes of the clip's GT as the al term sees them (a clip without GT: none).
    -> (dict of the four losses, new normaliser, al score [B, C] with 0 outside the windows)"""
    tc = cfg['train_cfg']
    pts = torch.cat(O.points(cfg, [c.shape[1] for c in cls_logits], cls_logits[0].dtype), dim=0)
    lab = [O.label_points_single(p, cfg, pts, s, l) for s, l in zip(segments, labels)]
    gt_cls = torch.stack([x[0] for x in lab])
    gt_off = torch.stack([x[1] for x in lab])
    w_cls, w_l, w_r = (torch.stack([x[i] for x in lab]) for i in (2, 3, 4))
    valid = torch.cat([m.squeeze(1) for m in masks], dim=1)
    pos = torch.logical_and(gt_cls.sum(-1) > 0, valid)            # a GT class below the window still makes the row positive
    num_pos = int(pos.sum().item())
    loss_normalizer = 0.9 * loss_normalizer + 0.1 * max(num_pos, 1)
    logits = torch.cat(cls_logits, dim=1)
    B, _, C = logits.shape
    cols = column_mask(cls_lo, B, C)                              # [B, C]
    ls = tc['label_smoothing']
    target = gt_cls * (1 - ls) + ls / (cfg['num_classes'] + 1)
    w_cls = torch.where(pos, w_cls, torch.ones_like(w_cls))
    focal = O.sigmoid_focal(logits, target) * cols[:, None, :].to(logits.dtype)
    cls_loss = (focal.sum(-1) * w_cls * valid.to(logits.dtype)).sum() / loss_normalizer
    score = torch.zeros(B, C, dtype=logits.dtype)
    if al_on:
        sc = logits.masked_fill(valid.unsqueeze(-1) == False, -1e7)     # noqa: E712
        sc = sc.masked_fill(~cols[:, None, :], float('-inf'))
        sc = torch.max(sc.softmax(-1), dim=1)[0]
        inv = torch.zeros_like(sc)
        for i, l in enumerate(al_labels):
            inv[i, list(l)] = 1
        score = torch.where(cols, sc, torch.zeros_like(sc))
        # one logarithm per (clip, class), of the score or of its complement -- the kernels' select: a window of one class
        # scores exactly 1, and 0 * log(0) must not enter.  Columns below the window take 1 and add -log(1) = 0.
        q = torch.where(inv > 0, sc, 1 - sc)
        al_loss = -torch.where(cols, q, torch.ones_like(q)).log().sum() / loss_normalizer
    else:
        al_loss = torch.zeros((), dtype=logits.dtype)
    pred = torch.cat(offsets, dim=1)[pos]
    if num_pos == 0:
        reg_loss = 0 * pred.sum()
    else:
        reg_loss = (O.diou_1d(pred, gt_off[pos]) * ((w_l[pos] + w_r[pos]) / 2.0) * w_cls[pos]).sum() / loss_normalizer
    final = cls_loss + reg_loss * tc['loss_weight'] + al_loss * tc['al_loss_weight']
    return {'cls_loss': cls_loss, 'reg_loss': reg_loss, 'al_loss': al_loss, 'final_loss': final}, loss_normalizer, score.detach()


# ------------------------------------------------------------------------------------------------- cases of any pyramid depth
def _cfg(case):
    from vilco_amd.core.config import make_config
    L = len(case.Ts)
    rr = [(0, 4), (4, 8), (8, 16), (16, 32), (32, 64), (64, 10000)][:L]
    rr[-1] = (rr[-1][0], 10000)
    return make_config(dataset=dict(input_dim=8, num_classes=case.ncls, max_seq_len=case.Ts[0]),
                       model=dict(embd_dim=8, fpn_dim=8, head_dim=8, n_head=2, backbone_arch=(2, 2, L - 1), use_xl=False,
                                  regression_range=rr),
                       train_cfg=dict(init_loss_norm=100, loss_weight=case.loss_weight, al_loss_weight=case.al,
                                      label_smoothing=case.smoothing, center_sample='radius' if case.radius > 0 else 'none',
                                      center_sample_radius=max(case.radius, 0.1)))['model']


def build(case):
    """loss_cases.build for a pyramid of len(case.Ts) levels (six levels: that function itself, the same numbers)"""
    L = len(case.Ts)
    if L == LC.L:
        return LC.build(case)
    torch.manual_seed(case.seed)
    ncls, Ts, B = case.ncls, list(case.Ts), len(case.gts)
    cfg = _cfg(case)
    pts = O.points(cfg, Ts, torch.float64)
    assert [p.shape[0] for p in pts] == Ts
    lvl_len = torch.tensor([[min(-(-ln // (1 << l)), Ts[l]) for l in range(L)] for ln in case.lens], dtype=torch.int32)
    masks = [(torch.arange(Ts[l])[None, :] < lvl_len[:, l:l + 1]).unsqueeze(1) for l in range(L)]
    logits = [case.logit_std * torch.randn(B, Ts[l], ncls, dtype=torch.float64) + case.logit_mean for l in range(L)]
    raw = [torch.randn(B, Ts[l], 2, dtype=torch.float64) * 3 for l in range(L)]
    scales = torch.rand(L, dtype=torch.float64) + 0.5

    def rn(mean, std=0.1):
        return mean + std * torch.randn(ncls, 1, dtype=torch.float64)

    def sg():
        return 1 + 0.2 * torch.rand(ncls, 1, dtype=torch.float64)
    p = {'mu': rn(0.0, 0.2), 'sigma': sg(), 'mu_reg_left': rn(-0.5), 'sigma_reg_left': sg(), 'mu_reg_right': rn(0.5),
         'sigma_reg_right': sg()}
    if not case.scale:
        raw = [torch.relu(r * scales[l]) for l, r in enumerate(raw)]
    for e in case.edits:
        if e[0] == 'logits':
            logits[e[2]][e[1], e[3]] = torch.tensor(e[4], dtype=torch.float64)
        elif e[0] == 'logit_shift':
            for t in logits:
                t[e[1], :, e[2]] += e[3]
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
        else:
            segs.append(torch.tensor([[max_len + 8.0, max_len + 16.0]], dtype=torch.float64)); labs.append(torch.tensor([0]))
    return dict(cfg=cfg, pts=pts, lvl_len=lvl_len, masks=masks, logits=logits, raw=raw, scales=scales, p=p, segs=segs, labs=labs)


_expected = {}


def expected(case, cls_lo=None):
    """the restatement + autograd in float64.  Cached per (case, windows): one evaluation, never modified."""
    lo = tuple(windows(cls_lo, len(case.gts), case.ncls))
    key = (case.name, lo)
    if key not in _expected:
        _expected[key] = _evaluate(case, lo)
    return _expected[key]


def _evaluate(case, lo, dtype=torch.float64):
    d = build(case)
    logits = [t.to(dtype).requires_grad_(True) for t in d['logits']]
    raw = [t.to(dtype).requires_grad_(True) for t in d['raw']]
    scales = d['scales'].to(dtype).requires_grad_(True)
    p = {k: v.to(dtype).requires_grad_(True) for k, v in d['p'].items()}
    offs = [torch.relu(r * scales[l]) for l, r in enumerate(raw)] if case.scale else raw
    segs = [s.to(dtype) for s in d['segs']]
    want, want_norm, score = losses(p, d['cfg'], d['masks'], logits, offs, segs, d['labs'], [g[1] for g in case.gts], INIT_NORM,
                                    lo, al_on=case.al_on)
    want, want_norm = {k: want[k].sum() for k in LOSS_KEYS}, float(want_norm)
    total = sum(g * want[k] for g, k in zip(case.gw, LOSS_KEYS) if g is not None)
    total.backward()

    def grad(t):
        return t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(losses={k: float(v.detach()) for k, v in want.items()}, norm=want_norm, dlogits=[grad(t) for t in logits],
                doffsets=[grad(t) for t in raw], dscale=grad(scales) if case.scale else None,
                dgauss=torch.cat([grad(p[k]) for k in GAUSS_KEYS], dim=1).t(), al_score=score, lo=lo)


# ------------------------------------------------------------------------------------------------- the device view
def device_inputs(case, dev):
    """loss_cases.device_inputs for a pyramid of len(case.Ts) levels"""
    d = build(case)
    ncls, Ts, B, L = case.ncls, list(case.Ts), len(case.gts), len(case.Ts)
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


def call(case, x, norm, cls_lo=None):
    """ops.mq_loss_ace over the device table `cls_lo`, or ops.mq_loss when it is None"""
    from vilco_amd import ops
    args = (x['lg'], x['of'], x['sc'], x['gauss'], x['tables'], x['lvl_len'], x['gt'], norm, case.radius, case.smoothing, 0.9,
            case.loss_weight, case.al, case.al_on)
    return ops.mq_loss(*args) if cls_lo is None else ops.mq_loss_ace(*args, cls_lo)


def run_device(case, dev, cls_lo=None, plain=False):
    """forward + backward on the device -> the dictionary loss_cases.check takes, plus the raw tensors ('raw': the four
    outputs, saved normaliser = loss_norm after the call, the four gradients as the op returned them).  cls_lo: ints per clip
    (uploaded as they are, out-of-range values included); plain=True calls ops.mq_loss instead."""
    from vilco_amd import ops
    x = device_inputs(case, dev)
    B, L, Ts = len(case.gts), len(case.Ts), list(case.Ts)
    tab = None if plain else torch.tensor([int(v) for v in (cls_lo if cls_lo is not None else [0] * B)], dtype=torch.int32, device=dev)
    norm = torch.full((1,), INIT_NORM, device=dev)
    got = call(case, x, norm, tab)
    sum(g * got[i] for i, g in enumerate(case.gw) if g is not None).backward()

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
    x2 = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in x.items()}
    again = call(case, x2, torch.full((1,), INIT_NORM, device=dev), tab)
    state = ops._almax_state[(dev.index, B * case.ncls)]
    raw = dict(out=torch.stack([g.detach() for g in got]).cpu(), norm=norm.detach().cpu(), dlogits=x['lg'].grad.detach().cpu(),
               doffsets=x['of'].grad.detach().cpu(), dscale=x['sc'].grad.detach().cpu() if case.scale else None,
               dgauss=x['gauss'].grad.detach().cpu())
    return dict(losses={k: float(got[i]) for i, k in enumerate(LOSS_KEYS)}, norm=float(norm), dlogits=dlogits, doffsets=doffsets,
                dscale=raw['dscale'], dgauss=raw['dgauss'], separator=max(sep_l, sep_o), final_again=float(again[3]),
                almax_clean=bool((state == 0).all()), raw=raw)


def raw_equal(a, b):
    """every tensor of two run_device(...)['raw'] dictionaries holds the same bits"""
    assert set(a) == set(b)
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    return True
