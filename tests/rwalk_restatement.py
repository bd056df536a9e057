"""float64 NumPy restatement of RWalk (Riemannian Walk: Chaudhry, Dokania, Ajanthan, Torr, ECCV 2018) as this project defines it
(DESIGN.md), written from the formulae.  Nothing here is shared with the code under test.

Per regularised element four states: F (moving average of the squared gradient, kept across tasks), s (accumulated path scores,
kept across tasks), w (path integral of the current interval), theta_ck (the parameter at the last checkpoint).

One optimizer update of the element, gr = the clipped gradient the update consumes (g * c, before SGD adds wd * p), p0 -> pv the
values the parameter holds before and after:
    F <- F + alpha (gr^2 - F)
    w <- w - gr (pv - p0)
    on a checkpoint update:   d = pv - theta_ck ;  s <- s + max(w, 0) / (0.5 F d^2 + eps)  (the new F and w) ;  w <- 0 ;  theta_ck <- pv
End of a task, over ALL regularised elements of all tensors:
    flush   s <- s + max(w, 0) / (0.5 F (p - theta_ck)^2 + eps) ;  w <- 0
    maxF = max F, maxS = max s
    importance = F / maxF + s / maxS   (a term whose max is 0 contributes 0) ;  optpar = p ;  s <- s / 2 ;  theta_ck <- p ;  F kept

alpha and eps enter as the doubles their C `float` arguments carry (`f32`)."""
import numpy as np


def f32(x):
    return float(np.float32(x))


def _d(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def update(F, s, w, theta_ck, gr, p0, pv, alpha, eps, checkpoint):
    """one update.  -> (F, s, w, theta_ck) after it, and `parts` = {'g2': gr^2, 'term': |gr (pv - p0)|, 'quot': the score's
    addend (zeros when no checkpoint), 'den': its denominator, 'w_closed': the w that was scored} for rounding bounds."""
    F, s, w, theta_ck, gr, p0, pv = map(_d, (F, s, w, theta_ck, gr, p0, pv))
    alpha, eps = f32(alpha), f32(eps)
    g2 = gr * gr
    F1 = F + alpha * (g2 - F)
    term = gr * (pv - p0)
    w1 = w - term
    parts = dict(g2=g2, term=np.abs(term), quot=np.zeros_like(s), den=None, w_closed=w1)
    if not checkpoint:
        return F1, s.copy(), w1, theta_ck.copy(), parts
    d = pv - theta_ck
    den = 0.5 * F1 * d * d + eps
    quot = np.maximum(w1, 0.0) / den
    parts.update(quot=quot, den=den)
    return F1, s + quot, np.zeros_like(w1), pv.copy(), parts


def consolidate(ps, Fs, ss, ws, cks, eps):
    """end of a task over lists of tensors.  -> dict of lists 'importance', 'optpar', 'F', 's', 'w', 'theta_ck' (after), scalars
    'maxF', 'maxS', and lists 'term_F', 'term_s' (the importance's two addends), 's_flushed', 'quot'."""
    eps = f32(eps)
    ps, Fs, ss, ws, cks = ([_d(x) for x in lst] for lst in (ps, Fs, ss, ws, cks))
    quot = [np.maximum(w, 0.0) / (0.5 * F * (p - ck) ** 2 + eps) for p, F, w, ck in zip(ps, Fs, ws, cks)]
    flushed = [s + q for s, q in zip(ss, quot)]
    maxF = max([float(F.max()) for F in Fs if F.size] or [0.0])
    maxS = max([float(s.max()) for s in flushed if s.size] or [0.0])
    tF = [F / maxF if maxF != 0 else np.zeros_like(F) for F in Fs]
    tS = [s / maxS if maxS != 0 else np.zeros_like(s) for s in flushed]
    return dict(importance=[a + b for a, b in zip(tF, tS)], optpar=[p.copy() for p in ps], F=[F.copy() for F in Fs],
                s=[0.5 * s for s in flushed], w=[np.zeros_like(w) for w in ws], theta_ck=[p.copy() for p in ps],
                maxF=maxF, maxS=maxS, term_F=tF, term_s=tS, s_flushed=flushed, quot=quot)
