"""float64 restatement of Synaptic Intelligence (Zenke, Poole, Ganguli 2017) as this project defines it, in plain
torch on the CPU, written from the definition.  Nothing here is shared with the code under test; the optimizer updates are
those of tests/optim_restatement.py.

Per optimizer step and regularised element:   omega <- omega - gr * (p_new - p_old)
  gr = g * c, the clipped gradient the update consumes (before SGD adds wd * p; whatever a penalty added to g is part of it),
  p_new - p_old the difference of the values the parameter holds after and before the update (weight decay included).
End of a task:   Omega <- Omega_old + max(omega, 0) / ((theta - theta_start)^2 + xi)   (Omega_old = 0 where there is none: no
  earlier task, or the rows a class head has gained since), theta* <- theta, omega <- 0, theta_start <- theta.
Later tasks:   penalty = lambda * sum Omega (theta* - theta[:len(theta*)])^2."""
import torch

import optim_restatement as R


def _d(x):
    return x.detach().double().cpu()


def path_integral(omega, g, coef, p_old, p_new):
    """one step of the path integral from the values the parameter HOLDS before and after the update.
    Returns (omega_new, |gr * (p_new - p_old)|)."""
    term = (_d(g) * coef) * (_d(p_new) - _d(p_old))
    return _d(omega) - term, term.abs()


def adamw_si_step(p, g, m, v, omega, step, lr, wd, beta1, beta2, eps, coef=1.0):
    """AdamW update (optim_restatement.adamw_step) + the path integral along it.  -> (p_new, m_new, v_new, omega_new)"""
    p_new, m_new, v_new, _ = R.adamw_step(p, g, m, v, step, lr, wd, beta1, beta2, eps, coef)
    return p_new, m_new, v_new, path_integral(omega, g, coef, p, p_new)[0]


def sgd_si_step(p, g, buf, omega, step, lr, wd, momentum, coef=1.0):
    """SGD-momentum update (optim_restatement.sgd_step) + the path integral along it; gr does not contain wd * p.
    -> (p_new, buf_new, omega_new)"""
    p_new, buf_new, _ = R.sgd_step(p, g, buf, step, lr, wd, momentum, coef)
    return p_new, buf_new, path_integral(omega, g, coef, p, p_new)[0]


def consolidate(theta, omega, theta_start, imp_old, xi):
    """end of a task.  imp_old: None, or a tensor covering the first imp_old.numel() elements of the flattened parameter.
    Returns (importance, optpar, omega, theta_start) after the consolidation, in theta's shape, and the two addends of the
    importance (old part, quotient) for rounding bounds."""
    theta, omega, theta_start = _d(theta), _d(omega), _d(theta_start)
    xi = R.f32(xi)
    old = torch.zeros_like(theta)
    if imp_old is not None:
        n = imp_old.numel()
        old.view(-1)[:n] = _d(imp_old).reshape(-1)
    quot = omega.clamp_min(0.0) / ((theta - theta_start) ** 2 + xi)
    return old + quot, theta.clone(), torch.zeros_like(theta), theta.clone(), (old, quot)


def penalty(params, entries, lam):
    """lam * sum over (param index, importance, optpar) entries of sum Omega (theta* - theta[:len(theta*)])^2"""
    zeros = [torch.zeros_like(_d(p)) for p in params]
    return R.penalty(params, zeros, entries, lam)[0]
