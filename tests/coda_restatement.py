"""Float64 NumPy restatement of CODA-Prompt (Smith et al., CVPR 2023) as this project defines it (include/vilco_hip.h:
vilco_coda_desc; vilco_amd/cl_methods/coda.py) -- forward and the hand-derived gradients.  The reference project has no
CODA-Prompt, so this file is the yardstick of ops.coda_prompt; tests/test_coda_cpu.py ties its gradients to torch float64
autograd of the forward written with einsum / F.normalize / .detach().

  xk[b]       = mean_l x[b][l]
  u[b][m]     = xk[b] * A[m],  alpha[b][m] = <u, K[m]> / (max(|u|, eps) max(|K[m]|, eps))   for m < f, 0 for m >= f
  p[b]        = sum_{m < f} alpha[b][m] prompt[m];   prompted[b] = [p[b] ; x[b]]
  ortho       = pen(K[:f]) + pen(A[:f]) + pen(prompt[:f] as [f, len C]),  pen(T) = mean((T T^t - I)^2)
Gradients for rows [s, f) only (rows below s are detached, rows from f on unused); the query is a constant."""
import numpy as np

EPS = 1e-12


def _f64(*ts):
    return [np.asarray(t, dtype=np.float64) for t in ts]


def pen(T):
    G = T @ T.T - np.eye(T.shape[0])
    return float((G * G).mean())


def pen_grad(T):
    """d pen / d T = 4 / f^2 (T T^t - I) T"""
    G = T @ T.T - np.eye(T.shape[0])
    return 4.0 / (T.shape[0] ** 2) * (G @ T)


def forward(x, prompt, key, attn, s, f, want_ortho=True):
    x, prompt, key, attn = _f64(x, prompt, key, attn)
    B, L, C = x.shape
    M, length, _ = prompt.shape
    assert 0 <= s < f <= M
    xk = x.sum(axis=1) / L
    u = xk[:, None, :] * attn[None, :f, :]                       # [B, f, C]
    nu = np.sqrt((u * u).sum(-1))                                # [B, f]
    nk = np.sqrt((key[:f] * key[:f]).sum(-1))                    # [f]
    alpha = np.zeros((B, M))
    alpha[:, :f] = (u * key[None, :f, :]).sum(-1) / (np.maximum(nu, EPS) * np.maximum(nk, EPS)[None, :])
    p = np.einsum('bm,mtc->btc', alpha[:, :f], prompt[:f])
    ortho = (pen(key[:f]) + pen(attn[:f]) + pen(prompt[:f].reshape(f, -1))) if want_ortho else 0.0
    return {'xk': xk, 'alpha': alpha, 'p': p, 'prompted': np.concatenate([p, x], axis=1), 'ortho': ortho,
            'norm_u': nu, 'norm_k': nk}


def backward(x, prompt, key, attn, s, f, g_prompted, g_ortho=0.0, want_ortho=True):
    """-> (d_prompt [M, len, C], d_key [M, C], d_attn [M, C], d_x [B, L, C]); rows outside [s, f) are zeros"""
    x, prompt, key, attn, g_prompted = _f64(x, prompt, key, attn, g_prompted)
    M, length, C = prompt.shape
    fw = forward(x, prompt, key, attn, s, f, want_ortho=False)
    xk, alpha = fw['xk'], fw['alpha']
    gp = g_prompted[:, :length]                                  # [B, len, C]
    d_prompt, d_key, d_attn = np.zeros_like(prompt), np.zeros_like(key), np.zeros_like(attn)
    for m in range(s, f):
        K, A = key[m], attn[m]
        sk = np.sqrt((K * K).sum())
        nk = max(sk, EPS)
        kh = K / nk
        for b in range(x.shape[0]):                              # in order of b
            ga = float((gp[b] * prompt[m]).sum())
            d_prompt[m] += alpha[b, m] * gp[b]
            u = xk[b] * A
            su = np.sqrt((u * u).sum())
            nu = max(su, EPS)
            uh = u / nu
            al = alpha[b, m]
            da_du = (kh - al * uh) / nu if su >= EPS else kh / nu        # below the clamp the norm is the clamp's constant
            da_dk = (uh - al * kh) / nk if sk >= EPS else uh / nk
            d_attn[m] += ga * xk[b] * da_du
            d_key[m] += ga * da_dk
    if want_ortho and g_ortho != 0.0:
        d_key[s:f] += g_ortho * pen_grad(key[:f])[s:f]
        d_attn[s:f] += g_ortho * pen_grad(attn[:f])[s:f]
        d_prompt[s:f] += g_ortho * pen_grad(prompt[:f].reshape(f, -1))[s:f].reshape(f - s, length, C)
    return d_prompt, d_key, d_attn, g_prompted[:, length:].copy()
