"""The yardstick of the differentiable solve's rows w.r.t. the start state and the obstacle circles, built on the
oracle alone (oracle/oracle.py; pinned to the reference and to finite differences by
tests/test_layer_geom_yardstick.py).  It uses none of the product's code.

With dlam = ddp_sensitivity_upper's delta_lambda (dlam_k = tilde V_x[k] + V_xx[k] dx_k, core/ddp.py:424-425) and
lam_k = dlam_k[3], the two terms of ift_gradient (core/ift.py:35-92) that involve delta_lambda are
    g_x0 = dlam_0                                                   (xi = x0_hat, xi_theta = I)
    c_m = B'(h(x_m)) ([m >= 1] lam_m - gamma [m <= N-1] lam_{m+1})                          m = 0 .. N
    g_cx_j = sum_m c_m w_j(x_m) (-2 (px_m - cx_j)),  g_cy_j alike,  g_r_j = 2 r_j sum_m c_m w_j(x_m) (-1)
with w_j = softmax_j(-beta h_j), h_j = (px - cx_j)^2 + (py - cy_j)^2 - r_j^2: only the barrier row of f_hat,
b' = B(h(x')) - gamma (B(h(x)) - b), depends on the circles.  h and B' are the oracle build's own (oracle_h_eval,
oracle_barrier); the weights and the sums are f64 numpy."""
from __future__ import annotations

import numpy as np


def circles_of(spec) -> np.ndarray:
    """[M, 3] (cx, cy, r) of a dtmpc_spec."""
    M = spec.n_obstacles
    return np.array([[spec.obs_cx[j], spec.obs_cy[j], spec.obs_r[j]] for j in range(M)], np.float64)


def geom_from_dlam(o, spec, X, dlam) -> dict:
    """{"x0" [B, 4], "obstacles" [B, M, 3]} (f64) from a tape X [B, N+1, 4] and delta_lambda [B, N+1, 4]."""
    X = np.asarray(X)
    B, N = X.shape[0], spec.horizon
    tab = circles_of(spec)
    X64, lam = X.astype(np.float64), np.asarray(dlam, np.float64)[..., 3]
    dx = X64[..., 0:1] - tab[:, 0]  # [B, N+1, M]
    dy = X64[..., 1:2] - tab[:, 1]
    z = -float(spec.obs_beta) * (dx * dx + dy * dy - tab[:, 2] ** 2)
    e = np.exp(z - z.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    h = o.h_eval(spec, X[..., 0].reshape(-1), X[..., 1].reshape(-1))[0]
    D = o.barrier(spec, h)[2].astype(np.float64).reshape(B, N + 1)
    zero = np.zeros((B, 1))
    c = D * (np.concatenate([zero, lam[:, 1:]], 1) - float(spec.dbas_gamma) * np.concatenate([lam[:, 1:], zero], 1))
    cw = c[..., None] * w
    obs = np.stack([(cw * (-2.0 * dx)).sum(1), (cw * (-2.0 * dy)).sum(1), -cw.sum(1) * (2.0 * tab[:, 2])], 2)
    return {"x0": np.asarray(dlam, np.float64)[:, 0].copy(), "obstacles": obs}


def geom_rows(o, spec, cost_c, X, V, gX, gU) -> dict:
    """The rows of one oracle build `o`: {"x0" [B, 4], "obstacles" [B, M, 3], "finite" [B] bool}."""
    dX, _, dlam, _ = o.ddp_sensitivity_upper(spec, cost_c, X, V, gX, gU)
    out = geom_from_dlam(o, spec, X, dlam)
    out["finite"] = np.isfinite(out["x0"]).all(1) & np.isfinite(out["obstacles"]).all((1, 2)) & \
        np.isfinite(dX[:, spec.horizon]).all(1)
    return out
