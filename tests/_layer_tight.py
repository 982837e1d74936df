"""The yardstick of the differentiable solve's rows under a per-trajectory constraint tightening s_i, and of the row
w.r.t. s_i itself, built on the oracle alone (oracle/oracle.py; pinned to oracle.ift_gradient's tightening column and to
finite differences by tests/test_layer_tight_yardstick.py).  It uses none of the product's code.

The dynamics of a tightened solve see z = h(x) - s everywhere (b' = B(h(x') - s) - gamma (B(h(x) - s) - b),
core/tube_mpc.py:235-238) while the reference linearises with B'(h) of the plain h (core/tube_mpc.py:315-320 against
:273-276), so ddp_sensitivity_upper's delta_lambda of a given tape does not depend on s.  With lam_k = dlam_k[3],
a = max(alpha, eps) and
    co_m = [m >= 1] lam_m - gamma [m <= N-1] lam_{m+1}                                          m = 0 .. N
the rows are
    g_tight     = -sum_{m=0..N} co_m B'(z_m)                  (oracle_general.h ift1's gs without the softplus chain)
    g_cx_j      = sum_m co_m B'(z_m) w_j(x_m) (-2 (px_m - cx_j)),  g_cy_j alike,  g_r_j = 2 r_j sum_m co_m B'(z_m) w_j (-1)
    g_alpha_eff = sum_m co_m dBa(z_m),   dBa(z) = 0 for z >= a, -3 (z - a)^2 / a^4 below
    g_gamma     = -sum_{k<N} lam_{k+1} (B(z_k) - b_k)
    g_x0        = dlam_0
(the obstacle and DBaS rows are tests/_layer_geom.py's and tests/_layer_dbas.py's formulas with h - s).  Trajectories
are grouped by their distinct s; per group the oracle runs at spec.h_offset = s (ddp_sensitivity_upper, h_eval), z is
formed in the build's own precision as the oracle's dynamics form it (h_eval - tight), B and B' are the build's
(oracle_barrier); the weights and the sums are f64 numpy."""
from __future__ import annotations

import numpy as np

from _layer_geom import circles_of


def with_offset(spec, s):
    """A copy of a dtmpc_spec with h_offset = s."""
    sp = type(spec).from_buffer_copy(spec)
    sp.h_offset = float(s)
    return sp


def groups_of(s):
    """[(value, indices)] of the distinct values of s [B]."""
    s = np.asarray(s, np.float64)
    return [(float(v), np.nonzero(s == v)[0]) for v in np.unique(s)]


def tight_from_dlam(o, spec, X, dlam, s) -> dict:
    """The rows of ONE group (a scalar s, spec.h_offset = s) from a tape X [B, N+1, 4] and delta_lambda [B, N+1, 4]:
    {"tight" [B, 1], "alpha" [B, 1] (the alpha_eff row), "gamma" [B, 1], "x0" [B, 4], "obstacles" [B, M, 3]} (f64)."""
    X = np.asarray(X)
    B, N = X.shape[0], spec.horizon
    real = np.dtype(o.dt).type
    lam = np.asarray(dlam, np.float64)[..., 3]
    h = o.h_eval(spec, X[..., 0].reshape(-1), X[..., 1].reshape(-1))[0]
    z = (h - real(s)).astype(o.dt)  # as the oracle's dynamics form it: h_eval(...) - s->tight
    Bd, Br, dB = o.barrier(spec, z)
    Bv = Br.astype(np.float64).reshape(B, N + 1)
    D = dB.astype(np.float64).reshape(B, N + 1)
    z = z.astype(np.float64).reshape(B, N + 1)
    a = max(float(spec.dbas_alpha), float(spec.dbas_eps))
    dBa = np.where(z >= a, 0.0, -3.0 * (z - a) ** 2 / a ** 4)
    zero = np.zeros((B, 1))
    co = np.concatenate([zero, lam[:, 1:]], 1) - float(spec.dbas_gamma) * np.concatenate([lam[:, 1:], zero], 1)
    c = co * D
    tab = circles_of(spec)
    X64 = X.astype(np.float64)
    dx = X64[..., 0:1] - tab[:, 0]  # [B, N+1, M]
    dy = X64[..., 1:2] - tab[:, 1]
    zz = -float(spec.obs_beta) * (dx * dx + dy * dy - tab[:, 2] ** 2)
    e = np.exp(zz - zz.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    cw = c[..., None] * w
    obs = np.stack([(cw * (-2.0 * dx)).sum(1), (cw * (-2.0 * dy)).sum(1), -cw.sum(1) * (2.0 * tab[:, 2])], 2)
    return {"tight": -c.sum(1, keepdims=True), "alpha": (co * dBa).sum(1, keepdims=True),
            "gamma": -(lam[:, 1:] * (Bv[:, :N] - X64[:, :N, 3])).sum(1, keepdims=True),
            "x0": np.asarray(dlam, np.float64)[:, 0].copy(), "obstacles": obs}


KEYS = ("tight", "alpha", "gamma", "x0", "obstacles")


def tight_rows(o, spec, cost_c, X, V, gX, gU, s) -> dict:
    """The rows of one oracle build `o` for per-trajectory tightenings s [B]: KEYS and "finite" [B] bool."""
    X = np.asarray(X)
    B, M = X.shape[0], spec.n_obstacles
    out = {"tight": np.zeros((B, 1)), "alpha": np.zeros((B, 1)), "gamma": np.zeros((B, 1)), "x0": np.zeros((B, 4)),
           "obstacles": np.zeros((B, M, 3)), "finite": np.zeros(B, bool)}
    for v, idx in groups_of(s):
        sp = with_offset(spec, v)
        dX, _, dlam, _ = o.ddp_sensitivity_upper(sp, cost_c, X[idx], np.asarray(V)[idx], np.asarray(gX)[idx],
                                                 np.asarray(gU)[idx])
        r = tight_from_dlam(o, sp, X[idx], dlam, v)
        fin = np.isfinite(dX[:, spec.horizon]).all(1)
        for k in KEYS:
            out[k][idx] = r[k]
            fin &= np.isfinite(r[k].reshape(len(idx), -1)).all(1)
        out["finite"][idx] = fin
    return out


def reroll(o, spec, X, V, s) -> np.ndarray:
    """The tape of the same start states and controls under per-trajectory tightenings s [B]: re-rolled by the oracle
    per group at spec.h_offset = s (positions and controls unchanged, the barrier column that of the tightened h)."""
    X = np.asarray(X)
    out = np.array(X, dtype=X.dtype)
    for v, idx in groups_of(s):
        out[idx] = o.dbas_rollout(with_offset(spec, v), np.array(X[idx, 0], np.float64), np.asarray(V)[idx])
    return out
