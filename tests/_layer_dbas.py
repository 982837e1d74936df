"""The yardstick of the differentiable solve's rows w.r.t. the barrier-state (DBaS) parameters alpha and gamma, built
on the oracle alone (oracle/oracle.py; pinned to oracle.ift_gradient and to finite differences by
tests/test_layer_dbas_yardstick.py).  It uses none of the product's code.

With dlam = ddp_sensitivity_upper's delta_lambda, lam_k = dlam_k[3], a = max(alpha, eps) and
    co_m = [m >= 1] lam_m - gamma [m <= N-1] lam_{m+1}                                          m = 0 .. N
only the barrier row b' = B(h(x')) - gamma (B(h(x)) - b) of f_hat depends on alpha and gamma, and the two rows are
    g_alpha_eff = sum_{m=0..N} co_m dBa(h(x_m)),   dBa(z) = 0 for z >= a, -3 (z - a)^2 / a^4 below
    g_gamma     = -sum_{k=0..N-1} lam_{k+1} (B(h(x_k)) - b_k)
(oracle/oracle_general.h ift1's ga / gg without the softplus / tanh chain and without d max(alpha, eps) / d alpha; h
at the tape rows x_m where ift1 recomputes x' = f(x_k, u_k): on a rolled-out tape the two agree to rounding).  h and
B are the oracle build's own (oracle_h_eval; oracle_barrier, whose index 1 is the DBaS barrier); the sums are f64
numpy.

The gamma row on a consistent tape: if b_0 = B(h(x_0)) then B(h(x_k)) - b_k = 0 for every k, whatever gamma is, and
the gamma row is identically zero in exact arithmetic.  It is non-zero only when the tape starts from a barrier state
that is not the barrier of its position (a plant state after a disturbance, the second of two chained solves):
offset_b0 below makes such tapes from the cases of tests/test_gpu_layer.py."""
from __future__ import annotations

import numpy as np


def dbas_from_dlam(o, spec, X, dlam) -> dict:
    """{"alpha" [B, 1] (the alpha_eff row), "gamma" [B, 1]} (f64) from a tape X [B, N+1, 4] and delta_lambda."""
    X = np.asarray(X)
    B, N = X.shape[0], spec.horizon
    lam = np.asarray(dlam, np.float64)[..., 3]
    h = o.h_eval(spec, X[..., 0].reshape(-1), X[..., 1].reshape(-1))[0]
    Bv = o.barrier(spec, h)[1].astype(np.float64).reshape(B, N + 1)
    h = h.astype(np.float64).reshape(B, N + 1)
    a = max(float(spec.dbas_alpha), float(spec.dbas_eps))
    dBa = np.where(h >= a, 0.0, -3.0 * (h - a) ** 2 / a ** 4)
    zero = np.zeros((B, 1))
    co = np.concatenate([zero, lam[:, 1:]], 1) - float(spec.dbas_gamma) * np.concatenate([lam[:, 1:], zero], 1)
    ga = (co * dBa).sum(1, keepdims=True)
    gg = -(lam[:, 1:] * (Bv[:, :N] - X[:, :N, 3].astype(np.float64))).sum(1, keepdims=True)
    return {"alpha": ga, "gamma": gg}


def dbas_rows(o, spec, cost_c, X, V, gX, gU) -> dict:
    """The rows of one oracle build `o`: {"alpha" [B, 1], "gamma" [B, 1], "finite" [B] bool}."""
    dX, _, dlam, _ = o.ddp_sensitivity_upper(spec, cost_c, X, V, gX, gU)
    out = dbas_from_dlam(o, spec, X, dlam)
    out["finite"] = np.isfinite(out["alpha"]).all(1) & np.isfinite(out["gamma"]).all(1) & \
        np.isfinite(dX[:, spec.horizon]).all(1)
    return out


def offset_b0(o, spec, X, V, seed) -> np.ndarray:
    """The tape of the same positions and controls from a barrier state that is not the barrier of its position:
    b_0 <- b_0 U[0.5, 1.5] + U[-0.2, 0.2] with default_rng(seed + 1000), re-rolled with the oracle."""
    rng = np.random.default_rng(seed + 1000)
    x0 = np.array(X[:, 0], np.float64)
    B = len(x0)
    x0[:, 3] = x0[:, 3] * rng.uniform(0.5, 1.5, B) + rng.uniform(-0.2, 0.2, B)
    return o.dbas_rollout(spec, x0, V)
