"""The yardstick of the differentiable solve's gradient rows, built on the oracle alone (oracle/oracle.py, pinned to
the reference by tests/test_oracle_general.py and, for this composition, tests/test_layer_yardstick.py).  It uses
none of the product's code.

rows = ddp_sensitivity_upper (core/ddp.py:317-427 with array upper gradients) followed by ift_gradient
(core/ift.py:35-92) with raw parameters chosen so that softplus(raw) are the case's plain weights; the plain rows
are the raw rows [0:9] divided, in f64, by the softplus derivatives.  A target cost is evaluated as a tracking cost
with X_ref = target and U_ref = 0 (per trajectory, so a per-trajectory target needs nothing else), and its
g_target is the row sum of g_xref."""
from __future__ import annotations

import numpy as np


def raw_of(w) -> np.ndarray:
    """raw with softplus(raw) = w (torch's softplus: the identity above 20); w > 0."""
    w = np.asarray(w, np.float64)
    assert (w > 0).all(), "the yardstick needs positive weights (softplus has no zero)"
    return np.where(w > 20.0, w, np.log(np.expm1(np.minimum(w, 20.0))))


def softplus_d(raw) -> np.ndarray:
    raw = np.asarray(raw, np.float64)
    return np.where(raw > 20.0, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(raw, 20.0))))


def weights_of(cost_c) -> np.ndarray:
    """Q(3) R(2) Qf(3) qb of a dtmpc_cost."""
    return np.array(list(cost_c.Q) + list(cost_c.R) + list(cost_c.Qf) + [cost_c.qb], np.float64)


def layer_rows(o, spec, cost_c, X, V, gX, gU, Xref=None, Uref=None, target=None) -> dict:
    """Gradient rows of one oracle build `o` for tapes X [B, N+1, 4], V [B, N, 2] and upper gradients gX, gU.
    cost_c: a dtmpc_cost with the plain weights (its kind says which rows come back); a tracking cost takes Xref
    [B, N+1, 3] / Uref [B, N, 2], a target cost `target` [3] or [B, 3] (default: cost_c.target).
    -> {"weights" [B, 9] f64, "target" [B, 3] | None, "X_ref" [B, N+1, 3] | None, "U_ref" [B, N, 2] | None,
        "finite" [B] bool}"""
    from diff_tube_mpc_strict_pt import _abi

    X = np.asarray(X)
    B, N = X.shape[0], spec.horizon
    track = cost_c.kind == _abi.COST_TRACK
    dX, dV, dlam, _ = o.ddp_sensitivity_upper(spec, cost_c, X, V, gX, gU)
    if not track:
        tg = np.asarray(list(cost_c.target) if target is None else target, np.float64)
        Xref = np.broadcast_to(tg.reshape(-1, 1, 3), (B, N + 1, 3)).copy()
        Uref = np.zeros((B, N, 2))
    tc = type(cost_c).from_buffer_copy(cost_c)
    tc.kind = _abi.COST_TRACK
    raw = np.concatenate([raw_of(weights_of(cost_c)), [0.0, 0.0, 0.0]])
    g, gxr, gur = o.ift_gradient(spec, tc, raw, X, V, dX, dV, dlam, Xref, Uref)
    w = g[:, :9].astype(np.float64) / softplus_d(raw[:9])
    gxr64 = gxr.astype(np.float64)
    out = {"weights": w, "target": None if track else gxr64.sum(1), "X_ref": gxr if track else None,
           "U_ref": gur if track else None}
    fin = np.isfinite(w).all(1) & np.isfinite(gxr64).all((1, 2)) & np.isfinite(gur).all((1, 2)) & \
        np.isfinite(dX[:, N]).all(1)
    out["finite"] = fin
    return out
