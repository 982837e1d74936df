"""The yardstick of tests/test_gpu_layer_dbas.py (tests/_layer_dbas.py: the oracle's ddp_sensitivity_upper and the
alpha / gamma formulas in f64 numpy, h evaluated at the tape rows) held to two independent references.  CPU only; it
passes with or without the product's new code by design.

1. oracle.ift_gradient's columns DTMPC_P_ALPHA (9) and DTMPC_P_GAMMA (10) divided by their chain factors
   softplus'(alpha_raw) and 1 - gamma^2: that function recomputes x' = f(x_k, u_k) where the yardstick reads the tape
   row, and tests/test_oracle_general.py holds it to the reference's KATs.  On the twelve cases of
   tests/test_gpu_layer.py with b_0 offset (tests/_layer_dbas.offset_b0: the gamma row is identically zero on a tape
   whose b_0 is the barrier of its start position), bar 1e-12 of the batch's largest row.
2. Central differences of loss = sum(gX * dbas_rollout(x0, V)) w.r.t. spec.dbas_alpha and spec.dbas_gamma on
   ALL-ACTIVE tapes (every control on a bound: du = 0 and the IFT row is the exact derivative of the rollout) with
   b_0 held fixed, the recipe of tests/test_layer_geom_yardstick.py: step 1e-6, trajectories with max |b| < 1e3, bar
   1e-6 of a row's scale (_common.rel_rows); for alpha also without the trajectories that have a tape row within 1e-3
   of the branch point h = a (dBa is continuous there but the difference quotient straddles two polynomials)."""
from __future__ import annotations

import numpy as np
import pytest

from _common import rel_rows
from _layer_dbas import dbas_rows, offset_b0

RAW_TIGHT = -800.0  # softplus(-800) = 0 exactly: the target cost's tightening (ift_gradient's nominal form) is off


def raw_theta(o, alpha, gamma):
    """(theta_raw [12], alpha', gamma', softplus'(alpha_raw), 1 - gamma'^2): raw parameters whose ift_gradient values
    alpha' = softplus(raw) + 1e-6 and gamma' = tanh(raw) are the given ones up to the inversion's rounding."""
    th = np.zeros(12)
    th[9] = np.log(np.expm1(alpha - 1e-6))
    th[10] = np.arctanh(gamma)
    th[11] = RAW_TIGHT
    real = np.dtype(o.dt).type
    a = float(o.softplus(np.array([th[9]], real))[0] + real(1e-6))
    g = float(np.tanh(real(th[10])))
    return th, a, g, float(1.0 / (1.0 + np.exp(-th[9]))), 1.0 - g * g


def _with(spec, **kw):
    s = type(spec).from_buffer_copy(spec)
    for k, v in kw.items():
        setattr(s, k, float(v))
    return s


def test_yardstick_matches_ift_gradient(oracle_lib):
    from test_gpu_layer import CASES, IDS, make_case

    o = oracle_lib.Oracle(np.float64, nthreads=8)
    worst, nz_alpha = 0.0, 0
    for case, label in zip(CASES, IDS):
        c = make_case(*case)
        th, a, g, da, dg = raw_theta(o, c["prob"].dbas_alpha, c["prob"].dbas_gamma)
        sp = _with(c["prob"].to_c(), dbas_alpha=a, dbas_gamma=g)
        cc = c["cost"].to_c()
        X = offset_b0(o, sp, c["X"], c["V"], case[5])
        assert np.array_equal(X[..., :3], c["X"][..., :3]) and not np.array_equal(X[..., 3], c["X"][..., 3])
        dX, dV, dlam, _ = o.ddp_sensitivity_upper(sp, cc, X, c["V"], c["gX"], c["gU"])
        gth = o.ift_gradient(sp, cc, th, X, c["V"], dX, dV, dlam, c["Xref"], c["Uref"])[0]
        rows = dbas_rows(o, sp, cc, X, c["V"], c["gX"], c["gU"])
        fin = rows["finite"] & np.isfinite(gth).all(1)
        assert fin.sum() >= 0.95 * len(fin), label
        ea = np.abs(rows["alpha"][fin, 0] - gth[fin, 9] / da).max() / max(1.0, np.abs(gth[fin, 9] / da).max())
        eg = np.abs(rows["gamma"][fin, 0] - gth[fin, 10] / dg).max() / max(1.0, np.abs(gth[fin, 10] / dg).max())
        print(f"[layer dbas yardstick {label}] alpha {ea:.3g}, gamma {eg:.3g} of the batch's largest row; "
              f"{int((rows['alpha'][fin, 0] != 0).sum())} non-zero alpha rows, gamma rows up to "
              f"{np.abs(rows['gamma'][fin]).max():.3g}")
        assert ea <= 1e-12 and eg <= 1e-12, (label, ea, eg)
        assert np.abs(rows["gamma"][fin]).max() > 0, label
        nz_alpha += int((rows["alpha"][fin, 0] != 0).any())
        worst = max(worst, ea, eg)
    assert nz_alpha >= 8, nz_alpha
    print(f"[layer dbas yardstick] worst {worst:.3g}")


def test_gamma_row_is_zero_on_a_consistent_tape(oracle_lib):
    """b_0 = B(h(x_0)): B(h(x_k)) - b_k = 0 along the rollout whatever gamma is, so the f64 row is (numerically)
    nothing -- the reason the device cases offset b_0."""
    from test_gpu_layer import CASES, make_case

    o = oracle_lib.Oracle(np.float64, nthreads=8)
    c = make_case(*CASES[9])
    assert c["prob"].dbas_gamma == 0.3
    rows = dbas_rows(o, c["prob"].to_c(), c["cost"].to_c(), c["X"], c["V"], c["gX"], c["gU"])
    fin = rows["finite"]
    scale = np.abs(rows["alpha"][fin]).max()
    assert scale > 0 and np.abs(rows["gamma"][fin]).max() <= 1e-9 * max(1.0, scale)


@pytest.mark.parametrize("idx", [2, 9])
def test_yardstick_matches_central_differences(oracle_lib, idx):
    from test_gpu_layer import CASES, IDS, make_case

    c = make_case(*CASES[idx])
    assert IDS[idx] in ("N2-B257-M8-target-g0.3", "N50-B65-M5-target-g0.3")
    o = oracle_lib.Oracle(np.float64, nthreads=8)
    prob = c["prob"]
    sp, cc = prob.to_c(), c["cost"].to_c()
    lo, hi = np.array(prob.u_min), np.array(prob.u_max)
    V = np.where(c["V"] > 0, hi, lo)  # every control on a bound: du = 0
    x0 = offset_b0(o, sp, c["X"], c["V"], CASES[idx][5])[:, 0].copy()  # b_0 off its position's barrier, held fixed
    gX, gU = c["gX"], c["gU"]
    X = o.dbas_rollout(sp, x0, V)
    a = max(sp.dbas_alpha, sp.dbas_eps)
    h = o.h_eval(sp, X[..., 0].reshape(-1), X[..., 1].reshape(-1))[0].reshape(X.shape[:2])
    use = np.abs(X[..., 3]).max(1) < 1e3
    use_a = use & (np.abs(h - a).min(1) > 1e-3)
    assert use.sum() >= 0.5 * len(use) and use_a.sum() >= 0.4 * len(use), (int(use.sum()), int(use_a.sum()))
    rows = dbas_rows(o, sp, cc, X, V, gX, gU)
    assert rows["finite"][use].all()
    loss = lambda s_: (gX * o.dbas_rollout(s_, x0, V)).sum((1, 2))  # noqa: E731
    step = 1e-6
    fd = {}
    for key, field in (("alpha", "dbas_alpha"), ("gamma", "dbas_gamma")):
        v = getattr(sp, field)
        fd[key] = ((loss(_with(sp, **{field: v + step})) - loss(_with(sp, **{field: v - step}))) / (2 * step))[:, None]
    ea = rel_rows(rows["alpha"][use_a], fd["alpha"][use_a])
    eg = rel_rows(rows["gamma"][use], fd["gamma"][use])
    print(f"[layer dbas fd {IDS[idx]}] alpha: {int(use_a.sum())} of {len(use)} trajectories, {ea.max():.3g}; gamma: "
          f"{int(use.sum())}, {eg.max():.3g} of a row's scale; |fd| up to {np.abs(fd['alpha'][use_a]).max():.3g} / "
          f"{np.abs(fd['gamma'][use]).max():.3g}")
    assert np.abs(fd["alpha"][use_a]).max() > 0 and np.abs(fd["gamma"][use]).max() > 0
    assert ea.max() <= 1e-6, ea.max()
    assert eg.max() <= 1e-6, eg.max()
