"""The yardstick of tests/test_gpu_layer_tight.py (tests/_layer_tight.py: the oracle's ddp_sensitivity_upper per group
of equal tightening and the formulas with z = h - s in f64 numpy, h evaluated at the tape rows) held to two independent
references.  CPU only; it passes with or without the product's new code by design.

1. oracle.ift_gradient's column DTMPC_P_TIGHT (11) divided by softplus'(raw): that function recomputes
   x' = f(x_k, u_k) where the yardstick reads the tape row, and tests/test_oracle_general.py holds it to the reference's
   KATs.  The column exists for the target cost only (the reference tightens the nominal solve), so the six
   target-kind cases of tests/test_gpu_layer.py are used, with b_0 offset (tests/_layer_dbas.offset_b0), s in
   {0.05, 0.3} and the tape re-rolled under the tightened spec; bar 1e-12 of the batch's largest row.
2. Central differences of loss = sum(gX * dbas_rollout(x0, V)) w.r.t. spec.h_offset on ALL-ACTIVE tapes (every control
   on a bound: du = 0 and the IFT row is the exact derivative of the rollout) with b_0 held fixed, the recipe of
   tests/test_layer_dbas_yardstick.py: step 1e-6, trajectories with max |b| < 1e3 and no tape row within 1e-3 of the
   branch points z = a and z = eps, bar 1e-6 of a row's scale.  Under the same s != 0 the obstacle, alpha and gamma rows
   are held to central differences by the sibling yardsticks' recipes (circles moved in the spec, dbas_alpha,
   dbas_gamma)."""
from __future__ import annotations

import numpy as np
import pytest

from _common import rel_rows
from _layer import raw_of, softplus_d
from _layer_dbas import offset_b0
from _layer_tight import reroll, tight_rows, with_offset
from test_layer_dbas_yardstick import _with, raw_theta

S_VALUES = (0.05, 0.3)


def test_yardstick_matches_ift_gradient(oracle_lib):
    from test_gpu_layer import CASES, IDS, make_case

    o = oracle_lib.Oracle(np.float64, nthreads=8)
    worst, n_cases = 0.0, 0
    for case, label in zip(CASES, IDS):
        if case[3] != "target":
            continue
        n_cases += 1
        c = make_case(*case)
        th, a, g, _, _ = raw_theta(o, c["prob"].dbas_alpha, c["prob"].dbas_gamma)
        sp0 = _with(c["prob"].to_c(), dbas_alpha=a, dbas_gamma=g)
        cc = c["cost"].to_c()
        B = c["X"].shape[0]
        for s in S_VALUES:
            raw_s = float(raw_of([s])[0])
            s_eff = float(o.softplus(np.array([raw_s]))[0])  # the value ift_gradient forms from the raw parameter
            sp = with_offset(sp0, s_eff)
            X = reroll(o, sp0, offset_b0(o, sp0, c["X"], c["V"], case[5]), c["V"], np.full(B, s_eff))
            assert np.array_equal(X[..., :3], c["X"][..., :3])
            dX, dV, dlam, _ = o.ddp_sensitivity_upper(sp, cc, X, c["V"], c["gX"], c["gU"])
            th[11] = raw_s
            gth = o.ift_gradient(sp, cc, th, X, c["V"], dX, dV, dlam)[0]
            rows = tight_rows(o, sp0, cc, X, c["V"], c["gX"], c["gU"], np.full(B, s_eff))
            fin = rows["finite"] & np.isfinite(gth).all(1)
            assert fin.sum() >= 0.95 * len(fin), (label, s)
            ref = gth[fin, 11] / float(softplus_d([raw_s])[0])
            e = np.abs(rows["tight"][fin, 0] - ref).max() / max(1.0, np.abs(ref).max())
            print(f"[layer tight yardstick {label} s={s}] {e:.3g} of the batch's largest row ({np.abs(ref).max():.3g}); "
                  f"{int((ref != 0).sum())} non-zero rows of {int(fin.sum())}")
            assert e <= 1e-12, (label, s, e)
            assert np.abs(ref).max() > 0, (label, s)
            worst = max(worst, e)
    assert n_cases == sum(c[3] == "target" for c in CASES) == 6
    print(f"[layer tight yardstick] worst {worst:.3g}")


def test_delta_lambda_does_not_depend_on_s(oracle_lib):
    """The reference linearises with the plain h: on a given tape ddp_sensitivity_upper's outputs are bitwise the same
    at every h_offset (the fact the fused kernel's unchanged backward sweep rests on)."""
    from test_gpu_layer import CASES, make_case

    o = oracle_lib.Oracle(np.float64, nthreads=8)
    c = make_case(*CASES[9])
    sp, cc = c["prob"].to_c(), c["cost"].to_c()
    a = o.ddp_sensitivity_upper(sp, cc, c["X"], c["V"], c["gX"], c["gU"])
    b = o.ddp_sensitivity_upper(with_offset(sp, 0.3), cc, c["X"], c["V"], c["gX"], c["gU"])
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("idx", [2, 9])
@pytest.mark.parametrize("s", S_VALUES)
def test_yardstick_matches_central_differences(oracle_lib, idx, s):
    from test_gpu_layer import CASES, IDS, make_case

    c = make_case(*CASES[idx])
    assert IDS[idx] in ("N2-B257-M8-target-g0.3", "N50-B65-M5-target-g0.3")
    o = oracle_lib.Oracle(np.float64, nthreads=8)
    prob = c["prob"]
    sp0, cc = prob.to_c(), c["cost"].to_c()
    sp = with_offset(sp0, s)
    lo, hi = np.array(prob.u_min), np.array(prob.u_max)
    V = np.where(c["V"] > 0, hi, lo)  # every control on a bound: du = 0
    x0 = offset_b0(o, sp0, c["X"], c["V"], CASES[idx][5])[:, 0].copy()  # b_0 off its position's barrier, held fixed
    gX, gU = c["gX"], c["gU"]
    B = len(x0)
    X = o.dbas_rollout(sp, x0, V)
    a = max(sp.dbas_alpha, sp.dbas_eps)
    z = o.h_eval(sp, X[..., 0].reshape(-1), X[..., 1].reshape(-1))[0].reshape(X.shape[:2]) - s
    use = np.abs(X[..., 3]).max(1) < 1e3
    use &= (np.abs(z - a).min(1) > 1e-3) & (np.abs(z - sp.dbas_eps).min(1) > 1e-3)
    assert use.sum() >= 0.5 * B, (int(use.sum()), B)
    rows = tight_rows(o, sp0, cc, X, V, gX, gU, np.full(B, s))
    assert rows["finite"][use].all()
    loss = lambda s_: (gX * o.dbas_rollout(s_, x0, V)).sum((1, 2))  # noqa: E731
    step = 1e-6
    fd = {}
    for key, field in (("tight", "h_offset"), ("alpha", "dbas_alpha"), ("gamma", "dbas_gamma")):
        v = getattr(sp, field)
        fd[key] = ((loss(_with(sp, **{field: v + step})) - loss(_with(sp, **{field: v - step}))) / (2 * step))[:, None]
    # the circles: every obstacle's cx, cy, r moved in the spec (tests/test_layer_geom_yardstick.py's recipe)
    M = sp.n_obstacles
    fdo = np.zeros((B, M, 3))
    for j in range(M):
        for q, field in enumerate(("obs_cx", "obs_cy", "obs_r")):
            sp_p, sp_m = with_offset(sp, s), with_offset(sp, s)
            getattr(sp_p, field)[j] += step
            getattr(sp_m, field)[j] -= step
            fdo[:, j, q] = (loss(sp_p) - loss(sp_m)) / (2 * step)
    errs = {k: rel_rows(rows[k][use], fd[k][use]).max() for k in ("tight", "alpha", "gamma")}
    errs["obstacles"] = rel_rows(rows["obstacles"][use].reshape(int(use.sum()), -1),
                                 fdo[use].reshape(int(use.sum()), -1)).max()
    print(f"[layer tight fd {IDS[idx]} s={s}] {int(use.sum())} of {B} trajectories; of a row's scale: "
          + ", ".join(f"{k} {v:.3g}" for k, v in errs.items())
          + f"; |fd tight| up to {np.abs(fd['tight'][use]).max():.3g}")
    assert np.abs(fd["tight"][use]).max() > 0 and np.abs(fdo[use]).max() > 0
    for k, v in errs.items():
        assert v <= 1e-6, (k, v)
