"""The yardstick of tests/test_gpu_layer_geom.py (tests/_layer_geom.py: the oracle's ddp_sensitivity_upper and the
x0 / obstacle formulas in f64 numpy) held to two independent references.  CPU only; it passes with or without the
product's new code by design.

1. The reference itself: tests/golden/layer_geom_f64.npz holds the reference's ddp_sensitivity + ift_gradient with
   theta_tensors = [x0_hat, centres, radii] (tests/golden/make_golden_layer_geom.py), at the tolerances of
   tests/test_layer_yardstick.py (1e-9 / 1e-10).
2. Central differences of loss = sum(gX * dbas_rollout(x0, V)) on ALL-ACTIVE tapes: every control sits on a bound
   of the box, so du = 0 and the IFT row is the exact derivative of the rollout w.r.t. x0_hat and w.r.t. every
   circle parameter.  Step 1e-6, trajectories with max |b| < 1e3, bar 1e-6 of a row's scale (_common.rel_rows; the
   yardstick was measured at 1.4e-8 on these tapes, two orders of margin for finite-difference noise)."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from _common import golden, paper_setup, rel_rows
from _layer_geom import circles_of, geom_rows
from test_layer_yardstick import close


def test_yardstick_matches_the_reference(oracle_lib):
    from diff_tube_mpc_strict_pt.core import QuadraticCost

    k = golden("layer_geom_f64")
    o = oracle_lib.Oracle(np.float64)
    base = paper_setup().problem
    assert np.array_equal(k["circles"], [[ob.center[0], ob.center[1], ob.radius] for ob in base.obstacles])
    kinds, gammas, below = set(), set(), 0
    for c in range(int(k["n_cases"])):
        p = f"c{c}_"
        X, V = k[p + "X"][None], k[p + "V"][None]
        N = V.shape[1]
        track = bool(k[p + "kind"])
        prob = dataclasses.replace(base, horizon=N, dbas_alpha=float(k["alpha"]), dbas_gamma=float(k[p + "gamma"]))
        W = k[p + "W"]
        cost = QuadraticCost(kind="track" if track else "target", Q=tuple(W[0:3]), R=tuple(W[3:5]), Qf=tuple(W[5:8]),
                             qb=float(W[8]), target=tuple(k[p + "target"]))
        sp = prob.to_c()
        r = geom_rows(o, sp, cost.to_c(), X, V, k[p + "gX"][None], k[p + "gU"][None])
        assert r["finite"].all(), c
        assert close(r["x0"][0], k[p + "g_x0"], 1e-9, 1e-10), (c, r["x0"][0], k[p + "g_x0"])
        assert close(r["obstacles"][0], k[p + "g_obs"], 1e-9, 1e-10), (c, r["obstacles"][0], k[p + "g_obs"])
        assert np.abs(k[p + "g_x0"]).max() > 0 and np.abs(k[p + "g_obs"]).max() > 0
        kinds.add(track)
        gammas.add(float(k[p + "gamma"]))
        h = o.h_eval(sp, X[0, :, 0], X[0, :, 1])[0]
        below += int((h < float(k["alpha"])).sum())
        assert N <= 5
    assert kinds == {True, False} and gammas == {0.0, 0.3} and below > 0


def _with_circles(spec, tab):
    s = type(spec).from_buffer_copy(spec)
    for j in range(s.n_obstacles):
        s.obs_cx[j], s.obs_cy[j], s.obs_r[j] = (float(v) for v in tab[j])
    return s


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
    x0 = c["X"][:, 0].copy()
    gX, gU = c["gX"], c["gU"]
    X = o.dbas_rollout(sp, x0, V)
    use = np.abs(X[..., 3]).max(1) < 1e3
    assert use.sum() >= 0.5 * len(use), int(use.sum())
    rows = geom_rows(o, sp, cc, X, V, gX, gU)
    assert rows["finite"][use].all()
    loss = lambda s_, x0_: (gX * o.dbas_rollout(s_, x0_, V)).sum((1, 2))  # noqa: E731
    step = 1e-6
    fd0 = np.empty((len(x0), 4))
    for j in range(4):
        e = np.zeros(4)
        e[j] = step
        fd0[:, j] = (loss(sp, x0 + e) - loss(sp, x0 - e)) / (2 * step)
    tab = circles_of(sp)
    M = len(tab)
    fdo = np.empty((len(x0), M, 3))
    for j in range(M):
        for f in range(3):
            e = np.zeros_like(tab)
            e[j, f] = step
            fdo[:, j, f] = (loss(_with_circles(sp, tab + e), x0) - loss(_with_circles(sp, tab - e), x0)) / (2 * step)
    e0 = rel_rows(rows["x0"][use], fd0[use])
    eo = rel_rows(rows["obstacles"][use], fdo[use])
    print(f"[layer geom fd {IDS[idx]}] {int(use.sum())} of {len(use)} trajectories: x0 {e0.max():.3g}, "
          f"obstacles {eo.max():.3g} of a row's scale")
    assert np.abs(fd0[use]).max() > 0 and np.abs(fdo[use]).max() > 0
    assert e0.max() <= 1e-6, e0.max()
    assert eo.max() <= 1e-6, eo.max()
