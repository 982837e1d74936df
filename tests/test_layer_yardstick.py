"""The yardstick of tests/test_gpu_layer.py (tests/_layer.py: the oracle's ddp_sensitivity_upper + ift_gradient,
softplus factors divided out) held to the reference: tests/golden/layer_f64.npz holds the reference's own
ddp_sensitivity + ift_gradient with the PLAIN Q, R, Qf, q_b, target / X_ref / U_ref as theta_tensors
(tests/golden/make_golden_layer.py).  CPU only; it passes with or without the product's new code by design."""
from __future__ import annotations

import dataclasses

import numpy as np

from _common import golden, paper_setup
from _layer import layer_rows


def close(a, b, rtol, atol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= atol + rtol * np.abs(b)))


def test_yardstick_matches_the_reference(oracle_lib):
    """The tolerances of test_ift_gradient_device_vs_reference_kats: 1e-9 / 1e-10 on the weight rows (and on the
    target's, a sum of reference rows), 1e-12 / 1e-13 on the reference rows."""
    from diff_tube_mpc_strict_pt.core import QuadraticCost

    k = golden("layer_f64")
    o = oracle_lib.Oracle(np.float64)
    base = paper_setup().problem
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
        r = layer_rows(o, sp, cost.to_c(), X, V, k[p + "gX"][None], k[p + "gU"][None],
                       k[p + "Xref"][None] if track else None, k[p + "Uref"][None] if track else None)
        assert r["finite"].all(), c
        assert close(r["weights"][0], k[p + "g_w"], 1e-9, 1e-10), (c, r["weights"][0], k[p + "g_w"])
        if track:
            assert r["target"] is None
            assert close(r["X_ref"][0], k[p + "g_xref"], 1e-12, 1e-13), c
            assert close(r["U_ref"][0], k[p + "g_uref"], 1e-12, 1e-13), c
        else:
            assert r["X_ref"] is None and r["U_ref"] is None
            assert close(r["target"][0], k[p + "g_target"], 1e-9, 1e-10), (c, r["target"][0], k[p + "g_target"])
        assert np.abs(k[p + "g_w"]).max() > 0
        kinds.add(track)
        gammas.add(float(k[p + "gamma"]))
        h = o.h_eval(sp, X[0, :, 0], X[0, :, 1])[0]
        below += int((h < float(k["alpha"])).sum())
        assert N <= 5
    assert kinds == {True, False} and gammas == {0.0, 0.3} and below > 0
