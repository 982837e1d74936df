"""The differentiable solve's rows w.r.t. the DBaS parameters alpha and gamma on the device (dtmpc_solve_backward_dbas,
core.solve_backward(want_dbas=), diff_ilqr_solve(dbas_alpha=, dbas_gamma=)): against the oracle yardstick
(tests/_layer_dbas.py, itself held to oracle.ift_gradient and to finite differences by
tests/test_layer_dbas_yardstick.py), exact zeros where they are expected, independence of the workspace's content, of
the requested outputs and of the other trajectories, per-trajectory scenes and weights, the refusals, and the autograd
layer, chained solves included.

The cases are tests/test_gpu_layer.py's twelve (N in {1, 2, 3, 50}, B in {1, 65, 257}, M in {1, 5, 8}, both kinds,
gamma 0 / 0.3, alpha 0.05) with b_0 offset (tests/_layer_dbas.offset_b0, rng = default_rng(seed + 1000): b_0 <- b_0
U[0.5, 1.5] + U[-0.2, 0.2], re-rolled with the oracle; positions and controls unchanged).  On a tape whose b_0 is the
barrier of its start position B(h(x_k)) - b_k = 0 for every k and the gamma row is identically zero in exact
arithmetic (rounding noise in f32): only a solve started from a disturbed or chained barrier state has one.  N = 1 is
the smallest horizon at which the co_0 / co_N end terms can be mis-indexed; B = 65 and 257 are one lane past a wave
and one past a workgroup.

The gate is tests/test_gpu_layer_geom.gate's conditions on the keys alpha and gamma, each its own key (their scales
differ by orders of magnitude), and on x0 / obstacles of the same launch against tests/_layer_geom.geom_rows on the
offset tapes; the weight / reference rows stand under tests/test_gpu_layer.gate.

The f32 base follows those files' rule: the parent-buildable composition on the device (ddp_sensitivity with array
upper gradients and want_lambda in f32, then the formulas as tensor operations, composition_dbas below) on the same
cases against the same three oracle builds; the base is twice its worst error on the informative trajectories.
Measured (profiles/r14/layer_dbas_errors.txt has the per-case table): the composition's worst error is 2.83e-2 of
a row's scale (N3-B257-M1-target-g0.3, the gamma rows; 1.06e-2 on that case's alpha rows, 5.6e-3 / 1.3e-3 at
N50-B257-M5-target-g0.0, 8.0e-4 / 6.0e-4 at N50-B65-M8-track-g0.3, under 3.4e-4 in the nine remaining cases), so the
base is 5.66e-2.  The fused kernel's own worst error on the same cases, for the record: 2.97e-2 (the same case and
key; alpha 9.0e-3 there), 3.5e-3 / 5.2e-4 at N50-B257-M5-target-g0.0, 8.3e-4 alpha at N2-B257-M8-target-g0.3 (the
composition: 1.8e-4), under 1.2e-3 elsewhere.  No trajectory is non-finite; at most 2 of 257 are uninformative.
Per case (worst informative error; composition alpha, gamma; fused kernel alpha, gamma):
    N1-B1-M5-target-g0.0               0  1.89e-07           0  1.89e-07
    N1-B65-M1-track-g0.3        4.63e-05  4.61e-05    4.61e-05  4.61e-05
    N2-B257-M8-target-g0.3      0.000176  4.93e-05    0.000826  0.000148
    N3-B65-M5-track-g0.0         0.00013  5.08e-05    3.98e-05  8.15e-05
    N50-B257-M5-target-g0.0      0.00558    0.0013     0.00352  0.000524
    N50-B65-M8-track-g0.3       0.000804  0.000604     0.00115  0.000588
    N50-B1-M1-track-g0.0               0  1.08e-08           0  3.39e-09
    N2-B65-M5-track-g0.0        3.48e-05  8.01e-05     3.5e-05  2.08e-05
    N3-B257-M1-target-g0.3        0.0106    0.0283     0.00902    0.0297
    N50-B65-M5-target-g0.3      0.000123  0.000336    0.000183  0.000228
    N1-B257-M8-track-g0.0       5.71e-05   5.7e-05    5.71e-05   5.7e-05
    N3-B1-M8-target-g0.0        1.16e-05  1.07e-05    1.58e-05  5.81e-08

Whether the rows the geom entry also writes come out bitwise equal from the new entry is measured and printed, not
asserted (test_rows_against_the_geom_entry): on the device they were bitwise equal in all twelve cases."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from _common import agreement, oracles
from _layer import layer_rows
from _layer_dbas import dbas_rows, offset_b0
from _layer_geom import geom_rows
from _weights import assignment, cost_of, pack, weight_sets
from test_gpu_layer import BASE_F32 as LAYER_BASE_F32
from test_gpu_layer import (BASE_F64, CASES, IDS, TARGET, WEIGHTS, _cast, _dev_inputs, _layer_setup, _same, _sum_of, _t,
                            _weights, make_case)
from test_gpu_layer import gate as layer_gate
from test_gpu_layer_geom import BASE_F32 as GEOM_BASE_F32

pytestmark = pytest.mark.gpu

COMPOSITION_WORST = 2.83e-2
BASE_F32 = 2.0 * COMPOSITION_WORST
KEYS = ("alpha", "gamma")
GEOM_KEYS = ("x0", "obstacles")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def dbas_case(case):
    """make_case's inputs with the tape re-rolled from an offset b_0 (computed once, left unchanged)."""
    from oracle.oracle import Oracle

    c = dict(make_case(*case))
    c["X"] = offset_b0(Oracle(np.float64), c["prob"].to_c(), c["X"], c["V"], case[5])
    assert np.array_equal(c["X"][..., :3], make_case(*case)["X"][..., :3])
    return c


@functools.lru_cache(maxsize=None)
def oracle_dbas(case, tag):
    """The three oracle builds' rows of an offset case, computed once: per build the DBaS rows, the x0 / obstacle rows
    and the weight / reference rows."""
    c = dbas_case(case)
    npdt = np.float32 if tag == "f32" else np.float64
    a = _cast(c, npdt)
    sp, cc = c["prob"].to_c(), c["cost"].to_c()
    out = {"dbas": [], "geom": [], "rows": []}
    for o in oracles(npdt):
        out["dbas"].append(dbas_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"]))
        out["geom"].append(geom_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"]))
        out["rows"].append(layer_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"], a["Xref"], a["Uref"]))
    return out


def composition_dbas(c, tdt, dev):
    """The route to the same rows that needs none of the new code: ddp_sensitivity with array upper gradients and
    delta_lambda, then the formulas of tests/_layer_dbas.py as tensor operations in the tape's dtype."""
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core import ddp_sensitivity
    from diff_tube_mpc_strict_pt.core.barrier import barrier_and_derivative

    t = _dev_inputs(c, tdt, dev)
    prob = c["prob"]
    N = prob.horizon
    s = ddp_sensitivity(problem=prob, cost=c["cost"], X=t["X"], V=t["V"], upper_grad_x=t["gX"], upper_grad_u=t["gU"],
                        want_lambda=True, check=False)
    X, lam = t["X"], s.delta_lambda[..., 3]
    tab = torch.tensor([[o.center[0], o.center[1], o.radius] for o in prob.obstacles], dtype=tdt, device=dev)
    dx, dy = X[..., 0:1] - tab[:, 0], X[..., 1:2] - tab[:, 1]
    h = -torch.logsumexp(-prob.obs_beta * (dx * dx + dy * dy - tab[:, 2] * tab[:, 2]), -1) / prob.obs_beta
    Bv = barrier_and_derivative(h, kind=_abi.BARRIER_INVERSE, alpha=prob.dbas_alpha, eps=prob.dbas_eps, want_B=True,
                                want_dB=False)[0]
    a = max(prob.dbas_alpha, prob.dbas_eps)
    dBa = torch.where(h >= a, torch.zeros_like(h), -3.0 * (h - a) ** 2 / a ** 4)
    zero = torch.zeros_like(lam[:, :1])
    co = torch.cat([zero, lam[:, 1:]], 1) - prob.dbas_gamma * torch.cat([lam[:, 1:], zero], 1)
    ga = (co * dBa).sum(1, keepdim=True)
    gg = -(lam[:, 1:] * (Bv[:, :N] - X[:, :N, 3])).sum(1, keepdim=True)
    return {"alpha": ga.cpu().numpy(), "gamma": gg.cpu().numpy()}


def fused_dbas(c, tdt, dev, prob=None, want_x0=True, want_obstacles=True, **kw):
    from diff_tube_mpc_strict_pt.core import solve_backward

    t = _dev_inputs(c, tdt, dev)
    g = solve_backward(problem=prob or c["prob"], cost=c["cost"], X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"],
                       X_ref=t["Xref"], U_ref=t["Uref"], check=False, want_x0=want_x0, want_obstacles=want_obstacles,
                       want_dbas=True, **kw)
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    assert g.dbas.shape == (t["X"].shape[0], 2)
    return {"alpha": host(g.dbas[:, 0:1]), "gamma": host(g.dbas[:, 1:2]), "x0": host(g.x0),
            "obstacles": host(g.obstacles), "status": host(g.status), "weights": host(g.weights),
            "target": host(g.target), "X_ref": host(g.X_ref), "U_ref": host(g.U_ref)}


def worst_informative(got, builds, base, keys=KEYS):
    """Worst error of `got` among the finite, informative trajectories, per key (no assertion)."""
    fin = np.all([b["finite"] for b in builds], axis=0)
    n = int(fin.sum())
    out = {}
    for key in keys:
        if not n:
            out[key] = 0.0
            continue
        _, e, s = agreement(np.asarray(got[key], np.float64)[fin].reshape(n, -1),
                            [np.asarray(b[key], np.float64)[fin].reshape(n, -1) for b in builds], base)
        inf = (s <= 1e-2) & np.isfinite(e)
        out[key] = float(e[inf].max()) if inf.any() else 0.0
    return out


def gate(got, builds, base, label, keys=KEYS):
    """tests/test_gpu_layer_geom.gate's conditions on the given keys: trajectories on which a build is non-finite are
    left out (at most 5 %), those whose build spread exceeds 1e-2 are uninformative (at most 20 %), the rest lie
    within max(base, 10 x spread) of one of the builds.  Returns the worst informative error per key."""
    fin = np.all([b["finite"] for b in builds], axis=0)
    B, n = len(fin), int(fin.sum())
    assert (~fin).sum() <= 0.05 * B, (label, "non-finite oracle rows", int((~fin).sum()), B)
    worst = {}
    for key in keys:
        g = np.asarray(got[key], np.float64)[fin].reshape(n, -1)
        _, e, s = agreement(g, [np.asarray(b[key], np.float64)[fin].reshape(n, -1) for b in builds], base)
        inf = s <= 1e-2
        w = float(e[inf].max()) if inf.any() else 0.0
        worst[key] = w
        print(f"[layer dbas {label}] {key}: worst error {w:.3g} (spread max "
              f"{float(s[inf].max()) if inf.any() else 0:.3g}), {int((~fin).sum())} non-finite, "
              f"{int((~inf).sum())} uninformative of {B}; largest |row| "
              f"{float(np.abs(builds[0][key][fin]).max()) if n else 0:.3g}, non-zero rows "
              f"{int((np.abs(builds[0][key][fin]).reshape(n, -1).max(1) > 0).sum()) if n else 0}")
        assert (~inf).sum() <= 0.2 * B, (label, key, "uninformative", int((~inf).sum()), B)
        assert np.isfinite(g[inf]).all(), (label, key, "device row not finite")
        ok = e[inf] <= np.maximum(base, 10.0 * s[inf])
        assert ok.all(), (label, key, float(e[inf][~ok].max()), np.nonzero(~ok)[0][:8].tolist())
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_vs_oracle_f32(dev, oracle_lib, case):
    c = dbas_case(case)
    ob = oracle_dbas(case, "f32")
    builds = ob["dbas"]
    label = IDS[CASES.index(case)]
    cw = worst_informative(composition_dbas(c, torch.float32, dev), builds, BASE_F32)
    print(f"[layer dbas {label}] composition on the device: worst error alpha {cw['alpha']:.3g}, "
          f"gamma {cw['gamma']:.3g}")
    got = fused_dbas(c, torch.float32, dev)
    fw = worst_informative(got, builds, BASE_F32)
    print(f"[layer dbas {label}] fused kernel: worst error alpha {fw['alpha']:.3g}, gamma {fw['gamma']:.3g}")
    fin = np.all([b["finite"] for b in builds], axis=0)
    gate(got, builds, BASE_F32, label)
    assert (got["status"][fin] == 0).all(), (label, got["status"])
    # x0 / obstacles of the same launch, and the rows dtmpc_solve_backward writes as well: their own gates and bases
    gw = gate(got, ob["geom"], GEOM_BASE_F32, label + " (dbas entry)", GEOM_KEYS)
    ow = layer_gate(got, ob["rows"], LAYER_BASE_F32, label + " (dbas entry)")
    print(f"[layer dbas {label}] fused kernel, x0 {gw['x0']:.3g}, obstacles {gw['obstacles']:.3g}, weight / reference "
          f"rows {ow:.3g}")


def test_rows_vs_oracle_f64_composition(dev, oracle_lib):
    """f64 takes the composition path of solve_backward."""
    case = CASES[3]
    got = fused_dbas(dbas_case(case), torch.float64, dev)
    ob = oracle_dbas(case, "f64")
    gate(got, ob["dbas"], BASE_F64, IDS[3] + "-f64")
    gate(got, ob["geom"], BASE_F64, IDS[3] + "-f64", GEOM_KEYS)
    assert np.abs(ob["dbas"][0]["gamma"]).max() > 0


@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[5]], ids=[IDS[2], IDS[4], IDS[5]])
def test_alpha_row_is_exactly_zero_where_no_tape_row_is_relaxed(dev, oracle_lib, case):
    """dBa(h) = 0 for h >= a: a trajectory none of whose f32 tape rows has h < a + 1e-3 (1 + |h|) has an alpha row
    of exactly 0.0 (the margin covers the f32 evaluation of h)."""
    c = dbas_case(case)
    a32 = _cast(c, np.float32)
    sp = c["prob"].to_c()
    X = a32["X"].astype(np.float64)
    h = oracle_lib.Oracle(np.float64).h_eval(sp, X[..., 0].reshape(-1), X[..., 1].reshape(-1))[0].reshape(X.shape[:2])
    a = max(sp.dbas_alpha, sp.dbas_eps)
    clear = ~(h < a + 1e-3 * (1.0 + np.abs(h))).any(1)
    got = fused_dbas(c, torch.float32, dev, want_x0=False, want_obstacles=False)
    ok = clear & (got["status"] == 0)
    assert ok.sum() > 0 and (~clear).sum() > 0, (int(ok.sum()), int((~clear).sum()))
    assert (got["alpha"][ok, 0] == 0.0).all()
    assert (got["alpha"][~clear, 0] != 0.0).any()


def test_alpha_below_eps_has_a_zero_row(dev):
    """alpha < eps: alpha_eff = eps does not depend on alpha, d max / d alpha = 0 on the host."""
    c = dbas_case(CASES[3])
    prob = dataclasses.replace(c["prob"], dbas_alpha=0.5 * c["prob"].dbas_eps)
    got = fused_dbas(c, torch.float32, dev, prob=prob)
    assert (got["alpha"] == 0.0).all() and got["alpha"].shape == (c["X"].shape[0], 1)
    got64 = fused_dbas(c, torch.float64, dev, prob=prob)
    assert (got64["alpha"] == 0.0).all()


def test_refusals_on_the_device(dev):
    from diff_tube_mpc_strict_pt.core import solve_backward

    c = dbas_case(CASES[3])
    for tdt in (torch.float32, torch.float64):
        t = _dev_inputs(c, tdt, dev)
        kw = dict(X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"], X_ref=t["Xref"], U_ref=t["Uref"], check=False)
        for over in (dict(obs_aggregation="min"), dict(barrier_type="log")):
            with pytest.raises(ValueError, match="DBaS rows need smooth-min aggregation and the relaxed inverse"):
                solve_backward(problem=dataclasses.replace(c["prob"], **over), cost=c["cost"], want_dbas=True, **kw)
        with pytest.raises(ValueError, match="wrap_angle"):
            solve_backward(problem=c["prob"], cost=dataclasses.replace(c["cost"], wrap_angle=True), want_dbas=True, **kw)


# ---------------------------------------------------------------------------------------------------------------
# the raw entry point
def raw_dbas(c, dev, scenes=None, fill=None, gX=None, sl=None, prob=None, cost=None, x0=True, obs=True, wt=None):
    """One dtmpc_solve_backward_dbas call on SoA tensors made here (the arguments of test_gpu_layer_geom.raw_geom; wt:
    a [9, B] weights tensor of the whole case or None; fill: a float or a tensor the workspace is filled with) -> dict
    of host arrays in the ABI layout."""
    from diff_tube_mpc_strict_pt import _abi, _lib
    from diff_tube_mpc_strict_pt.core.ddp import to_soa

    lib = _lib.load()
    prob, cost = prob or c["prob"], cost or c["cost"]
    sl = slice(None) if sl is None else sl
    f32 = torch.float32
    a = {k: (None if c[k] is None else to_soa(_t(c[k][sl], f32, dev))) for k in ("X", "V", "gX", "gU", "Xref", "Uref")}
    if gX is not None:
        a["gX"] = to_soa(_t(gX[sl], f32, dev))
    if wt is not None:
        wt = wt[:, sl].contiguous()
    N, B, M = prob.horizon, a["X"].shape[2], len(prob.obstacles)
    track = cost.kind == "track"
    kw = dict(dtype=f32, device=dev)
    gw = torch.full((9, B), 7.0, **kw)
    gt = None if track else torch.full((3, B), 7.0, **kw)
    gxr = torch.full((N + 1, 3, B), 7.0, **kw) if track else None
    gur = torch.full((N, 2, B), 7.0, **kw) if track else None
    gx0 = torch.full((4, B), 7.0, **kw) if x0 else None
    gob = torch.full((3 * M, B), 7.0, **kw) if obs else None
    gdb = torch.full((2, B), 7.0, **kw)
    wb = lib.dtmpc_solve_backward_dbas_workspace_bytes(_abi.F32, N, B)
    assert wb == N * 100 * B
    if fill is None:
        work = torch.zeros(wb // 4, **kw)
    elif isinstance(fill, torch.Tensor):
        work = fill.reshape(-1).repeat(wb // 4 // fill.numel() + 1)[:wb // 4].contiguous()
    else:
        work = torch.full((wb // 4,), fill, **kw)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    sp, cc = prob.to_c(), cost.to_c()
    rc = lib.dtmpc_solve_backward_dbas(_abi.F32, C.byref(sp), C.byref(cc), B, p(a["X"]), p(a["V"]), p(a["Xref"]),
                                       p(a["Uref"]), p(scenes), p(wt), p(a["gX"]), p(a["gU"]), p(gw), p(gt), p(gxr),
                                       p(gur), p(gx0), p(gob), p(gdb), p(work), wb, p(status), None)
    assert rc == 0, lib.dtmpc_last_error()
    torch.cuda.synchronize()
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in
           (("gw", gw), ("gt", gt), ("gxr", gxr), ("gur", gur), ("gx0", gx0), ("gob", gob), ("gdb", gdb),
            ("status", status))}
    out["work"] = work
    return out


def _same_dbas(a, b, cols=None, keys=("gx0", "gob", "gdb")):
    _same(a, b, cols)
    for k in keys:
        x, y = (a[k], b[k]) if cols is None else (a[k][..., cols], b[k][..., cols])
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), k


@pytest.mark.parametrize("case", [CASES[4], CASES[5], CASES[3], CASES[2]], ids=[IDS[4], IDS[5], IDS[3], IDS[2]])
def test_reuse_and_independence(dev, case):
    from diff_tube_mpc_strict_pt import _abi

    c = dbas_case(case)
    r0 = raw_dbas(c, dev)
    assert (r0["status"] == 0).sum() > 0
    _same_dbas(r0, raw_dbas(c, dev))
    _same_dbas(r0, raw_dbas(c, dev, fill=float("nan")))
    _same_dbas(r0, raw_dbas(c, dev, fill=3e38))
    # a workspace that holds another case's content
    other = raw_dbas(dbas_case(CASES[9]), dev)["work"]
    _same_dbas(r0, raw_dbas(c, dev, fill=other))
    # the outputs asked for: g_x0 / g_obs passed or NULL
    rx, ro, rn = raw_dbas(c, dev, obs=False), raw_dbas(c, dev, x0=False), raw_dbas(c, dev, x0=False, obs=False)
    assert rx["gob"] is None and ro["gx0"] is None and rn["gx0"] is None and rn["gob"] is None
    _same_dbas(r0, rx, keys=("gx0", "gdb"))
    _same_dbas(r0, ro, keys=("gob", "gdb"))
    _same_dbas(r0, rn, keys=("gdb",))
    for r in (rx, ro, rn):
        assert np.array_equal(r["status"], r0["status"])
    assert not (r0["gdb"] == 7.0).any() and not (r0["gx0"] == 7.0).any()
    assert (r0["gdb"][1] != 0).any()
    # trajectory i of the batch against the B = 1 launch on it
    B, N = c["X"].shape[0], c["prob"].horizon
    for i in sorted({0, 1, 31, 63, 64, B - 1} & set(range(B))):
        ri = raw_dbas(c, dev, sl=slice(i, i + 1))
        for k in ("gw", "gt", "gxr", "gur", "gx0", "gob", "gdb"):
            if ri[k] is not None:
                assert np.array_equal(ri[k][..., 0].view(np.int32), r0[k][..., i].view(np.int32)), (i, k)
        assert ri["status"][0] == r0["status"][i]
    # a NaN in one trajectory's gX flags that one only (the two new sums are part of the status)
    bad = int(np.nonzero(~c["on"][:, N - 1, 0])[0][B // 4])
    gX = c["gX"].copy()
    gX[bad, N, 0] = np.nan
    r1 = raw_dbas(c, dev, gX=gX)
    assert r1["status"][bad] == _abi.ST_NONFINITE
    others = np.arange(B) != bad
    assert (r1["status"][others] == r0["status"][others]).all()
    _same_dbas(r0, r1, cols=others)
    # ... and one that reaches lam alone: the barrier component of the terminal gradient
    gX = c["gX"].copy()
    gX[bad, N, 3] = np.nan
    r2 = raw_dbas(c, dev, gX=gX)
    assert r2["status"][bad] == _abi.ST_NONFINITE and (r2["status"][others] == r0["status"][others]).all()
    _same_dbas(r0, r2, cols=others)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_against_the_geom_entry(dev, case):
    """Measured, not asserted: whether the rows dtmpc_solve_backward_geom also writes are bitwise the new entry's."""
    from test_gpu_layer_geom import raw_geom

    c = dbas_case(case)
    a, b = raw_dbas(c, dev), raw_geom(c, dev)
    same = {k: bool(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)))
            for k in ("gw", "gt", "gxr", "gur", "gx0", "gob") if a[k] is not None}
    print(f"[layer dbas {IDS[CASES.index(case)]}] rows bitwise dtmpc_solve_backward_geom's: {same}")
    assert np.array_equal(a["status"], b["status"])


def test_scenes_and_weights(dev):
    """Per-trajectory scenes and weights, a few sets at B = 65: B copies of the shared table / of the cost's own weights
    are the shared launch, bitwise; with distinct sets the per-trajectory launch is, set by set, bitwise the shared
    launch on that set's own problem and cost."""
    from diff_tube_mpc_strict_pt.core import CircleObstacle, pack_scenes

    for case in (CASES[9], CASES[3]):
        c = dbas_case(case)
        prob, cost = c["prob"], c["cost"]
        B, M = c["X"].shape[0], len(prob.obstacles)
        assert B == 65
        tab = np.array([[o.center[0], o.center[1], o.radius] for o in prob.obstacles])
        sets = weight_sets(cost)
        r0 = raw_dbas(c, dev)
        shared_sc = pack_scenes(prob, np.broadcast_to(tab, (B, M, 3)), np.broadcast_to(np.array(cost.target), (B, 3)),
                                dtype=torch.float32, device=dev)
        _same_dbas(r0, raw_dbas(c, dev, scenes=shared_sc))
        own = pack(sets, np.zeros(B, np.int64), dev)
        ru = raw_dbas(c, dev, wt=own)
        print(f"[layer dbas {IDS[CASES.index(case)]}] uniform weights bitwise the shared cost's: "
              f"{bool(np.array_equal(ru['gdb'].view(np.int32), r0['gdb'].view(np.int32)))}")
        # S scene sets x W weight sets, trajectory i has scene i % S and weights i % W (every pair occurs)
        S = 4
        rng = np.random.default_rng(5)
        obs_s = tab[None] + np.concatenate([rng.uniform(-0.5, 0.5, (S, M, 2)), rng.uniform(-0.2, 0.3, (S, M, 1))], 2)
        tg_s = np.array(cost.target) + rng.uniform(-1.0, 1.0, (S, 3))
        ks, kw = np.arange(B) % S, assignment(B)
        sc = pack_scenes(prob, obs_s[ks], tg_s[ks], dtype=torch.float32, device=dev)
        wt = pack(sets, kw, dev)
        rs = raw_dbas(c, dev, scenes=sc, wt=wt)
        rs_sc = raw_dbas(c, dev, scenes=sc)
        assert not np.array_equal(rs["gdb"], r0["gdb"]) and not np.array_equal(rs_sc["gdb"], rs["gdb"])
        for s_ in range(S):
            pi = dataclasses.replace(prob, obstacles=tuple(CircleObstacle(center=(float(o[0]), float(o[1])),
                                                                          radius=float(o[2])) for o in obs_s[s_]))
            ci = dataclasses.replace(cost, target=tuple(float(v) for v in tg_s[s_]))
            cols = ks == s_
            rsh = raw_dbas(c, dev, prob=pi, cost=ci)  # the shared launch on scene set s_, the cost's own weights
            for k in ("gdb", "gx0", "gob", "gw"):
                assert np.array_equal(rsh[k][..., cols].view(np.int32), rs_sc[k][..., cols].view(np.int32)), (s_, k)
            for w_ in range(len(sets)):
                cols = (ks == s_) & (kw == w_)
                if not cols.any():
                    continue
                # the shared launch (no scenes, no weights array) on this pair's own problem and cost
                rsw = raw_dbas(c, dev, prob=pi, cost=cost_of(ci, sets[w_]))
                assert np.array_equal(rsw["gdb"][..., cols].view(np.int32), rs["gdb"][..., cols].view(np.int32)), (s_, w_)
                assert np.array_equal(rsw["status"][cols], rs["status"][cols])


def test_python_composes_with_scenes_weights_and_the_other_rows(dev):
    """solve_backward(want_dbas=) with scenes=, weights=, want_x0, want_obstacles in any combination gives the same
    dbas rows as the raw entry, and the other rows it returns are those of the same call without want_dbas up to the
    kernel family (reported)."""
    from diff_tube_mpc_strict_pt.core import pack_scenes, solve_backward

    c = dbas_case(CASES[9])
    prob, cost = c["prob"], c["cost"]
    B, M = c["X"].shape[0], len(prob.obstacles)
    tab = np.array([[o.center[0], o.center[1], o.radius] for o in prob.obstacles])
    rng = np.random.default_rng(7)
    obs = tab[None] + rng.uniform(-0.3, 0.3, (B, M, 3))
    tg = np.array(cost.target) + rng.uniform(-1.0, 1.0, (B, 3))
    sc = pack_scenes(prob, obs, tg, dtype=torch.float32, device=dev)
    wt = pack(weight_sets(cost), assignment(B), dev)
    t = _dev_inputs(c, torch.float32, dev)
    kw = dict(problem=prob, cost=cost, X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"], check=False)
    for scenes, weights in ((None, None), (sc, None), (None, wt), (sc, wt)):
        raw = raw_dbas(c, dev, scenes=scenes, wt=weights)
        for x0, ob in ((False, False), (True, False), (False, True), (True, True)):
            g = solve_backward(**kw, scenes=scenes, weights=weights, want_x0=x0, want_obstacles=ob, want_dbas=True)
            assert np.array_equal(g.dbas.cpu().numpy().T.view(np.int32), raw["gdb"].view(np.int32))
            assert (g.x0 is not None) == x0 and (g.obstacles is not None) == ob
            assert np.array_equal(g.weights.cpu().numpy().T.view(np.int32), raw["gw"].view(np.int32))
            if x0:
                assert np.array_equal(g.x0.cpu().numpy().T.view(np.int32), raw["gx0"].view(np.int32))
        assert solve_backward(**kw, scenes=scenes, weights=weights).dbas is None


# ---------------------------------------------------------------------------------------------------------------
# the autograd layer
def _perturbed_setup(dev, B=9, N=12, gamma=0.3):
    """_layer_setup with alpha = 0.05, the given gamma, every other start position on the rim of the first obstacle
    (|h| of a few 1e-2: tape rows on the relaxed branch, so the alpha rows are not all zero) and a start barrier state
    off its position's barrier."""
    from diff_tube_mpc_strict_pt.core import dbas_init

    st, prob, cfg, x0, V0, wX, wV = _layer_setup(dev, B=B, N=N)
    prob = dataclasses.replace(prob, dbas_alpha=0.05, dbas_gamma=gamma)
    g = torch.Generator().manual_seed(12)
    ob = prob.obstacles[0]
    ang = 3.4 + 1.2 * torch.rand(B, generator=g)  # the side that faces the start corner
    d = ob.radius * (1.0 + 0.04 * torch.rand(B, generator=g) - 0.015)
    rim = torch.stack([ob.center[0] + d * torch.cos(ang), ob.center[1] + d * torch.sin(ang)], 1).to(x0)
    x = x0[:, :3].clone()
    x[0::2, :2] = rim[0::2]
    x0 = torch.cat([x, dbas_init(prob, x)[:, None]], 1)
    x0[:, 3] = x0[:, 3] * (0.5 + torch.rand(B, generator=g)).to(dev) + (0.4 * torch.rand(B, generator=g) - 0.2).to(dev)
    return st, prob, cfg, x0, V0, wX, wV


def test_layer_dbas_gradients_are_the_row_sums(dev):
    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve, ilqr_solve, solve_backward

    st, prob, cfg, x0, V0, wX, wV = _perturbed_setup(dev)
    Q, R, Qf, qb = _weights(dev)
    tg = torch.tensor(TARGET, device=dev)
    al = torch.tensor(0.05, device=dev, requires_grad=True)
    ga = torch.tensor([0.3], device=dev, requires_grad=True)
    # the tensors' values replace the problem's floats: a problem with other values gives the same solve
    other = dataclasses.replace(prob, dbas_alpha=0.2, dbas_gamma=0.0)
    res = diff_ilqr_solve(problem=other, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0, target=tg,
                          dbas_alpha=al, dbas_gamma=ga)
    cost = QuadraticCost(kind="target", target=TARGET, **WEIGHTS)
    pv = dataclasses.replace(prob, dbas_alpha=float(al.detach().cpu()), dbas_gamma=float(ga.detach().cpu()[0]))
    ref = ilqr_solve(problem=pv, cost=cost, cfg=cfg, x0=x0, V_init=V0)
    assert torch.equal(res.X.detach(), ref.X) and torch.equal(res.V.detach(), ref.V)
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    g = solve_backward(problem=pv, cost=cost, X=ref.X, V=ref.V, grad_X=wX, grad_V=wV, want_dbas=True)
    assert (g.status == 0).all() and (res.backward_status() == 0).all()
    assert al.grad.shape == () and ga.grad.shape == (1,)
    assert g.dbas[:, 1].abs().sum() > 0
    assert _sum_of(al.grad.reshape(1), g.dbas[:, 0:1]) and _sum_of(ga.grad, g.dbas[:, 1:2])
    assert _sum_of(Q.grad, g.weights[:, 0:3]) and _sum_of(qb.grad.reshape(1), g.weights[:, 8:9])
    # only one of the two requires grad: the other gets none, the one the same value
    al2 = torch.tensor(0.05, device=dev)
    ga2 = torch.tensor(0.3, device=dev, requires_grad=True)
    r2 = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0, target=tg,
                         dbas_alpha=al2, dbas_gamma=ga2)
    ((r2.X * wX).sum() + (r2.V * wV).sum()).backward()
    assert al2.grad is None and torch.equal(ga2.grad.reshape(1), ga.grad)


def test_layer_dbas_flagged_trajectory_contributes_zero(dev):
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core import diff_ilqr_solve, solve_backward, QuadraticCost

    st, prob, cfg, x0, V0, wX, wV = _perturbed_setup(dev)
    Q, R, Qf, qb = _weights(dev)
    al = torch.tensor(0.05, device=dev, requires_grad=True)
    ga = torch.tensor(0.3, device=dev, requires_grad=True)
    res = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0,
                          target=torch.tensor(TARGET, device=dev), dbas_alpha=al, dbas_gamma=ga)
    wX = wX.clone()
    wX[2, 3, 1] = float("nan")
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    flags = res.backward_status()
    assert flags[2] == _abi.ST_NONFINITE and int((flags != 0).sum()) == 1
    cost = QuadraticCost(kind="target", target=TARGET, **WEIGHTS)
    g = solve_backward(problem=prob, cost=cost, X=res.X.detach(), V=res.V.detach(), grad_X=wX, grad_V=wV,
                       want_dbas=True, check=False)
    keep = torch.arange(x0.shape[0], device=dev) != 2
    assert torch.isfinite(al.grad) and torch.isfinite(ga.grad) and ga.grad.abs() > 0
    assert _sum_of(al.grad.reshape(1), g.dbas[keep, 0:1]) and _sum_of(ga.grad.reshape(1), g.dbas[keep, 1:2])


def test_layer_raw_parameters_vs_ift_gradient(dev, oracle_lib):
    """alpha = softplus(raw) + 1e-6 and gamma = tanh(raw) in torch: raw.grad is oracle.ift_gradient's raw columns
    (DTMPC_P_ALPHA, DTMPC_P_GAMMA) summed over the batch, at the tape the solve returned, for the three f32 builds.
    The bound is the new base times the largest magnitude of the reference sum (not base per row)."""
    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve

    st, prob, cfg, x0, V0, wX, wV = _perturbed_setup(dev, B=65, N=12)
    Q, R, Qf, qb = _weights(dev)
    raw_a = torch.tensor(float(np.log(np.expm1(0.05 - 1e-6))), device=dev, requires_grad=True)
    raw_g = torch.tensor(float(np.arctanh(0.3)), device=dev, requires_grad=True)
    al = torch.nn.functional.softplus(raw_a) + 1e-6
    ga = torch.tanh(raw_g)
    res = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0,
                          target=torch.tensor(TARGET, device=dev), dbas_alpha=al, dbas_gamma=ga)
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    assert (res.backward_status() == 0).all()
    got = np.array([float(raw_a.grad.cpu()), float(raw_g.grad.cpu())])
    pv = dataclasses.replace(prob, dbas_alpha=float(al.detach().cpu()), dbas_gamma=float(ga.detach().cpu()))
    sp, cc = pv.to_c(), QuadraticCost(kind="target", target=TARGET, **WEIGHTS).to_c()
    th = np.zeros(12)
    th[9], th[10], th[11] = float(raw_a.detach().cpu()), float(raw_g.detach().cpu()), -800.0  # tightening off
    X, V = res.X.detach().cpu().numpy(), res.V.detach().cpu().numpy()
    gX, gV = wX.cpu().numpy(), wV.cpu().numpy()
    refs = []
    for o in oracles(np.float32):
        dX, dV, dlam, _ = o.ddp_sensitivity_upper(sp, cc, X, V, gX, gV)
        gth = o.ift_gradient(sp, cc, th, X, V, dX, dV, dlam)[0].astype(np.float64)
        assert np.isfinite(gth[:, 9:11]).all()
        refs.append(gth[:, 9:11].sum(0))
    refs = np.stack(refs)
    scale = np.abs(refs).max(0)
    err = np.abs(refs - got).min(0)
    spread = np.abs(refs[1:] - refs[0]).max(0)
    print(f"[layer dbas raw] raw.grad {got}, oracle builds {refs.tolist()}, error {err / scale} of the reference sum "
          f"(build spread {spread / scale})")
    assert (scale > 0).all()
    assert (err <= BASE_F32 * scale).all(), (err / scale, BASE_F32)


def test_layer_chained_solves_reach_gamma(dev):
    """Plan, step the plant with a perturbation of b, plan again: one backward() delivers a non-zero, finite
    gamma.grad (the second solve starts from a barrier state that is not the barrier of its position)."""
    from diff_tube_mpc_strict_pt.core import diff_ilqr_solve
    from diff_tube_mpc_strict_pt.core.barrier import DBaSConfig, dbas_step
    from diff_tube_mpc_strict_pt.core.systems.dubins import DubinsConfig, dubins_step
    from diff_tube_mpc_strict_pt.core.systems.dubins_obstacles import h_multi_circle_obstacles

    st, prob, cfg, x0, V0, wX, wV = _layer_setup(dev, B=65, N=3)
    prob = dataclasses.replace(prob, dbas_alpha=0.05, dbas_gamma=0.3)
    tg = torch.tensor(TARGET, device=dev)
    dub = DubinsConfig(dt=prob.dt)
    dbc = DBaSConfig(barrier_type="inverse", alpha=prob.dbas_alpha, gamma=prob.dbas_gamma, eps=prob.dbas_eps)
    f = lambda x, u: dubins_step(x, u, cfg=dub)  # noqa: E731
    h = lambda x: h_multi_circle_obstacles(x, obstacles=list(prob.obstacles), beta=prob.obs_beta)  # noqa: E731
    g = torch.Generator().manual_seed(6)
    db = (0.1 * torch.randn(x0.shape[0], generator=g)).to(dev)

    def plant(xh, u):  # core.systems dynamics with the barrier state, b disturbed
        xn, bn = dbas_step(x_k=xh[:, :3], u_k=u, b_k=xh[:, 3], f=f, h=h, cfg=dbc)
        return torch.cat([xn, (bn + db)[:, None]], 1)

    Q, R, Qf, qb = _weights(dev)
    al = torch.tensor(0.05, device=dev, requires_grad=True)
    ga = torch.tensor(0.3, device=dev, requires_grad=True)
    kw = dict(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, V_init=V0, target=tg, dbas_alpha=al,
              dbas_gamma=ga)
    r1 = diff_ilqr_solve(x0=x0, **kw)
    r2 = diff_ilqr_solve(x0=plant(r1.X[:, 0], r1.V[:, 0]), wrt=("x0",), **kw)
    ((r2.X * wX).sum() + (r2.V * wV).sum()).backward()
    assert (r1.backward_status() == 0).all() and (r2.backward_status() == 0).all()
    assert torch.isfinite(ga.grad) and ga.grad.abs() > 0
    assert torch.isfinite(al.grad)
