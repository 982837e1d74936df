"""The differentiable solve's rows w.r.t. the start state and the obstacle circles on the device
(dtmpc_solve_backward_geom, core.solve_backward(want_x0=, want_obstacles=), diff_ilqr_solve(wrt=)): against the oracle
yardstick (tests/_layer_geom.py, itself held to the reference and to finite differences by
tests/test_layer_geom_yardstick.py), independence of the workspace's content, of the requested outputs and of the
other trajectories, per-trajectory scenes, and the autograd layer, chained solves included.

The rows both entries write (g_w, g_target, g_xref, g_uref) are NOT bitwise dtmpc_solve_backward's: measured on the
device, the new kernels' rows differ from the old kernels' in the last few bits (the compiler contracts some a b + c d
sums the other way round in the larger kernel; the sites were not pinned with explicit fmas here).
So those rows of the new entry stand under tests/test_gpu_layer.py's oracle gate with its own base instead.

The cases are tests/test_gpu_layer.py's twelve (N in {1, 2, 3, 50}, B in {1, 65, 257}, M in {1, 5, 8}, both kinds,
gamma 0 / 0.3, alpha 0.05), and the gate is its gate, per case and per key (x0, obstacles).

The f32 base is measured by that file's rule for BASE_F32: the parent-buildable composition on the device
(ddp_sensitivity with array upper gradients and want_lambda in f32, then the formulas as tensor operations,
composition_geom below) on the same cases against the same three oracle builds; the base is twice its worst error on
the informative trajectories.  Measured (profiles/r12/layer_geom_errors.txt has the per-case table):
the composition's worst error is 1.36e-2 of a row's scale (N3-B257-M1-target-g0.3, the x0 rows, a trajectory whose
build spread is 7e-3; 1.02e-2 on that case's obstacle rows; 4.5e-3 at N50-B257-M5-target-g0.0, 1.5e-3 at both other
N = 50 cases with M >= 5, under 3.2e-4 in the eight remaining cases), so the base is 2.72e-2.  The fused kernel's own
worst error on the same cases, for the record: 1.34e-2 (the same trajectory), and at most 2.1 times the composition's
in every case with an error above 1e-4.  The f32 oracle builds themselves sit up to 1.4e-2 from the f64 oracle on
these rows."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from _common import agreement, oracles
from _layer_geom import geom_rows
from test_gpu_layer import BASE_F32 as LAYER_BASE_F32
from test_gpu_layer import (BASE_F64, CASES, IDS, TARGET, WEIGHTS, _cast, _dev_inputs, _layer_setup, _same, _sum_of, _t,
                            _weights, make_case, oracle_rows)
from test_gpu_layer import gate as layer_gate

pytestmark = pytest.mark.gpu

COMPOSITION_WORST = 1.36e-2
BASE_F32 = 2.0 * COMPOSITION_WORST
KEYS = ("x0", "obstacles")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def oracle_geom(case, tag):
    """The three oracle builds' rows of a case, computed once."""
    c = make_case(*case)
    npdt = np.float32 if tag == "f32" else np.float64
    a = _cast(c, npdt)
    sp, cc = c["prob"].to_c(), c["cost"].to_c()
    return [geom_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"]) for o in oracles(npdt)]


def composition_geom(c, tdt, dev):
    """The route to the same rows that needs none of the new code: ddp_sensitivity with array upper gradients and
    delta_lambda, then the formulas of tests/_layer_geom.py as tensor operations in the tape's dtype."""
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core import ddp_sensitivity
    from diff_tube_mpc_strict_pt.core.barrier import barrier_and_derivative

    t = _dev_inputs(c, tdt, dev)
    prob = c["prob"]
    s = ddp_sensitivity(problem=prob, cost=c["cost"], X=t["X"], V=t["V"], upper_grad_x=t["gX"], upper_grad_u=t["gU"],
                        want_lambda=True, check=False)
    X, lam = t["X"], s.delta_lambda[..., 3]
    tab = torch.tensor([[o.center[0], o.center[1], o.radius] for o in prob.obstacles], dtype=tdt, device=dev)
    dx, dy = X[..., 0:1] - tab[:, 0], X[..., 1:2] - tab[:, 1]
    z = -prob.obs_beta * (dx * dx + dy * dy - tab[:, 2] * tab[:, 2])
    w = torch.softmax(z, -1)
    h = -torch.logsumexp(z, -1) / prob.obs_beta
    D = barrier_and_derivative(h, kind=_abi.BARRIER_INVERSE, alpha=prob.dbas_alpha, eps=prob.dbas_eps, want_B=False,
                               want_dB=True)[1]
    zero = torch.zeros_like(lam[:, :1])
    cw = (D * (torch.cat([zero, lam[:, 1:]], 1) - prob.dbas_gamma * torch.cat([lam[:, 1:], zero], 1)))[..., None] * w
    obs = torch.stack([(cw * (-2 * dx)).sum(1), (cw * (-2 * dy)).sum(1), -cw.sum(1) * (2 * tab[:, 2])], 2)
    return {"x0": s.delta_lambda[:, 0].cpu().numpy(), "obstacles": obs.cpu().numpy()}


def fused_geom(c, tdt, dev, **kw):
    from diff_tube_mpc_strict_pt.core import solve_backward

    t = _dev_inputs(c, tdt, dev)
    g = solve_backward(problem=c["prob"], cost=c["cost"], X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"],
                       X_ref=t["Xref"], U_ref=t["Uref"], check=False, want_x0=True, want_obstacles=True, **kw)
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return {"x0": host(g.x0), "obstacles": host(g.obstacles), "status": host(g.status), "weights": host(g.weights),
            "target": host(g.target), "X_ref": host(g.X_ref), "U_ref": host(g.U_ref)}


def worst_informative(got, builds, base):
    """Worst error of `got` among the finite, informative trajectories, per key (no assertion)."""
    fin = np.all([b["finite"] for b in builds], axis=0)
    n = int(fin.sum())
    out = {}
    for key in KEYS:
        if not n:
            out[key] = 0.0
            continue
        _, e, s = agreement(np.asarray(got[key], np.float64)[fin].reshape(n, -1),
                            [np.asarray(b[key], np.float64)[fin].reshape(n, -1) for b in builds], base)
        inf = (s <= 1e-2) & np.isfinite(e)
        out[key] = float(e[inf].max()) if inf.any() else 0.0
    return out


def gate(got, builds, base, label):
    """tests/test_gpu_layer.gate's conditions on the keys x0 and obstacles: trajectories on which a build is
    non-finite are left out (at most 5 %), those whose build spread exceeds 1e-2 are uninformative (at most 20 %),
    the rest lie within max(base, 10 x spread) of one of the builds.  Returns the worst informative error per key."""
    fin = np.all([b["finite"] for b in builds], axis=0)
    B, n = len(fin), int(fin.sum())
    assert (~fin).sum() <= 0.05 * B, (label, "non-finite oracle rows", int((~fin).sum()), B)
    worst = {}
    for key in KEYS:
        g = np.asarray(got[key], np.float64)[fin].reshape(n, -1)
        _, e, s = agreement(g, [np.asarray(b[key], np.float64)[fin].reshape(n, -1) for b in builds], base)
        inf = s <= 1e-2
        w = float(e[inf].max()) if inf.any() else 0.0
        worst[key] = w
        print(f"[layer geom {label}] {key}: worst error {w:.3g} (spread max "
              f"{float(s[inf].max()) if inf.any() else 0:.3g}), {int((~fin).sum())} non-finite, "
              f"{int((~inf).sum())} uninformative of {B}")
        assert (~inf).sum() <= 0.2 * B, (label, key, "uninformative", int((~inf).sum()), B)
        assert np.isfinite(g[inf]).all(), (label, key, "device row not finite")
        ok = e[inf] <= np.maximum(base, 10.0 * s[inf])
        assert ok.all(), (label, key, float(e[inf][~ok].max()), np.nonzero(~ok)[0][:8].tolist())
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_vs_oracle_f32(dev, oracle_lib, case):
    c = make_case(*case)
    builds = oracle_geom(case, "f32")
    label = IDS[CASES.index(case)]
    cw = worst_informative(composition_geom(c, torch.float32, dev), builds, BASE_F32)
    print(f"[layer geom {label}] composition on the device: worst error x0 {cw['x0']:.3g}, "
          f"obstacles {cw['obstacles']:.3g}")
    got = fused_geom(c, torch.float32, dev)
    fin = np.all([b["finite"] for b in builds], axis=0)
    fw = gate(got, builds, BASE_F32, label)
    assert (got["status"][fin] == 0).all(), (label, got["status"])
    print(f"[layer geom {label}] fused kernel: worst error x0 {fw['x0']:.3g}, obstacles {fw['obstacles']:.3g}")
    # the rows dtmpc_solve_backward writes as well, from the new entry: that entry's own gate and base
    ow = layer_gate(got, oracle_rows(case, "f32"), LAYER_BASE_F32, label + " (geom entry)")
    print(f"[layer geom {label}] fused kernel, weight / reference rows: worst error {ow:.3g}")


def test_rows_vs_oracle_f64_composition(dev, oracle_lib):
    """f64 takes the composition path of solve_backward."""
    case = CASES[3]
    got = fused_geom(make_case(*case), torch.float64, dev)
    gate(got, oracle_geom(case, "f64"), BASE_F64, IDS[3] + "-f64")


def test_obstacle_rows_refused_where_they_are_not_defined(dev):
    from diff_tube_mpc_strict_pt.core import pack_scenes, solve_backward

    c = make_case(*CASES[3])
    t = _dev_inputs(c, torch.float64, dev)
    kw = dict(cost=c["cost"], X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"], X_ref=t["Xref"], U_ref=t["Uref"],
              check=False)
    for over in (dict(obs_aggregation="min"), dict(barrier_type="log")):
        prob = dataclasses.replace(c["prob"], **over)
        with pytest.raises(ValueError, match="smooth-min aggregation and the relaxed inverse"):
            solve_backward(problem=prob, want_obstacles=True, **kw)
        g = solve_backward(problem=prob, want_x0=True, **kw)  # x0 rows come on every path
        assert g.x0.shape == (t["X"].shape[0], 4) and g.obstacles is None
    B, M = t["X"].shape[0], len(c["prob"].obstacles)
    sc = pack_scenes(c["prob"], np.ones((B, M, 3)), np.zeros((B, 3)), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="scenes need the fused kernel"):
        solve_backward(problem=c["prob"], want_obstacles=True, scenes=sc, **kw)


# ---------------------------------------------------------------------------------------------------------------
# the raw entry point
def raw_geom(c, dev, scenes=None, fill=None, gX=None, sl=None, prob=None, cost=None, x0=True, obs=True):
    """One dtmpc_solve_backward_geom call on SoA tensors made here (the arguments of test_gpu_layer.raw_backward;
    x0 / obs: whether g_x0 / g_obs are passed) -> dict of host arrays in the ABI layout."""
    from diff_tube_mpc_strict_pt import _abi, _lib
    from diff_tube_mpc_strict_pt.core.ddp import to_soa

    lib = _lib.load()
    prob, cost = prob or c["prob"], cost or c["cost"]
    sl = slice(None) if sl is None else sl
    f32 = torch.float32
    a = {k: (None if c[k] is None else to_soa(_t(c[k][sl], f32, dev))) for k in ("X", "V", "gX", "gU", "Xref", "Uref")}
    if gX is not None:
        a["gX"] = to_soa(_t(gX[sl], f32, dev))
    N, B, M = prob.horizon, a["X"].shape[2], len(prob.obstacles)
    track = cost.kind == "track"
    kw = dict(dtype=f32, device=dev)
    gw = torch.full((9, B), 7.0, **kw)
    gt = None if track else torch.full((3, B), 7.0, **kw)
    gxr = torch.full((N + 1, 3, B), 7.0, **kw) if track else None
    gur = torch.full((N, 2, B), 7.0, **kw) if track else None
    gx0 = torch.full((4, B), 7.0, **kw) if x0 else None
    gob = torch.full((3 * M, B), 7.0, **kw) if obs else None
    wb = lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, N, B)
    assert wb == N * 100 * B
    work = torch.zeros(wb // 4, **kw) if fill is None else torch.full((wb // 4,), fill, **kw)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    sp, cc = prob.to_c(), cost.to_c()
    rc = lib.dtmpc_solve_backward_geom(_abi.F32, C.byref(sp), C.byref(cc), B, p(a["X"]), p(a["V"]), p(a["Xref"]),
                                       p(a["Uref"]), p(scenes), p(a["gX"]), p(a["gU"]), p(gw), p(gt), p(gxr), p(gur),
                                       p(gx0), p(gob), p(work), wb, p(status), None)
    assert rc == 0, lib.dtmpc_last_error()
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in
            (("gw", gw), ("gt", gt), ("gxr", gxr), ("gur", gur), ("gx0", gx0), ("gob", gob), ("status", status))}


def _same_geom(a, b, cols=None, keys=("gx0", "gob")):
    _same(a, b, cols)
    for k in keys:
        x, y = (a[k], b[k]) if cols is None else (a[k][..., cols], b[k][..., cols])
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), k


@pytest.mark.parametrize("case", [CASES[4], CASES[5], CASES[3], CASES[2]], ids=[IDS[4], IDS[5], IDS[3], IDS[2]])
def test_reuse_and_independence(dev, case):
    c = make_case(*case)
    r0 = raw_geom(c, dev)
    assert (r0["status"] == 0).sum() > 0
    _same_geom(r0, raw_geom(c, dev))
    _same_geom(r0, raw_geom(c, dev, fill=float("nan")))
    _same_geom(r0, raw_geom(c, dev, fill=3e38))
    rx, ro = raw_geom(c, dev, obs=False), raw_geom(c, dev, x0=False)
    assert rx["gob"] is None and ro["gx0"] is None
    _same_geom(r0, rx, keys=("gx0",))
    _same_geom(r0, ro, keys=("gob",))
    assert np.array_equal(rx["status"], r0["status"]) and np.array_equal(ro["status"], r0["status"])
    assert not (r0["gx0"] == 7.0).any() and not (r0["gob"] == 7.0).all(0).any()
    B, N = c["X"].shape[0], c["prob"].horizon
    bad = int(np.nonzero(~c["on"][:, N - 1, 0])[0][B // 4])
    gX = c["gX"].copy()
    gX[bad, N, 0] = np.nan
    r1 = raw_geom(c, dev, gX=gX)
    from diff_tube_mpc_strict_pt import _abi

    assert r1["status"][bad] == _abi.ST_NONFINITE
    others = np.arange(B) != bad
    assert (r1["status"][others] == r0["status"][others]).all()
    _same_geom(r0, r1, cols=others)


def test_scenes(dev):
    """B copies of the shared table = scenes NULL, bitwise; distinct scenes: row i is the B = 1 call on trajectory
    i's own problem, bitwise."""
    from diff_tube_mpc_strict_pt.core import CircleObstacle, pack_scenes

    for case in (CASES[9], CASES[3]):
        c = make_case(*case)
        prob, cost = c["prob"], c["cost"]
        B, M = c["X"].shape[0], len(prob.obstacles)
        tab = np.array([[o.center[0], o.center[1], o.radius] for o in prob.obstacles])
        shared = pack_scenes(prob, np.broadcast_to(tab, (B, M, 3)), np.broadcast_to(np.array(cost.target), (B, 3)),
                             dtype=torch.float32, device=dev)
        r0 = raw_geom(c, dev)
        _same_geom(r0, raw_geom(c, dev, scenes=shared))
        rng = np.random.default_rng(5)
        obs = tab[None] + np.concatenate([rng.uniform(-0.5, 0.5, (B, M, 2)), rng.uniform(-0.2, 0.3, (B, M, 1))], 2)
        tg = np.array(cost.target) + rng.uniform(-1.0, 1.0, (B, 3))
        rs = raw_geom(c, dev, scenes=pack_scenes(prob, obs, tg, dtype=torch.float32, device=dev))
        assert not np.array_equal(rs["gob"], r0["gob"])
        for i in (0, 1, 31, 63, 64):
            pi = dataclasses.replace(prob, obstacles=tuple(CircleObstacle(center=(float(o[0]), float(o[1])),
                                                                          radius=float(o[2])) for o in obs[i]))
            ci = dataclasses.replace(cost, target=tuple(float(v) for v in tg[i]))
            ri = raw_geom(c, dev, sl=slice(i, i + 1), prob=pi, cost=ci)
            for k in ("gw", "gt", "gxr", "gur", "gx0", "gob"):
                if ri[k] is not None:
                    assert np.array_equal(ri[k][..., 0].view(np.int32), rs[k][..., i].view(np.int32)), (case, i, k)
            assert ri["status"][0] == rs["status"][i]


# ---------------------------------------------------------------------------------------------------------------
# the autograd layer
def _table(prob, dev):
    return torch.tensor([[o.center[0], o.center[1], o.radius] for o in prob.obstacles], device=dev)


@pytest.mark.parametrize("form", ["scenes", "shared"])
def test_layer_x0_and_obstacles(dev, form):
    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve, ilqr_solve, pack_scenes, solve_backward

    st, prob, cfg, x0, V0, wX, wV = _layer_setup(dev)
    B, M = x0.shape[0], len(prob.obstacles)
    Q, R, Qf, qb = _weights(dev)
    tg = torch.tensor(TARGET, device=dev)
    tab = _table(prob, dev)
    if form == "scenes":
        g = torch.Generator().manual_seed(4)
        obs = (tab + 0.2 * (torch.rand(B, M, 3, generator=g) - 0.5).to(dev)).requires_grad_(True)
        full = obs.detach()
    else:
        obs = tab.clone().requires_grad_(True)
        full = obs.detach().expand(B, M, 3)
    x0 = x0.clone().requires_grad_(True)
    res = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0, target=tg,
                          obstacles=obs, wrt=("x0", "obstacles"))
    cost = QuadraticCost(kind="target", target=TARGET, **WEIGHTS)
    scenes = pack_scenes(prob, full, tg.expand(B, 3), dtype=torch.float32, device=dev)
    ref = ilqr_solve(problem=prob, cost=cost, cfg=cfg, x0=x0.detach(), V_init=V0, scenes=scenes)
    assert torch.equal(res.X.detach(), ref.X) and torch.equal(res.V.detach(), ref.V)
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    g = solve_backward(problem=prob, cost=cost, X=ref.X, V=ref.V, grad_X=wX, grad_V=wV, scenes=scenes, want_x0=True,
                       want_obstacles=True)
    assert (g.status == 0).all() and (res.backward_status() == 0).all()
    assert g.x0.abs().sum() > 0 and g.obstacles.abs().sum() > 0
    assert torch.equal(x0.grad, g.x0)
    if form == "scenes":
        assert torch.equal(obs.grad, g.obstacles)
    else:
        assert obs.grad.shape == (M, 3) and _sum_of(obs.grad, g.obstacles)
    assert _sum_of(Q.grad, g.weights[:, 0:3]) and _sum_of(R.grad, g.weights[:, 3:5])
    # the rows one at a time are the same rows
    gx = solve_backward(problem=prob, cost=cost, X=ref.X, V=ref.V, grad_X=wX, grad_V=wV, scenes=scenes, want_x0=True)
    assert gx.obstacles is None and torch.equal(gx.x0, g.x0) and torch.equal(gx.weights, g.weights)


def test_layer_flagged_trajectory_contributes_zero(dev):
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core import diff_ilqr_solve

    st, prob, cfg, x0, V0, wX, wV = _layer_setup(dev)
    B, M = x0.shape[0], len(prob.obstacles)
    Q, R, Qf, qb = _weights(dev)
    x0 = x0.clone().requires_grad_(True)
    obs = _table(prob, dev).expand(B, M, 3).clone().requires_grad_(True)
    res = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0,
                          target=torch.tensor(TARGET, device=dev), obstacles=obs, wrt=("x0", "obstacles"))
    wX = wX.clone()
    wX[2, 3, 1] = float("nan")
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    flags = res.backward_status()
    assert flags[2] == _abi.ST_NONFINITE and int((flags != 0).sum()) == 1
    keep = torch.arange(B, device=dev) != 2
    assert (x0.grad[2] == 0).all() and (obs.grad[2] == 0).all()
    assert torch.isfinite(x0.grad).all() and torch.isfinite(obs.grad).all() and torch.isfinite(Q.grad).all()
    assert x0.grad[keep].abs().sum() > 0 and obs.grad[keep].abs().sum() > 0


def test_layer_chained_solves(dev):
    """Plan, step the plant, plan again, one backward() through both (N = 3, B = 65): the weights' gradients equal
    the same chain assembled by hand from solve_backward's rows and autograd's Jacobian of the step."""
    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve, ilqr_solve, solve_backward
    from diff_tube_mpc_strict_pt.core.barrier import DBaSConfig, dbas_step
    from diff_tube_mpc_strict_pt.core.systems.dubins import DubinsConfig, dubins_step
    from diff_tube_mpc_strict_pt.core.systems.dubins_obstacles import h_multi_circle_obstacles

    st, prob, cfg, x0, V0, wX, wV = _layer_setup(dev, B=65, N=3)
    tg = torch.tensor(TARGET, device=dev)
    dub = DubinsConfig(dt=prob.dt)
    dbc = DBaSConfig(barrier_type="inverse", alpha=prob.dbas_alpha, gamma=prob.dbas_gamma, eps=prob.dbas_eps)
    f = lambda x, u: dubins_step(x, u, cfg=dub)  # noqa: E731
    h = lambda x: h_multi_circle_obstacles(x, obstacles=list(prob.obstacles), beta=prob.obs_beta)  # noqa: E731

    def plant(xh, u):  # core.systems dynamics with the barrier state: [B, 4], [B, 2] -> [B, 4]
        xn, bn = dbas_step(x_k=xh[:, :3], u_k=u, b_k=xh[:, 3], f=f, h=h, cfg=dbc)
        return torch.cat([xn, bn[:, None]], 1)

    g = torch.Generator().manual_seed(6)
    wX1 = torch.randn(wX.shape, generator=g).to(dev)
    Q, R, Qf, qb = _weights(dev)
    kw = dict(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, V_init=V0, target=tg)
    r1 = diff_ilqr_solve(x0=x0, **kw)
    r2 = diff_ilqr_solve(x0=plant(r1.X[:, 0], r1.V[:, 0]), wrt=("x0",), **kw)
    ((r2.X * wX).sum() + (r2.V * wV).sum() + (r1.X * wX1).sum()).backward()
    assert (r1.backward_status() == 0).all() and (r2.backward_status() == 0).all()
    # by hand
    cost = QuadraticCost(kind="target", target=TARGET, **WEIGHTS)
    s1 = ilqr_solve(problem=prob, cost=cost, cfg=cfg, x0=x0, V_init=V0)
    xa, ua = s1.X[:, 0].clone().requires_grad_(True), s1.V[:, 0].clone().requires_grad_(True)
    x02 = plant(xa, ua)
    s2 = ilqr_solve(problem=prob, cost=cost, cfg=cfg, x0=x02.detach(), V_init=V0)
    assert torch.equal(r1.X.detach(), s1.X) and torch.equal(r2.X.detach(), s2.X) and torch.equal(r2.V.detach(), s2.V)
    g2 = solve_backward(problem=prob, cost=cost, X=s2.X, V=s2.V, grad_X=wX, grad_V=wV, want_x0=True)
    gxa, gua = torch.autograd.grad(x02, (xa, ua), grad_outputs=g2.x0)
    gX1, gV1 = wX1.clone(), torch.zeros_like(wV)
    gX1[:, 0] += gxa
    gV1[:, 0] += gua
    g1 = solve_backward(problem=prob, cost=cost, X=s1.X, V=s1.V, grad_X=gX1, grad_V=gV1)
    assert g2.x0.abs().sum() > 0 and gxa.abs().sum() > 0 and gua.abs().sum() > 0
    w1, w2 = g1.weights, g2.weights
    assert _sum_of(Q.grad, w1[:, 0:3], w2[:, 0:3]) and _sum_of(R.grad, w1[:, 3:5], w2[:, 3:5])
    assert _sum_of(Qf.grad, w1[:, 5:8], w2[:, 5:8]) and _sum_of(qb.grad.reshape(1), w1[:, 8:9], w2[:, 8:9])
    # the second solve alone does not explain the gradient: the chain reaches Q through the first as well
    assert not _sum_of(Q.grad, w2[:, 0:3])
