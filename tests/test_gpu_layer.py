"""The differentiable solve on the device: dtmpc_solve_backward's rows against the oracle yardstick (tests/_layer.py),
its independence of the workspace's content and of the other trajectories, per-trajectory scenes, and the autograd
layer on top (core/layer.py).

The tapes need not be optima (the backward is linear algebra on any tape): oracle rollouts of seeded random
controls, about a quarter of whose entries sit exactly on a bound of the box, from start states of which some lie
inside an obstacle's rim (the relaxed barrier branch)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from _common import agreement, oracles, paper_setup
from _layer import layer_rows

pytestmark = pytest.mark.gpu

# Agreement base of the f32 rows (tests/_common.agreement).  The starting point is 1e-4, the f32 base of
# test_sensitivity_upper_vs_oracle.  The parent's composition on the device (ddp_sensitivity(upper_grad_x=,
# upper_grad_u=) + the accumulation in torch, composition_rows below) was measured on these cases against the same
# three oracle builds: its worst error on the informative trajectories is 1.59e-3 (N50-B257-M5-target-g0.0, the
# g_target rows; 1.53e-3 at N50-B65-M5-target-g0.3, 5.5e-4 at N3-B257-M1-target-g0.3, under 1e-4 in eight of the
# twelve cases), which exceeds 1e-4, so the base is twice that figure (the fused kernel contracts the forward sums
# differently from separate tensor operations).  The fused kernel's own worst error on the same cases, for the record:
# 1.55e-3, and at most the composition's in every case but one (1.04e-6 against 8.9e-7).
COMPOSITION_WORST = 1.59e-3
BASE_F32 = 2.0 * COMPOSITION_WORST
BASE_F64 = 1e-10

WEIGHTS = dict(Q=(1.0, 1.5, 0.5), R=(1.0, 0.7), Qf=(30.0, 20.0, 10.0), qb=0.5)
TARGET = (10.0, 10.0, 0.7853981633974483)

# (N, B, M, kind, gamma, seed): each value of N in {1, 2, 3, 50}, B in {1, 65, 257} (one trajectory, one past a wave,
# one past a workgroup), M in {1, 5, 8}, both kinds, gamma in {0, 0.3}; both kinds at N = 1 and at N = 50
CASES = [
    (1, 1, 5, "target", 0.0, 11),
    (1, 65, 1, "track", 0.3, 12),
    (2, 257, 8, "target", 0.3, 13),
    (3, 65, 5, "track", 0.0, 14),
    (50, 257, 5, "target", 0.0, 15),
    (50, 65, 8, "track", 0.3, 16),
    (50, 1, 1, "track", 0.0, 17),
    (2, 65, 5, "track", 0.0, 18),
    (3, 257, 1, "target", 0.3, 19),
    (50, 65, 5, "target", 0.3, 20),
    (1, 257, 8, "track", 0.0, 21),
    (3, 1, 8, "target", 0.0, 22),
]
IDS = [f"N{c[0]}-B{c[1]}-M{c[2]}-{c[3]}-g{c[4]}" for c in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _obstacles(M):
    from diff_tube_mpc_strict_pt.core.problem import CircleObstacle

    base = paper_setup().problem.obstacles
    extra = (CircleObstacle(center=(2.0, 8.0), radius=0.8), CircleObstacle(center=(8.0, 8.0), radius=1.2),
             CircleObstacle(center=(8.0, 1.5), radius=0.7))
    # M = 1: one circle in the middle of the start box; any other count: the first M of the paper's five + the extras
    return (CircleObstacle(center=(5.0, 5.0), radius=2.5),) if M == 1 else (base + extra)[:M]


ALPHA = 0.05  # relaxed threshold of the cases' barrier: h < ALPHA takes the quadratic extension.  (With the paper's
# alpha = 0 the threshold is eps = 1e-4 and a point inside an obstacle has b ~ h^2 / 1e-12: rows of 1e13 .. 1e28 whose
# oracle builds disagree among themselves on a quarter of a batch -- measured on these seeds -- which the gate's 20 %
# limit on uninformative trajectories rules out.)


def _problem(N, M, gamma):
    return dataclasses.replace(paper_setup().problem, horizon=N, obstacles=_obstacles(M), dbas_gamma=gamma,
                               dbas_alpha=ALPHA)


def _cost(kind):
    from diff_tube_mpc_strict_pt.core import QuadraticCost

    return QuadraticCost(kind=kind, target=TARGET, **WEIGHTS)


@functools.lru_cache(maxsize=None)
def make_case(N, B, M, kind, gamma, seed):
    """Inputs (f64 numpy) of one case; the same arrays serve every test of it."""
    from oracle.oracle import Oracle

    prob = _problem(N, M, gamma)
    sp = prob.to_c()
    o = Oracle(np.float64)
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(0.0, 10.0, B), rng.uniform(0.0, 10.0, B), rng.uniform(-np.pi, np.pi, B)], 1)
    h0, _, _ = o.h_eval(sp, x0[:, 0], x0[:, 1])
    x0h = np.concatenate([x0, o.barrier(sp, h0)[1][:, None]], 1)
    lo, hi = np.array(prob.u_min), np.array(prob.u_max)
    V = rng.uniform(-0.6, 0.6, (B, N, 2)) * hi
    on = rng.random((B, N, 2)) < 0.25
    V = np.where(on, np.where(rng.random((B, N, 2)) < 0.5, lo, hi), V)
    X = o.dbas_rollout(sp, x0h, V)
    c = dict(prob=prob, cost=_cost(kind), X=X, V=V, gX=rng.normal(size=X.shape), gU=rng.normal(size=V.shape),
             Xref=None, Uref=None, on=on, at_lo=V == lo, at_hi=V == hi)
    if kind == "track":
        c["Xref"] = X[..., :3] + 0.1 * rng.normal(size=(B, N + 1, 3))
        c["Uref"] = V + 0.1 * rng.normal(size=V.shape)
    c["h"] = o.h_eval(sp, X[..., 0].reshape(-1), X[..., 1].reshape(-1))[0]
    return c


def _cast(c, npdt):
    return {k: (None if c[k] is None else c[k].astype(npdt)) for k in ("X", "V", "gX", "gU", "Xref", "Uref")}


@functools.lru_cache(maxsize=None)
def oracle_rows(case, tag):
    """The three oracle builds' rows of a case, computed once."""
    c = make_case(*case)
    npdt = np.float32 if tag == "f32" else np.float64
    a = _cast(c, npdt)
    sp, cc = c["prob"].to_c(), c["cost"].to_c()
    return [layer_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"], a["Xref"], a["Uref"]) for o in oracles(npdt)]


def _t(a, dt, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def _dev_inputs(c, tdt, dev):
    npdt = np.float32 if tdt == torch.float32 else np.float64
    a = _cast(c, npdt)
    return {k: _t(v, tdt, dev) for k, v in a.items()}


def composition_rows(c, tdt, dev):
    """The parent's route to the same rows: ddp_sensitivity with array upper gradients, then the accumulation of
    core/ift.py:35-92 for the plain weights and references as tensor operations."""
    from diff_tube_mpc_strict_pt.core import ddp_sensitivity

    t = _dev_inputs(c, tdt, dev)
    cost, N = c["cost"], c["prob"].horizon
    s = ddp_sensitivity(problem=c["prob"], cost=cost, X=t["X"], V=t["V"], upper_grad_x=t["gX"], upper_grad_u=t["gU"],
                        want_lambda=False, check=False)
    dX, dV = s.delta_X, s.delta_V
    kw = dict(dtype=tdt, device=dev)
    if cost.kind == "track":
        r, ub = t["Xref"], t["Uref"]
    else:
        r, ub = torch.tensor(cost.target, **kw).expand_as(t["X"][..., :3]), torch.zeros_like(t["V"])
    ex = t["X"][..., :3] - r
    Q, R, Qf = (torch.tensor(v, **kw) for v in (cost.Q, cost.R, cost.Qf))
    gw = torch.cat([(2 * ex[:, :N] * dX[:, :N, :3]).sum(1), (2 * (t["V"] - ub) * dV).sum(1),
                    2 * ex[:, N] * dX[:, N, :3], (2 * t["X"][..., 3] * dX[..., 3]).sum(1, keepdim=True)], 1)
    gxr = torch.cat([-2 * Q * dX[:, :N, :3], (-2 * Qf * dX[:, N, :3])[:, None]], 1)
    gur = -2 * R * dV
    track = cost.kind == "track"
    return {"weights": gw.cpu().numpy(), "target": None if track else gxr.sum(1).cpu().numpy(),
            "X_ref": gxr.cpu().numpy() if track else None, "U_ref": gur.cpu().numpy() if track else None}


def fused_rows(c, tdt, dev, check=False):
    from diff_tube_mpc_strict_pt.core import solve_backward

    t = _dev_inputs(c, tdt, dev)
    g = solve_backward(problem=c["prob"], cost=c["cost"], X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"],
                       X_ref=t["Xref"], U_ref=t["Uref"], check=check)
    return {"weights": g.weights.cpu().numpy(), "target": None if g.target is None else g.target.cpu().numpy(),
            "X_ref": None if g.X_ref is None else g.X_ref.cpu().numpy(),
            "U_ref": None if g.U_ref is None else g.U_ref.cpu().numpy(), "status": g.status.cpu().numpy()}


def gate(got, builds, base, label):
    """The issue's conditions on one case: trajectories on which a build is non-finite are left out (at most 5 %),
    those whose build spread exceeds 1e-2 are uninformative (at most 20 %), the rest agree.  Returns the worst error
    among the informative trajectories."""
    fin = np.all([b["finite"] for b in builds], axis=0)
    B = len(fin)
    assert (~fin).sum() <= 0.05 * B, (label, "non-finite oracle rows", int((~fin).sum()), B)
    worst = 0.0
    for key in ("weights", "target", "X_ref", "U_ref"):
        if builds[0][key] is None:
            assert got[key] is None, (label, key)
            continue
        B_ = [np.asarray(b[key], np.float64)[fin].reshape(int(fin.sum()), -1) for b in builds]
        g = np.asarray(got[key], np.float64)[fin].reshape(int(fin.sum()), -1)
        if not len(g):
            continue
        _, e, s = agreement(g, B_, base)
        inf = s <= 1e-2
        assert (~inf).sum() <= 0.2 * B, (label, key, "uninformative", int((~inf).sum()), B)
        ok = e[inf] <= np.maximum(base, 10.0 * s[inf])
        w = float(e[inf].max()) if inf.any() else 0.0
        worst = max(worst, w)
        print(f"[layer {label}] {key}: worst error {w:.3g} (spread max {float(s[inf].max()) if inf.any() else 0:.3g}), "
              f"{int((~fin).sum())} non-finite, {int((~inf).sum())} uninformative of {B}")
        assert np.isfinite(g[inf]).all(), (label, key, "device row not finite")
        assert ok.all(), (label, key, float(e[inf][~ok].max()), np.nonzero(~ok)[0][:8].tolist())
    return worst


def test_case_set_covers_the_branches():
    """Active and inactive entries in both channels and on both bounds, and tape points below the relaxed
    threshold, within the case set itself."""
    on = np.concatenate([make_case(*c)["on"].reshape(-1, 2) for c in CASES])
    lo = np.concatenate([make_case(*c)["at_lo"].reshape(-1, 2) for c in CASES])
    hi = np.concatenate([make_case(*c)["at_hi"].reshape(-1, 2) for c in CASES])
    for j in range(2):
        assert on[:, j].any() and (~on[:, j]).any() and lo[:, j].any() and hi[:, j].any(), j
    assert 0.15 < on.mean() < 0.35
    a = ALPHA
    below = [int((make_case(*c)["h"] < a).sum()) for c in CASES]
    assert sum(below) > 0 and sum(b > 0 for b in below) >= 4, below
    clear = [int((make_case(*c)["h"] >= a).sum()) for c in CASES]
    assert sum(clear) > sum(below), (clear, below)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_vs_oracle_f32(dev, oracle_lib, case):
    c = make_case(*case)
    builds = oracle_rows(case, "f32")
    label = IDS[CASES.index(case)]
    comp = composition_rows(c, torch.float32, dev)
    fin = np.all([b["finite"] for b in builds], axis=0)
    cw = 0.0
    for key in ("weights", "target", "X_ref", "U_ref"):
        if comp[key] is None or not fin.any():
            continue
        n = int(fin.sum())
        _, e, s = agreement(np.asarray(comp[key], np.float64)[fin].reshape(n, -1),
                            [np.asarray(b[key], np.float64)[fin].reshape(n, -1) for b in builds], BASE_F32)
        inf = (s <= 1e-2) & np.isfinite(e)
        cw = max(cw, float(e[inf].max()) if inf.any() else 0.0)
    print(f"[layer {label}] parent composition on the device: worst error {cw:.3g}")
    got = fused_rows(c, torch.float32, dev)
    assert (got["status"][fin] == 0).all(), (label, got["status"])
    fw = gate(got, builds, BASE_F32, label)
    print(f"[layer {label}] fused kernel: worst error {fw:.3g}")


def test_rows_vs_oracle_f64_fallback(dev, oracle_lib):
    """f64 takes the composition path of solve_backward."""
    case = CASES[3]
    c = make_case(*case)
    got = fused_rows(c, torch.float64, dev)
    gate(got, oracle_rows(case, "f64"), BASE_F64, IDS[3] + "-f64")


# ---------------------------------------------------------------------------------------------------------------
# the raw entry point: workspace, independence, scenes
def raw_backward(c, dev, scenes=None, fill=None, gX=None, sl=None, prob=None, cost=None):
    """One dtmpc_solve_backward call on SoA tensors made here; fill: the workspace's content before the call;
    sl: a slice of trajectories; -> dict of host arrays in the ABI layout."""
    from diff_tube_mpc_strict_pt import _abi, _lib
    from diff_tube_mpc_strict_pt.core.ddp import to_soa

    lib = _lib.load()
    prob, cost = prob or c["prob"], cost or c["cost"]
    sl = slice(None) if sl is None else sl
    f32 = torch.float32
    a = {k: (None if c[k] is None else to_soa(_t(c[k][sl], f32, dev))) for k in ("X", "V", "gX", "gU", "Xref", "Uref")}
    if gX is not None:
        a["gX"] = to_soa(_t(gX[sl], f32, dev))
    N, B = prob.horizon, a["X"].shape[2]
    track = cost.kind == "track"
    kw = dict(dtype=f32, device=dev)
    gw = torch.full((9, B), 7.0, **kw)
    gt = None if track else torch.full((3, B), 7.0, **kw)
    gxr = torch.full((N + 1, 3, B), 7.0, **kw) if track else None
    gur = torch.full((N, 2, B), 7.0, **kw) if track else None
    wb = lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, N, B)
    assert wb == N * 80 * B
    work = torch.zeros(wb // 4, **kw) if fill is None else torch.full((wb // 4,), fill, **kw)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    sp, cc = prob.to_c(), cost.to_c()
    rc = lib.dtmpc_solve_backward(_abi.F32, C.byref(sp), C.byref(cc), B, p(a["X"]), p(a["V"]), p(a["Xref"]),
                                  p(a["Uref"]), p(scenes), p(a["gX"]), p(a["gU"]), p(gw), p(gt), p(gxr), p(gur),
                                  p(work), wb, p(status), None)
    assert rc == 0, lib.dtmpc_last_error()
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in
            (("gw", gw), ("gt", gt), ("gxr", gxr), ("gur", gur), ("status", status))}


def _same(a, b, cols=None):
    for k in ("gw", "gt", "gxr", "gur"):
        if a[k] is None:
            assert b[k] is None
            continue
        x, y = (a[k], b[k]) if cols is None else (a[k][..., cols], b[k][..., cols])
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), k


@pytest.mark.parametrize("case", [CASES[4], CASES[5], CASES[3]], ids=[IDS[4], IDS[5], IDS[3]])
def test_reuse_and_independence(dev, case):
    c = make_case(*case)
    r0 = raw_backward(c, dev)
    _same(r0, raw_backward(c, dev))
    _same(r0, raw_backward(c, dev, fill=float("nan")))
    _same(r0, raw_backward(c, dev, fill=3e38))
    B = c["X"].shape[0]
    N = c["prob"].horizon
    # a trajectory whose last speed command is off the box: the terminal gradient reaches its feed-forward term
    bad = int(np.nonzero(~c["on"][:, N - 1, 0])[0][B // 4])
    gX = c["gX"].copy()
    gX[bad, N, 0] = np.nan
    r1 = raw_backward(c, dev, gX=gX)
    from diff_tube_mpc_strict_pt import _abi

    assert r1["status"][bad] == _abi.ST_NONFINITE
    others = np.arange(B) != bad
    assert (r1["status"][others] == r0["status"][others]).all()
    _same(r0, r1, cols=others)


def test_scenes(dev):
    """B copies of the shared table = scenes NULL, bitwise; distinct scenes: row i is the B = 1 call on trajectory
    i's own problem, bitwise (the pattern of tests/test_gpu_scenes.py)."""
    from diff_tube_mpc_strict_pt.core import CircleObstacle, pack_scenes

    for case in (CASES[9], CASES[3]):
        c = make_case(*case)
        prob, cost = c["prob"], c["cost"]
        B, M = c["X"].shape[0], len(prob.obstacles)
        tab = np.array([[o.center[0], o.center[1], o.radius] for o in prob.obstacles])
        shared = pack_scenes(prob, np.broadcast_to(tab, (B, M, 3)), np.broadcast_to(np.array(cost.target), (B, 3)),
                             dtype=torch.float32, device=dev)
        r0 = raw_backward(c, dev)
        _same(r0, raw_backward(c, dev, scenes=shared))
        rng = np.random.default_rng(5)
        obs = tab[None] + np.concatenate([rng.uniform(-0.5, 0.5, (B, M, 2)), rng.uniform(-0.2, 0.3, (B, M, 1))], 2)
        tg = np.array(cost.target) + rng.uniform(-1.0, 1.0, (B, 3))
        rs = raw_backward(c, dev, scenes=pack_scenes(prob, obs, tg, dtype=torch.float32, device=dev))
        assert not np.array_equal(rs["gw"], r0["gw"])
        for i in (0, 1, 31, 63, 64):
            pi = dataclasses.replace(prob, obstacles=tuple(CircleObstacle(center=(float(o[0]), float(o[1])),
                                                                          radius=float(o[2])) for o in obs[i]))
            ci = dataclasses.replace(cost, target=tuple(float(v) for v in tg[i]))
            ri = raw_backward(c, dev, sl=slice(i, i + 1), prob=pi, cost=ci)
            for k in ("gw", "gt", "gxr", "gur"):
                if ri[k] is not None:
                    assert np.array_equal(ri[k][..., 0].view(np.int32), rs[k][..., i].view(np.int32)), (case, i, k)
            assert ri["status"][0] == rs["status"][i]


# ---------------------------------------------------------------------------------------------------------------
# the autograd layer
def _layer_setup(dev, B=9, N=12):
    from diff_tube_mpc_strict_pt.core import ILQRConfig, dbas_init

    st = paper_setup()
    prob = dataclasses.replace(st.problem, horizon=N)
    cfg = ILQRConfig(horizon=N, max_iter=4, tol=1e-3, line_search_alphas=st.ilqr_nom.line_search_alphas)
    g = torch.Generator().manual_seed(3)
    x = torch.stack([torch.rand(B, generator=g), torch.rand(B, generator=g), 0.5 + torch.rand(B, generator=g)], 1).to(dev)
    x0 = torch.cat([x, dbas_init(prob, x)[:, None]], 1)
    V0 = (0.3 * torch.randn(B, N, 2, generator=g)).to(dev)
    wX = torch.randn(B, N + 1, 4, generator=g).to(dev)
    wV = torch.randn(B, N, 2, generator=g).to(dev)
    return st, prob, cfg, x0, V0, wX, wV


def _weights(dev):
    return [torch.tensor(v, device=dev, requires_grad=True) for v in
            ((1.0, 1.5, 0.5), (1.0, 0.7), (30.0, 20.0, 10.0), 0.5)]


def _sum_of(got, rows, *more):
    """got = the batch sum of the rows (f32 sums in another order: a few ulp of the terms' magnitudes)."""
    want = sum(r.sum(0) for r in (rows,) + more)
    mag = sum(r.abs().sum(0) for r in (rows,) + more)
    return bool((torch.isfinite(got) & ((got - want).abs() <= 1e-5 * mag)).all())


@pytest.mark.parametrize("form", ["target", "targets", "track"])
def test_layer_forward_and_backward(dev, form):
    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve, ilqr_solve, pack_scenes, solve_backward

    st, prob, cfg, x0, V0, wX, wV = _layer_setup(dev)
    B, N = x0.shape[0], prob.horizon
    Q, R, Qf, qb = _weights(dev)
    kind = "track" if form == "track" else "target"
    cost = QuadraticCost(kind=kind, target=TARGET, **WEIGHTS)
    kw, ref_kw, scenes = {}, {}, None
    if form == "target":
        kw["target"] = torch.tensor(TARGET, device=dev, requires_grad=True)
    elif form == "targets":
        g = torch.Generator().manual_seed(8)
        kw["target"] = (torch.tensor(TARGET) + torch.rand(B, 3, generator=g)).to(dev).requires_grad_(True)
        tab = torch.tensor([[o.center[0], o.center[1], o.radius] for o in prob.obstacles], dtype=torch.float64)
        scenes = pack_scenes(prob, tab.expand(B, -1, 3), kw["target"].detach(), dtype=torch.float32, device=dev)
    else:
        g = torch.Generator().manual_seed(9)
        Xr = torch.cat([torch.linspace(0, 1, N + 1)[None, :, None].expand(B, N + 1, 3) + 0.1 *
                        torch.randn(B, N + 1, 3, generator=g), torch.zeros(B, N + 1, 1)], 2)
        kw["X_ref"] = Xr.to(dev).requires_grad_(True)  # four columns: the fourth gets a zero gradient
        kw["U_ref"] = (0.2 * torch.randn(B, N, 2, generator=g)).to(dev).requires_grad_(True)
        ref_kw = dict(X_ref=kw["X_ref"].detach(), U_ref=kw["U_ref"].detach())
    res = diff_ilqr_solve(problem=prob, cfg=cfg, kind=kind, Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0, **kw)
    ref = ilqr_solve(problem=prob, cost=cost, cfg=cfg, x0=x0, V_init=V0, scenes=scenes, **ref_kw)
    assert torch.equal(res.X.detach(), ref.X) and torch.equal(res.V.detach(), ref.V)
    assert res.X.grad_fn is not None and res.V.grad_fn is not None and res.backward_status() is None
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    g = solve_backward(problem=prob, cost=cost, X=ref.X, V=ref.V, grad_X=wX, grad_V=wV, scenes=scenes, **ref_kw)
    assert (g.status == 0).all() and (res.backward_status() == 0).all()
    w = g.weights
    assert w.abs().sum() > 0
    assert _sum_of(Q.grad, w[:, 0:3]) and _sum_of(R.grad, w[:, 3:5])
    assert _sum_of(Qf.grad, w[:, 5:8]) and _sum_of(qb.grad.reshape(1), w[:, 8:9])
    if form == "target":
        assert _sum_of(kw["target"].grad, g.target)
    elif form == "targets":
        assert torch.equal(kw["target"].grad, g.target)
    else:
        assert torch.equal(kw["X_ref"].grad[..., :3], g.X_ref) and (kw["X_ref"].grad[..., 3] == 0).all()
        assert torch.equal(kw["U_ref"].grad, g.U_ref)


def test_layer_shared_tensor_and_flagged_trajectory(dev):
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve, solve_backward

    st, prob, cfg, x0, V0, wX, wV = _layer_setup(dev)
    W = torch.tensor((2.0, 3.0, 1.5), device=dev, requires_grad=True)
    R = torch.tensor((1.0, 0.7), device=dev, requires_grad=True)
    qb = torch.tensor(0.5, device=dev)
    tg = torch.tensor(TARGET, device=dev)
    res = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=W, R=R, Qf=W, qb=qb, x0=x0, V_init=V0, target=tg)
    wX = wX.clone()
    wX[2, 3, 1] = float("nan")  # trajectory 2's upper gradient: flagged in the backward, contributes nothing
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    cost = QuadraticCost(kind="target", Q=(2.0, 3.0, 1.5), R=(1.0, 0.7), Qf=(2.0, 3.0, 1.5), qb=0.5, target=TARGET)
    g = solve_backward(problem=prob, cost=cost, X=res.X.detach(), V=res.V.detach(), grad_X=wX, grad_V=wV, check=False)
    flags = res.backward_status()
    assert flags[2] == _abi.ST_NONFINITE and int((flags != 0).sum()) == 1 and torch.equal(flags, g.status)
    keep = torch.arange(x0.shape[0], device=dev) != 2
    w = g.weights[keep]
    assert w.abs().sum() > 0
    assert _sum_of(W.grad, w[:, 0:3], w[:, 5:8]) and _sum_of(R.grad, w[:, 3:5])
    with pytest.raises(FloatingPointError):
        solve_backward(problem=prob, cost=cost, X=res.X.detach(), V=res.V.detach(), grad_X=wX, grad_V=wV)
