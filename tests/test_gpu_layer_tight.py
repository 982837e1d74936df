"""The backward of a tightened solve and the row w.r.t. the tightening on the device (dtmpc_solve_backward_tight,
core.solve_backward(tightening=, want_tight=), diff_ilqr_solve(tightening=)): against the oracle yardstick
(tests/_layer_tight.py, itself held to oracle.ift_gradient's tightening column and to finite differences by
tests/test_layer_tight_yardstick.py), bitwise against dtmpc_solve_backward_dbas at s = 0, independence of the
workspace's content, of the requested outputs and of the other trajectories, per-trajectory scenes x weights x s, and
the autograd layer, chained solves included.

The cases are tests/test_gpu_layer.py's twelve (N in {1, 2, 3, 50}, B in {1, 65, 257}, M in {1, 5, 8}, both kinds,
gamma 0 / 0.3, alpha 0.05) with b_0 offset (tests/_layer_dbas.offset_b0), a per-trajectory s drawn from {0, 0.05, 0.3}
(default_rng(seed + 2000)) and the tape re-rolled by the oracle per group of equal s (positions and controls unchanged).
N = 1 is the smallest horizon at which the co_0 / co_N end terms can be mis-indexed; B = 65 and 257 are one lane past a
wave and one past a workgroup.

The gate is tests/test_gpu_layer_geom.gate's conditions (tests/test_gpu_layer_dbas.gate) per key: tight, alpha, gamma,
x0, obstacles; the weight / reference rows stand under tests/test_gpu_layer.gate.

The f32 base follows those files' rule: the parent-buildable composition on the device (ddp_sensitivity with array
upper gradients and want_lambda in f32 on the tightened tape -- delta_lambda does not depend on s -- then the formulas
as tensor operations with h - s, composition_tight below) on the same cases against the same three oracle builds; the
base is twice its worst error on the informative trajectories.  Measured on an MI355X
(profiles/r15/layer_tight_errors.txt has the per-case table): the composition's worst error is 2.83e-2 of a row's scale
(N3-B257-M1-target-g0.3, the gamma rows; 1.02e-2 / 1.06e-2 / 1.36e-2 / 1.02e-2 on that case's tight / alpha / x0 /
obstacle rows, 4.1e-3 tight and 5.0e-3 alpha at N50-B257-M5-target-g0.0, 3.3e-3 obstacles at N50-B65-M8-track-g0.3,
2.8e-3 tight at N50-B65-M5-target-g0.3, under 4.2e-4 in the eight remaining cases), so the base is 5.66e-2.  The fused
kernel's own worst error on the same cases, for the record: 2.97e-2 (the same case and key; tight 9.1e-3, x0 1.34e-2
there), 6.7e-3 obstacles at N50-B65-M8-track-g0.3, 2.7e-3 tight at N50-B257-M5-target-g0.0.  No trajectory is non-finite;
at most 3 of 257 are uninformative.  Per case (worst informative error of the tight row: composition, fused kernel):
    N1-B1-M5-target-g0.0        6.61e-09  6.61e-09
    N1-B65-M1-track-g0.3        4.61e-05  4.62e-05
    N2-B257-M8-target-g0.3      0.000419  0.000419
    N3-B65-M5-track-g0.0         0.00013  4.08e-05
    N50-B257-M5-target-g0.0      0.00406   0.00268
    N50-B65-M8-track-g0.3         0.0026   0.00301
    N50-B1-M1-track-g0.0         2.5e-09  1.23e-09
    N2-B65-M5-track-g0.0        3.47e-05  3.47e-05
    N3-B257-M1-target-g0.3        0.0102   0.00913
    N50-B65-M5-target-g0.3       0.00283   0.00252
    N1-B257-M8-track-g0.0        5.7e-05   5.7e-05
    N3-B1-M8-target-g0.0        1.17e-05  1.57e-05
With s = softplus(raw) in torch, raw.grad matched the three f32 builds' ift_gradient raw column 11 summed over B = 65 to
1.5e-7 of the sum (build spread 6.8e-7)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from _common import oracles
from _layer import layer_rows
from _layer_tight import KEYS, reroll, tight_rows
from _weights import assignment, cost_of, pack, weight_sets
from test_gpu_layer import BASE_F32 as LAYER_BASE_F32
from test_gpu_layer import CASES, IDS, TARGET, WEIGHTS, _cast, _dev_inputs, _layer_setup, _same, _sum_of, _t, _weights
from test_gpu_layer import gate as layer_gate
from test_gpu_layer_dbas import dbas_case, gate, raw_dbas, worst_informative

pytestmark = pytest.mark.gpu

COMPOSITION_WORST = 2.83e-2
BASE_F32 = 2.0 * COMPOSITION_WORST
S_SET = (0.0, 0.05, 0.3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def tight_case(case):
    """dbas_case's inputs (b_0 offset) with a per-trajectory s and the tape re-rolled under it (computed once)."""
    from oracle.oracle import Oracle

    c = dict(dbas_case(case))
    B = c["X"].shape[0]
    rng = np.random.default_rng(case[5] + 2000)
    c["s"] = np.array(S_SET, np.float32)[rng.integers(0, 3, B)] if B > 1 else np.array([0.3], np.float32)
    X = reroll(Oracle(np.float64), c["prob"].to_c(), c["X"], c["V"], c["s"])
    assert np.array_equal(X[..., :3], c["X"][..., :3])
    c["X"] = X
    return c


@functools.lru_cache(maxsize=None)
def oracle_tight(case):
    """The three f32 oracle builds' rows of a tightened case, computed once."""
    c = tight_case(case)
    a = _cast(c, np.float32)
    sp, cc = c["prob"].to_c(), c["cost"].to_c()
    out = {"tight": [], "rows": []}
    for o in oracles(np.float32):
        out["tight"].append(tight_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"], c["s"]))
        out["rows"].append(layer_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"], a["Xref"], a["Uref"]))
    return out


def composition_tight(c, dev):
    """The route to the same rows that needs none of the new code: ddp_sensitivity with array upper gradients and
    delta_lambda on the tightened tape, then the formulas of tests/_layer_tight.py as f32 tensor operations."""
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core import ddp_sensitivity
    from diff_tube_mpc_strict_pt.core.barrier import barrier_and_derivative

    tdt = torch.float32
    t = _dev_inputs(c, tdt, dev)
    prob = c["prob"]
    N = prob.horizon
    sn = ddp_sensitivity(problem=prob, cost=c["cost"], X=t["X"], V=t["V"], upper_grad_x=t["gX"], upper_grad_u=t["gU"],
                         want_lambda=True, check=False)
    X, lam = t["X"], sn.delta_lambda[..., 3]
    s = torch.as_tensor(c["s"], device=dev)[:, None]
    tab = torch.tensor([[o.center[0], o.center[1], o.radius] for o in prob.obstacles], dtype=tdt, device=dev)
    dx, dy = X[..., 0:1] - tab[:, 0], X[..., 1:2] - tab[:, 1]
    zz = -prob.obs_beta * (dx * dx + dy * dy - tab[:, 2] * tab[:, 2])
    w = torch.softmax(zz, -1)
    z = (-torch.logsumexp(zz, -1) / prob.obs_beta - s).contiguous()
    Bv, D = barrier_and_derivative(z, kind=_abi.BARRIER_INVERSE, alpha=prob.dbas_alpha, eps=prob.dbas_eps, want_B=True,
                                   want_dB=True)
    a = max(prob.dbas_alpha, prob.dbas_eps)
    dBa = torch.where(z >= a, torch.zeros_like(z), -3.0 * (z - a) ** 2 / a ** 4)
    zero = torch.zeros_like(lam[:, :1])
    co = torch.cat([zero, lam[:, 1:]], 1) - prob.dbas_gamma * torch.cat([lam[:, 1:], zero], 1)
    cw = (co * D)[..., None] * w
    obs = torch.stack([(cw * (-2.0 * dx)).sum(1), (cw * (-2.0 * dy)).sum(1), -cw.sum(1) * (2.0 * tab[:, 2])], 2)
    out = {"tight": -(co * D).sum(1, keepdim=True), "alpha": (co * dBa).sum(1, keepdim=True),
           "gamma": -(lam[:, 1:] * (Bv[:, :N] - X[:, :N, 3])).sum(1, keepdim=True), "x0": sn.delta_lambda[:, 0],
           "obstacles": obs}
    return {k: v.cpu().numpy() for k, v in out.items()}


def fused_tight(c, dev, want_x0=True, want_obstacles=True, want_dbas=True, want_tight=True, **kw):
    from diff_tube_mpc_strict_pt.core import solve_backward

    t = _dev_inputs(c, torch.float32, dev)
    g = solve_backward(problem=c["prob"], cost=c["cost"], X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"],
                       X_ref=t["Xref"], U_ref=t["Uref"], check=False, want_x0=want_x0, want_obstacles=want_obstacles,
                       want_dbas=want_dbas, tightening=torch.as_tensor(c["s"], device=dev), want_tight=want_tight, **kw)
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return {"tight": host(g.tight[:, None]) if g.tight is not None else None,
            "alpha": host(g.dbas[:, 0:1]) if g.dbas is not None else None,
            "gamma": host(g.dbas[:, 1:2]) if g.dbas is not None else None, "x0": host(g.x0),
            "obstacles": host(g.obstacles), "status": host(g.status), "weights": host(g.weights),
            "target": host(g.target), "X_ref": host(g.X_ref), "U_ref": host(g.U_ref)}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_vs_oracle_f32(dev, oracle_lib, case):
    c = tight_case(case)
    ob = oracle_tight(case)
    builds = ob["tight"]
    label = IDS[CASES.index(case)]
    cw = worst_informative(composition_tight(c, dev), builds, BASE_F32, KEYS)
    print(f"[layer tight {label}] composition on the device: worst error " + ", ".join(f"{k} {cw[k]:.3g}" for k in KEYS))
    got = fused_tight(c, dev)
    fw = worst_informative(got, builds, BASE_F32, KEYS)
    print(f"[layer tight {label}] fused kernel: worst error " + ", ".join(f"{k} {fw[k]:.3g}" for k in KEYS))
    fin = np.all([b["finite"] for b in builds], axis=0)
    gate(got, builds, BASE_F32, label, KEYS)
    assert (got["status"][fin] == 0).all(), (label, got["status"])
    ow = layer_gate(got, ob["rows"], LAYER_BASE_F32, label + " (tight entry)")
    print(f"[layer tight {label}] fused kernel, weight / reference rows {ow:.3g}; s values "
          f"{sorted(set(c['s'].tolist()))}, largest |g_tight| {np.abs(builds[0]['tight'][fin]).max():.3g}")
    assert np.abs(builds[0]["tight"][fin]).max() > 0


def test_refusals_on_the_device(dev):
    from diff_tube_mpc_strict_pt.core import solve_backward

    c = tight_case(CASES[3])
    s = torch.as_tensor(c["s"], device=dev)
    for tdt in (torch.float32, torch.float64):
        t = _dev_inputs(c, tdt, dev)
        kw = dict(X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"], X_ref=t["Xref"], U_ref=t["Uref"], check=False,
                  tightening=s, want_tight=True)
        for over in (dict(obs_aggregation="min"), dict(barrier_type="log")):
            with pytest.raises(ValueError, match="tightening needs the fused kernel"):
                solve_backward(problem=dataclasses.replace(c["prob"], **over), cost=c["cost"], **kw)
        if tdt == torch.float64:  # f64: the composition path has no tightening
            with pytest.raises(ValueError, match="tightening needs the fused kernel"):
                solve_backward(problem=c["prob"], cost=c["cost"], **kw)
    t = _dev_inputs(c, torch.float32, dev)
    kw = dict(problem=c["prob"], cost=c["cost"], X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"], X_ref=t["Xref"],
              U_ref=t["Uref"], check=False)
    with pytest.raises(ValueError, match=r"tightening must be \[65\]"):
        solve_backward(tightening=s[:-1].contiguous(), **kw)
    with pytest.raises(ValueError, match="float32"):
        solve_backward(tightening=s.double(), **kw)
    # tightening= without want_tight: every other row under the tightened h, no tight row
    g = solve_backward(tightening=s, want_dbas=True, **kw)
    g1 = solve_backward(tightening=s, want_dbas=True, want_tight=True, **kw)
    g0 = solve_backward(want_dbas=True, **kw)
    assert g.tight is None and g1.tight is not None and torch.equal(g.dbas, g1.dbas)
    assert not torch.equal(g.dbas, g0.dbas)


# ---------------------------------------------------------------------------------------------------------------
# the raw entry point
def raw_tight(c, dev, s=None, scenes=None, fill=None, gX=None, sl=None, prob=None, cost=None, x0=True, obs=True,
              dbas=True, wt=None):
    """One dtmpc_solve_backward_tight call on SoA tensors made here (the arguments of test_gpu_layer_dbas.raw_dbas; s:
    the tightening [B] of the whole case, default c["s"]; dbas: pass g_dbas) -> dict of host arrays in the ABI layout."""
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
    if scenes is not None:
        scenes = scenes[:, sl].contiguous()
    tg = _t(np.asarray(c["s"] if s is None else s, np.float32)[sl], f32, dev)
    N, B, M = prob.horizon, a["X"].shape[2], len(prob.obstacles)
    track = cost.kind == "track"
    kw = dict(dtype=f32, device=dev)
    gw = torch.full((9, B), 7.0, **kw)
    gt = None if track else torch.full((3, B), 7.0, **kw)
    gxr = torch.full((N + 1, 3, B), 7.0, **kw) if track else None
    gur = torch.full((N, 2, B), 7.0, **kw) if track else None
    gx0 = torch.full((4, B), 7.0, **kw) if x0 else None
    gob = torch.full((3 * M, B), 7.0, **kw) if obs else None
    gdb = torch.full((2, B), 7.0, **kw) if dbas else None
    gtg = torch.full((B,), 7.0, **kw)
    wb = lib.dtmpc_solve_backward_tight_workspace_bytes(_abi.F32, N, B)
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
    rc = lib.dtmpc_solve_backward_tight(_abi.F32, C.byref(sp), C.byref(cc), B, p(a["X"]), p(a["V"]), p(a["Xref"]),
                                        p(a["Uref"]), p(scenes), p(wt), p(tg), p(a["gX"]), p(a["gU"]), p(gw), p(gt),
                                        p(gxr), p(gur), p(gx0), p(gob), p(gdb), p(gtg), p(work), wb, p(status), None)
    assert rc == 0, lib.dtmpc_last_error()
    torch.cuda.synchronize()
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in
           (("gw", gw), ("gt", gt), ("gxr", gxr), ("gur", gur), ("gx0", gx0), ("gob", gob), ("gdb", gdb), ("gtg", gtg),
            ("status", status))}
    out["work"] = work
    return out


def _same_tight(a, b, cols=None, keys=("gx0", "gob", "gdb", "gtg")):
    _same(a, b, cols)
    for k in keys:
        x, y = (a[k], b[k]) if cols is None else (a[k][..., cols], b[k][..., cols])
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), k


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zero_tightening_is_the_dbas_entry_bitwise(dev, case):
    """s = 0 everywhere: every row but g_tight equals dtmpc_solve_backward_dbas's on the same inputs (hv - 0 is
    exact)."""
    c = tight_case(case)
    B = c["X"].shape[0]
    a, b = raw_tight(c, dev, s=np.zeros(B, np.float32)), raw_dbas(c, dev)
    _same_tight(a, b, keys=("gx0", "gob", "gdb"))
    assert np.array_equal(a["status"], b["status"])
    assert not (a["gtg"] == 7.0).any() and np.isfinite(a["gtg"][a["status"] == 0]).all()


@pytest.mark.parametrize("case", [CASES[4], CASES[5], CASES[3], CASES[2]], ids=[IDS[4], IDS[5], IDS[3], IDS[2]])
def test_reuse_and_independence(dev, case):
    from diff_tube_mpc_strict_pt import _abi

    c = tight_case(case)
    r0 = raw_tight(c, dev)
    assert (r0["status"] == 0).sum() > 0
    _same_tight(r0, raw_tight(c, dev))
    _same_tight(r0, raw_tight(c, dev, fill=float("nan")))
    _same_tight(r0, raw_tight(c, dev, fill=3e38))
    other = raw_tight(tight_case(CASES[9]), dev)["work"]  # a workspace that holds another case's content
    _same_tight(r0, raw_tight(c, dev, fill=other))
    # the outputs asked for: g_x0 / g_obs / g_dbas passed or NULL
    rx, ro = raw_tight(c, dev, obs=False, dbas=False), raw_tight(c, dev, x0=False)
    rn = raw_tight(c, dev, x0=False, obs=False, dbas=False)
    assert rx["gob"] is None and rx["gdb"] is None and ro["gx0"] is None and rn["gx0"] is None and rn["gdb"] is None
    _same_tight(r0, rx, keys=("gx0", "gtg"))
    _same_tight(r0, ro, keys=("gob", "gdb", "gtg"))
    _same_tight(r0, rn, keys=("gtg",))
    for r in (rx, ro, rn):
        assert np.array_equal(r["status"], r0["status"])
    assert not (r0["gtg"] == 7.0).any() and not (r0["gdb"] == 7.0).any() and (r0["gtg"] != 0).any()
    # the tightening is read: the same tape with s = 0 gives other obstacle and DBaS rows where s != 0
    B, N = c["X"].shape[0], c["prob"].horizon
    rz = raw_tight(c, dev, s=np.zeros(B, np.float32))
    nz = c["s"] != 0
    assert not np.array_equal(rz["gdb"][:, nz], r0["gdb"][:, nz])
    assert np.array_equal(rz["gdb"][:, ~nz].view(np.int32), r0["gdb"][:, ~nz].view(np.int32))
    # trajectory i of the batch against the B = 1 launch on it
    for i in sorted({0, 1, 31, 63, 64, B - 1} & set(range(B))):
        ri = raw_tight(c, dev, sl=slice(i, i + 1))
        for k in ("gw", "gt", "gxr", "gur", "gx0", "gob", "gdb", "gtg"):
            if ri[k] is not None:
                assert np.array_equal(ri[k][..., 0].view(np.int32), r0[k][..., i].view(np.int32)), (i, k)
        assert ri["status"][0] == r0["status"][i]
    # a NaN in one trajectory's gX flags that one only (g_tight is part of the status)
    bad = int(np.nonzero(~c["on"][:, N - 1, 0])[0][B // 4])
    others = np.arange(B) != bad
    for col in (0, 3):  # the terminal position gradient; the barrier component, which reaches lam alone
        gX = c["gX"].copy()
        gX[bad, N, col] = np.nan
        r1 = raw_tight(c, dev, gX=gX)
        assert r1["status"][bad] == _abi.ST_NONFINITE and not np.isfinite(r1["gtg"][bad])
        assert (r1["status"][others] == r0["status"][others]).all()
        _same_tight(r0, r1, cols=others)


def test_scenes_weights_and_tightenings(dev):
    """Per-trajectory scenes x weights x s at B = 65: set by set, the per-trajectory launch is bitwise the launch on
    that set's own problem and cost with a uniform tightening."""
    from diff_tube_mpc_strict_pt.core import CircleObstacle, pack_scenes

    for case in (CASES[9], CASES[3]):
        c = tight_case(case)
        prob, cost = c["prob"], c["cost"]
        B, M = c["X"].shape[0], len(prob.obstacles)
        assert B == 65
        tab = np.array([[o.center[0], o.center[1], o.radius] for o in prob.obstacles])
        sets = weight_sets(cost)
        S = 3
        rng = np.random.default_rng(5)
        obs_s = tab[None] + np.concatenate([rng.uniform(-0.5, 0.5, (S, M, 2)), rng.uniform(-0.2, 0.3, (S, M, 1))], 2)
        tg_s = np.array(cost.target) + rng.uniform(-1.0, 1.0, (S, 3))
        i = np.arange(B)
        ks, kw, kt = i % S, assignment(B), (i // 3) % 3
        s = np.array(S_SET, np.float32)[kt]
        sc = pack_scenes(prob, obs_s[ks], tg_s[ks], dtype=torch.float32, device=dev)
        wt = pack(sets, kw, dev)
        rs = raw_tight(c, dev, s=s, scenes=sc, wt=wt)
        n = 0
        for s_ in range(S):
            pi = dataclasses.replace(prob, obstacles=tuple(CircleObstacle(center=(float(o[0]), float(o[1])),
                                                                          radius=float(o[2])) for o in obs_s[s_]))
            ci = dataclasses.replace(cost, target=tuple(float(v) for v in tg_s[s_]))
            for w_ in range(len(sets)):
                for t_ in range(3):
                    cols = (ks == s_) & (kw == w_) & (kt == t_)
                    if not cols.any():
                        continue
                    n += 1
                    # the shared launch (no scenes, no weights array) on this triple's problem, cost and uniform s
                    rsw = raw_tight(c, dev, s=np.full(B, S_SET[t_], np.float32), prob=pi, cost=cost_of(ci, sets[w_]))
                    for k in ("gtg", "gdb", "gx0", "gob", "gw"):
                        assert np.array_equal(rsw[k][..., cols].view(np.int32), rs[k][..., cols].view(np.int32)), \
                            (s_, w_, t_, k)
                    assert np.array_equal(rsw["status"][cols], rs["status"][cols])
        assert n >= 20, n


# ---------------------------------------------------------------------------------------------------------------
# the autograd layer
def _tight_setup(dev, B=9, N=12):
    """_layer_setup with alpha = 0.05, every other start position on the rim of the first obstacle (tape rows on the
    relaxed branch), a per-trajectory s from S_SET and b_0 the consistent B(h(x_0) - s_i)."""
    from diff_tube_mpc_strict_pt.core import dbas_init

    st, prob, cfg, x0, V0, wX, wV = _layer_setup(dev, B=B, N=N)
    prob = dataclasses.replace(prob, dbas_alpha=0.05)
    g = torch.Generator().manual_seed(12)
    ob = prob.obstacles[0]
    ang = 3.4 + 1.2 * torch.rand(B, generator=g)
    d = ob.radius * (1.0 + 0.25 * torch.rand(B, generator=g) + 0.1)
    rim = torch.stack([ob.center[0] + d * torch.cos(ang), ob.center[1] + d * torch.sin(ang)], 1).to(x0)
    x = x0[:, :3].clone()
    x[0::2, :2] = rim[0::2]
    s = torch.as_tensor(np.array(S_SET, np.float32)[np.arange(B) % 3], device=dev)
    x0 = torch.cat([x, dbas_init(prob, x, tightening=s)[:, None]], 1)
    return st, prob, cfg, x0, V0, wX, wV, s


def test_layer_forward_is_ilqr_solve_and_grad_is_the_rows(dev):
    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve, ilqr_solve, solve_backward

    st, prob, cfg, x0, V0, wX, wV, s = _tight_setup(dev)
    Q, R, Qf, qb = _weights(dev)
    tg = torch.tensor(TARGET, device=dev)
    cost = QuadraticCost(kind="target", target=TARGET, **WEIGHTS)
    sg = s.clone().requires_grad_(True)
    res = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0, target=tg,
                          tightening=sg)
    ref = ilqr_solve(problem=prob, cost=cost, cfg=cfg, x0=x0, V_init=V0, tightening=s)
    plain = ilqr_solve(problem=prob, cost=cost, cfg=cfg, x0=x0, V_init=V0)
    assert torch.equal(res.X.detach(), ref.X) and torch.equal(res.V.detach(), ref.V)
    assert not torch.equal(ref.X, plain.X)
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    g = solve_backward(problem=prob, cost=cost, X=ref.X, V=ref.V, grad_X=wX, grad_V=wV, tightening=s, want_tight=True)
    assert (g.status == 0).all() and (res.backward_status() == 0).all()
    assert sg.grad.shape == s.shape and torch.equal(sg.grad, g.tight) and g.tight.abs().sum() > 0
    assert _sum_of(Q.grad, g.weights[:, 0:3]) and _sum_of(qb.grad.reshape(1), g.weights[:, 8:9])
    # a shared value: the sum of the rows (zero-dim and one-element), and the same solve as the uniform [B]
    for shared in (torch.tensor(0.3, device=dev, requires_grad=True), torch.tensor([0.3], device=dev, requires_grad=True)):
        u = torch.full_like(s, 0.3)
        r2 = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0, target=tg,
                             tightening=shared)
        ref2 = ilqr_solve(problem=prob, cost=cost, cfg=cfg, x0=x0, V_init=V0, tightening=u)
        assert torch.equal(r2.X.detach(), ref2.X) and torch.equal(r2.V.detach(), ref2.V)
        ((r2.X * wX).sum() + (r2.V * wV).sum()).backward()
        g2 = solve_backward(problem=prob, cost=cost, X=ref2.X, V=ref2.V, grad_X=wX, grad_V=wV, tightening=u,
                            want_tight=True)
        assert shared.grad.shape == shared.shape and _sum_of(shared.grad.reshape(1), g2.tight[:, None])
    # composes with wrt=("x0", "obstacles"), dbas_alpha= and obstacles=
    tab = torch.tensor([[o.center[0], o.center[1], o.radius] for o in prob.obstacles], device=dev, requires_grad=True)
    x0g = x0.clone().requires_grad_(True)
    al = torch.tensor(0.05, device=dev, requires_grad=True)
    sg3 = s.clone().requires_grad_(True)
    r3 = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0g, V_init=V0, target=tg,
                         tightening=sg3, obstacles=tab, wrt=("x0", "obstacles"), dbas_alpha=al)
    ((r3.X * wX).sum() + (r3.V * wV).sum()).backward()
    assert (r3.backward_status() == 0).all()
    assert torch.isfinite(sg3.grad).all() and torch.isfinite(tab.grad).all() and torch.isfinite(x0g.grad).all()
    assert torch.isfinite(al.grad) and tab.grad.abs().sum() > 0 and sg3.grad.abs().sum() > 0


def test_layer_flagged_trajectory_contributes_zero(dev):
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve, solve_backward

    st, prob, cfg, x0, V0, wX, wV, s = _tight_setup(dev)
    Q, R, Qf, qb = _weights(dev)
    cost = QuadraticCost(kind="target", target=TARGET, **WEIGHTS)
    wX = wX.clone()
    wX[2, 3, 1] = float("nan")
    keep = torch.arange(x0.shape[0], device=dev) != 2
    for t in (s.clone().requires_grad_(True), torch.tensor(0.3, device=dev, requires_grad=True)):
        res = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0,
                              target=torch.tensor(TARGET, device=dev), tightening=t)
        ((res.X * wX).sum() + (res.V * wV).sum()).backward()
        flags = res.backward_status()
        assert flags[2] == _abi.ST_NONFINITE and int((flags != 0).sum()) == 1
        u = t.detach().reshape(-1).expand(x0.shape[0]).contiguous()
        g = solve_backward(problem=prob, cost=cost, X=res.X.detach(), V=res.V.detach(), grad_X=wX, grad_V=wV,
                           tightening=u, want_tight=True, check=False)
        assert torch.isfinite(t.grad).all()
        if t.dim() == 1:
            assert t.grad[2] == 0 and torch.equal(t.grad[keep], g.tight[keep])
        else:
            assert _sum_of(t.grad.reshape(1), g.tight[keep][:, None])


def test_layer_raw_parameter_vs_ift_gradient(dev, oracle_lib):
    """s = softplus(raw) in torch: raw.grad is oracle.ift_gradient's raw column DTMPC_P_TIGHT (11) summed over the
    batch, at the tape the solve returned, for the three f32 builds.  The bound is the base times the largest magnitude
    of the reference sum (tests/test_gpu_layer_dbas.py's form), target kind."""
    from diff_tube_mpc_strict_pt.core import QuadraticCost, dbas_init, diff_ilqr_solve

    st, prob, cfg, x0, V0, wX, wV, _ = _tight_setup(dev, B=65, N=12)
    Q, R, Qf, qb = _weights(dev)
    raw = torch.tensor(float(np.log(np.expm1(0.3))), device=dev, requires_grad=True)
    s = torch.nn.functional.softplus(raw)
    x0 = torch.cat([x0[:, :3], dbas_init(prob, x0[:, :3], tightening=s.detach())[:, None]], 1)
    res = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0,
                          target=torch.tensor(TARGET, device=dev), tightening=s)
    ((res.X * wX).sum() + (res.V * wV).sum()).backward()
    assert (res.backward_status() == 0).all()
    got = float(raw.grad.cpu())
    sp, cc = prob.to_c(), QuadraticCost(kind="target", target=TARGET, **WEIGHTS).to_c()
    th = np.zeros(12)
    th[9] = float(np.log(np.expm1(prob.dbas_alpha - 1e-6)))
    th[10] = 0.0  # tanh(0) = 0 = gamma
    th[11] = float(raw.detach().cpu())
    X, V = res.X.detach().cpu().numpy(), res.V.detach().cpu().numpy()
    gX, gV = wX.cpu().numpy(), wV.cpu().numpy()
    refs = []
    for o in oracles(np.float32):
        dX, dV, dlam, _ = o.ddp_sensitivity_upper(sp, cc, X, V, gX, gV)
        gth = o.ift_gradient(sp, cc, th, X, V, dX, dV, dlam)[0].astype(np.float64)
        assert np.isfinite(gth[:, 11]).all()
        refs.append(gth[:, 11].sum())
    refs = np.array(refs)
    scale, err, spread = np.abs(refs).max(), np.abs(refs - got).min(), np.abs(refs[1:] - refs[0]).max()
    print(f"[layer tight raw] raw.grad {got}, oracle builds {refs.tolist()}, error {err / scale:.3g} of the reference "
          f"sum (build spread {spread / scale:.3g})")
    assert scale > 0
    assert err <= BASE_F32 * scale, (err / scale, BASE_F32)


def test_layer_chained_solves_reach_the_tightening(dev):
    """Plan, step the plant, plan again: one backward() delivers a finite, non-zero tightening.grad from both solves."""
    from diff_tube_mpc_strict_pt.core import diff_ilqr_solve

    st, prob, cfg, x0, V0, wX, wV, s = _tight_setup(dev, B=65, N=3)
    Q, R, Qf, qb = _weights(dev)
    sg = s.clone().requires_grad_(True)
    kw = dict(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, V_init=V0,
              target=torch.tensor(TARGET, device=dev), tightening=sg)
    r1 = diff_ilqr_solve(x0=x0, **kw)
    r2 = diff_ilqr_solve(x0=r1.X[:, 1], wrt=("x0",), **kw)  # the plan's own next state: b_1 = B(h(x_1) - s)
    ((r2.X * wX).sum() + (r2.V * wV).sum()).backward()
    assert (r1.backward_status() == 0).all() and (r2.backward_status() == 0).all()
    assert torch.isfinite(sg.grad).all() and sg.grad.abs().sum() > 0
    # both solves contribute: the second alone gives another gradient
    sg2 = s.clone().requires_grad_(True)
    r2b = diff_ilqr_solve(x0=r1.X[:, 1].detach(), **dict(kw, tightening=sg2))
    ((r2b.X * wX).sum() + (r2b.V * wV).sum()).backward()
    assert not torch.equal(sg.grad, sg2.grad)
