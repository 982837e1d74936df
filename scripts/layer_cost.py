"""What the differentiable solve costs: the fused dtmpc_solve_backward against the composition that produces the same
rows (dtmpc_ddp_sensitivity_upper, which writes the dX / dU tapes, plus the accumulation of core/ift.py:35-92 as
tensor operations), same process, runs alternated; then forward and backward of diff_ilqr_solve.

  python scripts/layer_cost.py [--batch 65536] [--rounds 5] [--reps 20] [--out FILE]

B = 65,536, N = 50, M = 5, f32, the paper's target cost and ten iLQR iterations; the tape is the solve's own result
and the upper gradients are seeded normals.  Both backward variants run on SoA buffers made once (no layout copies
in the timed region); each figure is the median over `reps` calls between device events after a warm-up of 3, the
spread max - min of the per-round medians.  `layer_forward` / `layer_backward` time diff_ilqr_solve(...) and
loss.backward() as a user calls them (layout copies, the weights' device-to-host read and autograd included).  The
bytes the fused kernel moves by construction are printed beside the times.  `fused_geom` / `composition_geom`: the
same pair for dtmpc_solve_backward_geom (the rows w.r.t. x0 and the obstacle circles as well) -- its composition
also writes delta_lambda and forms the obstacle rows as tensor operations -- timed in the same alternated rounds, so
`fused` beside it shows whether the old entry moved.  One JSON line.

--weights adds the per-trajectory-weights entries to the same alternated rounds: `fused_weights` /
`fused_geom_weights` (dtmpc_solve_backward_weights with the plain / the GEOM record) beside `fused` / `fused_geom`, and
the forward at one lane -- `solve_scenes` (dtmpc_ilqr_solve_scenes, B copies of the paper's scene: the parent's
kernel), `solve_weights_scenes` and `solve_weights` (dtmpc_ilqr_solve_weights with and without the scenes) and
`solve_shared` (dtmpc_ilqr_solve_ws).  The weights are B copies of the cost's own, so every variant does bitwise the
same work (checked here) and the difference is the kernel form's; `solve_weights_mixed` (five weight sets, factors in
[0.5, 2], trajectory i -> set i % 5) is other work -- other iterates and exits -- and is printed for scale only.  Each
forward call starts from the same zero warm start (the reset is inside the timed region of every variant alike).  The
weights add 36 B read per trajectory and launch by construction.

--dbas adds dtmpc_solve_backward_dbas (the rows w.r.t. the DBaS alpha / gamma as well: 8 B more written per trajectory
and launch, the same record) to the same alternated rounds, each call timed right after its twin of the same (M, kind):
`fused_dbas` after `fused_geom` (M = 5, target cost), and for the tracking cost `fused_geom_track` / `fused_dbas_track`
(references = the tape's own positions and controls; both entries with g_xref / g_uref, g_x0 and g_obs passed).  The
rows both entries write are compared bitwise here.

--tight adds the per-trajectory-tightening entries, each timed right after its twin in the same rounds, with s = 0 for
every trajectory so that both do the same work (compared bitwise here): `tight_fused_dbas` then `tight_fused`
(dtmpc_solve_backward_dbas / dtmpc_solve_backward_tight, target cost, g_x0, g_obs and g_dbas passed), and the forward at
one lane from the same zero warm start, `tight_solve_shared` then `tight_solve` (dtmpc_ilqr_solve_ws /
dtmpc_ilqr_solve_tight).  The tightening adds 4 B read per trajectory and launch each way and 4 B written (g_tight)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "differentiable-tube-mpc_amd")]
import torch  # noqa: E402

from diff_tube_mpc_strict_pt import _abi, _lib  # noqa: E402
from diff_tube_mpc_strict_pt.core import dbas_init, diff_ilqr_solve, ilqr_solve  # noqa: E402
from diff_tube_mpc_strict_pt.core.barrier import barrier_and_derivative  # noqa: E402
from diff_tube_mpc_strict_pt.core.ddp import to_soa  # noqa: E402
from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--weights", action="store_true", help="also time the per-trajectory-weights entries")
    ap.add_argument("--dbas", action="store_true", help="also time dtmpc_solve_backward_dbas beside its geom twins")
    ap.add_argument("--tight", action="store_true", help="also time the per-trajectory-tightening entries at s = 0")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    st = paper_setup_from_config(paper_config())
    prob, cost, cfg = st.problem, st.nominal_cost, st.ilqr_nom
    B, N = a.batch, prob.horizon
    f32 = torch.float32
    g = torch.Generator().manual_seed(1)
    x = torch.stack([torch.rand(B, generator=g), torch.rand(B, generator=g), torch.rand(B, generator=g) * 1.5], 1).to(dev)
    x0 = torch.cat([x, dbas_init(prob, x)[:, None]], 1)
    V0 = torch.zeros(B, N, 2, device=dev)
    res = ilqr_solve(problem=prob, cost=cost, cfg=cfg, x0=x0, V_init=V0, check=False)
    gX = torch.randn(B, N + 1, 4, generator=g).to(dev)
    gU = torch.randn(B, N, 2, generator=g).to(dev)
    lib = _lib.load()
    spec, cc = prob.to_c(), cost.to_c()
    Xs, Us, gx, gu = to_soa(res.X), to_soa(res.V), to_soa(gX), to_soa(gU)
    kw = dict(dtype=f32, device=dev)
    gw, gt = torch.empty(9, B, **kw), torch.empty(3, B, **kw)
    wb = lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, N, B)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    stream = _lib.stream_of(Xs)

    def fused():
        _lib.check(lib.dtmpc_solve_backward(_abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(), None,
                                            None, None, gx.data_ptr(), gu.data_ptr(), gw.data_ptr(), gt.data_ptr(),
                                            None, None, work.data_ptr(), wb, status.data_ptr(), stream),
                   "dtmpc_solve_backward")

    dX, dU = torch.empty(N + 1, 4, B, **kw), torch.empty(N, 2, B, **kw)
    work2 = torch.empty(lib.dtmpc_sensitivity_upper_workspace_bytes(_abi.F32, N, B), dtype=torch.uint8, device=dev)
    tg = torch.tensor(cost.target, **kw).view(1, 3, 1)
    Qw, Qfw = torch.tensor(cost.Q, **kw).view(1, 3, 1), torch.tensor(cost.Qf, **kw).view(3, 1)
    comp = {}

    def composition():
        _lib.check(lib.dtmpc_ddp_sensitivity_upper(_abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(),
                                                   gx.data_ptr(), gu.data_ptr(), dX.data_ptr(), dU.data_ptr(), None,
                                                   work2.data_ptr(), status.data_ptr(), stream),
                   "dtmpc_ddp_sensitivity_upper")
        composition_rows()

    def composition_rows():
        ex = Xs[:, :3] - tg
        gQ = (2 * ex[:N] * dX[:N, :3]).sum(0)
        gR = (2 * Us * dU).sum(0)
        gQf = 2 * ex[N] * dX[N, :3]
        gqb = (2 * Xs[:, 3] * dX[:, 3]).sum(0, keepdim=True)
        comp["gw"] = torch.cat([gQ, gR, gQf, gqb], 0)
        comp["gt"] = (-2 * Qw * dX[:N, :3]).sum(0) + -2 * Qfw * dX[N, :3]

    M = len(prob.obstacles)
    gx0, gob = torch.empty(4, B, **kw), torch.empty(3 * M, B, **kw)
    wbg = lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, N, B)
    workg = torch.empty(wbg, dtype=torch.uint8, device=dev)
    gwg, gtg = torch.empty(9, B, **kw), torch.empty(3, B, **kw)

    def fused_geom():
        _lib.check(lib.dtmpc_solve_backward_geom(_abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(),
                                                 None, None, None, gx.data_ptr(), gu.data_ptr(), gwg.data_ptr(),
                                                 gtg.data_ptr(), None, None, gx0.data_ptr(), gob.data_ptr(),
                                                 workg.data_ptr(), wbg, status.data_ptr(), stream),
                   "dtmpc_solve_backward_geom")

    dL = torch.empty(N + 1, 4, B, **kw)
    tab = torch.tensor([[o.center[0], o.center[1], o.radius] for o in prob.obstacles], **kw)
    ocx, ocy, orr = (tab[:, j].view(1, M, 1) for j in range(3))
    zero = torch.zeros(1, B, **kw)

    def composition_geom():
        _lib.check(lib.dtmpc_ddp_sensitivity_upper(_abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(),
                                                   gx.data_ptr(), gu.data_ptr(), dX.data_ptr(), dU.data_ptr(),
                                                   dL.data_ptr(), work2.data_ptr(), status.data_ptr(), stream),
                   "dtmpc_ddp_sensitivity_upper")
        composition_rows()
        dx, dy = Xs[:, 0:1] - ocx, Xs[:, 1:2] - ocy  # [N+1, M, B]
        z = -prob.obs_beta * (dx * dx + dy * dy - orr * orr)
        w = torch.softmax(z, 1)
        h = -torch.logsumexp(z, 1) / prob.obs_beta
        D = barrier_and_derivative(h, kind=_abi.BARRIER_INVERSE, alpha=prob.dbas_alpha, eps=prob.dbas_eps,
                                   want_B=False, want_dB=True)[1]
        lam = dL[:, 3]
        cw = (D * (torch.cat([zero, lam[1:]], 0) - prob.dbas_gamma * torch.cat([lam[1:], zero], 0)))[:, None] * w
        comp["gx0"] = dL[0]
        comp["gob"] = torch.cat([(cw * (-2 * dx)).sum(0), (cw * (-2 * dy)).sum(0), -cw.sum(0)], 0)  # cx, cy, r2 rows

    Q, R, Qf, qb = (torch.tensor(v, device=dev, requires_grad=True) for v in (cost.Q, cost.R, cost.Qf, cost.qb))
    tgt = torch.tensor(cost.target, device=dev, requires_grad=True)
    hold = {}

    def layer_forward():
        hold["res"] = diff_ilqr_solve(problem=prob, cfg=cfg, kind="target", Q=Q, R=R, Qf=Qf, qb=qb, x0=x0, V_init=V0,
                                      target=tgt, check=False)

    def layer_backward():
        r = hold["res"]
        ((r.X * gX).sum() + (r.V * gU).sum()).backward(retain_graph=True)

    ms = {k: [] for k in ("fused", "composition", "fused_geom", "composition_geom", "layer_forward", "layer_backward")}
    wfn = {}
    if a.weights:
        import numpy as np

        from diff_tube_mpc_strict_pt.core import pack_scenes, pack_weights

        ic = cfg.to_c()
        nine = torch.tensor([*cost.Q, *cost.R, *cost.Qf, cost.qb], dtype=torch.float64)
        wu = nine.expand(B, 9)
        wts = pack_weights(wu[:, 0:3], wu[:, 3:5], wu[:, 5:8], wu[:, 8], device=dev)
        rng = np.random.default_rng(23)
        sets = torch.cat([nine[None], nine[None] * torch.as_tensor(np.exp(rng.uniform(np.log(0.5), np.log(2.0), (4, 9))))])
        wm = sets[torch.arange(B) % 5]
        wts_mixed = pack_weights(wm[:, 0:3], wm[:, 3:5], wm[:, 5:8], wm[:, 8], device=dev)
        tab64 = torch.tensor([[o.center[0], o.center[1], o.radius] for o in prob.obstacles], dtype=torch.float64)
        sc = pack_scenes(prob, tab64.expand(B, M, 3), torch.tensor(cost.target, dtype=torch.float64).expand(B, 3),
                         dtype=f32, device=dev)
        gww, gtw = torch.empty(9, B, **kw), torch.empty(3, B, **kw)
        gwgw, gtgw, gx0w, gobw = torch.empty(9, B, **kw), torch.empty(3, B, **kw), torch.empty(4, B, **kw), torch.empty(3 * M, B, **kw)

        def fused_weights():
            _lib.check(lib.dtmpc_solve_backward_weights(
                _abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(), None, None, None, wts.data_ptr(),
                gx.data_ptr(), gu.data_ptr(), gww.data_ptr(), gtw.data_ptr(), None, None, None, None, work.data_ptr(), wb,
                status.data_ptr(), stream), "dtmpc_solve_backward_weights")

        def fused_geom_weights():
            _lib.check(lib.dtmpc_solve_backward_weights(
                _abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(), None, None, None, wts.data_ptr(),
                gx.data_ptr(), gu.data_ptr(), gwgw.data_ptr(), gtgw.data_ptr(), None, None, gx0w.data_ptr(),
                gobw.data_ptr(), workg.data_ptr(), wbg, status.data_ptr(), stream), "dtmpc_solve_backward_weights")

        x0s = x0.t().contiguous()
        fX, fU = torch.empty(N + 1, 4, B, **kw), torch.empty(N, 2, B, **kw)
        fK, fk = torch.empty(N, 8, B, **kw), torch.empty(N, 2, B, **kw)
        fit, fst = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        fwb = lib.dtmpc_ilqr_workspace_bytes(_abi.F32, N, B, 1)
        fwork = torch.empty(fwb, dtype=torch.uint8, device=dev)

        def solve(scenes, weights):
            def run():
                fU.zero_()
                fst.zero_()
                _lib.check(lib.dtmpc_ilqr_solve_weights(
                    _abi.F32, C.byref(spec), C.byref(cc), C.byref(ic), B, x0s.data_ptr(), None, None, fX.data_ptr(),
                    fU.data_ptr(), fK.data_ptr(), fk.data_ptr(), fit.data_ptr(), fst.data_ptr(), None, None, 1,
                    fwork.data_ptr(), fwb, None if scenes is None else scenes.data_ptr(),
                    None if weights is None else weights.data_ptr(), stream), "dtmpc_ilqr_solve_weights")
            return run

        wfn = {"fused_weights": fused_weights, "fused_geom_weights": fused_geom_weights,
               "solve_shared": solve(None, None), "solve_scenes": solve(sc, None), "solve_weights": solve(None, wts),
               "solve_weights_scenes": solve(sc, wts), "solve_weights_mixed": solve(None, wts_mixed)}
        ms.update({k: [] for k in wfn})
    dfn = {}
    if a.dbas:
        import dataclasses

        gdb, gwd, gtd = torch.empty(2, B, **kw), torch.empty(9, B, **kw), torch.empty(3, B, **kw)
        gx0d, gobd = torch.empty(4, B, **kw), torch.empty(3 * M, B, **kw)
        ct = dataclasses.replace(cost, kind="track").to_c()
        Xr, Ur = Xs[:, :3].contiguous(), Us.clone()
        trk = {k: (torch.empty(9, B, **kw), torch.empty(N + 1, 3, B, **kw), torch.empty(N, 2, B, **kw),
                   torch.empty(4, B, **kw), torch.empty(3 * M, B, **kw)) for k in ("geom", "dbas")}
        gdbt = torch.empty(2, B, **kw)

        def fused_dbas():
            _lib.check(lib.dtmpc_solve_backward_dbas(
                _abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(), None, None, None, None,
                gx.data_ptr(), gu.data_ptr(), gwd.data_ptr(), gtd.data_ptr(), None, None, gx0d.data_ptr(),
                gobd.data_ptr(), gdb.data_ptr(), workg.data_ptr(), wbg, status.data_ptr(), stream),
                "dtmpc_solve_backward_dbas")

        def fused_geom_track():
            w9, xr, ur, g0, go = trk["geom"]
            _lib.check(lib.dtmpc_solve_backward_geom(
                _abi.F32, C.byref(spec), C.byref(ct), B, Xs.data_ptr(), Us.data_ptr(), Xr.data_ptr(), Ur.data_ptr(), None,
                gx.data_ptr(), gu.data_ptr(), w9.data_ptr(), None, xr.data_ptr(), ur.data_ptr(), g0.data_ptr(),
                go.data_ptr(), workg.data_ptr(), wbg, status.data_ptr(), stream), "dtmpc_solve_backward_geom")

        def fused_dbas_track():
            w9, xr, ur, g0, go = trk["dbas"]
            _lib.check(lib.dtmpc_solve_backward_dbas(
                _abi.F32, C.byref(spec), C.byref(ct), B, Xs.data_ptr(), Us.data_ptr(), Xr.data_ptr(), Ur.data_ptr(), None,
                None, gx.data_ptr(), gu.data_ptr(), w9.data_ptr(), None, xr.data_ptr(), ur.data_ptr(), g0.data_ptr(),
                go.data_ptr(), gdbt.data_ptr(), workg.data_ptr(), wbg, status.data_ptr(), stream),
                "dtmpc_solve_backward_dbas")

        assert lib.dtmpc_solve_backward_dbas_workspace_bytes(_abi.F32, N, B) == wbg
        dfn = {"fused_dbas": fused_dbas, "fused_geom_track": fused_geom_track, "fused_dbas_track": fused_dbas_track}
        ms.update({k: [] for k in dfn})
    tfn = {}
    if a.tight:
        ict = cfg.to_c()
        s0 = torch.zeros(B, **kw)
        tb = {k: (torch.empty(9, B, **kw), torch.empty(3, B, **kw), torch.empty(4, B, **kw), torch.empty(3 * M, B, **kw),
                  torch.empty(2, B, **kw)) for k in ("dbas", "tight")}
        gts = torch.empty(B, **kw)
        tst = {k: torch.zeros(B, dtype=torch.int32, device=dev) for k in ("dbas", "tight")}

        def tight_fused_dbas():
            w9, t3, g0, go, gd = tb["dbas"]
            _lib.check(lib.dtmpc_solve_backward_dbas(
                _abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(), None, None, None, None,
                gx.data_ptr(), gu.data_ptr(), w9.data_ptr(), t3.data_ptr(), None, None, g0.data_ptr(), go.data_ptr(),
                gd.data_ptr(), workg.data_ptr(), wbg, tst["dbas"].data_ptr(), stream), "dtmpc_solve_backward_dbas")

        def tight_fused():
            w9, t3, g0, go, gd = tb["tight"]
            _lib.check(lib.dtmpc_solve_backward_tight(
                _abi.F32, C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(), None, None, None, None,
                s0.data_ptr(), gx.data_ptr(), gu.data_ptr(), w9.data_ptr(), t3.data_ptr(), None, None, g0.data_ptr(),
                go.data_ptr(), gd.data_ptr(), gts.data_ptr(), workg.data_ptr(), wbg, tst["tight"].data_ptr(), stream),
                "dtmpc_solve_backward_tight")

        tx0 = x0.t().contiguous()
        tf = {k: (torch.empty(N + 1, 4, B, **kw), torch.empty(N, 2, B, **kw), torch.empty(N, 8, B, **kw),
                  torch.empty(N, 2, B, **kw), torch.zeros(B, dtype=torch.int32, device=dev),
                  torch.zeros(B, dtype=torch.int32, device=dev)) for k in ("shared", "tight")}
        twb = lib.dtmpc_ilqr_solve_tight_workspace_bytes(_abi.F32, N, B, 1)
        assert twb == lib.dtmpc_ilqr_workspace_bytes(_abi.F32, N, B, 1)
        twork = torch.empty(twb, dtype=torch.uint8, device=dev)

        def tight_solve_shared():
            X_, U_, K_, k_, it_, st_ = tf["shared"]
            U_.zero_()
            st_.zero_()
            _lib.check(lib.dtmpc_ilqr_solve_ws(
                _abi.F32, C.byref(spec), C.byref(cc), C.byref(ict), B, tx0.data_ptr(), None, None, X_.data_ptr(),
                U_.data_ptr(), K_.data_ptr(), k_.data_ptr(), it_.data_ptr(), st_.data_ptr(), None, None, 1,
                twork.data_ptr(), twb, stream), "dtmpc_ilqr_solve_ws")

        def tight_solve():
            X_, U_, K_, k_, it_, st_ = tf["tight"]
            U_.zero_()
            st_.zero_()
            _lib.check(lib.dtmpc_ilqr_solve_tight(
                _abi.F32, C.byref(spec), C.byref(cc), C.byref(ict), B, tx0.data_ptr(), None, None, X_.data_ptr(),
                U_.data_ptr(), K_.data_ptr(), k_.data_ptr(), it_.data_ptr(), st_.data_ptr(), None, None, 1,
                twork.data_ptr(), twb, None, s0.data_ptr(), stream), "dtmpc_ilqr_solve_tight")

        tfn = {"tight_fused_dbas": tight_fused_dbas, "tight_fused": tight_fused,
               "tight_solve_shared": tight_solve_shared, "tight_solve": tight_solve}
        ms.update({k: [] for k in tfn})
    for _ in range(a.rounds):
        for k, fn in tfn.items():  # each entry right after its twin
            ms[k].append(timed(fn, a.reps))
        for k, fn in wfn.items():
            ms[k].append(timed(fn, a.reps))
        ms["fused"].append(timed(fused, a.reps))
        ms["composition"].append(timed(composition, a.reps))
        ms["fused_geom"].append(timed(fused_geom, a.reps))
        for k, fn in dfn.items():  # fused_dbas right after its twin fused_geom, then the tracking pair
            ms[k].append(timed(fn, a.reps))
        ms["composition_geom"].append(timed(composition_geom, a.reps))
        ms["layer_forward"].append(timed(layer_forward, max(a.reps // 4, 3)))
        ms["layer_backward"].append(timed(layer_backward, max(a.reps // 4, 3)))
    fused()
    composition()
    torch.cuda.synchronize()
    ok = status == 0
    err = float(((gw - comp["gw"]).abs().amax(0) / comp["gw"].abs().amax(0).clamp_min(1.0))[ok].max())
    # target cost: backward reads X (three fields) 12, U 8, gX 16, gU 8 and writes the 80 B record; forward reads the
    # record and X 16, U 8
    per_step = 44 + 80 + 80 + 24
    fused_geom()
    composition_geom()
    torch.cuda.synchronize()
    okg = status == 0
    errg = {k: float(((v - comp[k]).abs().amax(0) / comp[k].abs().amax(0).clamp_min(1.0))[okg].max())
            for k, v in (("gx0", gx0), ("gob", gob))}
    same_old_rows = bool(torch.equal(gw.view(torch.int32), gwg.view(torch.int32)) and
                         torch.equal(gt.view(torch.int32), gtg.view(torch.int32)))
    rec = {"B": B, "N": N, "M": len(prob.obstacles), "rounds": a.rounds, "reps": a.reps,
           "bytes_per_traj_step_by_construction": per_step,
           "bytes_per_launch_by_construction": per_step * N * B + (16 + 16 + 48) * B,
           "flagged": int((~ok).sum()), "fused_vs_composition_max_rel": err,
           # GEOM: the record grows by 20 B written and 20 B read per step; per launch 16 B (g_x0) + 12 M B (g_obs)
           "geom_bytes_per_traj_step_by_construction": per_step + 40,
           "geom_bytes_per_launch_by_construction": (per_step + 40) * N * B + (16 + 16 + 48 + 16 + 12 * M + 4) * B,
           "geom_flagged": int((~okg).sum()), "geom_fused_vs_composition_max_rel": errg,
           "geom_old_rows_bitwise": same_old_rows}
    if a.weights:
        fused_weights()
        fused_geom_weights()
        outs = {}
        for k in ("solve_shared", "solve_scenes", "solve_weights", "solve_weights_scenes", "solve_weights_mixed"):
            wfn[k]()
            torch.cuda.synchronize()
            outs[k] = (fX.clone(), fU.clone(), fit.clone(), fst.clone())
        same = lambda p, q: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(p, q))  # noqa: E731
        rec["weights"] = {
            "bytes_added_per_traj_and_launch_by_construction": 36,
            "backward_uniform_rows_bitwise_shared": bool(same((gw, gt), (gww, gtw))),
            "backward_geom_uniform_rows_bitwise_shared": bool(same((gwg, gtg, gx0, gob), (gwgw, gtgw, gx0w, gobw))),
            "forward_uniform_bitwise_shared": bool(same(outs["solve_shared"], outs["solve_weights"]) and
                                                   same(outs["solve_scenes"], outs["solve_weights_scenes"]) and
                                                   same(outs["solve_shared"], outs["solve_scenes"])),
            "forward_mean_iters": {k: round(float(v[2].float().mean()), 3) for k, v in outs.items()},
            "forward_status_nonzero": {k: int((v[3] != 0).sum()) for k, v in outs.items()}}
    if a.dbas:
        for fn in dfn.values():
            fn()
        torch.cuda.synchronize()
        bits = lambda p, q: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(p, q))  # noqa: E731
        rec["dbas"] = {"bytes_added_per_traj_and_launch_by_construction": 8,
                       "flagged": int((status != 0).sum()),
                       "rows_bitwise_geom": bool(bits((gwg, gtg, gx0, gob), (gwd, gtd, gx0d, gobd))),
                       "track_rows_bitwise_geom": bool(bits(trk["geom"], trk["dbas"])),
                       "alpha_rows_nonzero": int((gdb[0] != 0).sum()), "gamma_row_abs_max": float(gdb[1].abs().max())}
    if a.tight:
        for fn in tfn.values():
            fn()
        torch.cuda.synchronize()
        bits = lambda p, q: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(p, q))  # noqa: E731
        rec["tight"] = {"bytes_added_per_traj_and_launch_by_construction": {"forward": 4, "backward": 8},
                        "backward_rows_bitwise_dbas_at_s0": bool(bits(tb["dbas"], tb["tight"]) and
                                                                 bits((tst["dbas"],), (tst["tight"],))),
                        "forward_bitwise_shared_at_s0": bool(bits(tf["shared"], tf["tight"])),
                        "backward_flagged": int((tst["tight"] != 0).sum()),
                        "forward_status_nonzero": int((tf["tight"][5] != 0).sum()),
                        "forward_mean_iters": round(float(tf["tight"][4].float().mean()), 3),
                        "g_tight_abs_max": float(gts[tst["tight"] == 0].abs().max())}
    for n, v in ms.items():
        rec[n] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                  "spread": round(max(v) - min(v), 4)}
    rec["fused_GBps_by_construction"] = round(rec["bytes_per_launch_by_construction"] / rec["fused"]["ms_median"] / 1e6, 1)
    rec["fused_geom_GBps_by_construction"] = round(rec["geom_bytes_per_launch_by_construction"] /
                                                   rec["fused_geom"]["ms_median"] / 1e6, 1)
    if a.weights:
        med = lambda k: rec[k]["ms_median"]  # noqa: E731
        rec["weights"]["ratio_of_medians"] = {
            "solve_weights_scenes / solve_scenes": round(med("solve_weights_scenes") / med("solve_scenes"), 4),
            "solve_weights / solve_shared": round(med("solve_weights") / med("solve_shared"), 4),
            "fused_weights / fused": round(med("fused_weights") / med("fused"), 4),
            "fused_geom_weights / fused_geom": round(med("fused_geom_weights") / med("fused_geom"), 4)}
    if a.dbas:
        med = lambda k: rec[k]["ms_median"]  # noqa: E731
        rec["dbas"]["ratio_of_medians"] = {"fused_dbas / fused_geom": round(med("fused_dbas") / med("fused_geom"), 4),
                                           "fused_dbas_track / fused_geom_track":
                                               round(med("fused_dbas_track") / med("fused_geom_track"), 4)}
    if a.tight:
        med = lambda k: rec[k]["ms_median"]  # noqa: E731
        rec["tight"]["ratio_of_medians"] = {"tight_fused / tight_fused_dbas": round(med("tight_fused") / med("tight_fused_dbas"), 4),
                                            "tight_solve / tight_solve_shared":
                                                round(med("tight_solve") / med("tight_solve_shared"), 4)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
