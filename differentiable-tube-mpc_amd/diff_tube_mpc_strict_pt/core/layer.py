"""The iLQR solve as a differentiable layer: ``loss(X*, V*).backward()`` reaches the cost weights, the target and
the tracking references.

What the gradient is.  ``solve_backward`` evaluates the reference's implicit-function gradient AT THE TAPE IT IS
GIVEN: ddp_sensitivity (core/ddp.py:317-427 -- the backward pass with the active set of the box frozen, reg = 1e-9,
the Gauss-Newton L_zz, i.e. no second derivatives of the dynamics) with the incoming ``grad_X`` / ``grad_V`` as the
upper gradients, then ift_gradient's accumulation (core/ift.py:35-92) restricted to the plain weights Q, R, Qf, q_b
and the references.  It is the quantity the paper's Algorithm 2 descends along.  It is the gradient of the solver's
output only where the solve has converged: on a tape that is not a stationary point of the lower problem (an
iteration cap, a failed line search) it is still well defined, but it is the sensitivity of the KKT system
linearised there, not of the iterate.  On request (``want_x0`` / ``want_obstacles``; ``wrt=`` of the layer) the rows
w.r.t. the start state and the obstacle circles come with them: the two terms of ift_gradient that involve
delta_lambda,
    g_x0 = dlam_0 = tilde V_x[0]
    c_m = B'(h(x_m)) ([m >= 1] lam_m - gamma [m <= N-1] lam_{m+1}),  lam_k = dlam_k[3]          m = 0 .. N
    g_cx_j = sum_m c_m w_j(x_m) (-2 (px_m - cx_j)),  g_cy_j alike,  g_r_j = 2 r_j sum_m c_m w_j(x_m) (-1)
with w_j = softmax_j(-beta h_j) (only the barrier row of f_hat sees the obstacles).  b_0's own dependence on the
position and the scene is the caller's to express (``dbas_init_b0`` is differentiable).

On request (``want_dbas``; ``dbas_alpha=`` / ``dbas_gamma=`` of the layer) also the rows w.r.t. the barrier-state
parameters alpha and gamma, the remaining delta_lambda terms: with co_m = [m >= 1] lam_m - gamma [m <= N-1] lam_{m+1}
and a = max(alpha, eps),
    g_alpha = dmax sum_{m=0..N} co_m dBa(h(x_m)),   dBa(z) = 0 for z >= a, -3 (z - a)^2 / a^4 below
    g_gamma = -sum_{k=0..N-1} lam_{k+1} (B(h(x_k)) - b_k)
with dmax = d max(alpha, eps) / d alpha = 1 (alpha > eps), 0.5 (alpha == eps), 0 (alpha < eps), applied on the host
(``ift_gradient``'s alpha / gamma columns without the softplus / tanh chain, h evaluated at the tape rows, which a
rolled-out tape makes x' = f(x_k, u_k) to rounding).  If b_0 = B(h(x_0)) then B(h(x_k)) - b_k = 0 for every k
whatever gamma is: the gamma row is then zero in exact arithmetic (rounding noise in f32).  It is non-zero only when
the solve starts from a barrier state that is not the barrier of its position: a plant state after a disturbance, the
second of two chained solves.

With a per-trajectory constraint tightening (``tightening=`` [B]: trajectory i's barrier saw h(x) - s_i, the nominal
solve of the tube MPC, core/tube_mpc.py:235-238) the factors above are taken at z = h(x_m) - s_i -- B'(z) in the
obstacle rows, dBa(z), B(z) - b_k -- and on request (``want_tight``) the eleventh of ``ift_gradient``'s terms is returned,
    g_tight_i = -sum_{m=0..N} co_m B'(h(x_m) - s_i)
(its tightening column without the softplus chain).  The reference linearises with B'(h) of the PLAIN h
(core/tube_mpc.py:315-320 against :273-276), so delta_lambda of a given tape does not depend on s and the weight,
reference and x0 rows keep their formulas.  Gradients w.r.t. the warm start, dbas_eps and obs_beta are not provided.

Where ``dtmpc_solve_backward_supported`` says yes (f32, smooth-min, 1..8 obstacles, relaxed inverse barrier) the
rows come from ONE launch of the fused kernel (csrc/dtmpc_fast_layer.hip; dtmpc_solve_backward_geom when x0 or
obstacle rows are wanted, dtmpc_solve_backward_dbas when the DBaS rows are, dtmpc_solve_backward_tight under a
tightening), which writes no sensitivity tape;
elsewhere (f64, min / single aggregation, log barrier) from ``dtmpc_ddp_sensitivity_upper`` and a few tensor
operations."""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
from torch import Tensor

from .. import _abi, _lib
from .barrier import barrier_and_derivative
from .ddp import (ILQRResult, _ddp_sensitivity_upper, _dtype_code, _ptr, _require_device, from_soa, ilqr_solve,
                  raise_for_status, to_soa)
from .problem import (DubinsDBaSProblem, ILQRConfig, QuadraticCost, check_scenes, check_tightening, check_weights,
                      pack_scenes, pack_weights)

__all__ = ["SolveGradient", "solve_backward", "diff_ilqr_solve"]


@dataclass(frozen=True)
class SolveGradient:
    """Per-trajectory rows of d loss / d (plain weights, references) at one tape."""

    weights: Tensor            # [B, 9]: Q(3) R(2) Qf(3) qb
    target: Optional[Tensor]   # [B, 3] (target cost)
    X_ref: Optional[Tensor]    # [B, N+1, 3] (tracking cost)
    U_ref: Optional[Tensor]    # [B, N, 2]
    status: Tensor             # [B] int32, DTMPC_ST_NONFINITE where a row is not finite
    dbas: Optional[Tensor] = None       # [B, 2]: the DBaS alpha, gamma (want_dbas)
    tight: Optional[Tensor] = None      # [B]: the tightening s_i (want_tight)
    x0: Optional[Tensor] = None         # [B, 4] (want_x0)
    obstacles: Optional[Tensor] = None  # [B, M, 3]: (cx, cy, r) of each circle (want_obstacles)


def _nonfinite_status(*rows: Optional[Tensor]) -> Tensor:
    bad = None
    for r in rows:
        if r is None:
            continue
        b = ~torch.isfinite(r.reshape(r.shape[0], -1)).all(1)
        bad = b if bad is None else bad | b
    return bad.to(torch.int32) * _abi.ST_NONFINITE


def _obstacle_rows(problem: DubinsDBaSProblem, X: Tensor, dlam: Tensor) -> Tensor:
    """The obstacle rows [B, M, 3] (cx, cy, r) from a sensitivity's delta_lambda [B, N+1, 4] as tensor operations
    (the module docstring's formulas; smooth-min and the relaxed inverse barrier, the problem's shared circles)."""
    kw = dict(dtype=X.dtype, device=X.device)
    tab = torch.tensor([[o.center[0], o.center[1], o.radius] for o in problem.obstacles], **kw)
    dx = X[..., 0:1] - tab[:, 0]  # [B, N+1, M]
    dy = X[..., 1:2] - tab[:, 1]
    z = -float(problem.obs_beta) * (dx * dx + dy * dy - tab[:, 2] * tab[:, 2])
    w = torch.softmax(z, -1)
    h = -torch.logsumexp(z, -1) / float(problem.obs_beta)
    D = barrier_and_derivative(h, kind=_abi.BARRIER_INVERSE, alpha=float(problem.dbas_alpha),
                               eps=float(problem.dbas_eps), want_B=False, want_dB=True)[1]
    lam = dlam[..., 3]
    zero = torch.zeros_like(lam[:, :1])
    c = D * (torch.cat([zero, lam[:, 1:]], 1) - float(problem.dbas_gamma) * torch.cat([lam[:, 1:], zero], 1))
    cw = c[..., None] * w
    return torch.stack([(cw * (-2.0 * dx)).sum(1), (cw * (-2.0 * dy)).sum(1), -cw.sum(1) * (2.0 * tab[:, 2])], 2)


def _dbas_dmax(problem: DubinsDBaSProblem) -> float:
    """d max(alpha, eps) / d alpha: the factor between the alpha_eff row and the alpha row."""
    a, e = float(problem.dbas_alpha), float(problem.dbas_eps)
    return 1.0 if a > e else (0.5 if a == e else 0.0)


def _dbas_host(problem: DubinsDBaSProblem, gdb: Tensor) -> Tensor:
    """[2, B] (alpha_eff, gamma) -> [B, 2] (alpha, gamma): the dmax factor on the alpha row (exact zeros at 0)."""
    d = _dbas_dmax(problem)
    ga = gdb[0] * d if d != 0.0 else torch.zeros_like(gdb[0])
    return torch.stack([ga, gdb[1]], 1)


def _dbas_rows(problem: DubinsDBaSProblem, X: Tensor, dlam: Tensor) -> Tensor:
    """The DBaS rows [B, 2] (alpha_eff, gamma) from a sensitivity's delta_lambda [B, N+1, 4] as tensor operations (the
    module docstring's formulas; smooth-min and the relaxed inverse barrier, the problem's shared circles)."""
    kw = dict(dtype=X.dtype, device=X.device)
    N = X.shape[1] - 1
    tab = torch.tensor([[o.center[0], o.center[1], o.radius] for o in problem.obstacles], **kw)
    dx = X[..., 0:1] - tab[:, 0]  # [B, N+1, M]
    dy = X[..., 1:2] - tab[:, 1]
    z = -float(problem.obs_beta) * (dx * dx + dy * dy - tab[:, 2] * tab[:, 2])
    h = -torch.logsumexp(z, -1) / float(problem.obs_beta)
    Bv = barrier_and_derivative(h, kind=_abi.BARRIER_INVERSE, alpha=float(problem.dbas_alpha),
                                eps=float(problem.dbas_eps), want_B=True, want_dB=False)[0]
    a = max(float(problem.dbas_alpha), float(problem.dbas_eps))
    dBa = torch.where(h >= a, torch.zeros_like(h), -3.0 * (h - a) ** 2 / a ** 4)
    lam = dlam[..., 3]
    zero = torch.zeros_like(lam[:, :1])
    co = torch.cat([zero, lam[:, 1:]], 1) - float(problem.dbas_gamma) * torch.cat([lam[:, 1:], zero], 1)
    ga = (co * dBa).sum(1)
    gg = -(lam[:, 1:] * (Bv[:, :N] - X[:, :N, 3])).sum(1)
    return torch.stack([ga, gg], 1)


def solve_backward(*, problem: DubinsDBaSProblem, cost: QuadraticCost, X: Tensor, V: Tensor, grad_X: Tensor,
                   grad_V: Tensor, X_ref: Optional[Tensor] = None, U_ref: Optional[Tensor] = None,
                   scenes: Optional[Tensor] = None, check: bool = True, want_x0: bool = False,
                   want_obstacles: bool = False, weights: Optional[Tensor] = None,
                   want_dbas: bool = False, tightening: Optional[Tensor] = None,
                   want_tight: bool = False) -> SolveGradient:
    """The gradient of an upper loss w.r.t. the plain cost weights and the references, per trajectory, from the
    loss's gradients ``grad_X`` [B, N+1, 4] / ``grad_V`` [B, N, 2] w.r.t. the tape (X [B, N+1, 4], V [B, N, 2]).

    The reference's IFT at the given tape with the Gauss-Newton L_zz of ddp_sensitivity and the active set frozen
    (see the module docstring): the gradient of the solver's output only where the solve has converged; the
    quantity the paper's Algorithm 2 uses.

    cost.kind 'track' needs X_ref [B, N+1, >=3] and U_ref [B, N, 2] and returns their gradient rows; 'target'
    returns the target's.  scenes ([3M + 3, B], pack_scenes): trajectory i linearises with its own obstacles and a
    target cost uses its own target (fused f32 kernel only).  check: raise FloatingPointError on a non-finite row
    (else see ``status``).

    want_x0 / want_obstacles: also the rows w.r.t. the start state (``x0`` [B, 4]: x, y, heading, b) and the circles
    (``obstacles`` [B, M, 3]: cx, cy, r -- trajectory i's own circles with scenes, whose radii are the roots of the
    scene's squared radii).  x0 rows come on every path; obstacle rows need smooth-min aggregation and the relaxed
    inverse barrier (the fused kernel, or on f64 the composition without scenes).

    weights ([9, B] float32, pack_weights): trajectory i is differentiated with its own Q, R, Qf, qb (``cost``'s nine
    weights are then unused), so ``X_ref`` / ``target`` rows carry its own Q / Qf and row i of ``weights`` in the
    result is the gradient w.r.t. column i of the array.  Fused f32 kernel only (dtmpc_solve_backward_weights, any
    dbas_gamma): the composition paths (f64, min / single aggregation, the log barrier) raise ValueError.

    want_dbas: also the rows w.r.t. the barrier-state parameters (``dbas`` [B, 2]: alpha, gamma; the module docstring's
    formulas, the alpha row with d max(alpha, eps) / d alpha applied).  The fused kernel (dtmpc_solve_backward_dbas:
    composes with scenes, weights, want_x0 and want_obstacles in the one launch) or, on f64, the composition without
    scenes; like the obstacle rows they need smooth-min aggregation and the relaxed inverse barrier, else ValueError.
    On a tape whose b_0 is the barrier of its own start position the gamma row is zero up to rounding (see the module
    docstring): it carries information only for a solve started from a disturbed or chained barrier state.

    tightening ([B] float32): the tape is that of a solve whose barrier saw h(x) - s_i (``ilqr_solve(tightening=)``);
    every row is then evaluated under the tightened h (see the module docstring) and, with want_tight, ``tight`` [B]
    holds d loss / d s_i.  ``problem.h_offset`` stays 0: the array is the only source of s.  Fused f32 kernel only
    (dtmpc_solve_backward_tight, any dbas_gamma; composes with scenes, weights, want_x0, want_obstacles and want_dbas in
    the one launch): the composition paths (f64, min / single aggregation, the log barrier) raise ValueError."""
    if want_tight and tightening is None:
        raise ValueError("solve_backward: want_tight needs tightening ([B])")
    if cost.wrap_angle:
        raise ValueError("solve_backward: a cost with wrap_angle is not supported (the reference's sensitivity "
                         "closures carry no wrapped heading error)")
    _require_device(X, V, grad_X, grad_V, X_ref, U_ref, scenes, weights, tightening)
    B, N = X.shape[0], problem.horizon
    if X.shape != (B, N + 1, 4) or V.shape != (B, N, 2):
        raise ValueError(f"X must be [B, {N + 1}, 4] and V [B, {N}, 2]")
    if grad_X.shape != (B, N + 1, 4) or grad_V.shape != (B, N, 2):
        raise ValueError(f"grad_X must be [{B}, {N + 1}, 4] and grad_V [{B}, {N}, 2]")
    track = cost.kind == "track"
    if track and (X_ref is None or U_ref is None):
        raise ValueError("the tracking cost needs X_ref and U_ref")
    if not track and (X_ref is not None or U_ref is not None):
        raise ValueError("X_ref / U_ref go with the tracking cost")
    lib = _lib.load()
    spec, cc = problem.to_c(), cost.to_c()
    dt, dev = X.dtype, X.device
    kw = dict(dtype=dt, device=dev)
    geom = want_x0 or want_obstacles
    M = len(problem.obstacles)
    fused = bool(lib.dtmpc_solve_backward_supported(_dtype_code(X), C.byref(spec), C.byref(cc)))
    if fused:
        if scenes is not None:
            check_scenes(scenes, M, B, dt, dev)
        if weights is not None:
            check_weights(weights, B, dev)
        if tightening is not None:
            check_tightening(tightening, B, dev)
        Xs, Us, gx, gu = to_soa(X), to_soa(V.to(dt)), to_soa(grad_X.to(dt)), to_soa(grad_V.to(dt))
        Xr = to_soa(X_ref[..., :3].to(dt)) if track else None
        Ur = to_soa(U_ref.to(dt)) if track else None
        gw = torch.empty(9, B, **kw)
        gt = None if track else torch.empty(3, B, **kw)
        gxr = torch.empty(N + 1, 3, B, **kw) if track else None
        gur = torch.empty(N, 2, B, **kw) if track else None
        gx0 = torch.empty(4, B, **kw) if want_x0 else None
        gob = torch.empty(3, M, B, **kw) if want_obstacles else None
        gdb = torch.empty(2, B, **kw) if want_dbas else None
        gtg = torch.empty(B, **kw) if tightening is not None else None
        if tightening is not None:
            wb = int(lib.dtmpc_solve_backward_tight_workspace_bytes(_dtype_code(X), N, B))
        elif want_dbas:
            wb = int(lib.dtmpc_solve_backward_dbas_workspace_bytes(_dtype_code(X), N, B))
        elif weights is not None:
            wb = int(lib.dtmpc_solve_backward_weights_workspace_bytes(_dtype_code(X), N, B, 1 if geom else 0))
        else:
            nbytes = (lib.dtmpc_solve_backward_geom_workspace_bytes if geom
                      else lib.dtmpc_solve_backward_workspace_bytes)
            wb = int(nbytes(_dtype_code(X), N, B))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        head = (_dtype_code(X), C.byref(spec), C.byref(cc), B, Xs.data_ptr(), Us.data_ptr(), _ptr(Xr), _ptr(Ur),
                _ptr(scenes), gx.data_ptr(), gu.data_ptr(), gw.data_ptr(), _ptr(gt), _ptr(gxr), _ptr(gur))
        tail = (work.data_ptr(), wb, status.data_ptr(), _lib.stream_of(X))
        if tightening is not None:  # the TIGHT family: the GEOM record, weights / x0 / obstacle / DBaS rows as asked for
            _lib.check(lib.dtmpc_solve_backward_tight(*head[:9], _ptr(weights), tightening.data_ptr(), *head[9:],
                                                      _ptr(gx0), _ptr(gob), _ptr(gdb), gtg.data_ptr(), *tail),
                       "dtmpc_solve_backward_tight")
        elif want_dbas:  # the DBAS family: the GEOM record, weights / x0 / obstacle rows as asked for
            _lib.check(lib.dtmpc_solve_backward_dbas(*head[:9], _ptr(weights), *head[9:], _ptr(gx0), _ptr(gob),
                                                     gdb.data_ptr(), *tail), "dtmpc_solve_backward_dbas")
        elif weights is not None:  # the WTS family: the plain record, or the GEOM one when x0 / obstacle rows are wanted
            _lib.check(lib.dtmpc_solve_backward_weights(*head[:9], weights.data_ptr(), *head[9:], _ptr(gx0), _ptr(gob),
                                                        *tail), "dtmpc_solve_backward_weights")
        elif geom:  # the GEOM variant of the kernel: the same rows, and those w.r.t. x0 / (cx, cy, r^2)
            _lib.check(lib.dtmpc_solve_backward_geom(*head, _ptr(gx0), _ptr(gob), *tail), "dtmpc_solve_backward_geom")
        else:
            _lib.check(lib.dtmpc_solve_backward(*head, *tail), "dtmpc_solve_backward")
        rows = None
        if want_obstacles:  # d r^2 / d r = 2 r; a scene holds r^2 only
            if scenes is not None:
                r = torch.sqrt(scenes[2 * M:3 * M])  # [M, B]
            else:
                r = torch.tensor([o.radius for o in problem.obstacles], **kw)[:, None]
            rows = torch.stack([gob[0], gob[1], gob[2] * (2.0 * r)], 2).permute(1, 0, 2).contiguous()
        out = SolveGradient(weights=gw.t().contiguous(), target=None if track else gt.t().contiguous(),
                            X_ref=from_soa(gxr) if track else None, U_ref=from_soa(gur) if track else None,
                            status=status, x0=gx0.t().contiguous() if want_x0 else None, obstacles=rows,
                            dbas=_dbas_host(problem, gdb) if want_dbas else None,
                            tight=gtg if want_tight else None)
    else:
        if tightening is not None:
            raise ValueError("solve_backward: a per-trajectory tightening needs the fused kernel "
                             "(dtmpc_solve_backward_supported: f32, smooth-min, 1..8 obstacles, inverse barrier)")
        if weights is not None:
            raise ValueError("solve_backward: per-trajectory weights need the fused kernel "
                             "(dtmpc_solve_backward_supported: f32, smooth-min, 1..8 obstacles, inverse barrier)")
        if scenes is not None:
            raise ValueError("solve_backward: per-trajectory scenes need the fused kernel "
                             "(dtmpc_solve_backward_supported: f32, smooth-min, 1..8 obstacles, inverse barrier)")
        if spec.h_offset != 0.0:
            raise ValueError("solve_backward: a tightened h (h_offset) is not supported")
        if want_obstacles and (problem.obs_aggregation != "smoothmin" or problem.barrier_type != "inverse" or M < 1):
            raise ValueError("solve_backward: obstacle rows need smooth-min aggregation and the relaxed inverse "
                             "barrier (min / single aggregation have no softmax weights; the log barrier's rows "
                             "are not provided)")
        if want_dbas and (problem.obs_aggregation != "smoothmin" or problem.barrier_type != "inverse" or M < 1):
            raise ValueError("solve_backward: the DBaS rows need smooth-min aggregation and the relaxed inverse "
                             "barrier (the log barrier's rows are not provided)")
        s = _ddp_sensitivity_upper(problem, cost, X, V, grad_X, grad_V, geom or want_dbas, False)
        dX, dV = s.delta_X, s.delta_V
        Q = torch.tensor(cost.Q, **kw)
        R = torch.tensor(cost.R, **kw)
        Qf = torch.tensor(cost.Qf, **kw)
        if track:
            r, ub = X_ref[..., :3].to(dt), U_ref.to(dt)
        else:
            r = torch.tensor(cost.target, **kw).expand(B, N + 1, 3)
            ub = torch.zeros(B, N, 2, **kw)
        ex = X[..., :3] - r
        gQ = (2.0 * ex[:, :N] * dX[:, :N, :3]).sum(1)
        gR = (2.0 * (V.to(dt) - ub) * dV).sum(1)
        gQf = 2.0 * ex[:, N] * dX[:, N, :3]
        gqb = (2.0 * X[..., 3] * dX[..., 3]).sum(1, keepdim=True)
        gxr = torch.cat([-2.0 * Q * dX[:, :N, :3], (-2.0 * Qf * dX[:, N, :3])[:, None]], 1)
        gur = -2.0 * R * dV
        gw = torch.cat([gQ, gR, gQf, gqb], 1)
        gt = None if track else gxr.sum(1)
        gx0 = s.delta_lambda[:, 0].contiguous() if want_x0 else None
        gob = _obstacle_rows(problem, X, s.delta_lambda) if want_obstacles else None
        gdb = _dbas_rows(problem, X, s.delta_lambda) if want_dbas else None
        status = _nonfinite_status(gw, gt, gxr if track else None, gur if track else None, dX[:, N], gx0, gob, gdb)
        out = SolveGradient(weights=gw, target=gt, X_ref=gxr if track else None, U_ref=gur if track else None,
                            status=status, x0=gx0, obstacles=gob,
                            dbas=_dbas_host(problem, gdb.t()) if want_dbas else None)
    if check:
        raise_for_status(out.status, "solve_backward")
    return out


class _Solve(torch.autograd.Function):
    """X*, V* of a finished solve as functions of the weight / reference tensors (and, named in ``wrt``, of the
    start state and the obstacle circles: x0 / obstacles are None otherwise; dbas_alpha / dbas_gamma: the layer's
    arguments of those names or None; tight: the packed [B] tightening the solve ran with, tightening: the layer's
    argument it came from): forward hands the tape through, backward is solve_backward at that tape."""

    @staticmethod
    def forward(ctx, X, V, problem, cost, scenes, per_traj_target, nref, Q, R, Qf, qb, target, X_ref, U_ref,
                x0=None, obstacles=None, weights=None, dbas_alpha=None, dbas_gamma=None, tight=None, tightening=None):
        ctx.problem, ctx.cost, ctx.scenes = problem, cost, scenes
        ctx.weights = weights  # [9, B] packed (detached) or None: Q, R, Qf, qb are then [B, .] and get their rows
        ctx.per_traj_target, ctx.nref = per_traj_target, nref
        ctx.shapes = tuple(None if t is None else (t.shape, t.dtype)
                           for t in (Q, R, Qf, qb, target, X_ref, U_ref, x0, obstacles))
        ctx.dbas_shapes = tuple(None if t is None else (t.shape, t.dtype) for t in (dbas_alpha, dbas_gamma))
        ctx.tight = tight  # [B] float32 (detached) or None
        ctx.tight_shape = None if tightening is None else (tightening.shape, tightening.dtype)
        ctx.save_for_backward(X, V, *(t for t in (X_ref, U_ref) if t is not None))
        ctx.flagged = None
        return X.clone(), V.clone()

    @staticmethod
    def backward(ctx, gX, gV):
        X, V, *refs = ctx.saved_tensors
        Xr, Ur = (refs + [None, None])[:2]
        gX = torch.zeros_like(X) if gX is None else gX
        gV = torch.zeros_like(V) if gV is None else gV
        sh = ctx.shapes
        need = ctx.needs_input_grad[7:]
        dsh = ctx.dbas_shapes
        need_db = tuple(dsh[j] is not None and need[10 + j] for j in range(2))
        g = solve_backward(problem=ctx.problem, cost=ctx.cost, X=X, V=V, grad_X=gX.contiguous(),
                           grad_V=gV.contiguous(), X_ref=None if Xr is None else Xr.detach(),
                           U_ref=None if Ur is None else Ur.detach(), scenes=ctx.scenes, weights=ctx.weights,
                           check=False,
                           want_x0=sh[7] is not None and need[7], want_obstacles=sh[8] is not None and need[8],
                           want_dbas=any(need_db), tightening=ctx.tight,
                           want_tight=ctx.tight is not None and need[13])
        keep = (g.status == 0)
        ctx.flagged = g.status  # [B] int32: the trajectories left out of this backward

        def rows(t):  # flagged trajectories contribute zero rows (where, not a product: their rows may hold NaN)
            return None if t is None else torch.where(keep.view(-1, *([1] * (t.dim() - 1))), t, torch.zeros_like(t))

        w = rows(g.weights)
        ws = w if ctx.weights is not None else w.sum(0)  # per-trajectory weights: the rows, unsummed
        out = [None] * 9
        for j, sl in enumerate((slice(0, 3), slice(3, 5), slice(5, 8), slice(8, 9))):
            if sh[j] is not None and need[j]:
                out[j] = ws[..., sl].reshape(sh[j][0]).to(sh[j][1])
        if sh[4] is not None and need[4] and g.target is not None:
            t = rows(g.target)
            out[4] = (t if ctx.per_traj_target else t.sum(0)).reshape(sh[4][0]).to(sh[4][1])
        if sh[5] is not None and need[5] and g.X_ref is not None:
            gx = rows(g.X_ref)
            if ctx.nref > 3:  # the solver reads three columns of X_ref: the others get zeros
                gx = torch.cat([gx, gx.new_zeros(*gx.shape[:2], ctx.nref - 3)], 2)
            out[5] = gx.to(sh[5][1])
        if sh[6] is not None and need[6] and g.U_ref is not None:
            out[6] = rows(g.U_ref).to(sh[6][1])
        if g.x0 is not None:
            out[7] = rows(g.x0).to(sh[7][1])
        if g.obstacles is not None:  # [M, 3]: the shared circles get the sum over the batch
            o = rows(g.obstacles)
            out[8] = (o.sum(0) if len(sh[8][0]) == 2 else o).to(sh[8][1])
        gdb = [None, None]
        if g.dbas is not None:  # one value each: the sum of the unflagged trajectories' rows
            d = rows(g.dbas).sum(0)
            for j in range(2):
                if need_db[j]:
                    gdb[j] = d[j].reshape(dsh[j][0]).to(dsh[j][1])
        gtg = None
        if g.tight is not None:  # [B]: the rows, unsummed; a shared value: the sum of the unflagged trajectories' rows
            t = rows(g.tight)
            tsh, tdt = ctx.tight_shape
            gtg = (t.sum(0) if tsh.numel() == 1 else t).reshape(tsh).to(tdt)
        return (None,) * 7 + tuple(out) + (None,) + tuple(gdb) + (None, gtg)


@dataclass(frozen=True)
class DiffILQRResult(ILQRResult):
    """ILQRResult whose X / V carry a grad_fn; ``backward_status()`` gives the last backward's per-trajectory
    status ([B] int32, None before any backward): non-zero trajectories contributed zero rows."""

    _node: object = None

    def backward_status(self) -> Optional[Tensor]:
        return getattr(self._node, "flagged", None)


def diff_ilqr_solve(*, problem: DubinsDBaSProblem, cfg: ILQRConfig, kind: str, Q: Tensor, R: Tensor, Qf: Tensor,
                    qb: Tensor, x0: Tensor, V_init: Tensor, target: Optional[Tensor] = None,
                    X_ref: Optional[Tensor] = None, U_ref: Optional[Tensor] = None,
                    obstacles: Optional[Tensor] = None, lanes: int = 0, check: bool = True,
                    wrt: Sequence[str] = (), dbas_alpha: Optional[Tensor] = None,
                    dbas_gamma: Optional[Tensor] = None, tightening: Optional[Tensor] = None) -> ILQRResult:
    """``ilqr_solve`` whose X* / V* are differentiable w.r.t. Q [3], R [2], Qf [3], qb [], the target ([3] shared
    or [B, 3] per trajectory; kind 'target') and X_ref [B, N+1, >=3] / U_ref [B, N, 2] (kind 'track').

    Per-trajectory weights: each of Q, R, Qf may also be [B, k] and qb [B].  With all four shared the path is the
    shared one, unchanged; with any of them per trajectory the shared ones are expanded, the solve runs
    ``ilqr_solve(weights=)`` and the backward ``solve_backward(weights=)``: a [B, k] tensor's ``.grad`` is its rows,
    unsummed, a shared one's the column sum.  float32 on a configuration ``dtmpc_weights_supported`` accepts
    (dbas_gamma == 0 among the rest), else ValueError.

    Forward is exactly ``ilqr_solve`` (the same kernels, bitwise the same X*, V*): with a [B, 3] target or
    ``obstacles`` [B, M, 3] it runs ``ilqr_solve(..., scenes=pack_scenes(...))``.  The QuadraticCost is built from
    the weight tensors' VALUES -- host doubles in the ABI -- so every call makes one device-to-host read of the
    nine weights (and of a shared target): it synchronises the stream.

    Backward is ``solve_backward`` at the returned tape with the incoming gradients (a missing one is zeros): the
    reference's IFT with the Gauss-Newton L_zz of ddp_sensitivity and the active set frozen -- the gradient of the
    solver's output only where the solve has converged, the quantity the paper's Algorithm 2 uses.  Shared tensors
    (Q, R, Qf, qb, a [3] target) receive the sum of the per-trajectory rows, a [B, 3] target and the references
    their rows; a fourth column of X_ref gets zeros.  A trajectory whose backward is flagged (non-finite row)
    contributes zero rows; ``result.backward_status()`` holds the flags of the last backward.  The same tensor
    passed twice (say as Q and Qf) accumulates both gradients, as autograd does.

    wrt (opt-in): ``"x0"`` -- x0 [B, 4] may require grad and receives its rows (g_x0 = dlam_0; b_0's dependence on
    the position is the caller's: ``dbas_init_b0`` is differentiable), so solves chain: plan, step the plant, plan
    again, one ``backward()`` through both.  ``"obstacles"`` -- ``obstacles`` ([B, M, 3] per trajectory, or [M, 3]
    shared, expanded through ``pack_scenes``) may require grad and receives its rows (the [M, 3] form their sum over
    the batch), see the module docstring.

    dbas_alpha / dbas_gamma (opt-in): a zero-dim or one-element tensor each, whose VALUE replaces ``problem``'s float
    of that name in the forward and the backward (read in the same device-to-host read as the weights) and which, if
    it requires grad, receives the sum of the unflagged trajectories' rows of ``solve_backward(want_dbas=True)`` (the
    module docstring's formulas; a learnable parameterisation such as softplus / tanh is the caller's, in torch).  On
    a solve whose b_0 is the barrier of its start position the gamma gradient is zero up to rounding: it carries
    information for a disturbed or chained start state.  A [B] tensor is refused: per-trajectory DBaS parameters
    are not built (they would need forward kernels).  Passing neither leaves every path as it is.

    tightening (opt-in): a [B] tensor (trajectory i's barrier sees h(x) - s_i) or a zero-dim / one-element tensor (one
    s for the batch), used in the forward (``ilqr_solve(tightening=)``) and the backward
    (``solve_backward(tightening=)``).  If it requires grad a [B] tensor receives the unsummed rows (flagged
    trajectories zero), a shared one the sum over the unflagged trajectories; a softplus parameterisation is the
    caller's, in torch.  x0[:, 3] is the caller's: ``dbas_init(problem, x, tightening=)`` gives the consistent
    B(h(x_0) - s_i).  float32 on a configuration ``dtmpc_tight_supported`` accepts; refused together with
    per-trajectory weights and with a non-zero ``problem.dbas_gamma`` / ``dbas_gamma=`` (the tightened forward has
    neither).  Composes with ``wrt``, ``dbas_alpha=``, ``obstacles=`` and shared weights.

    Refused: without ``wrt`` gradients w.r.t. x0 and obstacles; always w.r.t. V_init (the warm start is not an
    argument of the optimum), a wrapped heading error, ``problem.dbas_*`` / ``problem.obs_beta`` as tensors (alpha
    and gamma go through ``dbas_alpha=`` / ``dbas_gamma=``; gradients w.r.t. dbas_eps and obs_beta are not provided).
    check: the forward raises as ``ilqr_solve`` does."""
    if kind not in ("target", "track"):
        raise ValueError(f"unknown cost kind {kind!r}")
    if isinstance(wrt, str) or any(w not in ("x0", "obstacles") for w in wrt):
        raise ValueError(f"diff_ilqr_solve: wrt is a sequence of 'x0' and / or 'obstacles', got {wrt!r}")
    wrt_x0, wrt_obs = "x0" in wrt, "obstacles" in wrt
    if wrt_obs and not isinstance(obstacles, Tensor):
        raise ValueError("diff_ilqr_solve: wrt 'obstacles' needs obstacles as a tensor ([B, M, 3] or [M, 3])")
    if V_init.requires_grad and wrt_x0:
        raise ValueError("diff_ilqr_solve: no gradient w.r.t. V_init -- the warm start is not an argument of the "
                         "optimum; detach it")
    if (x0.requires_grad and not wrt_x0) or V_init.requires_grad:
        raise ValueError("diff_ilqr_solve: no gradient w.r.t. x0 or V_init -- the reference's IFT detaches the "
                         "initial state (xi), and the warm start is not an argument of the optimum; detach them")
    if obstacles is not None and isinstance(obstacles, Tensor) and obstacles.requires_grad and not wrt_obs:
        raise ValueError("diff_ilqr_solve: no gradient w.r.t. the obstacle geometry; detach obstacles")
    for name in ("dbas_alpha", "dbas_gamma"):
        if isinstance(getattr(problem, name), Tensor):
            raise ValueError(f"diff_ilqr_solve: problem.{name} must be a float -- pass the tensor as the argument "
                             f"{name}= of diff_ilqr_solve to receive its gradient (the raw-parameter chain stays "
                             "ift_gradient's)")
    for name in ("dbas_eps", "obs_beta"):
        if isinstance(getattr(problem, name), Tensor):
            raise ValueError(f"diff_ilqr_solve: problem.{name} must be a float -- gradients w.r.t. dbas_eps and "
                             "obs_beta are not provided")
    B, N = x0.shape[0], problem.horizon
    dbas = tuple((name, t) for name, t in (("dbas_alpha", dbas_alpha), ("dbas_gamma", dbas_gamma)) if t is not None)
    for name, t in dbas:
        if not isinstance(t, Tensor):
            raise ValueError(f"diff_ilqr_solve: {name} is a zero-dim or one-element tensor (a float goes in problem)")
        if t.numel() != 1:
            raise ValueError(f"diff_ilqr_solve: {name} must be a zero-dim or one-element tensor, got "
                             f"{tuple(t.shape)} -- per-trajectory DBaS parameters are not built (they would need "
                             "forward kernels)")
    if tightening is not None:
        if not isinstance(tightening, Tensor):
            raise ValueError("diff_ilqr_solve: tightening is a tensor ([B], or zero-dim / one-element for a shared value)")
        if tightening.numel() != 1 and tuple(tightening.shape) != (B,):
            raise ValueError(f"diff_ilqr_solve: tightening must be [{B}] or a zero-dim / one-element tensor, got "
                             f"{tuple(tightening.shape)}")
        if x0.dtype != torch.float32:
            raise ValueError("diff_ilqr_solve: a tightening needs float32 (dtmpc_tight_supported)")
        if dbas_gamma is not None or float(problem.dbas_gamma) != 0.0:
            raise ValueError("diff_ilqr_solve: a tightening needs dbas_gamma == 0 in the forward solve "
                             "(dtmpc_tight_supported); solve_backward(tightening=) takes any gamma")
    # the weights' shapes (before anything needs a device): all four shared -- today's path -- or any per trajectory
    # (a one-element qb beside 1-D Q, R, Qf is the shared form, as it always was)
    shared_w = not (Q.dim() == 2 or R.dim() == 2 or Qf.dim() == 2 or (qb.dim() == 1 and qb.numel() != 1))
    if shared_w:
        if Q.shape != (3,) or R.shape != (2,) or Qf.shape != (3,) or qb.numel() != 1:
            raise ValueError("Q [3], R [2], Qf [3], qb [] (shared weights)")
    else:
        for name, t, k in (("Q", Q, 3), ("R", R, 2), ("Qf", Qf, 3)):
            if tuple(t.shape) not in ((k,), (B, k)):
                raise ValueError(f"{name} must be [{k}] (shared) or [{B}, {k}] (per trajectory), got {tuple(t.shape)}")
        if tuple(qb.shape) not in ((), (B,)):
            raise ValueError(f"qb must be [] (shared) or [{B}] (per trajectory), got {tuple(qb.shape)}")
    if tightening is not None and not shared_w:
        raise ValueError("diff_ilqr_solve: per-trajectory weights together with a tightening are not built in the "
                         "forward solve; solve_backward takes both")
    _require_device(x0, V_init, Q, R, Qf, qb, target, X_ref, U_ref,
                    obstacles if isinstance(obstacles, Tensor) else None, tightening)
    track = kind == "track"
    if track and (X_ref is None or U_ref is None):
        raise ValueError("kind 'track' needs X_ref and U_ref")
    if track and target is not None:
        raise ValueError("target goes with kind 'target'")
    if not track and (X_ref is not None or U_ref is not None):
        raise ValueError("X_ref / U_ref go with kind 'track'")
    if not track and target is None:
        raise ValueError("kind 'target' needs target ([3] or [B, 3])")
    per_traj = (not track) and target.dim() == 2
    if not track and tuple(target.shape) not in ((3,), (B, 3)):
        raise ValueError(f"target must be [3] or [{B}, 3]")
    wts = None
    if not shared_w:
        # per-trajectory weights: the shared ones expanded to [B, .] OUTSIDE the autograd Function (autograd sums their
        # rows), the packed array to the kWts kernels; the QuadraticCost below keeps trajectory 0's values, unread
        if x0.dtype != torch.float32:
            raise ValueError("diff_ilqr_solve: per-trajectory weights need float32 (dtmpc_weights_supported)")
        Q = Q if Q.dim() == 2 else Q.expand(B, 3)
        R = R if R.dim() == 2 else R.expand(B, 2)
        Qf = Qf if Qf.dim() == 2 else Qf.expand(B, 3)
        qb = qb if qb.dim() == 1 else qb.expand(B)
        wts = pack_weights(Q, R, Qf, qb, device=x0.device)
    # one device-to-host read: the ABI's cost weights are host doubles
    host = torch.cat([t.detach().reshape(-1)[:k].to(torch.float64) for t, k in
                      ((Q, 3), (R, 2), (Qf, 3), (qb, 1)) + (((target, 3),) if (not track and not per_traj) else ())]
                     + [t.detach().reshape(-1).to(device=x0.device, dtype=torch.float64) for _, t in dbas]
                     ).cpu().tolist()
    if dbas:  # the DBaS values ride at the end of the same read
        problem = dataclasses.replace(problem, **{name: v for (name, _), v in zip(dbas, host[-len(dbas):])})
        host = host[:-len(dbas)]
    cost = QuadraticCost(kind=kind, Q=tuple(host[0:3]), R=tuple(host[3:5]), Qf=tuple(host[5:8]), qb=host[8],
                         target=tuple(host[9:12]) if len(host) > 9 else (0.0, 0.0, 0.0))
    tgt = None
    if tightening is not None:  # the packed [B] array both kernels read (a shared value broadcast)
        tgt = tightening.detach().to(device=x0.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    scenes = None
    if per_traj or obstacles is not None:
        obs = obstacles
        if isinstance(obs, Tensor) and obs.dim() == 2:  # shared circles: every trajectory's scene
            obs = obs.detach().expand(B, *obs.shape)
        if obs is None:
            obs = torch.tensor([[o.center[0], o.center[1], o.radius] for o in problem.obstacles],
                               dtype=torch.float64).expand(B, -1, 3)
        tg = target.detach() if per_traj else (torch.tensor(cost.target, dtype=torch.float64).expand(B, 3))
        scenes = pack_scenes(problem, obs, tg, dtype=x0.dtype, device=x0.device)
    res = ilqr_solve(problem=problem, cost=cost, cfg=cfg, x0=x0.detach(), V_init=V_init,
                     X_ref=None if X_ref is None else X_ref.detach(), U_ref=None if U_ref is None else U_ref.detach(),
                     check=check, debug_name="diff_ilqr_solve", lanes=lanes, scenes=scenes,
                     **({} if wts is None else {"weights": wts}), **({} if tgt is None else {"tightening": tgt}))
    nref = 0 if X_ref is None else X_ref.shape[-1]
    Xd, Vd = _Solve.apply(res.X, res.V, problem, cost, scenes, per_traj, nref, Q, R, Qf, qb, target, X_ref, U_ref,
                          x0 if wrt_x0 else None, obstacles if wrt_obs else None, wts, dbas_alpha, dbas_gamma, tgt, tightening)
    fields = {f.name: getattr(res, f.name) for f in dataclasses.fields(ILQRResult)}
    fields.update(X=Xd, V=Vd)
    return DiffILQRResult(**fields, _node=Xd.grad_fn)
