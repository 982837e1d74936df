"""Golden vectors for the differentiable solve's rows w.r.t. the start state and the obstacle circles, produced by
RUNNING THE REFERENCE on CPU: ddp_sensitivity (core/ddp.py:317-427) with array upper gradients, then ift_gradient
(core/ift.py:35-92) with theta_tensors = [x0_hat, centres [M, 2], radii [M]], xi_fn = lambda: x0_hat and an f_fn
built from CircleObstacles whose fields are those tensors (h_circle_obstacle takes them as they are); f_jac sees
float copies of the same circles.

Usage (where make_golden.py finds the reference checkout; CPU only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_layer_geom.py

Like make_golden_layer.py the reference runs from a temporary copy and only inputs + outputs are stored
(layer_geom_f64.npz): six tapes, N <= 5, both cost kinds, gamma 0 and 0.3, alpha 0.05, rollouts of random controls
(a quarter of the entries on a bound of the box) from starts at an obstacle's rim, so both barrier branches occur."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

ALPHA = 0.05
CASES = [(1, "target", 0.0), (2, "track", 0.3), (3, "target", 0.3), (4, "track", 0.0), (5, "target", 0.0),
         (5, "track", 0.3)]


def main() -> None:
    sys.dont_write_bytecode = True
    root, cfg = _import_reference()
    import torch

    torch.set_num_threads(1)
    from diff_tube_mpc_strict_pt.core import barrier as rbar
    from diff_tube_mpc_strict_pt.core import ddp as rddp
    from diff_tube_mpc_strict_pt.core import ift as rift
    from diff_tube_mpc_strict_pt.core.control import BoxClampControl
    from diff_tube_mpc_strict_pt.core.systems import dubins as rdub
    from diff_tube_mpc_strict_pt.core.systems import dubins_aug_jac as raj
    from diff_tube_mpc_strict_pt.core.systems import dubins_obstacles as robs

    dtype = torch.float64
    sc = cfg["system"]
    circles = [(tuple(o["center"]), float(o["radius"])) for o in cfg["environment"]["obstacles"]]
    obs_f = [robs.CircleObstacle(center=c, radius=r) for c, r in circles]  # float copies: f_jac, the rollout
    beta = float(cfg["environment"]["obstacle_smoothmin_beta"])
    eps = float(cfg["dbas"]["eps"])
    dub = rdub.DubinsConfig(dt=float(sc["dt"]), v_max=10.0, omega_max=math.pi, x_target=tuple(sc["target"]))
    lo = torch.tensor([-10.0, -math.pi], dtype=dtype)
    hi = torch.tensor([10.0, math.pi], dtype=dtype)
    ctrl = BoxClampControl(u_min=lo, u_max=hi)
    f = lambda x, u: rdub.dubins_step(x, u, cfg=dub)  # noqa: E731
    g = torch.Generator().manual_seed(1357)
    out = {"n_cases": np.asarray(len(CASES)), "alpha": np.asarray(ALPHA),
           "circles": np.array([[c[0], c[1], r] for c, r in circles])}
    for ci, (N, kind, gamma) in enumerate(CASES):
        dbc = rbar.DBaSConfig(barrier_type="inverse", alpha=torch.tensor(ALPHA, dtype=dtype),
                              gamma=torch.tensor(gamma, dtype=dtype), eps=eps)
        fjac = lambda xh_, vk: raj.dubins_augmented_jacobian(xh_, vk, cfg=dub, obs=obs_f, obs_beta=beta,  # noqa: E731
                                                              obs_agg="smoothmin", db_cfg=dbc)
        centres = torch.tensor([c for c, _ in circles], dtype=dtype).requires_grad_(True)  # [M, 2]
        radii = torch.tensor([r for _, r in circles], dtype=dtype).requires_grad_(True)    # [M]
        obs_t = [robs.CircleObstacle(center=(centres[j, 0], centres[j, 1]), radius=radii[j])
                 for j in range(len(circles))]

        def f_hat_of(obstacles):
            h = lambda x_in: robs.h_multi_circle_obstacles(x_in, obstacles=obstacles, beta=beta)  # noqa: E731

            def f_hat(xk, uk):
                xn, bn = rbar.dbas_step(x_k=xk[:-1], u_k=uk, b_k=xk[-1], f=f, h=h, cfg=dbc)
                return torch.cat([xn, bn.view(1)], 0)

            return f_hat, h

        f_hat, h = f_hat_of(obs_f)
        f_hat_t, _ = f_hat_of(obs_t)
        o = obs_f[ci % len(obs_f)]
        ang = 2 * math.pi * torch.rand(1, generator=g, dtype=dtype).item()
        r0 = o.radius + 0.02 * (ci - 2)  # just inside .. just outside the rim
        x = torch.tensor([o.center[0] + r0 * math.cos(ang), o.center[1] + r0 * math.sin(ang), ang + math.pi + 0.3],
                         dtype=dtype)
        b0 = rbar.dbas_init_b0(x, h=h, cfg=dbc)
        V = (torch.rand(N, 2, generator=g, dtype=dtype) * 1.2 - 0.6) * hi
        on = torch.rand(N, 2, generator=g, dtype=dtype) < 0.25
        side = torch.rand(N, 2, generator=g, dtype=dtype) < 0.5
        V = torch.where(on, torch.where(side, lo.expand(N, 2), hi.expand(N, 2)), V)
        if N >= 2:
            V[0, 0], V[1, 1] = hi[0], lo[1]  # both channels on a bound somewhere
        X = [torch.cat([x, torch.as_tensor(b0, dtype=dtype).view(1)])]
        for k in range(N):
            X.append(f_hat(X[-1], V[k]))
        X = torch.stack(X).detach()
        gX = torch.randn(N + 1, 4, generator=g, dtype=dtype)
        gU = torch.randn(N, 2, generator=g, dtype=dtype)
        W = torch.cat([torch.rand(3, generator=g, dtype=dtype) * 2 + 0.1, torch.rand(2, generator=g, dtype=dtype) + 0.2,
                       torch.rand(3, generator=g, dtype=dtype) * 30 + 1, torch.rand(1, generator=g, dtype=dtype) + 0.1])
        Q, R, Qf, qb = W[0:3], W[3:5], W[5:8], W[8]
        track = kind == "track"
        tgt = torch.tensor(dub.x_target, dtype=dtype)
        Xr = X[:, :3] + 0.1 * torch.randn(N + 1, 3, generator=g, dtype=dtype)
        Ur = V + 0.1 * torch.randn(N, 2, generator=g, dtype=dtype)

        def sc_(xh, v, k):
            d = xh[:-1] - (Xr[k] if track else tgt)
            du = v - Ur[k] if track else v
            return (Q * d * d).sum() + (R * du * du).sum() + qb * (xh[-1] * xh[-1])

        def tc_(xh):
            d = xh[:-1] - (Xr[N] if track else tgt)
            return (Qf * d * d).sum() + qb * (xh[-1] * xh[-1])

        lxx = torch.diag(torch.cat([2 * W[0:3], 2 * W[8:9]]))
        luu = torch.diag(2 * W[3:5])
        pxx = torch.diag(torch.cat([2 * W[5:8], 2 * W[8:9]]))
        s = rddp.ddp_sensitivity(X=X, V=V, f=f_hat, f_jac=fjac, ctrl=ctrl,
                                 stage_hess=lambda x_, v_, k: (lxx, luu, torch.zeros(2, 4, dtype=dtype)),
                                 terminal_hess=lambda x_: pxx, upper_grad_x=lambda x_, k: gX[k],
                                 upper_grad_u=lambda u_, k: gU[k], upper_grad_xN=lambda x_: gX[N])
        x0_hat = X[0].detach().clone().requires_grad_(True)
        tens = [x0_hat, centres, radii]
        gr = rift.ift_gradient(inputs=rift.IFTInputs(X=X, V=V, delta_X=s.delta_X, delta_V=s.delta_V,
                                                     delta_lambda=s.delta_lambda),
                               theta_tensors=tens, xi_fn=lambda: x0_hat, f_fn=f_hat_t, stage_cost_fn=sc_,
                               terminal_cost_fn=tc_)
        gr = [torch.zeros_like(t) if gi is None else gi.detach() for gi, t in zip(gr, tens)]
        p = f"c{ci}_"
        out[p + "kind"] = np.asarray(1 if track else 0)
        out[p + "gamma"] = np.asarray(gamma)
        for nm, v in (("X", X), ("V", V), ("gX", gX), ("gU", gU), ("W", W), ("target", tgt), ("Xref", Xr), ("Uref", Ur)):
            out[p + nm] = v.numpy()
        out[p + "g_x0"] = gr[0].numpy()
        out[p + "g_obs"] = torch.cat([gr[1], gr[2][:, None]], 1).numpy()  # [M, 3]: cx, cy, r
        hv = torch.stack([h(xx[:3]) for xx in X])
        print(f"[layer geom {ci}] N={N} {kind} gamma={gamma}: h in [{float(hv.min()):.3f}, {float(hv.max()):.3f}], "
              f"|g_x0| max {float(np.abs(out[p + 'g_x0']).max()):.3g}, |g_obs| max "
              f"{float(np.abs(out[p + 'g_obs']).max()):.3g}, active {int(ctrl.active_mask(V).sum())}/{2 * N}")
    np.savez_compressed(os.path.join(HERE, "layer_geom_f64.npz"), **out)
    print("layer geometry golden vectors written to", HERE)


if __name__ == "__main__":
    main()
