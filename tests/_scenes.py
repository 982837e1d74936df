"""Scene tables for the per-trajectory-scenes tests (tests/test_gpu_scenes.py, tests/test_scenes_host.py).

A scene is one trajectory's environment: M circle obstacles (cx, cy, r) and the nominal target (x, y, heading).
Scene 0 is the base table and the paper's target; the others move each centre by up to +-0.3, draw the radii from
[0.8, 1.1] and move the target by up to +-1 in x and y and +-0.2 in heading, from a fixed seed.  Trajectory i of a
batch gets scene i % S, so every wave mixes all of them."""
from __future__ import annotations

import dataclasses

import numpy as np

from _common import paper_setup

S = 4
SEED = 11
# the base obstacle tables: the paper's five, the paper's five and three more, and the paper's central one
EXTRA = ((8.0, 8.0, 1.0), (2.0, 8.0, 1.0), (8.0, 2.0, 1.0))


def fixed_setup():
    """The paper setup at fixed iterations (tol = -1), N = 50."""
    st = paper_setup()
    return dataclasses.replace(st, ilqr_nom=dataclasses.replace(st.ilqr_nom, tol=-1.0),
                               ilqr_aux=dataclasses.replace(st.ilqr_aux, tol=-1.0))


def base_table(M: int) -> np.ndarray:
    """[M, 3] float64 (cx, cy, r): M = 5 the paper's table, 8 with EXTRA appended, 1 the circle at (6, 6)."""
    paper = np.array([[o.center[0], o.center[1], o.radius] for o in paper_setup().problem.obstacles], np.float64)
    if M == 5:
        return paper
    if M == 8:
        return np.concatenate([paper, np.array(EXTRA, np.float64)], 0)
    if M == 1:
        return paper[4:5].copy()
    raise ValueError(M)


def scene_table(M: int = 5, seed: int = SEED):
    """(obstacles [S, M, 3], targets [S, 3]) float64; scene 0 is the base table and the paper's target."""
    rng = np.random.default_rng(seed)
    base = base_table(M)
    tg0 = np.array(paper_setup().nominal_cost.target, np.float64)
    obs, tgs = [base], [tg0]
    for _ in range(1, S):
        o = base.copy()
        o[:, :2] += rng.uniform(-0.3, 0.3, (M, 2))
        o[:, 2] = rng.uniform(0.8, 1.1, M)
        obs.append(o)
        tgs.append(tg0 + rng.uniform(-1.0, 1.0, 3) * np.array([1.0, 1.0, 0.2]))
    return np.stack(obs), np.stack(tgs)


def setup_of(st, obstacles: np.ndarray, target: np.ndarray):
    """`st` with one scene as its (shared) problem and nominal target."""
    from diff_tube_mpc_strict_pt.core.problem import CircleObstacle

    obs = tuple(CircleObstacle(center=(float(o[0]), float(o[1])), radius=float(o[2])) for o in obstacles)
    return dataclasses.replace(st, problem=dataclasses.replace(st.problem, obstacles=obs),
                               nominal_cost=dataclasses.replace(st.nominal_cost,
                                                                target=tuple(float(v) for v in target)))


def starts(B: int, seed: int = 5) -> np.ndarray:
    """tests/test_gpu_lanes.py _x0: [B, 3] float64."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, 1, B), rng.uniform(0, 1, B), rng.uniform(0, np.pi / 2, B)], 1)
