"""Weight sets for the per-trajectory-weights tests (tests/test_gpu_weights.py, tests/test_gpu_layer_weights.py,
tests/test_weights_host.py).

A weight set is one trajectory's nine plain cost weights Q(3) R(2) Qf(3) qb -- the row order of the weights array
[9][B] and of dtmpc_solve_backward's g_w.  Set 0 is a cost's own weights; the others multiply each of the nine by
exp(U(log 0.5, log 2)) from a fixed seed (a zero weight, the paper's Q2, stays zero).  Trajectory i of a batch gets
set i % W, so every wave mixes all of them; W = 5 is coprime to tests/_scenes.py's S = 4, so with heterogeneous
scenes every (scene, set) pair occurs."""
from __future__ import annotations

import dataclasses

import numpy as np

W = 5
SEED = 23


def nine_of(cost) -> np.ndarray:
    """[9] float64 of a QuadraticCost."""
    return np.array([*cost.Q, *cost.R, *cost.Qf, cost.qb], np.float64)


def weight_sets(cost, seed: int = SEED, tied_terminal: bool = False) -> np.ndarray:
    """[W, 9] float64; set 0 is `cost`'s own.  tied_terminal (the ancillary tracking cost, whose terminal weight is its
    stage weight): the six theta weights are scaled and Qf follows Q."""
    rng = np.random.default_rng(seed)
    base = nine_of(cost)
    sets = [base]
    for _ in range(1, W):
        w = base * np.exp(rng.uniform(np.log(0.5), np.log(2.0), 9))
        if tied_terminal:
            w[5:8] = w[0:3]
        sets.append(w)
    return np.stack(sets)


def cost_of(cost, w9):
    """`cost` with the nine weights w9 (its kind, target and wrap_angle kept)."""
    w = [float(v) for v in w9]
    return dataclasses.replace(cost, Q=tuple(w[0:3]), R=tuple(w[3:5]), Qf=tuple(w[5:8]), qb=w[8])


def assignment(n: int, chunk: int = 0) -> np.ndarray:
    """Trajectory i's set: i % W, or (i + i // chunk) % W, which shifts by one from launch chunk to launch chunk."""
    i = np.arange(n)
    return (i + (i // chunk if chunk else 0)) % W


def pack(sets: np.ndarray, k: np.ndarray, device):
    """The [9, B] weights tensor of a batch whose trajectory i has set k[i]."""
    from diff_tube_mpc_strict_pt.core import pack_weights

    w = sets[k]
    return pack_weights(w[:, 0:3], w[:, 3:5], w[:, 5:8], w[:, 8], device=device)
