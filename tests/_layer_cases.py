"""Cases, launches and reference evaluations of tests/test_gpu_layer_all_m.py and tests/test_layer_gate_teeth.py (and of
scripts/layer_sharp_gate.py, which measures the gate's constants from them).

Cases: tests/test_gpu_layer.py's twelve (M in {1, 5, 8}) and ten more by the same recipe (make_case: an oracle rollout
of random controls, a quarter of the entries on a bound, dbas_alpha = 0.05, starts uniform on [0, 10]^2 so that some lie
inside a rim) at M in {2, 3, 4, 6, 7} x both kinds; the obstacles are the first M of the paper's five circles followed
by test_gpu_layer._obstacles' three extras.  Every new M sees N = 50 once, B = 257 once and each gamma once.

A launch is one call of core.solve_backward; LAUNCHES maps each to the kernel family it reaches (core/layer.py's choice
of entry point and csrc/dtmpc_fast_layer.hip's LayerOpt / launch_block) and to the tape it runs on:
    tape "plain": make_case's;  "dbas": b_0 offset (test_gpu_layer_dbas.dbas_case), without which the gamma row is zero;
    "tight": that with a per-trajectory s and re-rolled (test_gpu_layer_tight.tight_case).
With wts the trajectories carry tests/_weights.py's five weight sets (trajectory i -> set i % 5) and every reference is
evaluated sub-batch by sub-batch with that set's cost, as tests/test_gpu_layer_weights.py does."""
from __future__ import annotations

import functools

import numpy as np

from _layer import layer_rows
from _layer_dbas import dbas_rows
from _layer_geom import geom_rows
from _layer_tight import tight_rows
from _weights import W, assignment, cost_of, weight_sets
from test_gpu_layer import CASES as OLD_CASES
from test_gpu_layer import make_case

# (N, B, M, kind, gamma, seed)
NEW_CASES = [
    (50, 65, 2, "target", 0.3, 41),
    (3, 257, 2, "track", 0.0, 42),
    (3, 257, 3, "target", 0.3, 43),
    (50, 65, 3, "track", 0.0, 51),  # (seed 44 has no trajectory with two significant obstacles and a band of 1e-3)
    (50, 65, 4, "target", 0.0, 45),
    (3, 257, 4, "track", 0.3, 46),
    (3, 257, 6, "target", 0.0, 47),
    (50, 65, 6, "track", 0.3, 48),
    (50, 65, 7, "target", 0.3, 49),
    (3, 257, 7, "track", 0.0, 50),
]
ALL_CASES = list(OLD_CASES) + NEW_CASES


def case_id(c):
    return f"N{c[0]}-B{c[1]}-M{c[2]}-{c[3]}-g{c[4]}"


ROW_KEYS = ("weights", "target", "X_ref", "U_ref")
GEOM_KEYS = ("x0", "obstacles")
DBAS_KEYS = ("alpha", "gamma")
TIGHT_KEYS = ("tight",)
FAMILY = {**{k: "rows" for k in ROW_KEYS}, **{k: "geom" for k in GEOM_KEYS}, **{k: "dbas" for k in DBAS_KEYS},
          **{k: "tight" for k in TIGHT_KEYS}}
FAMILIES = ("rows", "geom", "dbas", "tight")

# name: (kernel family, its flag FL or None, tape, per-trajectory weights, output keys beside the weight / reference
# rows)
LAUNCHES = {
    "plain": ("LK", None, "plain", False, ()),
    "geom": ("LKG", None, "plain", False, GEOM_KEYS),
    "weights": ("LKW", False, "plain", True, ()),
    "weights-geom": ("LKW", True, "plain", True, GEOM_KEYS),
    "dbas": ("LKD", False, "dbas", False, GEOM_KEYS + DBAS_KEYS),
    "dbas-weights": ("LKD", True, "dbas", True, GEOM_KEYS + DBAS_KEYS),
    "tight": ("LKT", False, "tight", False, GEOM_KEYS + DBAS_KEYS + TIGHT_KEYS),
    "tight-weights": ("LKT", True, "tight", True, GEOM_KEYS + DBAS_KEYS + TIGHT_KEYS),
}

# (tape, weights): the launch on it with the most outputs, i.e. every key a reference set of that context is used for
WIDEST = {("plain", False): "geom", ("plain", True): "weights-geom", ("dbas", False): "dbas",
          ("dbas", True): "dbas-weights", ("tight", False): "tight", ("tight", True): "tight-weights"}


def keys_of(launch, c):
    """The output keys of a launch on the case dict c (a target cost has no X_ref / U_ref rows and conversely)."""
    rows = ("weights", "X_ref", "U_ref") if c["cost"].kind == "track" else ("weights", "target")
    return rows + LAUNCHES[launch][4]


def tape_case(case, tape):
    """The case dict of a tape (module docstring); computed once per case and tape, left unchanged."""
    if tape == "plain":
        return make_case(*case)
    if tape == "dbas":
        from test_gpu_layer_dbas import dbas_case

        return dbas_case(tuple(case))
    from test_gpu_layer_tight import tight_case

    return tight_case(tuple(case))


def parts_of(c, wts):
    """[(trajectory indices, cost)]: one part with the case's cost, or one per weight set in use."""
    B = c["X"].shape[0]
    if not wts:
        return [(np.arange(B), c["cost"])]
    sets, k = weight_sets(c["cost"]), assignment(B)
    return [(np.nonzero(k == s)[0], cost_of(c["cost"], sets[s])) for s in range(W) if (k == s).any()]


def sub_case(c, idx, cost):
    """The case restricted to the trajectories idx, with another cost."""
    out = dict(c)
    for n in ("X", "V", "gX", "gU", "Xref", "Uref", "s"):
        if n in c:
            out[n] = None if c[n] is None else c[n][idx]
    out["cost"] = cost
    return out


def assemble(parts, B):
    """[(idx, {key: rows of idx | None})] -> {key: rows of the whole batch | None}"""
    out = {}
    for key in parts[0][1]:
        if parts[0][1][key] is None:
            out[key] = None
            continue
        first = np.asarray(parts[0][1][key])
        full = np.zeros((B,) + first.shape[1:], first.dtype)
        for idx, r in parts:
            full[idx] = np.asarray(r[key])
        out[key] = full
    return out


def _oracle_eval(o, c, a, tape):
    """Every row of the tape's yardsticks for one oracle build on one (sub-)case: ROW_KEYS, GEOM_KEYS and, by tape,
    DBAS_KEYS / TIGHT_KEYS; "finite" where each yardstick says so."""
    sp, cc = c["prob"].to_c(), c["cost"].to_c()
    out = dict(layer_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"], a["Xref"], a["Uref"]))
    fin = out.pop("finite")
    more = [tight_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"], c["s"])] if tape == "tight" else \
        [geom_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"])]
    if tape == "dbas":
        more.append(dbas_rows(o, sp, cc, a["X"], a["V"], a["gX"], a["gU"]))
    for r in more:
        fin = fin & r.pop("finite")
        out.update(r)
    out["finite"] = fin
    return out


def _inputs(c, npdt):
    """The f32 inputs the device sees, in npdt: the truth is the f64 evaluation of the SAME (f32-rounded) inputs."""
    return {n: (None if c[n] is None else c[n].astype(np.float32).astype(npdt))
            for n in ("X", "V", "gX", "gU", "Xref", "Uref")}


@functools.lru_cache(maxsize=None)
def references(case, tape, wts):
    """(the three f32 oracle builds' rows, the f64 oracle's rows) of a case on a tape, by weight set if wts; computed
    once and left unchanged."""
    from _common import oracles
    from oracle.oracle import Oracle

    c = tape_case(case, tape)
    B = c["X"].shape[0]
    parts = parts_of(c, wts)
    out = []
    for o, npdt in [(o, np.float32) for o in oracles(np.float32)] + [(Oracle(np.float64, nthreads=8), np.float64)]:
        a = _inputs(c, npdt)
        pr = []
        for idx, cost in parts:
            cs = sub_case(c, idx, cost)
            pr.append((idx, _oracle_eval(o, cs, {n: (None if v is None else v[idx]) for n, v in a.items()}, tape)))
        out.append(assemble(pr, B))
    return out[:3], out[3]


# ---------------------------------------------------------------------------------------------------------------
# on the device
def composition(case, tape, wts, dev):
    """The parent-buildable route to the same rows on the device, in f32: ddp_sensitivity on the generic kernels with
    array upper gradients, then tensor operations (composition_rows / _geom / _dbas / _tight of the layer tests), by
    weight set if wts.  None of it is the fused backward."""
    import torch
    from test_gpu_layer import composition_rows
    from test_gpu_layer_dbas import composition_dbas
    from test_gpu_layer_geom import composition_geom
    from test_gpu_layer_tight import composition_tight

    c = tape_case(case, tape)
    pr = []
    for idx, cost in parts_of(c, wts):
        cs = sub_case(c, idx, cost)
        r = dict(composition_rows(cs, torch.float32, dev))
        if tape == "tight":
            r.update(composition_tight(cs, dev))
        else:
            r.update(composition_geom(cs, torch.float32, dev))
            if tape == "dbas":
                r.update(composition_dbas(cs, torch.float32, dev))
        pr.append((idx, r))
    return assemble(pr, c["X"].shape[0])


def fused(case, launch, dev):
    """One core.solve_backward call that reaches the launch's kernel: {key: host rows, "status"}."""
    import torch
    from _weights import pack
    from diff_tube_mpc_strict_pt.core import solve_backward
    from test_gpu_layer import _dev_inputs

    _, _, tape, wts, more = LAUNCHES[launch]
    c = tape_case(case, tape)
    B = c["X"].shape[0]
    t = _dev_inputs(c, torch.float32, dev)
    kw = {}
    if wts:
        kw["weights"] = pack(weight_sets(c["cost"]), assignment(B), dev)
    if "x0" in more:
        kw.update(want_x0=True, want_obstacles=True)
    if "alpha" in more:
        kw["want_dbas"] = True
    if "tight" in more:
        kw.update(tightening=torch.as_tensor(c["s"], device=dev), want_tight=True)
    g = solve_backward(problem=c["prob"], cost=c["cost"], X=t["X"], V=t["V"], grad_X=t["gX"], grad_V=t["gU"],
                       X_ref=t["Xref"], U_ref=t["Uref"], check=False, **kw)
    host = lambda v: None if v is None else v.cpu().numpy()  # noqa: E731
    out = {"weights": host(g.weights), "target": host(g.target), "X_ref": host(g.X_ref), "U_ref": host(g.U_ref),
           "x0": host(g.x0), "obstacles": host(g.obstacles), "status": host(g.status)}
    if g.dbas is not None:
        out["alpha"], out["gamma"] = host(g.dbas[:, 0:1]), host(g.dbas[:, 1:2])
    if g.tight is not None:
        out["tight"] = host(g.tight[:, None])
    return out
