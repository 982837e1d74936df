"""Every instantiation of the differentiable solve's backward kernel on the device, each output under the scale-aware
gate (tests/_layer_gate.sharp_gate: per trajectory, in the trajectory's own row scale, against the f64 oracle; for the
obstacle rows also per obstacle).

csrc/dtmpc_fast_layer*.hip compile solve_backward_kernel<K, M, TRACK[, FL]> 128 times: M = 1..8 x both cost kinds x
    block   entry point                      flag FL                     kernels   run before this file   new here
    LK      dtmpc_solve_backward             --                             16      6 (M = 1, 5, 8)          10
    LKG     dtmpc_solve_backward_geom        --                             16      6                        10
    LKW     dtmpc_solve_backward_weights     the GEOM record                32     12                        20
    LKD     dtmpc_solve_backward_dbas        per-trajectory weights         32     12                        20
    LKT     dtmpc_solve_backward_tight       per-trajectory weights         32     12                        20
                                                                           128     48                        80
(the older layer tests all draw from tests/test_gpu_layer.CASES, whose M is 1, 5 or 8).  core.solve_backward picks the
entry point (core/layer.py: tightening= -> LKT, else want_dbas -> LKD, else weights= -> LKW, else want_x0 /
want_obstacles -> LKG, else LK) and launch_block the flag (weights != NULL where the record is always GEOM, else the
GEOM record, i.e. g_x0 or g_obs asked for).  The eight launches of tests/_layer_cases.LAUNCHES are one per (block,
flag); on the ten cases with M in {2, 3, 4, 6, 7} x {target, track} they are the 80 kernels no other test runs, and
the twelve older cases run under the same gate.

References of a launch: the three f32 oracle builds of the matching yardsticks (tests/_layer.py, _layer_geom.py,
_layer_dbas.py, _layer_tight.py; by weight set where the launch has per-trajectory weights) and the composition on the
device out of ddp_sensitivity on the generic kernels and tensor operations -- none is the fused backward.  Truth: the
f64 oracle on the same f32 inputs.

The constants (floor, k) per key family are derived from the references alone -- leave-one-out among the four over all
twenty-two cases, tapes and weight modes, floor the smallest of {1e-5, 1e-4, 1e-3} with a worst ratio of at most 20, k
twice that ratio -- by scripts/layer_sharp_gate.py; profiles/r17/layer_sharp_gate.txt holds the table, the constants
and every fused kernel's own worst error / band under them (which do not enter the choice)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _layer_gate as LG
from _layer_cases import (ALL_CASES, FAMILY, LAUNCHES, NEW_CASES, case_id, composition, fused, keys_of, references,
                          tape_case)

pytestmark = pytest.mark.gpu

# (floor, k) per key family: profiles/r17/layer_sharp_gate.txt, "the three f32 oracle builds + the composition on the
# device"
CONSTANTS = {"rows": (1e-5, 15.67), "geom": (1e-5, 26.04), "dbas": (1e-5, 37.36), "tight": (1e-5, 23.83)}

# Findings: (case, launch, key) outside the band so fixed, each with its cause; test_findings holds them as strict
# expected failures (a fix, or a change that moves them, shows) and test_launch_under_the_sharp_gate gates every other
# key of the same launch.
# The gamma row of trajectory 6 of N3-B257-M1-target-g0.3, from both families that write it: e = 3.02e-5 of the row
# against a band of 1e-5 (ratio 3.02; 3.01 with per-trajectory weights).  There g_gamma = -sum_k lam_{k+1} (B(h(x_k)) -
# b_k) = 2.40e-3 is a sum of differences of nearly equal numbers (B = 0.608 against b_0 = 0.606: one ulp of B, 6e-8, is
# 3.2e-5 of B - b_0 = 1.85e-3), the kernel's B is vbarrier's v_rcp_f32 reciprocal (within one ulp, the reciprocal of
# every fused f32 kernel) of an h formed as geom_row forms it, and all four references -- which
# share the IEEE division and the oracle's order of operations -- land within 2.7e-7 of the f64 row on this trajectory,
# so their spread does not show the row's conditioning (the row evaluated in f32 on the host with the correctly rounded
# B is within 1e-7; with the B of step 2 alone moved by one ulp it is off by 3.01e-5 / 3.03e-5).  The reciprocal is the
# forward solver's on purpose: on a tape the fused forward produced, b_k was formed with this very B and the difference
# is the propagated offset exactly.
GAMMA_RCP = ("the gamma row's B(h) - b_k cancels to 3e-3 of B on trajectory 6 and vbarrier's v_rcp_f32 is within one "
             "ulp: error / band {:.3g} measured on an MI355X (profiles/r17/layer_sharp_gate.txt)")
FINDINGS = {
    ("N3-B257-M1-target-g0.3", "dbas", "gamma"): GAMMA_RCP.format(3.02),
    ("N3-B257-M1-target-g0.3", "dbas-weights", "gamma"): GAMMA_RCP.format(3.01),
    ("N3-B257-M1-target-g0.3", "tight", "gamma"): GAMMA_RCP.format(3.02),
    ("N3-B257-M1-target-g0.3", "tight-weights", "gamma"): GAMMA_RCP.format(3.01),
}

IDS = [case_id(c) for c in ALL_CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_comp = {}


def _composition(case, tape, wts, dev):
    """The device composition of a (case, tape, weights mode), computed once and shared by the launches on it."""
    key = (tuple(case), tape, wts)
    if key not in _comp:
        _comp[key] = composition(case, tape, wts, dev)
    return _comp[key]


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_launch_under_the_sharp_gate(dev, oracle_lib, case, launch):
    block, fl, tape, wts, _ = LAUNCHES[launch]
    label = f"{case_id(case)} {launch} ({block}{'' if fl is None else '<' + str(int(fl)) + '>'})"
    c = tape_case(case, tape)
    refs, truth = references(tuple(case), tape, wts)
    evals = list(refs) + [_composition(case, tape, wts, dev)]
    got = fused(case, launch, dev)
    for key in ("target", "X_ref", "U_ref", "x0", "obstacles", "alpha", "gamma", "tight"):
        assert (got.get(key) is not None) == (key in keys_of(launch, c)), (label, key)
    fin = np.asarray(truth["finite"]) & np.all([r["finite"] for r in refs], axis=0)
    assert (got["status"][fin] == 0).all(), (label, got["status"])
    for key in keys_of(launch, c):
        if (case_id(case), launch, key) in FINDINGS:
            continue  # test_findings
        floor, k = CONSTANTS[FAMILY[key]]
        LG.sharp_gate(got, evals, truth, key, floor, k, label)


@pytest.mark.parametrize("finding", [pytest.param(f, marks=pytest.mark.xfail(strict=True, reason=why,
                                                                             raises=AssertionError))
                                     for f, why in FINDINGS.items()], ids=["-".join(f) for f in FINDINGS])
def test_findings(dev, oracle_lib, finding):
    """The keys test_launch_under_the_sharp_gate leaves out, under the same gate: each is outside its band for the
    cause written beside it in FINDINGS."""
    cid, launch, key = finding
    case = ALL_CASES[IDS.index(cid)]
    _, _, tape, wts, _ = LAUNCHES[launch]
    refs, truth = references(tuple(case), tape, wts)
    floor, k = CONSTANTS[FAMILY[key]]
    LG.sharp_gate(fused(case, launch, dev), list(refs) + [_composition(case, tape, wts, dev)], truth, key, floor, k,
                  f"{cid} {launch} finding")


SCENE_CASES = [NEW_CASES[i] for i in (1, 2, 4, 7, 9)]  # one per new M, both kinds, both shapes


@pytest.mark.parametrize("case", SCENE_CASES, ids=[case_id(c) for c in SCENE_CASES])
def test_uniform_scenes_are_the_shared_table_bitwise(dev, case):
    """B copies of the shared table as a [B, M, 3] scene array give the rows of the call without scenes, bitwise (LKG),
    as tests/test_gpu_layer_geom.test_scenes has it at M = 5: one case per new M."""
    from diff_tube_mpc_strict_pt.core import pack_scenes
    from test_gpu_layer_geom import _same_geom, raw_geom

    c = tape_case(case, "plain")
    prob, cost = c["prob"], c["cost"]
    B, M = c["X"].shape[0], len(prob.obstacles)
    assert M == case[2]
    tab = np.array([[o.center[0], o.center[1], o.radius] for o in prob.obstacles])
    shared = pack_scenes(prob, np.broadcast_to(tab, (B, M, 3)), np.broadcast_to(np.array(cost.target), (B, 3)),
                         dtype=torch.float32, device=dev)
    r0 = raw_geom(c, dev)
    assert (r0["status"] == 0).sum() > 0 and not (r0["gob"] == 7.0).all(0).any()
    r1 = raw_geom(c, dev, scenes=shared)
    _same_geom(r0, r1)
    assert np.array_equal(r0["status"], r1["status"])
