"""tests/_layer_gate.sharp_gate can fail: oracle rows alone, no device.

Accepted as is: the plain f32 oracle build's rows, held to the band of the other two builds around the f64 oracle with
the builds-only constants of profiles/r17/layer_sharp_gate.txt, on all twenty-two cases of tests/_layer_cases.py.

Rejected: the same rows with ONE trajectory mutated, the trajectory being the one of smallest truth scale among those
whose band is at most 1e-3 --
    scale   the block times 0.9 (obstacles; the largest element of weights and of target times 0.9)
    zero    the block zeroed, on a trajectory whose truth scale is below 1 (obstacles, x0, weights)
    swap    the rows of two obstacles swapped, on a trajectory where both are significant
    radius  the radius column times 0.5
-- in every case with B >= 65 (a case with B = 1 is mutated where its one trajectory qualifies).

The old gates on the same mutants (tests/test_gpu_layer_geom.gate at its base 2.72e-2 for x0 / obstacles,
tests/test_gpu_layer.gate at 3.18e-3 for the weight rows), measured here on the nineteen cases with B >= 65: they ACCEPT
the scaled obstacle block in 19 of 19 cases, the zeroed one in 16 of 19, the swapped rows in 5 of 17 (the cases with
M >= 2) and the halved radius column in 19 of 19; the scaled element of weights in 7 of 19 and of target in 4 of 9, the
zeroed weights block in 3 of 14 (the cases that have a trajectory of scale below 1), the zeroed x0 block in 0 of 11.
test_old_gates_accept_small_scale_mutants prints the counts and asserts that each of the first three kinds is
accepted somewhere, which is what this gate is for.

Input conditions: the case set holds the trajectories every mutation needs, and in every case with B >= 65 each
obstacle index is significant (its row at least 1e-2 of the trajectory's largest) on at least 5 % of the trajectories --
otherwise "obstacle j" would be untested at that M."""
from __future__ import annotations

import numpy as np
import pytest

import _layer_gate as LG
from _layer_cases import ALL_CASES, FAMILY, LAUNCHES, NEW_CASES, case_id, references

# builds-only constants per key family (floor, k): profiles/r17/layer_sharp_gate.txt, "the three f32 oracle builds"
BUILDS_ONLY = {"rows": (1e-5, 38.84), "geom": (1e-3, 14.35)}
IDS = [case_id(c) for c in ALL_CASES]
KEYS = ("obstacles", "x0", "weights", "target")
TIGHT_BAND = 1e-3  # a mutated trajectory's band is at most this


def _refs(case):
    refs, truth = references(tuple(case), "plain", False)
    return refs, truth


def _eligible(case, key):
    """(trajectories whose band under the two other builds is at most TIGHT_BAND, in ascending truth scale; the truth
    scales [B])."""
    refs, truth = _refs(case)
    floor, k = BUILDS_ONLY[FAMILY[key]]
    fin = np.all([LG.finite_of(r, key) for r in refs + [truth]], axis=0)
    band, _ = LG.band_of(refs[1:], truth, key, floor, k, fin)
    t = np.asarray(truth[key], np.float64)
    sc = np.abs(t.reshape(t.shape[0], -1)).max(1)
    idx = np.nonzero((band <= TIGHT_BAND) & (sc > 0))[0]
    return idx[np.argsort(sc[idx], kind="stable")], sc


def mutants(case):
    """[(kind, key, trajectory, mutated rows of the plain build)] of a case: each kind where the case has a trajectory
    for it."""
    refs, truth = _refs(case)
    out = []
    for key in KEYS:
        if refs[0][key] is None:
            continue
        idx, sc = _eligible(case, key)
        base = np.asarray(refs[0][key], np.float64)

        def mut(i, f):
            a = base.copy()
            a[i] = f(a[i].copy())
            return a

        if len(idx):
            i = int(idx[0])
            if key == "obstacles":
                out.append(("scale", key, i, mut(i, lambda b: 0.9 * b)))
            elif key in ("weights", "target"):
                def one(b):
                    b.flat[int(np.argmax(np.abs(b)))] *= 0.9
                    return b
                out.append(("scale", key, i, mut(i, one)))
        small = idx[sc[idx] < 1.0]
        if len(small) and key != "target":
            out.append(("zero", key, int(small[0]), mut(int(small[0]), lambda b: 0.0 * b)))
        if key == "obstacles":
            t = np.asarray(truth[key], np.float64)
            sig = LG.significant_rows(t)
            two = [int(i) for i in idx if sig[i].sum() >= 2]
            if two:
                i = two[0]
                j0, j1 = np.nonzero(sig[i])[0][:2]

                def swap(b, j0=j0, j1=j1):
                    b[[j0, j1]] = b[[j1, j0]]
                    return b
                out.append(("swap", key, i, mut(i, swap)))
            rad = [int(i) for i in idx if np.abs(t[i, :, 2]).max() >= 1e-2 * sc[i]]
            if rad:
                def half(b):
                    b[:, 2] *= 0.5
                    return b
                out.append(("radius", key, rad[0], mut(rad[0], half)))
    return out


def _with(rows, key, a):
    out = dict(rows)
    out[key] = a
    return out


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_plain_build_is_accepted(oracle_lib, case):
    refs, truth = _refs(case)
    for key in ("weights", "target", "X_ref", "U_ref", "x0", "obstacles"):
        if refs[0][key] is None:
            continue
        floor, k = BUILDS_ONLY[FAMILY[key]]
        w = LG.sharp_gate(refs[0], refs[1:], truth, key, floor, k, case_id(case))
        assert w <= 1.0


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_mutants_are_rejected(oracle_lib, case):
    refs, truth = _refs(case)
    ms = mutants(case)
    have = {(kind, key) for kind, key, _, _ in ms}
    B, M = case[1], case[2]
    if B >= 65:  # the case set contains the trajectories each mutation needs
        need = {("scale", "obstacles"), ("zero", "obstacles"), ("radius", "obstacles"), ("scale", "weights")}
        if M >= 2:
            need.add(("swap", "obstacles"))
        if case[3] == "target":
            need.add(("scale", "target"))
        assert need <= have, (case_id(case), sorted(need - have))
    for kind, key, i, a in ms:
        floor, k = BUILDS_ONLY[FAMILY[key]]
        with pytest.raises(AssertionError, match="outside the band"):
            LG.sharp_gate(_with(refs[0], key, a), refs[1:], truth, key, floor, k, f"{case_id(case)} {kind} traj {i}")


def test_a_zero_truth_block_must_be_exactly_zero():
    truth = {"alpha": np.array([[0.0], [2.0], [0.0]])}
    refs = [{"alpha": np.array([[0.0], [2.0], [0.0]])}, {"alpha": np.array([[0.0], [2.0 + 1e-6], [0.0]])}]
    assert LG.sharp_gate({"alpha": np.array([[0.0], [2.0], [0.0]])}, refs, truth, "alpha", 1e-4, 10.0, "zero") <= 1.0
    with pytest.raises(AssertionError, match="outside the band"):
        LG.sharp_gate({"alpha": np.array([[0.0], [2.0], [1e-30]])}, refs, truth, "alpha", 1e-4, 10.0, "zero")
    with pytest.raises(AssertionError, match="outside the band"):
        LG.sharp_gate({"alpha": np.array([[0.0], [np.nan], [0.0]])}, refs, truth, "alpha", 1e-4, 10.0, "nan")


def test_caps_are_conditions():
    rng = np.random.default_rng(0)
    t = rng.normal(size=(20, 4))
    truth = {"x0": t}
    noisy = t * (1.0 + 1e-2 * rng.normal(size=t.shape))  # a reference this far off makes the band uninformative
    few, many = t.copy(), t.copy()
    few[:4], many[:5] = noisy[:4], noisy[:5]
    assert LG.sharp_gate({"x0": t}, [{"x0": few}], truth, "x0", 1e-4, 10.0, "4 of 20") == 0.0
    with pytest.raises(AssertionError, match="uninformative"):
        LG.sharp_gate({"x0": t}, [{"x0": many}], truth, "x0", 1e-4, 10.0, "5 of 20")
    nan = t.copy()
    nan[:2] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        LG.sharp_gate({"x0": t}, [{"x0": nan}], truth, "x0", 1e-4, 10.0, "2 of 20 non-finite")


def test_every_obstacle_counts(oracle_lib):
    """In every case with B >= 65 each obstacle index is significant on at least 5 % of the trajectories."""
    for case in ALL_CASES:
        if case[1] < 65:
            continue
        _, truth = _refs(case)
        fin = LG.finite_of(truth, "obstacles")
        share = LG.significant_rows(np.asarray(truth["obstacles"])[fin]).mean(0)
        print(f"[teeth {case_id(case)}] share of trajectories on which obstacle j is significant: "
              + " ".join(f"{v:.2f}" for v in share))
        assert (share >= 0.05).all(), (case_id(case), share.tolist())


def test_old_gates_accept_small_scale_mutants(oracle_lib):
    """What the old gates say to the same mutants (module docstring)."""
    from test_gpu_layer import BASE_F32 as ROWS_BASE
    from test_gpu_layer import gate as rows_gate
    from test_gpu_layer_geom import BASE_F32 as GEOM_BASE
    from test_gpu_layer_geom import gate as geom_gate

    seen, accepted = {}, {}
    for case in ALL_CASES:
        if case[1] < 65:
            continue
        refs, _ = _refs(case)
        for kind, key, i, a in mutants(case):
            got = _with(refs[0], key, a)
            try:
                if FAMILY[key] == "geom":
                    geom_gate(got, refs, GEOM_BASE, "old")
                else:
                    rows_gate(got, refs, ROWS_BASE, "old")
                ok = True
            except AssertionError:
                ok = False
            seen[(kind, key)] = seen.get((kind, key), 0) + 1
            accepted[(kind, key)] = accepted.get((kind, key), 0) + ok
    for kk in sorted(seen):
        print(f"[teeth] old gate accepts the mutant '{kk[0]}' of {kk[1]} in {accepted[kk]} of {seen[kk]} cases")
    for kk in (("scale", "obstacles"), ("zero", "obstacles"), ("swap", "obstacles")):
        assert accepted[kk] > 0, kk


def test_the_new_cases_cover_what_the_docstring_says():
    """Every M of {2, 3, 4, 6, 7} with both kinds, N = 50 once, B = 257 once and each gamma once; one seed per case."""
    assert len({c[5] for c in ALL_CASES}) == len(ALL_CASES)
    for M in (2, 3, 4, 6, 7):
        cs = [c for c in NEW_CASES if c[2] == M]
        assert sorted(c[3] for c in cs) == ["target", "track"], M
        assert sorted(c[0] for c in cs) == [3, 50] and sorted(c[1] for c in cs) == [65, 257], M
        assert sorted(c[4] for c in cs) == [0.0, 0.3], M
    assert {c[2] for c in ALL_CASES} == set(range(1, 9))
    assert {(v[0], v[1]) for v in LAUNCHES.values()} == {("LK", None), ("LKG", None), ("LKW", False), ("LKW", True),
                                                          ("LKD", False), ("LKD", True), ("LKT", False), ("LKT", True)}
