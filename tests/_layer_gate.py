"""The scale-aware gate of the differentiable solve's rows (host only, numpy only).

tests/test_gpu_layer.gate and its descendants compare a trajectory's block with rel() = max|a - b| / max(1, max|b|)
against one base per file, sized by the worst-conditioned trajectory of the whole case set: a trajectory whose rows are
below 1 in size is allowed an absolute error as large as the row, and one obstacle's row among several is not seen at
all.  sharp_gate works per trajectory, in the trajectory's own scale, against the f64 oracle:

    e(a)_i = max|a_i - truth_i| / max|truth_i|          over trajectory i's block of `key` (no floor of 1)
    e(device)_i <= max(floor, k * max_r e(r)_i)         r over the reference evaluations

where the reference evaluations are valid f32 evaluations of the same rows that are not the code under test (the three
f32 oracle builds and, on the device, the composition out of ddp_sensitivity and tensor operations).  Their own error
against the f64 oracle is what f32 arithmetic does to trajectory i, so the band follows each trajectory's conditioning
instead of the batch's worst.  A trajectory whose truth block is exactly zero must be exactly zero.  For
key == "obstacles" the same rule holds per (trajectory, obstacle) row of three entries as well, wherever that row's
truth size is at least SIGNIFICANT of the trajectory's largest row: the check that sees a swapped or dropped obstacle.

Conditions on the case (not measurements): at most 5 % of a case's trajectories may have a non-finite reference, at
most 20 % a band above 1e-2 (uninformative); for the obstacle rows the latter also holds among the significant rows.

floor and k come from leave_one_out below -- each reference evaluation held to the band of the others with k = 1 --
never from the code under test: floor is the smallest of FLOORS whose worst leave-one-out ratio is at most LOO_MAX, k
twice that ratio (choose)."""
from __future__ import annotations

import numpy as np

SIGNIFICANT = 1e-2    # an obstacle row counts where its truth size is at least this share of the trajectory's largest
UNINFORMATIVE = 1e-2  # a band above this says nothing
MAX_NONFINITE = 0.05
MAX_UNINFORMATIVE = 0.20
FLOORS = (1e-5, 1e-4, 1e-3)
LOO_MAX = 20.0


def _err(a, t):
    """e(a) per leading index: max|a - t| / max|t|; where t is exactly zero, 0 if a is too, else inf.  A non-finite
    a gives inf."""
    n = t.shape[0]
    a, t = np.asarray(a, np.float64).reshape(n, -1), np.asarray(t, np.float64).reshape(n, -1)
    sc = np.abs(t).max(1)
    d = np.abs(a - t).max(1)
    d = np.where(np.isfinite(a).all(1), d, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(sc > 0, d / np.where(sc > 0, sc, 1.0), np.where(d == 0, 0.0, np.inf))
    return e, sc


def finite_of(r, key):
    """[B] bool: the evaluation r (a dict of rows, with or without a "finite" entry) is finite on the trajectory."""
    a = np.asarray(r[key])
    f = np.isfinite(a.reshape(a.shape[0], -1)).all(1)
    return f & np.asarray(r["finite"], bool) if "finite" in r else f


def significant_rows(truth_obs):
    """[B, M] bool: obstacle rows whose truth size is at least SIGNIFICANT of their trajectory's largest row."""
    mag = np.abs(np.asarray(truth_obs, np.float64)).max(2)
    top = mag.max(1, keepdims=True)
    return (mag >= SIGNIFICANT * top) & (top > 0)


def _units(key, truth, fin):
    """The units the rule applies to: [(name, pick)] where pick(a) -> [U, ...] takes an evaluation's rows of `key`
    to the blocks compared (the finite trajectories; for the obstacles also their significant rows)."""
    out = [("trajectory", lambda a: np.asarray(a, np.float64)[fin])]
    if key == "obstacles":
        sig = significant_rows(np.asarray(truth[key])[fin])
        out.append(("obstacle row", lambda a: np.asarray(a, np.float64)[fin][sig]))
    return out


def band_of(refs, truth, key, floor, k, fin=None):
    """Per trajectory: (band [B], e of each reference [R, B]) with inf where a reference is non-finite."""
    t = np.asarray(truth[key], np.float64)
    e = np.stack([_err(r[key], t)[0] for r in refs])
    band = np.maximum(floor, k * e.max(0))
    if fin is not None:
        band = np.where(fin, band, np.inf)
    return band, e


def sharp_gate(got, refs32, truth64, key, floor, k, label):
    """The module docstring's conditions on one key of one case.  got, truth64 and each of refs32 are dicts of rows
    [B, ...] (refs32 / truth64 may carry "finite" [B]).  Returns the worst e(device) / band over the informative units;
    raises AssertionError where a condition does not hold."""
    B = np.asarray(truth64[key]).shape[0]
    fin = np.all([finite_of(r, key) for r in list(refs32) + [truth64]], axis=0)
    assert (~fin).sum() <= MAX_NONFINITE * B, (label, key, "non-finite reference rows", int((~fin).sum()), B)
    worst = 0.0
    g = np.asarray(got[key], np.float64)
    assert g.shape == np.asarray(truth64[key]).shape, (label, key, g.shape)
    for name, pick in _units(key, truth64, fin):
        t = pick(truth64[key])
        n = t.shape[0]
        if not n:
            continue
        e_dev, sc = _err(pick(g), t)
        e_ref = np.stack([_err(pick(r[key]), t)[0] for r in refs32])
        band = np.maximum(floor, k * e_ref.max(0))
        inf = band <= UNINFORMATIVE
        total = B if name == "trajectory" else n
        assert (~inf).sum() <= MAX_UNINFORMATIVE * total, (label, key, name, "uninformative", int((~inf).sum()), total)
        ratio = e_dev[inf] / band[inf]
        w = float(ratio.max()) if inf.any() else 0.0
        worst = max(worst, w)
        print(f"[sharp gate {label}] {key} per {name}: worst error / band {w:.3g} (floor {floor:g}, k {k:g}; "
              f"{int(inf.sum())} informative of {total}, {int((~fin).sum())} of {B} trajectories non-finite, median "
              f"scale {float(np.median(sc)):.3g}, median band {float(np.median(band[inf])) if inf.any() else 0:.3g})")
        bad = np.nonzero(inf)[0][~(ratio <= 1.0)]
        assert not len(bad), (label, key, name, "outside the band", w, bad[:8].tolist(),
                              e_dev[bad[:8]].tolist(), band[bad[:8]].tolist())
    return worst


def leave_one_out(evals, truth64, key, floor):
    """Each evaluation held to the band the others form with k = 1: the worst e(x) / max(floor, max_others e) per
    evaluation, over the trajectories (and significant obstacle rows) on which every evaluation is finite and the truth
    is not exactly zero (a zero block is an exactness condition, not a band).  -> [len(evals)] floats."""
    fin = np.all([finite_of(r, key) for r in list(evals) + [truth64]], axis=0)
    out = np.zeros(len(evals))
    for _, pick in _units(key, truth64, fin):
        t = pick(truth64[key])
        if not t.shape[0]:
            continue
        E = np.stack([_err(pick(r[key]), t)[0] for r in evals])
        nz = _err(t, t)[1] > 0
        E = E[:, nz]
        if not E.shape[1]:
            continue
        for i in range(len(evals)):
            others = np.delete(E, i, 0).max(0)
            with np.errstate(invalid="ignore"):
                r = E[i] / np.maximum(floor, others)
            r = np.where(np.isnan(r), 0.0, r)  # inf / inf: the others are no better
            out[i] = max(out[i], float(r.max()))
    return out


def choose(worst_by_floor):
    """{floor: worst leave-one-out ratio} -> (floor, k): the smallest floor of FLOORS whose worst ratio is at most
    LOO_MAX, and twice that ratio (the standing rule for bases: twice the references' own worst)."""
    for f in FLOORS:
        if worst_by_floor[f] <= LOO_MAX:
            return f, float(f"{2.0 * worst_by_floor[f]:.4g}")  # four digits: the figure the tests quote
    raise AssertionError(("no floor of FLOORS holds the references to one another within LOO_MAX", worst_by_floor))
