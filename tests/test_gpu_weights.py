"""Per-trajectory cost weights in the fused f32 standalone iLQR (GPU).

The kWts kernels (csrc/dtmpc_fast_weights.hip) differ from the shared ones only before the solve: a lane fills the nine
weights of its cost from its own column of the weights array instead of the kernarg block.  Every later instruction is
the shared ilqr<>()'s, so the gate is a chain of BITWISE equalities to the shared path -- over X, V, K, kff, iters,
status and the decision record (choices and candidate costs) -- as tests/test_gpu_scenes.py holds the scene kernels:

  1. uniform weights (B copies of set 0) == the shared ilqr_solve: both kinds, lanes 1 / 2 / 4, with and without scenes;
  2. heterogeneous weights (W = 5, trajectory i -> set i % 5) == per set s the SHARED path with a QuadraticCost of set s
     on the sub-batch i % 5 == s: target cost at lanes 1 / 2 / 4, tracking cost at lane 1, M = 5, and M = 8 and M = 1 at
     lane 1, and once with the heterogeneous scenes of tests/_scenes.py (S = 4: every (scene, set) pair occurs);
  3. the same solve in three launch chunks == in one launch (the weights index is taken within the batch);
  4. refusals raise and run nothing.

f32, paper setup at fixed iterations (tol = -1, ten iterations), N = 50, B = 65 (one past a wave)."""
import dataclasses

import numpy as np
import pytest
import torch

from _scenes import S, base_table, fixed_setup, scene_table, setup_of, starts
from _weights import W, assignment, cost_of, pack, weight_sets

pytestmark = pytest.mark.gpu
B = 65
TDT = torch.float32
FIELDS = ("X", "V", "K", "k", "iters", "status", "choices", "costs")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _same(a, b):  # tests/test_gpu_lanes.py: NaN-aware bitwise equality
    return torch.equal(a, b) or (a.is_floating_point() and torch.equal(torch.isnan(a), torch.isnan(b)) and
                                 torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


def _x0(n, dev):
    return torch.as_tensor(starts(n), dtype=TDT, device=dev)


def _inputs(problem, x3, scenes=None):
    from diff_tube_mpc_strict_pt.core import dbas_init

    b0 = dbas_init(problem, x3, scenes=scenes)
    return torch.cat([x3, b0[:, None]], 1), torch.zeros(x3.shape[0], problem.horizon, 2, dtype=TDT, device=x3.device)


def _solve(problem, cost, x0, V0, lanes, **kw):
    from diff_tube_mpc_strict_pt.core import ilqr_solve

    r = ilqr_solve(problem=problem, cost=cost, cfg=fixed_setup().ilqr_nom, x0=x0, V_init=V0, lanes=lanes, check=False,
                   record_choices=True, record_costs=True, **kw)
    torch.cuda.synchronize()
    assert r.choices is not None and r.costs is not None
    return tuple(getattr(r, f) for f in FIELDS)


def _pack_scenes(st, obs, tgs, k, dev):
    from diff_tube_mpc_strict_pt.core import pack_scenes

    return pack_scenes(st.problem, obs[k], tgs[k], dtype=TDT, device=dev)


def _costs(st, track):
    """(the cost whose kind / target the solves use, its W weight sets)"""
    from diff_tube_mpc_strict_pt.core import tracking_cost

    cost = tracking_cost(st.theta0) if track else st.nominal_cost
    return cost, weight_sets(cost, tied_terminal=track)


def _refs(st, x0, V0, track):
    """A tracking cost's references: the shared nominal solve's plan (one call, every trajectory)."""
    if not track:
        return {}
    nom = _solve(st.problem, st.nominal_cost, x0, V0, 1)
    return dict(X_ref=nom[0], U_ref=nom[1])


# ---------------------------------------------------------------------------------------------
# 1. uniform weights == the shared path

@pytest.mark.parametrize("kind", ["target", "track"])
def test_uniform_weights_equal_shared_ilqr(dev, kind):
    st = fixed_setup()
    track = kind == "track"
    cost, sets = _costs(st, track)
    obs, tgs = scene_table(5)
    zero = np.zeros(B, np.int64)
    wt = pack(sets, zero, dev)
    sc = _pack_scenes(st, obs, tgs, zero, dev)  # B copies of the paper's table and target
    x0, V0 = _inputs(st.problem, _x0(B, dev))
    kw = _refs(st, x0, V0, track)
    for lanes in (1, 2, 4):
        ref = _solve(st.problem, cost, x0, V0, lanes, **kw)
        assert (ref[5] == 0).float().mean() >= 0.95
        for scenes in (None, sc):
            got = _solve(st.problem, cost, x0, V0, lanes, weights=wt, scenes=scenes, **kw)
            for f, a, b in zip(FIELDS, ref, got):
                assert _same(a, b), (kind, lanes, scenes is not None, f)
    # the cost's own nine weights are not read beside the array
    other = cost_of(cost, sets[3])
    got = _solve(st.problem, other, x0, V0, 1, weights=wt, **kw)
    ref = _solve(st.problem, cost, x0, V0, 1, **kw)
    for f, a, b in zip(FIELDS, ref, got):
        assert _same(a, b), (kind, "cost weights read", f)


# ---------------------------------------------------------------------------------------------
# 2. heterogeneous weights == the shared path set by set

def _by_set(dev, M, lanes_list, track=False):
    st = fixed_setup()
    if M != 5:
        st = setup_of(st, base_table(M), np.array(st.nominal_cost.target))
    cost, sets = _costs(st, track)
    k = assignment(B)
    wt = pack(sets, k, dev)
    x0, V0 = _inputs(st.problem, _x0(B, dev))
    kw = _refs(st, x0, V0, track)
    n_ok = 0
    for lanes in lanes_list:
        got = _solve(st.problem, cost, x0, V0, lanes, weights=wt, **kw)
        for s in range(W):
            idx = torch.as_tensor(np.nonzero(k == s)[0], device=dev)
            ref = _solve(st.problem, cost_of(cost, sets[s]), x0[idx], V0[idx], lanes,
                         **{n: v[idx] for n, v in kw.items()})
            n_ok += int((ref[5] == 0).sum())
            for f, a, b in zip(FIELDS, ref, got):
                assert _same(a, b[idx]), (M, track, lanes, s, f)
        # the weights matter: the batch does not end where set 0 would take every trajectory
        all0 = _solve(st.problem, cost, x0, V0, lanes, weights=pack(sets, np.zeros(B, np.int64), dev), **kw)
        assert not _same(all0[0], got[0]) and not _same(all0[1], got[1])
    assert n_ok >= 0.95 * B * len(lanes_list), n_ok  # failed solves are not what is compared


def test_heterogeneous_weights_equal_shared_ilqr_by_set_target(dev):
    _by_set(dev, 5, (1, 2, 4))


def test_heterogeneous_weights_equal_shared_ilqr_by_set_tracking(dev):
    _by_set(dev, 5, (1,), track=True)


@pytest.mark.parametrize("M", [8, 1])
def test_heterogeneous_weights_m8_and_m1(dev, M):
    _by_set(dev, M, (1,))


def test_heterogeneous_weights_with_heterogeneous_scenes(dev):
    """Trajectory i: scene i % 4 and set i % 5 -- twenty pairs, each == the shared path on that pair's problem / cost."""
    st = fixed_setup()
    obs, tgs = scene_table(5)
    cost, sets = _costs(st, False)
    i = np.arange(B)
    ks, kw_ = i % S, assignment(B)
    sc, wt = _pack_scenes(st, obs, tgs, ks, dev), pack(sets, kw_, dev)
    x0, V0 = _inputs(st.problem, _x0(B, dev), scenes=sc)
    got = _solve(st.problem, cost, x0, V0, 1, weights=wt, scenes=sc)
    n_ok, pairs = 0, 0
    for s in range(S):
        ss = setup_of(st, obs[s], tgs[s])
        for w in range(W):
            sel = np.nonzero((ks == s) & (kw_ == w))[0]
            assert len(sel) >= 3, (s, w)
            pairs += 1
            idx = torch.as_tensor(sel, device=dev)
            ref = _solve(ss.problem, cost_of(ss.nominal_cost, sets[w]), x0[idx], V0[idx], 1)
            n_ok += int((ref[5] == 0).sum())
            for f, a, b in zip(FIELDS, ref, got):
                assert _same(a, b[idx]), (s, w, f)
    assert pairs == S * W and n_ok >= 0.95 * B, n_ok
    only_scenes = _solve(st.problem, cost, x0, V0, 1, scenes=sc)
    only_weights = _solve(st.problem, cost, x0, V0, 1, weights=wt)
    assert not _same(only_scenes[0], got[0]) and not _same(only_weights[0], got[0])


# ---------------------------------------------------------------------------------------------
# 3. chunked launch

@pytest.mark.parametrize("lanes", [1, 4])
def test_chunked_launch_takes_the_weights_index_within_the_batch(dev, lanes, monkeypatch):
    """DTMPC_FAST_CHUNK = 256 and B = 600 = 256 + 256 + 88: three launches, the last with a partly masked tail wave.
    Trajectory i gets set (i + i // 256) % W, which shifts by one from chunk to chunk: an index taken within the chunk
    would pick another set."""
    st = fixed_setup()
    cost, sets = _costs(st, False)
    n = 600
    k = assignment(n, 256)
    wt = pack(sets, k, dev)
    assert not torch.equal(wt[:, :88], wt[:, 256:344]) and not torch.equal(wt[:, :88], wt[:, 512:])
    x0, V0 = _inputs(st.problem, _x0(n, dev))
    monkeypatch.delenv("DTMPC_FAST_CHUNK", raising=False)
    one = _solve(st.problem, cost, x0, V0, lanes, weights=wt)
    monkeypatch.setenv("DTMPC_FAST_CHUNK", "256")
    got = _solve(st.problem, cost, x0, V0, lanes, weights=wt)
    assert (one[5] == 0).float().mean() >= 0.95
    for f, a, b in zip(FIELDS, one, got):
        assert _same(a, b), (lanes, f)
    # and the chunks did run apart: the second chunk's set-0 trajectories equal the shared path's
    idx = torch.as_tensor(np.nonzero(k[256:512] == 0)[0] + 256, device=dev)
    ref = _solve(st.problem, cost, x0[idx], V0[idx], lanes)
    for f, a, b in zip(FIELDS, ref, got):
        assert _same(a, b[idx]), (lanes, "chunk 2", f)


# ---------------------------------------------------------------------------------------------
# 4. refusals

def test_unsupported_configurations_are_refused_not_run_on_the_shared_weights(dev, monkeypatch):
    from diff_tube_mpc_strict_pt.core import ilqr_solve

    monkeypatch.delenv("DTMPC_FAST", raising=False)
    st = fixed_setup()
    cost, sets = _costs(st, False)
    wt = pack(sets, assignment(B), dev)
    x0, V0 = _inputs(st.problem, _x0(B, dev))
    cfg = st.ilqr_nom
    with pytest.raises(ValueError, match="weights"):  # f64
        ilqr_solve(problem=st.problem, cost=cost, cfg=cfg, x0=x0.double(), V_init=V0.double(), weights=wt)
    with pytest.raises(ValueError, match="weights"):  # gamma != 0 in the forward
        ilqr_solve(problem=dataclasses.replace(st.problem, dbas_gamma=0.3), cost=cost, cfg=cfg, x0=x0, V_init=V0,
                   weights=wt)
    with pytest.raises(ValueError, match="weights"):  # a wrapped heading error
        ilqr_solve(problem=st.problem, cost=dataclasses.replace(cost, wrap_angle=True), cfg=cfg, x0=x0, V_init=V0,
                   weights=wt)
    with pytest.raises(ValueError, match=r"weights must be \[9, 65\]"):
        ilqr_solve(problem=st.problem, cost=cost, cfg=cfg, x0=x0, V_init=V0, weights=pack(sets, assignment(B + 1), dev))
    with pytest.raises(TypeError, match="weights go with the typed form"):  # the closure form
        ilqr_solve(cfg=cfg, x0=x0, V_init=V0, f=object(), weights=wt)
    monkeypatch.setenv("DTMPC_FAST", "0")
    with pytest.raises(ValueError, match="weights"):
        ilqr_solve(problem=st.problem, cost=cost, cfg=cfg, x0=x0, V_init=V0, weights=wt)
