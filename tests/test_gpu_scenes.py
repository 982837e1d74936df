"""Per-trajectory scenes (obstacles and nominal target) in the fused f32 solvers (GPU).

The scene kernels (csrc/dtmpc_fast_scenes.hip) differ from the shared ones only at a phase start: a lane fills the
pinned obstacle table and the nominal target from its own column of the scenes array instead of the kernarg block.
Every later instruction is the shared form's, so the gate is a chain of BITWISE equalities to the shared path, which
the rest of the suite holds to the oracle and the reference (a chaotic solver amplifies a 1-ulp difference, so no
weaker gate would mean anything):

  1. uniform scenes (every trajectory the paper's table and target) == the run without scenes;
  2. heterogeneous scenes (S = 4, trajectory i -> scene i % 4) == per scene s the SHARED path on a problem / cost built
     from scene s, on the sub-batch i % 4 == s (injected disturbances, so the draw does not depend on the batch index);
  3. the same step in three launch chunks == in one launch (the scene index is taken within the batch);
  4. the standalone solve with eight obstacles and with one;
  5. the split step (overlap) == the fused step; set_scenes between episodes changes the second;
  6. two resets with the same scenes give the same first step.

f32, paper setup at fixed iterations (tol = -1), N = 50, theta held (adapt=False), B = 200 (not a multiple of 64: the
tail wave runs partly masked)."""
import dataclasses

import numpy as np
import pytest
import torch

from _scenes import S, fixed_setup, scene_table, setup_of, starts

pytestmark = pytest.mark.gpu
NAMES = ("x", "b", "xbar", "bbar", "Xnom", "Unom", "Xaux", "Uaux", "status", "log")
B = 200
TDT = torch.float32


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


def _w(n, steps=2):
    rng = np.random.default_rng(3)
    return [torch.as_tensor(rng.uniform(-0.05, 0.05, (n, 3)), dtype=TDT) for _ in range(steps)]


def _pack(st, obs, tgs, n, dev, k=None):
    """scenes tensor of a batch of n: trajectory i gets scene i % len(obs) (or scene k[i])."""
    from diff_tube_mpc_strict_pt.core import pack_scenes

    k = np.arange(n) % len(obs) if k is None else k
    return pack_scenes(st.problem, obs[k], tgs[k], dtype=TDT, device=dev)


def _tube(st, dev, x, ws, scenes=None, idx=None, **kw):
    """Two held-theta steps with injected disturbances ws (the rows idx of them); every state array afterwards."""
    from diff_tube_mpc_strict_pt.core import TubeMPC

    n = x.shape[0]
    m = TubeMPC(st, batch=n, device=dev, dtype=TDT, disturbance="injected", write_log=True, scenes=scenes, **kw)
    m.reset(x)
    for w in ws:
        m.step(w if idx is None else w[idx], adapt=False)
    torch.cuda.synchronize()
    return {k: getattr(m, k).clone() for k in NAMES}, m


def _ilqr_inputs(problem, x3, scenes=None):
    from diff_tube_mpc_strict_pt.core import dbas_init

    b0 = dbas_init(problem, x3, scenes=scenes)
    return torch.cat([x3, b0[:, None]], 1), torch.zeros(x3.shape[0], problem.horizon, 2, dtype=TDT, device=x3.device)


def _solve(problem, cost, x0, V0, lanes, scenes=None, X_ref=None, U_ref=None):
    from diff_tube_mpc_strict_pt.core import ilqr_solve

    cfg = dataclasses.replace(fixed_setup().ilqr_nom)
    r = ilqr_solve(problem=problem, cost=cost, cfg=cfg, x0=x0, V_init=V0, lanes=lanes, scenes=scenes, X_ref=X_ref,
                   U_ref=U_ref, check=False)
    torch.cuda.synchronize()
    return (r.X, r.V, r.K, r.k, r.iters, r.status)


# ---------------------------------------------------------------------------------------------
# 1. uniform scenes == no scenes

@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_uniform_scenes_equal_shared_tube_step(dev, lanes, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", lanes)
    st = fixed_setup()
    obs, tgs = scene_table(5)
    x, ws = _x0(B, dev), _w(B)
    ref, m = _tube(st, dev, x, ws)
    assert m.lanes == int(lanes)
    got, m = _tube(st, dev, x, ws, scenes=_pack(st, obs[:1], tgs[:1], B, dev))
    assert m.lanes == int(lanes) and m.state.scenes
    assert (ref["status"] == 0).float().mean() >= 0.95
    bad = [k for k in NAMES if not _same(ref[k], got[k])]
    assert not bad, bad


@pytest.mark.parametrize("kind", ["target", "track"])
def test_uniform_scenes_equal_shared_ilqr(dev, kind):
    from diff_tube_mpc_strict_pt.core import tracking_cost

    st = fixed_setup()
    obs, tgs = scene_table(5)
    sc = _pack(st, obs[:1], tgs[:1], B, dev)
    x0, V0 = _ilqr_inputs(st.problem, _x0(B, dev))
    assert _same(x0, _ilqr_inputs(st.problem, _x0(B, dev), scenes=sc)[0])
    cost, ref_kw = st.nominal_cost, {}
    if kind == "track":  # track the nominal solve's plan with the ancillary weights
        nom = _solve(st.problem, st.nominal_cost, x0, V0, 1)
        cost, ref_kw = tracking_cost(st.theta0), dict(X_ref=nom[0], U_ref=nom[1])
    for lanes in (1, 2, 4):
        ref = _solve(st.problem, cost, x0, V0, lanes, **ref_kw)
        got = _solve(st.problem, cost, x0, V0, lanes, scenes=sc, **ref_kw)
        assert (ref[5] == 0).float().mean() >= 0.95
        for j, (a, b) in enumerate(zip(ref, got)):
            assert _same(a, b), (kind, lanes, j)


# ---------------------------------------------------------------------------------------------
# 2. heterogeneous scenes == the shared path scene by scene

def _shared_tube_by_scene(st, dev, obs, tgs, x, ws):
    """Per scene s the shared path's run on the sub-batch i % S == s: [(indices, arrays)]."""
    out = []
    for s in range(S):
        idx = torch.arange(s, x.shape[0], S)
        out.append((idx, _tube(setup_of(st, obs[s], tgs[s]), dev, x[idx.to(x.device)], ws, idx=idx)[0]))
    return out


def _assert_by_scene(got, shared, names=NAMES):
    ok = sum(int((r["status"] == 0).sum()) for _, r in shared)
    n = sum(len(i) for i, _ in shared)
    assert ok >= 0.95 * n, (ok, n)  # failed solves are not what is compared
    for s, (idx, r) in enumerate(shared):
        j = idx.to(got["x"].device)
        bad = [k for k in names if not _same(got[k][..., j], r[k])]
        assert not bad, (s, bad)


@pytest.mark.parametrize("lanes", ["1", "4"])
def test_heterogeneous_scenes_equal_shared_tube_step_by_scene(dev, lanes, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", lanes)
    st = fixed_setup()
    obs, tgs = scene_table(5)
    x, ws = _x0(B, dev), _w(B)
    got, m = _tube(st, dev, x, ws, scenes=_pack(st, obs, tgs, B, dev))
    assert m.lanes == int(lanes)
    _assert_by_scene(got, _shared_tube_by_scene(st, dev, obs, tgs, x, ws))
    # the scenes matter: a trajectory of scene 1 does not end where the paper's scene would take it
    ref, _ = _tube(st, dev, x, ws)
    assert not _same(ref["Xnom"], got["Xnom"])


def _ilqr_by_scene(dev, M, lanes_list, track=False):
    from diff_tube_mpc_strict_pt.core import dbas_init, tracking_cost

    st = fixed_setup()
    obs, tgs = scene_table(M)
    base = setup_of(st, obs[0], tgs[0])  # M obstacles: the count every scene shares
    sc = _pack(base, obs, tgs, B, dev)
    x3 = _x0(B, dev)
    x0, V0 = _ilqr_inputs(base.problem, x3, scenes=sc)
    n_ok = 0
    for s in range(S):
        idx = torch.arange(s, B, S, device=dev)
        ss = setup_of(st, obs[s], tgs[s])
        # dbas_init with scenes == the shared one with scene s's problem
        assert _same(x0[idx, 3], dbas_init(ss.problem, x3[idx])), s
        for lanes in lanes_list:
            cost, kw, kws = ss.nominal_cost, {}, {}
            if track:
                nom = _solve(ss.problem, ss.nominal_cost, x0[idx], V0[idx], 1)
                Xr = torch.zeros(B, *nom[0].shape[1:], dtype=TDT, device=dev)
                Ur = torch.zeros(B, *nom[1].shape[1:], dtype=TDT, device=dev)
                Xr[idx], Ur[idx] = nom[0], nom[1]
                cost, kw, kws = tracking_cost(st.theta0), dict(X_ref=nom[0], U_ref=nom[1]), dict(X_ref=Xr, U_ref=Ur)
            ref = _solve(ss.problem, cost, x0[idx], V0[idx], lanes, **kw)
            # (the whole batch with scenes; with a tracking cost only the rows of scene s carry a reference)
            got = _solve(base.problem, base.nominal_cost if not track else cost, x0, V0, lanes, scenes=sc, **kws)
            n_ok += int((ref[5] == 0).sum())
            for j, (a, b) in enumerate(zip(ref, got)):
                assert _same(a, b[idx]), (M, s, lanes, j)
    assert n_ok >= 0.95 * B * len(lanes_list), n_ok


def test_heterogeneous_scenes_equal_shared_ilqr_and_dbas_init_by_scene(dev):
    _ilqr_by_scene(dev, 5, (1, 2, 4))


def test_heterogeneous_scenes_tracking_cost_ignores_the_target_rows(dev):
    _ilqr_by_scene(dev, 5, (1,), track=True)


# ---------------------------------------------------------------------------------------------
# 3. chunked launch

@pytest.mark.parametrize("lanes", ["1", "4"])
def test_chunked_launch_takes_the_scene_index_within_the_batch(dev, lanes, monkeypatch):
    """DTMPC_FAST_CHUNK = 256 (the smallest chunk dtmpc_tube_chunk accepts: one 256-thread workgroup's multiple) and
    B = 2 * 256 + 88: three launches, the last with a partly masked tail wave.  The chunk is a multiple of S, so with
    test 2's assignment i % S an index taken within the chunk would pick the same scene as the right one; here
    trajectory i gets scene (i + i // 256) % S, which shifts by one from chunk to chunk."""
    monkeypatch.setenv("DTMPC_TUBE_LANES", lanes)
    st = fixed_setup()
    obs, tgs = scene_table(5)
    n = 2 * 256 + 88
    x, ws = _x0(n, dev), _w(n)
    i = np.arange(n)
    sc = _pack(st, obs, tgs, n, dev, k=(i + i // 256) % S)
    assert not torch.equal(sc[:, :88], sc[:, 256:344]) and not torch.equal(sc[:, :88], sc[:, 512:])
    one, m = _tube(st, dev, x, ws, scenes=sc)
    assert m.chunk >= n
    monkeypatch.setenv("DTMPC_FAST_CHUNK", "256")
    got, m = _tube(st, dev, x, ws, scenes=sc)
    assert m.chunk == 256
    assert (one["status"] == 0).float().mean() >= 0.95
    bad = [k for k in NAMES if not _same(one[k], got[k])]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 4. the largest table and the degenerate smooth-min

@pytest.mark.parametrize("M", [8, 1])
def test_heterogeneous_scenes_ilqr_m8_and_m1(dev, M):
    _ilqr_by_scene(dev, M, (1,))


# ---------------------------------------------------------------------------------------------
# 5. split step, set_scenes

def test_split_step_equals_fused_and_set_scenes_changes_the_episode(dev, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    st = fixed_setup()
    obs, tgs = scene_table(5)
    x, ws = _x0(B, dev), _w(B)
    sc = _pack(st, obs, tgs, B, dev)
    fused, _ = _tube(st, dev, x, ws, scenes=sc)
    split, m = _tube(st, dev, x, ws, scenes=sc, overlap=True)
    assert m.overlap and m.lanes == 1
    bad = [k for k in NAMES if not _same(fused[k], split[k])]
    assert not bad, bad
    # a second episode on the same object with other scenes (every trajectory scene 2): its result is that of a
    # fresh object with those scenes, and not the first episode's
    sc2 = _pack(st, obs[2:3], tgs[2:3], B, dev)
    m.set_scenes(sc2)
    m.reset(x)
    for w in ws:
        m.step(w, adapt=False)
    torch.cuda.synchronize()
    second = {k: getattr(m, k).clone() for k in NAMES}
    fresh, _ = _tube(st, dev, x, ws, scenes=sc2, overlap=True)
    assert not _same(second["Xnom"], split["Xnom"]) and not _same(second["b"], split["b"])
    bad = [k for k in NAMES if not _same(second[k], fresh[k])]
    assert not bad, bad
    # and back to the shared problem
    m.set_scenes(None)
    m.reset(x)
    for w in ws:
        m.step(w, adapt=False)
    torch.cuda.synchronize()
    shared, _ = _tube(st, dev, x, ws, overlap=True)
    bad = [k for k in NAMES if not _same(getattr(m, k), shared[k])]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 6. scenes persist across episodes

def test_two_resets_with_the_same_scenes_give_the_same_first_step(dev, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", "4")
    from diff_tube_mpc_strict_pt.core import TubeMPC

    st = fixed_setup()
    obs, tgs = scene_table(5)
    x, ws = _x0(B, dev), _w(B, 3)
    m = TubeMPC(st, batch=B, device=dev, dtype=TDT, disturbance="injected", write_log=True,
                scenes=_pack(st, obs, tgs, B, dev))
    firsts = []
    for _ in range(2):
        m.reset(x)
        m.step(ws[0], adapt=False)
        torch.cuda.synchronize()
        firsts.append({k: getattr(m, k).clone() for k in NAMES})
        m.step(ws[1], adapt=False)  # move the state and the workspace on before the next episode
        m.step(ws[2], adapt=False)
    bad = [k for k in NAMES if not _same(firsts[0][k], firsts[1][k])]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
def test_unsupported_configurations_are_refused_not_run_on_the_shared_table(dev):
    from diff_tube_mpc_strict_pt.core import TubeMPC, ilqr_solve

    st = fixed_setup()
    obs, tgs = scene_table(5)
    with pytest.raises(ValueError, match="scenes"):
        TubeMPC(st, batch=B, device=dev, dtype=torch.float64, disturbance="injected",
                scenes=_pack(st, obs, tgs, B, dev).double())
    gam = dataclasses.replace(st, problem=dataclasses.replace(st.problem, dbas_gamma=0.3))
    with pytest.raises(ValueError, match="scenes"):
        TubeMPC(gam, batch=B, device=dev, dtype=TDT, disturbance="injected", scenes=_pack(st, obs, tgs, B, dev))
    with pytest.raises(ValueError, match="scenes must be"):
        TubeMPC(st, batch=B, device=dev, dtype=TDT, disturbance="injected", scenes=_pack(st, obs, tgs, B + 1, dev))
    x0, V0 = _ilqr_inputs(st.problem, _x0(B, dev))
    mn = dataclasses.replace(st.problem, obs_aggregation="min")
    with pytest.raises(ValueError, match="scenes"):
        ilqr_solve(problem=mn, cost=st.nominal_cost, cfg=st.ilqr_nom, x0=x0, V_init=V0,
                   scenes=_pack(st, obs, tgs, B, dev))
