"""Own theta: per-trajectory ancillary weights adapted inside the fused f32 tube step (GPU).

In own-theta mode (TubeMPC(own_theta=True), csrc/dtmpc_fast_own.hip) trajectory i solves its ancillary problem with
its own column of theta [6, B] and updates that column from its own gradient row at the end of the step, so a batch
is B independent closed loops.  The contract is that trajectory i IS the shared path run at B = 1 on that trajectory,
which tests/test_gpu_parity.py ties to the reference; the solver is chaotic, so the gate is a chain of BITWISE
equalities to the shared path:

  1. held, uniform theta0                     == the shared run;
  2. held, four theta0 rows (i -> row i % 4)  == per row the shared path with that theta0 on the sub-batch;
  3. adapting, three steps                    == per trajectory the shared TubeMPC at B = 1, theta and vel included;
  4. a step that leaves every trajectory out  == the same (momentum decays, theta moves by it);
  5. rows 64..135 of the batch                == a batch of those rows alone;
  6. three launch chunks                      == one launch (the column index is taken within the batch);
  7. a shard (global_offset, Philox)          == its rows of the global batch;
  8. with per-trajectory scenes               == the shared path built from that scene and that theta0;
  9. episodes restart from theta0; unsupported configurations are refused and leave the device usable.

f32, paper setup at fixed iterations (tol = -1), N = 50, injected disturbances, B = 200 (not a multiple of 64: the
tail wave runs partly masked)."""
import dataclasses

import numpy as np
import pytest
import torch

from _scenes import fixed_setup, scene_table, setup_of, starts

pytestmark = pytest.mark.gpu
NAMES = ("x", "b", "xbar", "bbar", "Xnom", "Unom", "Xaux", "Uaux", "status", "log")
OWN = NAMES + ("theta", "vel")
B = 200
R = 4  # theta0 rows
TDT = torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _same(a, b):  # tests/test_gpu_scenes.py: NaN-aware bitwise equality
    return torch.equal(a, b) or (a.is_floating_point() and torch.equal(torch.isnan(a), torch.isnan(b)) and
                                 torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


def _x0(n, dev):
    return torch.as_tensor(starts(n), dtype=TDT, device=dev)


def _w(n, steps=2):  # tests/test_gpu_scenes.py _w
    rng = np.random.default_rng(3)
    return [torch.as_tensor(rng.uniform(-0.05, 0.05, (n, 3)), dtype=TDT) for _ in range(steps)]


def theta_rows(st):
    """[R][6] float64: the setup's theta0, and its Q and R entries scaled by 0.5, 2 and 1.5 (qba scaled too and kept
    inside [qb_min, qb_max])."""
    t0 = np.array(st.theta0, np.float64)
    rows = [t0]
    for k in (0.5, 2.0, 1.5):
        r = t0 * k
        r[5] = min(st.adapt.qb_max, max(st.adapt.qb_min, t0[5] * k))
        rows.append(r)
    return np.stack(rows)


def _theta0(st, n, dev, k=None):
    """[n, 6] theta0 of a batch: trajectory i gets row i % R (or row k[i])."""
    k = np.arange(n) % R if k is None else k
    return torch.as_tensor(theta_rows(st)[k], dtype=TDT, device=dev)


def _snap(m, names):
    torch.cuda.synchronize()
    return {k: getattr(m, k).clone() for k in names}


def _run(st, dev, x, ws, adapt, idx=None, every=False, **kw):
    """Steps with injected disturbances ws (the rows idx of them); the arrays afterwards (every: after each step)."""
    from diff_tube_mpc_strict_pt.core import TubeMPC

    m = TubeMPC(st, batch=x.shape[0], device=dev, dtype=TDT, disturbance="injected", write_log=True, **kw)
    names = OWN if kw.get("own_theta") else NAMES
    m.reset(x)
    snaps = []
    for w in ws:
        m.step(w if idx is None else w[idx], adapt=adapt)
        if every:
            snaps.append(_snap(m, names))
    return (snaps if every else _snap(m, names)), m


def _ok_share(parts):
    ok = sum(int((r["status"] == 0).sum()) for r in parts)
    n = sum(r["status"].numel() for r in parts)
    return ok, n


# ---------------------------------------------------------------------------------------------
# 1. held, uniform

@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_held_uniform_theta_equals_the_shared_run(dev, lanes, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", lanes)
    st = fixed_setup()
    x, ws = _x0(B, dev), _w(B)
    ref, m = _run(st, dev, x, ws, adapt=False)
    assert m.lanes == int(lanes)
    got, m = _run(st, dev, x, ws, adapt=False, own_theta=True)
    assert m.lanes == int(lanes) and m.own_theta and tuple(m.theta.shape) == (6, B) == tuple(m.vel.shape)
    assert (ref["status"] == 0).float().mean() >= 0.95
    bad = [k for k in NAMES if not _same(ref[k], got[k])]
    assert not bad, bad
    # held: every column is still the setup's theta0, the momentum zero
    assert torch.equal(got["theta"], torch.tensor(st.theta0, dtype=TDT, device=dev)[:, None].expand(6, B))
    assert not got["vel"].any()


# ---------------------------------------------------------------------------------------------
# 2. held, heterogeneous

@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_held_heterogeneous_theta_equals_the_shared_run_row_by_row(dev, lanes, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", lanes)
    st = fixed_setup()
    x, ws = _x0(B, dev), _w(B)
    t0 = _theta0(st, B, dev)
    got, m = _run(st, dev, x, ws, adapt=False, own_theta=True, theta0=t0)
    assert m.lanes == int(lanes) and torch.equal(got["theta"], t0.t())
    rows, shared = theta_rows(st), []
    for s in range(R):
        idx = torch.arange(s, B, R)
        ss = dataclasses.replace(st, theta0=tuple(float(v) for v in rows[s]))
        shared.append((idx, _run(ss, dev, x[idx.to(dev)], ws, adapt=False, idx=idx)[0]))
    ok, n = _ok_share([r for _, r in shared])
    assert ok >= 0.95 * n, (ok, n)
    for s, (idx, r) in enumerate(shared):
        bad = [k for k in NAMES if not _same(got[k][..., idx.to(dev)], r[k])]
        assert not bad, (s, bad)
    # the weights matter: row 1's trajectories do not plan as they would with the setup's theta0
    idx = shared[1][0]
    plain, _ = _run(st, dev, x[idx.to(dev)], ws, adapt=False, idx=idx)
    assert not _same(plain["Xaux"], shared[1][1]["Xaux"])


# ---------------------------------------------------------------------------------------------
# 3. / 4. adapting: trajectory i == the shared TubeMPC at B = 1 on trajectory i

PICK = (0, 63, 64, 137, 199)


def _adapting_vs_b1(dev, steps, bound_before=None):
    """Own mode on the batch against the shared mode at B = 1 on each of PICK, after every step; bound_before = k:
    grad_bound = 1e-30 from step k on in both, so that step leaves every trajectory out.  Returns the B = 1 runs."""
    from diff_tube_mpc_strict_pt.core import TubeMPC

    st = fixed_setup()
    x, ws = _x0(B, dev), _w(B, steps)

    def run(xs, wl, **kw):
        m = TubeMPC(st, batch=xs.shape[0], device=dev, dtype=TDT, disturbance="injected", write_log=True, **kw)
        m.reset(xs)
        out = []
        for k, w in enumerate(wl):
            if bound_before is not None and k >= bound_before:
                m.cfg.grad_bound = 1e-30
            m.step(w)
            out.append(_snap(m, OWN))
        return out, m

    got, m = run(x, ws, own_theta=True)
    lanes = m.lanes
    ones = {}
    for i in PICK:
        ref, m1 = run(x[i:i + 1], [w[i:i + 1] for w in ws])
        assert m1.lanes == lanes and not m1.own_theta
        ones[i] = ref
        for k in range(steps):
            bad = [n for n in NAMES if not _same(got[k][n][..., i:i + 1], ref[k][n])]
            bad += [n for n in ("theta", "vel") if not _same(got[k][n][:, i], ref[k][n])]
            assert not bad, (i, k, bad)
    ok = sum(int(ones[i][-1]["status"][0] == 0) for i in PICK)
    assert ok >= 0.95 * len(PICK), ok
    return st, got, ones


@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_adapting_trajectory_equals_the_shared_run_at_batch_one(dev, lanes, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", lanes)
    st, got, ones = _adapting_vs_b1(dev, 3)
    t0 = torch.tensor(st.theta0, dtype=TDT, device=dev)
    for i in PICK:  # the B = 1 run adapted, or the comparison shows nothing
        assert not torch.equal(ones[i][0]["theta"], t0), i
    # and the trajectories adapted apart
    assert not torch.equal(got[-1]["theta"][:, 0], got[-1]["theta"][:, 199])


def test_a_trajectory_left_out_of_a_step_still_decays_its_momentum(dev, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", "2")
    st, got, ones = _adapting_vs_b1(dev, 3, bound_before=1)
    mom = torch.tensor(st.adapt.momentum, dtype=TDT, device=dev)
    assert got[0]["vel"].any()
    assert _same(got[1]["vel"], mom * got[0]["vel"])
    assert _same(got[2]["vel"], mom * got[1]["vel"])
    moved = got[1]["theta"] != got[0]["theta"]
    assert moved.any()  # theta still moves by the decayed momentum


# ---------------------------------------------------------------------------------------------
# 5. independence

def test_rows_of_a_batch_equal_a_batch_of_those_rows(dev, monkeypatch):
    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    st = fixed_setup()
    x, ws = _x0(B, dev), _w(B)
    t0 = _theta0(st, B, dev)
    full, _ = _run(st, dev, x, ws, adapt=True, own_theta=True, theta0=t0)
    idx = torch.arange(64, 136)
    part, m = _run(st, dev, x[64:136], ws, adapt=True, idx=idx, own_theta=True, theta0=t0[64:136])
    assert m.B == 72
    assert (part["status"] == 0).float().mean() >= 0.95
    bad = [k for k in OWN if not _same(full[k][..., 64:136], part[k])]
    assert not bad, bad
    assert part["vel"].any()


# ---------------------------------------------------------------------------------------------
# 6. chunks

@pytest.mark.parametrize("lanes", ["1", "4"])
def test_chunked_launch_takes_the_column_within_the_batch(dev, lanes, monkeypatch):
    """DTMPC_FAST_CHUNK = 256 and B = 2 * 256 + 88: three launches.  Trajectory i gets theta0 row (i + i // 256) % R,
    which shifts from chunk to chunk, so a column taken within the chunk would read another row's weights."""
    monkeypatch.setenv("DTMPC_TUBE_LANES", lanes)
    st = fixed_setup()
    n = 2 * 256 + 88
    x, ws = _x0(n, dev), _w(n)
    i = np.arange(n)
    t0 = _theta0(st, n, dev, k=(i + i // 256) % R)
    assert not torch.equal(t0[:88], t0[256:344]) and not torch.equal(t0[:88], t0[512:])
    one, m = _run(st, dev, x, ws, adapt=True, own_theta=True, theta0=t0)
    assert m.chunk >= n and m.lanes == int(lanes)
    monkeypatch.setenv("DTMPC_FAST_CHUNK", "256")
    got, m = _run(st, dev, x, ws, adapt=True, own_theta=True, theta0=t0)
    assert m.chunk == 256
    assert (one["status"] == 0).float().mean() >= 0.95
    bad = [k for k in OWN if not _same(one[k], got[k])]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 7. sharding without a process group

def test_a_shard_equals_its_rows_of_the_global_batch(dev, monkeypatch):
    from diff_tube_mpc_strict_pt.core import TubeMPC

    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    st = fixed_setup()
    x = _x0(B, dev)
    t0 = _theta0(st, B, dev)

    def run(lo, hi):
        m = TubeMPC(st, batch=hi - lo, device=dev, dtype=TDT, disturbance="philox", seed=7, write_log=True,
                    global_offset=lo, global_batch=B, own_theta=True, theta0=t0[lo:hi])
        m.reset(x[lo:hi])
        m.step()
        m.step()
        return _snap(m, OWN)

    full, shard = run(0, B), run(100, B)
    assert (full["status"] == 0).float().mean() >= 0.95
    bad = [k for k in OWN if not _same(full[k][..., 100:], shard[k])]
    assert not bad, bad
    # the disturbance is keyed by the global index: the first hundred rows are another draw
    assert not _same(full["x"][..., :100], shard["x"])


# ---------------------------------------------------------------------------------------------
# 8. with per-trajectory scenes

@pytest.mark.parametrize("lanes", ["1", "4"])
def test_own_theta_composes_with_scenes(dev, lanes, monkeypatch):
    from diff_tube_mpc_strict_pt.core import pack_scenes

    monkeypatch.setenv("DTMPC_TUBE_LANES", lanes)
    st = fixed_setup()
    obs, tgs = scene_table(5)
    x, ws = _x0(B, dev), _w(B)
    i = np.arange(B)
    ks, kr = i % 4, (i // 4) % R  # scene and theta0 row of trajectory i
    sc = pack_scenes(st.problem, obs[ks], tgs[ks], dtype=TDT, device=dev)
    got, m = _run(st, dev, x, ws, adapt=False, own_theta=True, theta0=_theta0(st, B, dev, k=kr), scenes=sc)
    assert m.lanes == int(lanes) and m.state.scenes
    rows, shared = theta_rows(st), []
    for s, r in ((0, 0), (1, 2), (2, 1), (3, 3)):
        idx = torch.as_tensor(np.nonzero((ks == s) & (kr == r))[0])
        assert len(idx) >= 12
        ss = dataclasses.replace(setup_of(st, obs[s], tgs[s]), theta0=tuple(float(v) for v in rows[r]))
        shared.append((idx, _run(ss, dev, x[idx.to(dev)], ws, adapt=False, idx=idx)[0]))
    ok, n = _ok_share([r for _, r in shared])
    assert ok >= 0.95 * n, (ok, n)
    for j, (idx, r) in enumerate(shared):
        bad = [k for k in NAMES if not _same(got[k][..., idx.to(dev)], r[k])]
        assert not bad, (j, bad)


# ---------------------------------------------------------------------------------------------
# 9. episodes and refusals

def test_two_resets_give_the_same_first_step(dev, monkeypatch):
    from diff_tube_mpc_strict_pt.core import TubeMPC

    monkeypatch.setenv("DTMPC_TUBE_LANES", "4")
    st = fixed_setup()
    x, ws = _x0(B, dev), _w(B, 3)
    t0 = _theta0(st, B, dev)
    m = TubeMPC(st, batch=B, device=dev, dtype=TDT, disturbance="injected", write_log=True, own_theta=True, theta0=t0)
    firsts = []
    for _ in range(2):
        m.reset(x)
        assert torch.equal(m.theta, t0.t()) and not m.vel.any()
        m.step(ws[0])
        firsts.append(_snap(m, OWN))
        m.step(ws[1])  # move the state, the weights and the momentum on before the next episode
        m.step(ws[2])
    assert firsts[0]["vel"].any() and not torch.equal(firsts[0]["theta"], t0.t())
    bad = [k for k in OWN if not _same(firsts[0][k], firsts[1][k])]
    assert not bad, bad


def test_unsupported_configurations_are_refused_and_the_device_stays_usable(dev):
    from diff_tube_mpc_strict_pt.core import TubeMPC

    st = fixed_setup()
    x, ws = _x0(B, dev), _w(B, 1)

    def shared_step_runs():
        m = TubeMPC(st, batch=B, device=dev, dtype=TDT, disturbance="injected")
        m.reset(x)
        m.step(ws[0])
        torch.cuda.synchronize()
        assert (m.status == 0).float().mean() >= 0.95 and tuple(m.theta.shape) == (6,)

    with pytest.raises(ValueError, match="dtmpc_own_theta_supported"):
        TubeMPC(st, batch=B, device=dev, dtype=torch.float64, disturbance="injected", own_theta=True)
    shared_step_runs()
    gam = dataclasses.replace(st, problem=dataclasses.replace(st.problem, dbas_gamma=0.3))
    with pytest.raises(ValueError, match="dtmpc_own_theta_supported"):
        TubeMPC(gam, batch=B, device=dev, dtype=TDT, disturbance="injected", own_theta=True)
    shared_step_runs()
    with pytest.raises(ValueError, match="overlap"):
        TubeMPC(st, batch=B, device=dev, dtype=TDT, disturbance="injected", own_theta=True, overlap=True)
    shared_step_runs()
    with pytest.raises(ValueError, match="theta0 must be"):
        TubeMPC(st, batch=B, device=dev, dtype=TDT, disturbance="injected", own_theta=True,
                theta0=torch.zeros(B + 1, 6))
