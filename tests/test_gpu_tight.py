"""Per-trajectory constraint tightening in the fused f32 standalone iLQR (GPU): ilqr_solve(tightening=),
dtmpc_ilqr_solve_tight, dbas_init(tightening=).

The kTight | kTightPT kernels (csrc/dtmpc_fast_tight.hip) differ from the shared ones before the solve -- a lane fills
p.tight from its own element of the tight array -- and in h_sm's last operation, hv - p.tight.  So the gate has two
parts.

Bitwise chains, over X, V, K, k, iters, status and the decision record (choices and candidate costs):
  1. trajectory i of a batch with four distinct s (0, 0.05, 0.3, 0.12; trajectory i takes value i % 4) == the B = 1
     launch with its own s;
  2. a uniform [B] == the broadcast zero-dim tensor;
  3. the same solve in three launch chunks == in one launch (the tight index is taken within the batch);
  4. with the heterogeneous scenes of tests/_scenes.py (S = 4, trajectory i -> scene (i // 4) % 4, so every (scene, s)
     pair occurs) every pair == its own B = 1 launch;
  5. s = 0 everywhere == the existing shared fused ilqr_solve, at lanes 1 / 2 / 4 and both kinds (hv - 0 is exact and
     h_sm is compiled without contraction).

Correctness of s != 0, against two references, per group of equal s:
  6. the three oracle builds' ilqr_solve at spec.h_offset = s under _common.agreement with base 1e-3 and the 0.99 share
     of tests/test_gpu_parity.py::test_ilqr_batched_vs_oracle (the fused f32 iLQR-vs-oracle test);
  7. the generic f32 kernel through the raw dtmpc_ilqr_solve with spec.h_offset = s.  Its bar is twice the parent's
     fused-vs-generic difference at s = 0 on the same starts (the shared fused kernel is the parent's instruction for
     instruction, profiles/r15/isa_identity.txt), both as the largest per-trajectory rel_rows of X among the
     trajectories both kernels finish with status 0.  Measured on an MI355X (profiles/r15/tight_forward_errors.txt):
     the s = 0 difference is 1.19e-3 (65 of 65 trajectories), so the bar is 2.38e-3; the tightened groups' differences
     are 1.32e-3 (s = 0.05), 5.6e-4 (s = 0.3) and 5.5e-4 (s = 0.12).  Against the oracle builds every trajectory of every
     group is within the band (worst error 9.9e-4 at s = 0.05 beside a build spread of 4.4e-3; 2.3e-5 at s = 0.3),
     while the oracle's own s = 0 solve is 0.12 to 0.30 away (median).
  8. refusals raise and run nothing.

f32, paper setup at fixed iterations (tol = -1, ten iterations), N = 50, B = 65 (one past a wave)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from _common import agreement, oracles, rel_rows
from _layer_tight import with_offset
from _scenes import S, fixed_setup, scene_table, setup_of, starts

pytestmark = pytest.mark.gpu
B = 65
TDT = torch.float32
FIELDS = ("X", "V", "K", "k", "iters", "status", "choices", "costs")
S_VALUES = (0.0, 0.05, 0.3, 0.12)
# the parent's fused-vs-generic difference at s = 0 on these starts (largest per-trajectory rel_rows of X): measured
GENERIC_S0 = 1.19e-3
GENERIC_BAR = 2.0 * GENERIC_S0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same(a, b):  # tests/test_gpu_lanes.py: NaN-aware bitwise equality
    return torch.equal(a, b) or (a.is_floating_point() and torch.equal(torch.isnan(a), torch.isnan(b)) and
                                 torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


def _s_of(n):
    return np.array(S_VALUES, np.float32)[np.arange(n) % 4]


def _inputs(problem, n, dev, s=None, scenes=None):
    from diff_tube_mpc_strict_pt.core import dbas_init

    x3 = torch.as_tensor(starts(n), dtype=TDT, device=dev)
    b0 = dbas_init(problem, x3, scenes=scenes) if s is None else dbas_init(problem, x3, scenes=scenes, tightening=s)
    return torch.cat([x3, b0[:, None]], 1), torch.zeros(n, problem.horizon, 2, dtype=TDT, device=dev)


def _solve(problem, cost, x0, V0, lanes, **kw):
    from diff_tube_mpc_strict_pt.core import ilqr_solve

    r = ilqr_solve(problem=problem, cost=cost, cfg=fixed_setup().ilqr_nom, x0=x0, V_init=V0, lanes=lanes, check=False,
                   record_choices=True, record_costs=True, **kw)
    torch.cuda.synchronize()
    assert r.choices is not None and r.costs is not None
    return tuple(getattr(r, f) for f in FIELDS)


def test_dbas_init_with_a_tightening(dev, oracle_lib):
    """B(h(x) - s_i) against the f64 oracle, with the shared table and with per-trajectory scenes; s = 0 is
    dbas_init's own value to f32 rounding."""
    from diff_tube_mpc_strict_pt.core import dbas_init, pack_scenes

    st = fixed_setup()
    p = st.problem
    s = torch.as_tensor(_s_of(B), device=dev)
    rng = np.random.default_rng(3)
    x = torch.as_tensor(np.stack([rng.uniform(0, 10, B), rng.uniform(0, 10, B), rng.uniform(-3, 3, B)], 1), dtype=TDT,
                        device=dev)
    o = oracle_lib.Oracle(np.float64)
    sp = p.to_c()
    xn = x.cpu().numpy().astype(np.float64)
    z = o.h_eval(sp, xn[:, 0], xn[:, 1])[0] - s.cpu().numpy().astype(np.float64)
    ref = o.barrier(sp, z)[1]
    got = dbas_init(p, x, tightening=s).cpu().numpy()
    # B'(z) amplifies the f32 rounding of h (|h| up to 1e2, so 1e-5 absolute) by up to 1 / a^2 near an obstacle's rim
    tol = 1e-5 * np.maximum(1.0, np.abs(o.barrier(sp, z)[2])) * 4 + 1e-5 * np.abs(ref)
    assert (np.abs(got - ref) <= tol).all(), np.abs(got - ref).max()
    assert not np.allclose(got, dbas_init(p, x).cpu().numpy())
    assert np.allclose(dbas_init(p, x, tightening=torch.zeros(B, device=dev)).cpu().numpy(),
                       dbas_init(p, x).cpu().numpy(), rtol=1e-5, atol=1e-6)
    # a zero-dim tensor is the uniform [B]
    assert torch.equal(dbas_init(p, x, tightening=torch.tensor(0.3, device=dev)),
                       dbas_init(p, x, tightening=torch.full((B,), 0.3, device=dev)))
    # scenes: B copies of the shared table give the shared values to f32 rounding
    obs, tgs = scene_table(5)
    zero = np.zeros(B, np.int64)
    sc = pack_scenes(p, obs[zero], tgs[zero], dtype=TDT, device=dev)
    assert np.allclose(dbas_init(p, x, scenes=sc, tightening=s).cpu().numpy(), got, rtol=1e-4, atol=1e-5)


def test_each_trajectory_equals_its_own_launch_and_broadcast_equals_uniform(dev):
    st = fixed_setup()
    p, cost = st.problem, st.nominal_cost
    s = torch.as_tensor(_s_of(B), device=dev)
    x0, V0 = _inputs(p, B, dev, s)
    for lanes in (1, 4):
        got = _solve(p, cost, x0, V0, lanes, tightening=s)
        assert (got[5] == 0).float().mean() >= 0.95
        for i in sorted({0, 1, 2, 3, 31, 62, 63, 64} if lanes == 1 else {1, 2, 63, 64}):
            one = _solve(p, cost, x0[i:i + 1], V0[i:i + 1], lanes, tightening=s[i:i + 1])
            for f, a, b in zip(FIELDS, one, got):
                assert _same(a, b[i:i + 1]), (lanes, i, f)
        # the tightening matters: the s = 0.3 trajectories do not end where an untightened solve takes them
        plain = _solve(p, cost, x0, V0, lanes)
        sel = torch.as_tensor(np.nonzero(np.arange(B) % 4 == 2)[0], device=dev)
        assert not _same(plain[0][sel], got[0][sel])
    # a uniform [B] == the broadcast zero-dim and one-element tensors
    u = torch.full((B,), 0.3, device=dev)
    x0u, _ = _inputs(p, B, dev, u)
    ref = _solve(p, cost, x0u, V0, 1, tightening=u)
    for t in (torch.tensor(0.3, device=dev), torch.tensor([0.3], device=dev)):
        got = _solve(p, cost, x0u, V0, 1, tightening=t)
        for f, a, b in zip(FIELDS, ref, got):
            assert _same(a, b), ("broadcast", f)


@pytest.mark.parametrize("lanes", [1, 4])
def test_chunked_launch_takes_the_tight_index_within_the_batch(dev, lanes, monkeypatch):
    """DTMPC_FAST_CHUNK = 256 and B = 600 = 256 + 256 + 88: three launches, the last with a partly masked tail wave.
    Trajectory i gets value (i + i // 256) % 4, which shifts by one from chunk to chunk: an index taken within the
    chunk would pick another value."""
    st = fixed_setup()
    p, cost = st.problem, st.nominal_cost
    n = 600
    k = (np.arange(n) + np.arange(n) // 256) % 4
    s = torch.as_tensor(np.array(S_VALUES, np.float32)[k], device=dev)
    assert not torch.equal(s[:88], s[256:344]) and not torch.equal(s[:88], s[512:])
    x0, V0 = _inputs(p, n, dev, s)
    monkeypatch.delenv("DTMPC_FAST_CHUNK", raising=False)
    one = _solve(p, cost, x0, V0, lanes, tightening=s)
    monkeypatch.setenv("DTMPC_FAST_CHUNK", "256")
    got = _solve(p, cost, x0, V0, lanes, tightening=s)
    assert (one[5] == 0).float().mean() >= 0.95
    for f, a, b in zip(FIELDS, one, got):
        assert _same(a, b), (lanes, f)


def test_heterogeneous_scenes_and_tightenings_pair_by_pair(dev):
    from diff_tube_mpc_strict_pt.core import pack_scenes

    st = fixed_setup()
    obs, tgs = scene_table(5)
    i = np.arange(B)
    ks, kt = (i // 4) % S, i % 4
    sc = pack_scenes(st.problem, obs[ks], tgs[ks], dtype=TDT, device=dev)
    s = torch.as_tensor(np.array(S_VALUES, np.float32)[kt], device=dev)
    x0, V0 = _inputs(st.problem, B, dev, s, scenes=sc)
    got = _solve(st.problem, st.nominal_cost, x0, V0, 1, tightening=s, scenes=sc)
    assert (got[5] == 0).float().mean() >= 0.95
    pairs = set()
    for j in range(B):
        if (ks[j], kt[j]) in pairs:
            continue
        pairs.add((ks[j], kt[j]))
        ss = setup_of(st, obs[ks[j]], tgs[ks[j]])  # the shared problem of this scene: no scenes array
        one = _solve(ss.problem, ss.nominal_cost, x0[j:j + 1], V0[j:j + 1], 1, tightening=s[j:j + 1])
        for f, a, b in zip(FIELDS, one, got):
            assert _same(a, b[j:j + 1]), (ks[j], kt[j], f)
    assert len(pairs) == 16
    only_scenes = _solve(st.problem, st.nominal_cost, x0, V0, 1, scenes=sc)
    only_tight = _solve(st.problem, st.nominal_cost, x0, V0, 1, tightening=s)
    assert not _same(only_scenes[0], got[0]) and not _same(only_tight[0], got[0])


@pytest.mark.parametrize("kind", ["target", "track"])
def test_zero_tightening_equals_shared_ilqr(dev, kind):
    from diff_tube_mpc_strict_pt.core import pack_scenes, tracking_cost

    st = fixed_setup()
    p = st.problem
    track = kind == "track"
    cost = tracking_cost(st.theta0) if track else st.nominal_cost
    x0, V0 = _inputs(p, B, dev)
    kw = {}
    if track:
        nom = _solve(p, st.nominal_cost, x0, V0, 1)
        kw = dict(X_ref=nom[0], U_ref=nom[1])
    zero = torch.zeros(B, device=dev)
    obs, tgs = scene_table(5)
    k0 = np.zeros(B, np.int64)
    sc = pack_scenes(p, obs[k0], tgs[k0], dtype=TDT, device=dev)
    for lanes in (1, 2, 4):
        ref = _solve(p, cost, x0, V0, lanes, **kw)
        assert (ref[5] == 0).float().mean() >= 0.95
        for scenes in (None, sc):
            got = _solve(p, cost, x0, V0, lanes, tightening=zero, scenes=scenes, **kw)
            for f, a, b in zip(FIELDS, ref, got):
                assert _same(a, b), (kind, lanes, scenes is not None, f)


def _generic(p, cost, x0, V0, s):
    """The generic f32 kernel through the raw dtmpc_ilqr_solve with spec.h_offset = s -> X [n, N+1, 4], status."""
    from diff_tube_mpc_strict_pt import _abi, _lib
    from diff_tube_mpc_strict_pt.core.ddp import from_soa, to_soa

    lib = _lib.load()
    n, N = x0.shape[0], p.horizon
    sp, cc, ic = with_offset(p.to_c(), s), cost.to_c(), fixed_setup().ilqr_nom.to_c()
    kw = dict(dtype=TDT, device=x0.device)
    x0s, Us = x0.t().contiguous(), to_soa(V0)
    Xs, Ks, ks = torch.empty(N + 1, 4, n, **kw), torch.zeros(N, 8, n, **kw), torch.zeros(N, 2, n, **kw)
    it = torch.zeros(n, dtype=torch.int32, device=x0.device)
    stt = torch.zeros(n, dtype=torch.int32, device=x0.device)
    rc = lib.dtmpc_ilqr_solve(_abi.F32, C.byref(sp), C.byref(cc), C.byref(ic), n, x0s.data_ptr(), None, None,
                              Xs.data_ptr(), Us.data_ptr(), Ks.data_ptr(), ks.data_ptr(), it.data_ptr(), stt.data_ptr(),
                              None, None)
    assert rc == 0, lib.dtmpc_last_error()
    torch.cuda.synchronize()
    return from_soa(Xs).cpu().numpy(), stt.cpu().numpy()


def test_tightened_solves_vs_oracle_and_generic_kernel(dev, oracle_lib):
    st = fixed_setup()
    p, cost = st.problem, st.nominal_cost
    sv = _s_of(B)
    s = torch.as_tensor(sv, device=dev)
    x0, V0 = _inputs(p, B, dev, s)
    got = _solve(p, cost, x0, V0, 1, tightening=s)
    X, status = got[0].cpu().numpy(), got[5].cpu().numpy()
    x0n, V0n = x0.cpu().numpy(), V0.cpu().numpy()
    ic = fixed_setup().ilqr_nom.to_c()
    ors = oracles(np.float32)
    # the parent's own fused-vs-generic difference at s = 0 on the same starts (measured here again, printed)
    x00, _ = _inputs(p, B, dev)
    Xf0 = _solve(p, cost, x00, V0, 1)
    Xg0, sg0 = _generic(p, cost, x00, V0, 0.0)
    k0 = (Xf0[5].cpu().numpy() == 0) & (sg0 == 0)
    d0 = rel_rows(Xf0[0].cpu().numpy()[k0], Xg0[k0]).max()
    print(f"[tight forward] s = 0: fused (shared) vs generic kernel, {int(k0.sum())} of {B}: {d0:.3g} "
          f"(GENERIC_S0 {GENERIC_S0:.3g}, bar {GENERIC_BAR:.3g})")
    ok_all, n_all, worst_g = 0, 0, 0.0
    for v in S_VALUES:
        idx = np.nonzero(sv == np.float32(v))[0]
        sp = with_offset(p.to_c(), float(np.float32(v)))
        outs = [o.ilqr_solve(sp, cost.to_c(), ic, x0n[idx], V0n[idx]) for o in ors]
        keep = (outs[0][5] == 0) & (status[idx] == 0)
        assert keep.mean() >= 0.95, (v, keep.mean())
        frac, e, sprd = agreement(X[idx][keep], [o_[0][keep] for o_ in outs], 1e-3)
        ok_all += int(round(frac * keep.sum()))
        n_all += int(keep.sum())
        Xg, sg = _generic(p, cost, x0[torch.as_tensor(idx, device=dev)], V0[torch.as_tensor(idx, device=dev)], float(np.float32(v)))
        kg = (sg == 0) & (status[idx] == 0)
        dg = rel_rows(X[idx][kg], Xg[kg]).max()
        worst_g = max(worst_g, float(dg))
        print(f"[tight forward] s = {v}: {int(keep.sum())} of {len(idx)} vs the oracle builds: share {frac:.3f}, worst "
              f"error {e.max():.3g} (spread max {sprd.max():.3g}); vs the generic kernel at h_offset = s "
              f"({int(kg.sum())}): {dg:.3g}")
        if v != 0.0:  # the tightening is visible to this check: the oracle's own s = 0 solve is further than the base
            o0 = ors[0].ilqr_solve(p.to_c(), cost.to_c(), ic, x0n[idx], V0n[idx])
            vis = rel_rows(o0[0][keep], outs[0][0][keep])
            print(f"[tight forward] s = {v}: the oracle's s = 0 solve differs by up to {vis.max():.3g}, median "
                  f"{np.median(vis):.3g}")
            assert np.median(vis) > 1e-3, v
    print(f"[tight forward] oracle share over the batch {ok_all / n_all:.3f}; generic worst {worst_g:.3g}")
    assert ok_all / n_all >= 0.99, (ok_all, n_all)
    assert worst_g <= GENERIC_BAR, (worst_g, GENERIC_BAR)


def test_unsupported_configurations_are_refused_not_run_untightened(dev, monkeypatch):
    from diff_tube_mpc_strict_pt.core import ilqr_solve
    from _weights import assignment, pack, weight_sets

    monkeypatch.delenv("DTMPC_FAST", raising=False)
    st = fixed_setup()
    p, cost, cfg = st.problem, st.nominal_cost, st.ilqr_nom
    s = torch.as_tensor(_s_of(B), device=dev)
    x0, V0 = _inputs(p, B, dev, s)
    with pytest.raises(ValueError, match="tightening"):  # f64
        ilqr_solve(problem=p, cost=cost, cfg=cfg, x0=x0.double(), V_init=V0.double(), tightening=s)
    with pytest.raises(ValueError, match="tightening"):  # gamma != 0 in the forward
        ilqr_solve(problem=dataclasses.replace(p, dbas_gamma=0.3), cost=cost, cfg=cfg, x0=x0, V_init=V0, tightening=s)
    with pytest.raises(ValueError, match="tightening"):  # a wrapped heading error
        ilqr_solve(problem=p, cost=dataclasses.replace(cost, wrap_angle=True), cfg=cfg, x0=x0, V_init=V0, tightening=s)
    with pytest.raises(ValueError, match="weights together with a tightening"):
        ilqr_solve(problem=p, cost=cost, cfg=cfg, x0=x0, V_init=V0, tightening=s,
                   weights=pack(weight_sets(cost), assignment(B), dev))
    with pytest.raises(ValueError, match=r"tightening must be a tensor \[65\]"):
        ilqr_solve(problem=p, cost=cost, cfg=cfg, x0=x0, V_init=V0, tightening=torch.zeros(B + 1, device=dev))
    with pytest.raises(ValueError, match="float32"):
        ilqr_solve(problem=p, cost=cost, cfg=cfg, x0=x0, V_init=V0, tightening=s.double())
    with pytest.raises(TypeError, match="tightening goes with the typed form"):  # the closure form
        ilqr_solve(cfg=cfg, x0=x0, V_init=V0, f=object(), tightening=s)
    monkeypatch.setenv("DTMPC_FAST", "0")
    with pytest.raises(ValueError, match="tightening"):
        ilqr_solve(problem=p, cost=cost, cfg=cfg, x0=x0, V_init=V0, tightening=s)
    # the tube step and the receding driver take no tightening
    import inspect

    from diff_tube_mpc_strict_pt.core.receding import nominal_receding
    from diff_tube_mpc_strict_pt.core.tube_mpc import TubeMPC

    for fn in (nominal_receding, TubeMPC.__init__, TubeMPC.reset, TubeMPC.step):
        assert "tightening" not in inspect.signature(fn).parameters, fn.__qualname__
