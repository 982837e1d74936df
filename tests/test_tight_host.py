"""The per-trajectory constraint tightening, host side (no device): the five entry points beside ABI 8 and their
prototypes, the workspace sizes, the argument validation of dtmpc_ilqr_solve_tight and dtmpc_solve_backward_tight before
any device call (fake pointers, never dereferenced), that the existing entries keep refusing spec.h_offset != 0, the
Python defaults, and the refusals of ilqr_solve / solve_backward / diff_ilqr_solve / dbas_init that need no device.

The forward entry has dtmpc_ilqr_solve_scenes' arguments and tight: it has no weights argument, so per-trajectory
weights together with a tightening are refused where they can be asked for together, in core.ilqr_solve and
core.diff_ilqr_solve (and in the launcher behind the entries, which no public entry reaches with both)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import inspect

import pytest

from test_layer_dbas_host import _decl, _setup


@pytest.fixture(scope="module")
def lib():
    from diff_tube_mpc_strict_pt import _lib

    return _lib.load()


NEW = ("dtmpc_tight_supported", "dtmpc_ilqr_solve_tight_workspace_bytes", "dtmpc_ilqr_solve_tight",
       "dtmpc_solve_backward_tight_workspace_bytes", "dtmpc_solve_backward_tight")


def test_tight_entry_points_are_exported_beside_abi_8(lib):
    from diff_tube_mpc_strict_pt import _abi, core

    assert _abi.ABI_VERSION == 8 and lib.dtmpc_abi_version() == 8
    for name in NEW:
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
    P = _abi.PROTOTYPES
    # forward: dtmpc_ilqr_solve_scenes' arguments with one more pointer (tight) after scenes
    old, new = P["dtmpc_ilqr_solve_scenes"], P["dtmpc_ilqr_solve_tight"]
    assert new[0] is old[0] and new[1] == old[1][:-1] + [C.c_void_p] + old[1][-1:]
    rs, ps = _decl("dtmpc_ilqr_solve_scenes")
    rt, pt = _decl("dtmpc_ilqr_solve_tight")
    assert rt == rs == "int" and pt == ps[:-1] + ["const void*"] + ps[-1:] and len(pt) == len(new[1])
    assert P["dtmpc_tight_supported"] == P["dtmpc_scenes_supported"]
    assert _decl("dtmpc_tight_supported") == _decl("dtmpc_scenes_supported")
    assert P["dtmpc_ilqr_solve_tight_workspace_bytes"] == P["dtmpc_ilqr_workspace_bytes"]
    assert _decl("dtmpc_ilqr_solve_tight_workspace_bytes") == _decl("dtmpc_ilqr_workspace_bytes")
    # backward: dtmpc_solve_backward_dbas' arguments with tight after weights and g_tight after g_dbas
    old, new = P["dtmpc_solve_backward_dbas"], P["dtmpc_solve_backward_tight"]
    assert new[0] is old[0] and new[1] == old[1][:10] + [C.c_void_p] + old[1][10:19] + [C.c_void_p] + old[1][19:]
    rd, pd = _decl("dtmpc_solve_backward_dbas")
    rt, pt = _decl("dtmpc_solve_backward_tight")
    assert rt == rd == "int" and pt == pd[:10] + ["const void*"] + pd[10:19] + ["void*"] + pd[19:]
    assert len(pt) == len(new[1])
    assert _decl("dtmpc_solve_backward_tight_workspace_bytes") == ("size_t", ["int", "int32_t", "int64_t"])
    assert P["dtmpc_solve_backward_tight_workspace_bytes"] == P["dtmpc_solve_backward_geom_workspace_bytes"]
    # Python defaults: nothing changes unless asked for
    f = {x.name: x for x in dataclasses.fields(core.SolveGradient)}
    assert f["tight"].default is None and list(f)[-2:] == ["x0", "obstacles"]
    sb = inspect.signature(core.solve_backward).parameters
    assert sb["tightening"].default is None and sb["want_tight"].default is False
    assert inspect.signature(core.diff_ilqr_solve).parameters["tightening"].default is None
    assert inspect.signature(core.ilqr_solve).parameters["tightening"].default is None
    assert inspect.signature(core.dbas_init).parameters["tightening"].default is None


def test_tight_workspace_bytes(lib):
    from diff_tube_mpc_strict_pt import _abi

    f = lib.dtmpc_solve_backward_tight_workspace_bytes
    for N, B in ((50, 65536), (1, 1), (3, 257)):
        assert f(_abi.F32, N, B) == lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, N, B) == N * 100 * B
    assert f(_abi.F64, 50, 4) == 0 and f(_abi.F32, 0, 4) == 0 and f(_abi.F32, 50, 0) == 0
    g = lib.dtmpc_ilqr_solve_tight_workspace_bytes
    for N, B, lanes in ((50, 65, 0), (50, 65, 1), (50, 65, 2), (50, 65, 4), (1, 1, 1), (50, 65536, 1)):
        assert g(_abi.F32, N, B, lanes) == lib.dtmpc_ilqr_workspace_bytes(_abi.F32, N, B, lanes) > 0
    assert g(_abi.F64, 50, 65, 1) == 0 and g(_abi.F32, 50, 65, 3) == 0 and g(_abi.F32, 0, 65, 1) == 0


def test_tight_supported(lib):
    from diff_tube_mpc_strict_pt import _abi

    st = _setup()
    p, ic = st.problem, st.ilqr_nom.to_c()
    q = lambda prob, dt=_abi.F32: lib.dtmpc_tight_supported(dt, C.byref(prob), C.byref(ic))  # noqa: E731
    assert q(p.to_c()) == 1
    assert q(p.to_c(), _abi.F64) == 0
    assert q(dataclasses.replace(p, dbas_gamma=0.3).to_c()) == 0
    assert q(dataclasses.replace(p, obs_aggregation="min").to_c()) == 0
    assert q(dataclasses.replace(p, barrier_type="log").to_c()) == 0
    off = p.to_c()
    off.h_offset = 0.05
    assert q(off) == 0


def _fwd(lib, st, B=8):
    from diff_tube_mpc_strict_pt import _abi

    p, c = st.problem, st.nominal_cost
    wb = lib.dtmpc_ilqr_solve_tight_workspace_bytes(_abi.F32, p.horizon, B, 1)
    base = dict(dtype=_abi.F32, spec=p.to_c(), cost=c.to_c(), cfg=st.ilqr_nom.to_c(), B=B, x0=1, Xref=None, Uref=None,
                X=1, U=1, K=1, kff=1, iters=1, status=1, choices=None, costs=None, lanes=1, work=1, work_bytes=wb,
                scenes=None, tight=1)

    def call(**over):
        a = dict(base, **over)
        return lib.dtmpc_ilqr_solve_tight(a["dtype"], C.byref(a["spec"]), C.byref(a["cost"]), C.byref(a["cfg"]), a["B"],
                                          a["x0"], a["Xref"], a["Uref"], a["X"], a["U"], a["K"], a["kff"], a["iters"],
                                          a["status"], a["choices"], a["costs"], a["lanes"], a["work"], a["work_bytes"],
                                          a["scenes"], a["tight"], None)

    return call, wb


def test_forward_refuses_before_any_device_call(lib, monkeypatch):
    from diff_tube_mpc_strict_pt import _abi

    st = _setup()
    p, c = st.problem, st.nominal_cost
    call, wb = _fwd(lib, st)

    def refused(word, **over):
        rc = call(**over)
        assert rc == _abi.ERR_BAD_ARG, (over, rc)
        assert word in lib.dtmpc_last_error(), (over, lib.dtmpc_last_error())

    refused(b"NULL tight", tight=None)
    refused(b"NULL tight", tight=None, scenes=1)
    off = p.to_c()
    off.h_offset = 0.05
    refused(b"h_offset", spec=off)  # the array is the only source of s
    refused(b"dbas_gamma == 0", spec=dataclasses.replace(p, dbas_gamma=0.3).to_c())
    refused(b"f32", dtype=_abi.F64)
    refused(b"smooth-min", spec=dataclasses.replace(p, obs_aggregation="min").to_c())
    refused(b"inverse barrier", spec=dataclasses.replace(p, barrier_type="log").to_c())
    refused(b"wrap", cost=dataclasses.replace(c, wrap_angle=True).to_c())
    refused(b"lanes", lanes=3)
    refused(b"work_bytes", work_bytes=wb - 1)
    refused(b"work_bytes", work=None)
    for f in ("x0", "X", "U", "K", "kff", "status"):
        refused(b"NULL", **{f: None})
    monkeypatch.setenv("DTMPC_FAST", "0")
    refused(b"DTMPC_FAST", tight=1)


def test_existing_entries_keep_refusing_h_offset(lib):
    """No existing entry takes a tightening through spec.h_offset: the fused standalone solve falls back to the generic
    kernel (dtmpc_ilqr_fused_eligible 0), the scenes / weights entries and every dtmpc_solve_backward* entry refuse."""
    from diff_tube_mpc_strict_pt import _abi

    st = _setup()
    p, c = st.problem, st.nominal_cost
    off = p.to_c()
    off.h_offset = 0.05
    cc, ic = c.to_c(), st.ilqr_nom.to_c()
    assert lib.dtmpc_ilqr_fused_eligible(_abi.F32, C.byref(p.to_c()), C.byref(cc), C.byref(ic)) == 1
    assert lib.dtmpc_ilqr_fused_eligible(_abi.F32, C.byref(off), C.byref(cc), C.byref(ic)) == 0
    assert lib.dtmpc_scenes_supported(_abi.F32, C.byref(off), C.byref(ic)) == 0
    assert lib.dtmpc_weights_supported(_abi.F32, C.byref(off), C.byref(ic)) == 0
    assert lib.dtmpc_solve_backward_supported(_abi.F32, C.byref(off), C.byref(cc)) == 0


def test_backward_refuses_before_any_device_call(lib):
    """Every BAD_ARG condition of dtmpc_solve_backward and the new entry's own (tight or g_tight NULL, h_offset != 0,
    work_bytes below its size), with fake pointers; weights, g_x0, g_obs and g_dbas may each be NULL -- those calls get
    past the argument rules (they are not made here: they would reach the device)."""
    from diff_tube_mpc_strict_pt import _abi

    st = _setup()
    p, c = st.problem, st.nominal_cost
    B, N = 8, p.horizon
    wb = lib.dtmpc_solve_backward_tight_workspace_bytes(_abi.F32, N, B)
    tgt = dict(dtype=_abi.F32, spec=p.to_c(), cost=c.to_c(), B=B, X=1, U=1, Xref=None, Uref=None, scenes=None,
               weights=None, tight=1, gX=1, gU=1, g_w=1, g_target=1, g_xref=None, g_uref=None, g_x0=1, g_obs=1, g_dbas=1,
               g_tight=1, work=1, work_bytes=wb, status=1)
    trk = dict(tgt, cost=dataclasses.replace(c, kind="track").to_c(), Xref=1, Uref=1, g_target=None, g_xref=1,
               g_uref=1)

    def call(base, **over):
        a = dict(base, **over)
        sp, cc = a["spec"], a["cost"]
        return lib.dtmpc_solve_backward_tight(a["dtype"], None if sp is None else C.byref(sp),
                                              None if cc is None else C.byref(cc), a["B"], a["X"], a["U"], a["Xref"],
                                              a["Uref"], a["scenes"], a["weights"], a["tight"], a["gX"], a["gU"],
                                              a["g_w"], a["g_target"], a["g_xref"], a["g_uref"], a["g_x0"], a["g_obs"],
                                              a["g_dbas"], a["g_tight"], a["work"], a["work_bytes"], a["status"], None)

    def refused(base, word, **over):
        rc = call(base, **over)
        assert rc == _abi.ERR_BAD_ARG, (over, rc)
        assert word in lib.dtmpc_last_error(), (over, lib.dtmpc_last_error())

    for base in (tgt, trk, dict(tgt, weights=1), dict(tgt, g_x0=None, g_obs=None, g_dbas=None), dict(trk, g_dbas=None)):
        refused(base, b"NULL tight or g_tight", tight=None)
        refused(base, b"NULL tight or g_tight", g_tight=None)
        refused(base, b"dtmpc_solve_backward_tight_workspace_bytes", work_bytes=wb - 1)
        refused(base, b"dtmpc_solve_backward_tight_workspace_bytes",
                work_bytes=lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, N, B))
        refused(base, b"work_bytes", work=None)
    off = p.to_c()
    off.h_offset = 0.05
    refused(tgt, b"h_offset", spec=off)  # the array is the only source of s
    for f in ("X", "U", "gX", "gU", "g_w", "status"):
        refused(tgt, b"NULL", **{f: None})
    refused(tgt, b"NULL", spec=None)
    refused(tgt, b"NULL", cost=None)
    refused(tgt, b"batch", B=0)
    for f in ("Xref", "Uref", "g_xref", "g_uref"):
        refused(tgt, b"tracking cost", **{f: 1})
    refused(trk, b"g_target", g_target=1)
    refused(trk, b"Xref", Xref=None)
    refused(tgt, b"f32 only", dtype=_abi.F64)
    refused(tgt, b"smooth-min", spec=dataclasses.replace(p, obs_aggregation="min").to_c())
    refused(tgt, b"inverse barrier", spec=dataclasses.replace(p, barrier_type="log").to_c())
    refused(tgt, b"wrapped", cost=dataclasses.replace(c, wrap_angle=True).to_c())
    # any dbas_gamma is supported: the refusal of a too small workspace is reached, not one of the configuration
    refused(tgt, b"work_bytes", spec=dataclasses.replace(p, dbas_gamma=0.3).to_c(), work_bytes=wb - 1)
    # the older entries still refuse a tightened spec
    rc = lib.dtmpc_solve_backward_dbas(_abi.F32, C.byref(off), C.byref(c.to_c()), B, 1, 1, None, None, None, None, 1, 1,
                                       1, 1, None, None, 1, 1, 1, 1, wb, 1, None)
    assert rc == _abi.ERR_BAD_ARG and b"h_offset" in lib.dtmpc_last_error()


def test_python_refusals_without_a_device():
    import torch

    from diff_tube_mpc_strict_pt.core import dbas_init, diff_ilqr_solve, ilqr_solve, solve_backward
    from diff_tube_mpc_strict_pt.core.closures import DBaSDynamics  # noqa: F401  (the closure form exists)

    st = _setup()
    p, cost = st.problem, st.nominal_cost
    B, N = 3, p.horizon
    s = torch.full((B,), 0.05)
    w = dict(Q=torch.ones(3), R=torch.ones(2), Qf=torch.ones(3), qb=torch.tensor(1.0), target=torch.zeros(3))
    kw = dict(cfg=st.ilqr_nom, kind="target", x0=torch.zeros(B, 4), V_init=torch.zeros(B, N, 2), **w)
    # diff_ilqr_solve: shapes, f64, gamma, per-trajectory weights
    for bad in (torch.zeros(B + 1), torch.zeros(B, 1, 2), torch.zeros(2)):
        with pytest.raises(ValueError, match="tightening must be"):
            diff_ilqr_solve(problem=p, tightening=bad, **kw)
    with pytest.raises(ValueError, match="tightening is a tensor"):
        diff_ilqr_solve(problem=p, tightening=0.05, **kw)
    with pytest.raises(ValueError, match="float32"):
        diff_ilqr_solve(problem=p, tightening=s, **dict(kw, x0=torch.zeros(B, 4, dtype=torch.float64)))
    with pytest.raises(ValueError, match="dbas_gamma == 0"):
        diff_ilqr_solve(problem=dataclasses.replace(p, dbas_gamma=0.3), tightening=s, **kw)
    with pytest.raises(ValueError, match="dbas_gamma == 0"):
        diff_ilqr_solve(problem=p, tightening=s, dbas_gamma=torch.tensor(0.0), **kw)
    with pytest.raises(ValueError, match="per-trajectory weights together with a tightening"):
        diff_ilqr_solve(problem=p, tightening=s, **dict(kw, Q=torch.ones(B, 3)))
    # a [B], a zero-dim and a one-element tensor are admitted: the next refusal is the device's (these are host tensors)
    for t in (s.clone().requires_grad_(), torch.tensor(0.05, requires_grad=True), torch.tensor([0.05])):
        with pytest.raises(ValueError, match="no CPU fallback"):
            diff_ilqr_solve(problem=p, tightening=t, **kw)
    # the closure form takes no tightening
    with pytest.raises(TypeError, match="tightening goes with the typed form"):
        ilqr_solve(cfg=st.ilqr_nom, x0=torch.zeros(4), V_init=torch.zeros(N, 2), f=object(), tightening=s)
    # solve_backward: want_tight needs the array
    z = dict(X=torch.zeros(B, N + 1, 4), V=torch.zeros(B, N, 2), grad_X=torch.zeros(B, N + 1, 4),
             grad_V=torch.zeros(B, N, 2))
    with pytest.raises(ValueError, match="want_tight needs tightening"):
        solve_backward(problem=p, cost=cost, want_tight=True, **z)
    with pytest.raises(ValueError, match="no CPU fallback"):
        solve_backward(problem=p, cost=cost, tightening=s, want_tight=True, **z)
    with pytest.raises(ValueError, match="no CPU fallback"):
        dbas_init(p, torch.zeros(B, 3), tightening=s)
