"""The differentiable solve's rows w.r.t. x0 and the obstacle circles, host side (no device): the entry points beside
ABI 8, their ctypes signatures, dtmpc_solve_backward_geom's argument validation before any device call, and the
``wrt=`` truth table of diff_ilqr_solve as far as it needs no device."""
from __future__ import annotations

import ctypes as C
import dataclasses
import inspect

import pytest


@pytest.fixture(scope="module")
def lib():
    from diff_tube_mpc_strict_pt import _lib

    return _lib.load()


def _setup():
    from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config

    return paper_setup_from_config(paper_config())


def test_geom_entry_points_are_exported_beside_abi_8(lib):
    from diff_tube_mpc_strict_pt import _abi, core

    assert _abi.ABI_VERSION == 8 and lib.dtmpc_abi_version() == 8
    for name in ("dtmpc_solve_backward_geom_workspace_bytes", "dtmpc_solve_backward_geom"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
    # dtmpc_solve_backward's arguments plus two pointers (g_x0, g_obs) in front of the workspace
    old, new = _abi.PROTOTYPES["dtmpc_solve_backward"], _abi.PROTOTYPES["dtmpc_solve_backward_geom"]
    assert new[0] is old[0] and len(new[1]) == len(old[1]) + 2
    assert new[1][:15] == old[1][:15] and new[1][15:17] == [C.c_void_p, C.c_void_p] and new[1][17:] == old[1][15:]
    assert _abi.PROTOTYPES["dtmpc_solve_backward_geom_workspace_bytes"] == \
        _abi.PROTOTYPES["dtmpc_solve_backward_workspace_bytes"]
    f = {x.name: x for x in dataclasses.fields(core.SolveGradient)}
    assert list(f)[-2:] == ["x0", "obstacles"] and f["x0"].default is None and f["obstacles"].default is None
    sb = inspect.signature(core.solve_backward).parameters
    assert sb["want_x0"].default is False and sb["want_obstacles"].default is False
    assert tuple(inspect.signature(core.diff_ilqr_solve).parameters["wrt"].default) == ()


def test_geom_workspace_bytes(lib):
    from diff_tube_mpc_strict_pt import _abi

    # the 20 values of dtmpc_solve_backward and the barrier row of V_xx (4) and of tilde V_x (1): 25 f32 values
    assert lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, 50, 65536) == 50 * 100 * 65536
    assert lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, 1, 1) == 100
    assert lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F64, 50, 4) == 0
    assert lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, 0, 4) == 0
    assert lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, 50, 0) == 0
    assert lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, 50, 65536) == 50 * 80 * 65536  # untouched


def test_geom_refuses_before_any_device_call(lib):
    """Every BAD_ARG condition of dtmpc_solve_backward, the two of the new entry (both outputs NULL, work_bytes below
    the new size), with fake (never dereferenced) pointers: no device is needed."""
    from diff_tube_mpc_strict_pt import _abi

    st = _setup()
    p, c = st.problem, st.nominal_cost
    B, N = 8, p.horizon
    wb = lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, N, B)
    tgt = dict(dtype=_abi.F32, spec=p.to_c(), cost=c.to_c(), B=B, X=1, U=1, Xref=None, Uref=None, scenes=None, gX=1,
               gU=1, g_w=1, g_target=1, g_xref=None, g_uref=None, g_x0=1, g_obs=1, work=1, work_bytes=wb, status=1)
    trk = dict(tgt, cost=dataclasses.replace(c, kind="track").to_c(), Xref=1, Uref=1, g_target=None, g_xref=1,
               g_uref=1)

    def call(base, **over):
        a = dict(base, **over)
        sp, cc = a["spec"], a["cost"]
        return lib.dtmpc_solve_backward_geom(a["dtype"], None if sp is None else C.byref(sp),
                                             None if cc is None else C.byref(cc), a["B"], a["X"], a["U"], a["Xref"],
                                             a["Uref"], a["scenes"], a["gX"], a["gU"], a["g_w"], a["g_target"],
                                             a["g_xref"], a["g_uref"], a["g_x0"], a["g_obs"], a["work"],
                                             a["work_bytes"], a["status"], None)

    def refused(base, word, **over):
        rc = call(base, **over)
        assert rc == _abi.ERR_BAD_ARG, (over, rc)
        assert word in lib.dtmpc_last_error(), (over, lib.dtmpc_last_error())

    # the new rules
    refused(tgt, b"both NULL", g_x0=None, g_obs=None)
    refused(trk, b"both NULL", g_x0=None, g_obs=None)
    refused(tgt, b"dtmpc_solve_backward_geom_workspace_bytes", work_bytes=wb - 1)
    refused(tgt, b"dtmpc_solve_backward_geom_workspace_bytes",
            work_bytes=lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, N, B))
    refused(tgt, b"work_bytes", work=None)
    # dtmpc_solve_backward's
    for f in ("X", "U", "gX", "gU", "g_w", "status"):
        refused(tgt, b"NULL", **{f: None})
    refused(tgt, b"NULL", spec=None)
    refused(tgt, b"NULL", cost=None)
    refused(tgt, b"batch", B=0)
    h0 = p.to_c()
    h0.horizon = 0
    refused(tgt, b"horizon", spec=h0)
    for f in ("Xref", "Uref", "g_xref", "g_uref"):
        refused(tgt, b"tracking cost", **{f: 1})
    refused(trk, b"g_target", g_target=1)
    refused(trk, b"Xref", Xref=None)
    refused(trk, b"Xref", Uref=None)
    refused(tgt, b"f32 only", dtype=_abi.F64)
    refused(tgt, b"smooth-min", spec=dataclasses.replace(p, obs_aggregation="min").to_c())
    refused(tgt, b"inverse barrier", spec=dataclasses.replace(p, barrier_type="log").to_c())
    tight = p.to_c()
    tight.h_offset = 0.05
    refused(tgt, b"h_offset", spec=tight)
    refused(tgt, b"wrapped", cost=dataclasses.replace(c, wrap_angle=True).to_c())


def test_wrt_truth_table():
    """What ``wrt`` lets through reaches the device check ("no CPU fallback": these are host tensors); what it does
    not is refused with the default call's messages."""
    import torch

    from diff_tube_mpc_strict_pt.core import diff_ilqr_solve

    st = _setup()
    p = st.problem
    B, N, M = 2, p.horizon, len(p.obstacles)
    V = torch.zeros(B, N, 2)
    w = dict(Q=torch.ones(3), R=torch.ones(2), Qf=torch.ones(3), qb=torch.tensor(1.0), target=torch.zeros(3))
    x0g = lambda: torch.zeros(B, 4, requires_grad=True)  # noqa: E731
    obg = lambda *s: torch.ones(*s, M, 3, requires_grad=True)  # noqa: E731

    def solve(**kw):
        kw.setdefault("x0", torch.zeros(B, 4))
        kw.setdefault("V_init", V)
        return diff_ilqr_solve(problem=p, cfg=st.ilqr_nom, kind="target", **w, **kw)

    # the default still refuses, and naming one input does not admit the other
    for kw in (dict(x0=x0g()), dict(x0=x0g(), wrt=()), dict(x0=x0g(), wrt=("obstacles",), obstacles=obg(B))):
        with pytest.raises(ValueError, match="x0 or V_init"):
            solve(**kw)
    for kw in (dict(obstacles=obg(B)), dict(obstacles=obg(B), wrt=("x0",))):
        with pytest.raises(ValueError, match="obstacle geometry"):
            solve(**kw)
    # admitted: the next refusal is the device's
    for kw in (dict(x0=x0g(), wrt=("x0",)), dict(x0=x0g(), wrt=["x0", "obstacles"], obstacles=obg(B)),
               dict(obstacles=obg(B), wrt=("obstacles",)), dict(obstacles=obg(), wrt=("obstacles",)),
               dict(wrt=("x0",)), dict(obstacles=obg(B).detach(), wrt=("obstacles",))):
        with pytest.raises(ValueError, match="no CPU fallback"):
            solve(**kw)
    # V_init and the DBaS parameters stay refused whatever wrt says
    with pytest.raises(ValueError, match="V_init"):
        solve(x0=x0g(), V_init=V.clone().requires_grad_(True), wrt=("x0",))
    with pytest.raises(ValueError, match="V_init"):
        solve(V_init=V.clone().requires_grad_(True), wrt=("obstacles",), obstacles=obg(B))
    with pytest.raises(ValueError, match="ift_gradient"):
        diff_ilqr_solve(problem=dataclasses.replace(p, dbas_gamma=torch.tensor(0.1)), cfg=st.ilqr_nom, kind="target",
                        x0=x0g(), V_init=V, wrt=("x0",), **w)
    # wrt itself
    for bad in (("V_init",), ("x0", "alpha"), "x0"):
        with pytest.raises(ValueError, match="wrt"):
            solve(wrt=bad)
    with pytest.raises(ValueError, match="obstacles as a tensor"):
        solve(wrt=("obstacles",))
