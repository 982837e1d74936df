"""The differentiable solve, host side (no device): the entry points beside ABI 8, the
dtmpc_solve_backward_supported truth table, dtmpc_solve_backward's argument validation before any device call, and
the Python refusals that need no device."""
from __future__ import annotations

import ctypes as C
import dataclasses

import pytest


@pytest.fixture(scope="module")
def lib():
    from diff_tube_mpc_strict_pt import _lib

    return _lib.load()


def _setup():
    from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config

    return paper_setup_from_config(paper_config())


def test_layer_entry_points_are_exported_beside_abi_8(lib):
    from diff_tube_mpc_strict_pt import _abi

    assert _abi.ABI_VERSION == 8 and lib.dtmpc_abi_version() == 8
    for name in ("dtmpc_solve_backward_supported", "dtmpc_solve_backward_workspace_bytes", "dtmpc_solve_backward"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
    from diff_tube_mpc_strict_pt import core

    for name in ("SolveGradient", "solve_backward", "diff_ilqr_solve"):
        assert hasattr(core, name) and name in core.__all__, name


def test_solve_backward_supported_truth_table(lib):
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core.problem import CircleObstacle

    st = _setup()
    p, c = st.problem, st.nominal_cost
    nine = tuple(CircleObstacle(center=(20.0 + 3 * j, 20.0), radius=1.0) for j in range(9))
    tight = p.to_c()
    tight.h_offset = 0.05
    cases = [
        ("f32 paper", _abi.F32, p.to_c(), c.to_c(), 1),
        ("f64", _abi.F64, p.to_c(), c.to_c(), 0),
        ("min aggregation", _abi.F32, dataclasses.replace(p, obs_aggregation="min").to_c(), c.to_c(), 0),
        ("log barrier", _abi.F32, dataclasses.replace(p, barrier_type="log").to_c(), c.to_c(), 0),
        ("nine obstacles", _abi.F32, dataclasses.replace(p, obstacles=nine).to_c(), c.to_c(), 0),
        ("h_offset", _abi.F32, tight, c.to_c(), 0),
        ("wrapped cost", _abi.F32, p.to_c(), dataclasses.replace(c, wrap_angle=True).to_c(), 0),
        ("gamma 0.3", _abi.F32, dataclasses.replace(p, dbas_gamma=0.3).to_c(), c.to_c(), 1),
        ("eight obstacles", _abi.F32, dataclasses.replace(p, obstacles=nine[:8]).to_c(), c.to_c(), 1),
        ("one obstacle", _abi.F32, dataclasses.replace(p, obstacles=nine[:1]).to_c(), c.to_c(), 1),
        ("tracking cost", _abi.F32, p.to_c(), dataclasses.replace(c, kind="track").to_c(), 1),
    ]
    for name, dtype, sp, cc, want in cases:
        assert lib.dtmpc_solve_backward_supported(dtype, C.byref(sp), C.byref(cc)) == want, name
    assert lib.dtmpc_solve_backward_supported(_abi.F32, None, None) == 0


def test_solve_backward_workspace_bytes(lib):
    from diff_tube_mpc_strict_pt import _abi

    # K (8), k_ff (2), nine Jacobian entries and the active mask: 20 f32 values per step and trajectory
    assert lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, 50, 65536) == 50 * 80 * 65536
    assert lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, 1, 1) == 80
    assert lib.dtmpc_solve_backward_workspace_bytes(_abi.F64, 50, 4) == 0
    assert lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, 0, 4) == 0
    assert lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, 50, 0) == 0


def test_solve_backward_refuses_before_any_device_call(lib):
    """Every BAD_ARG condition of include/dtmpc.h, with fake (never dereferenced) pointers: no device is needed."""
    from diff_tube_mpc_strict_pt import _abi

    st = _setup()
    p, c = st.problem, st.nominal_cost
    B, N = 8, p.horizon
    wb = lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, N, B)
    tgt = dict(dtype=_abi.F32, spec=p.to_c(), cost=c.to_c(), B=B, X=1, U=1, Xref=None, Uref=None, scenes=None, gX=1,
               gU=1, g_w=1, g_target=1, g_xref=None, g_uref=None, work=1, work_bytes=wb, status=1)
    trk = dict(tgt, cost=dataclasses.replace(c, kind="track").to_c(), Xref=1, Uref=1, g_target=None, g_xref=1,
               g_uref=1)

    def call(base, **over):
        a = dict(base, **over)
        sp, cc = a["spec"], a["cost"]
        return lib.dtmpc_solve_backward(a["dtype"], None if sp is None else C.byref(sp),
                                        None if cc is None else C.byref(cc), a["B"], a["X"], a["U"], a["Xref"],
                                        a["Uref"], a["scenes"], a["gX"], a["gU"], a["g_w"], a["g_target"],
                                        a["g_xref"], a["g_uref"], a["work"], a["work_bytes"], a["status"], None)

    def refused(base, word, **over):
        rc = call(base, **over)
        assert rc == _abi.ERR_BAD_ARG, (over, rc)
        assert word in lib.dtmpc_last_error(), (over, lib.dtmpc_last_error())

    for f in ("X", "U", "gX", "gU", "g_w", "status"):
        refused(tgt, b"NULL", **{f: None})
    refused(tgt, b"NULL", spec=None)
    refused(tgt, b"NULL", cost=None)
    refused(tgt, b"work_bytes", work=None)
    refused(tgt, b"batch", B=0)
    h0 = p.to_c()
    h0.horizon = 0
    refused(tgt, b"horizon", spec=h0)
    refused(tgt, b"work_bytes", work_bytes=wb - 1)
    for f in ("Xref", "Uref", "g_xref", "g_uref"):
        refused(tgt, b"tracking cost", **{f: 1})
    refused(trk, b"g_target", g_target=1)
    refused(trk, b"Xref", Xref=None)
    refused(trk, b"Xref", Uref=None)
    # unsupported configurations: never a silent fallback inside the library
    refused(tgt, b"f32 only", dtype=_abi.F64)
    refused(tgt, b"smooth-min", spec=dataclasses.replace(p, obs_aggregation="min").to_c())
    refused(tgt, b"inverse barrier", spec=dataclasses.replace(p, barrier_type="log").to_c())
    tight = p.to_c()
    tight.h_offset = 0.05
    refused(tgt, b"h_offset", spec=tight)
    refused(tgt, b"wrapped", cost=dataclasses.replace(c, wrap_angle=True).to_c())


def test_python_refusals():
    """Host tensors (there is no CPU path), gradients w.r.t. x0 / V_init, and a wrapped cost."""
    import torch

    from diff_tube_mpc_strict_pt.core import QuadraticCost, diff_ilqr_solve, solve_backward

    st = _setup()
    p = st.problem
    B, N = 2, p.horizon
    X, V = torch.zeros(B, N + 1, 4), torch.zeros(B, N, 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        solve_backward(problem=p, cost=st.nominal_cost, X=X, V=V, grad_X=X, grad_V=V)
    with pytest.raises(ValueError, match="wrap_angle"):
        solve_backward(problem=p, cost=dataclasses.replace(st.nominal_cost, wrap_angle=True), X=X, V=V, grad_X=X,
                       grad_V=V)
    w = dict(Q=torch.ones(3), R=torch.ones(2), Qf=torch.ones(3), qb=torch.tensor(1.0), target=torch.zeros(3))
    with pytest.raises(ValueError, match="x0 or V_init"):
        diff_ilqr_solve(problem=p, cfg=st.ilqr_nom, kind="target", x0=torch.zeros(B, 4, requires_grad=True),
                        V_init=V, **w)
    with pytest.raises(ValueError, match="x0 or V_init"):
        diff_ilqr_solve(problem=p, cfg=st.ilqr_nom, kind="target", x0=torch.zeros(B, 4),
                        V_init=V.clone().requires_grad_(True), **w)
    with pytest.raises(ValueError, match="obstacle geometry"):
        diff_ilqr_solve(problem=p, cfg=st.ilqr_nom, kind="target", x0=torch.zeros(B, 4), V_init=V,
                        obstacles=torch.ones(B, 5, 3, requires_grad=True), **w)
    with pytest.raises(ValueError, match="no CPU fallback"):
        diff_ilqr_solve(problem=p, cfg=st.ilqr_nom, kind="target", x0=torch.zeros(B, 4), V_init=V, **w)
    assert QuadraticCost().wrap_angle is False
