"""The differentiable solve's rows w.r.t. the DBaS parameters alpha and gamma, host side (no device): the two entry
points beside ABI 8 and their prototypes, the workspace size, dtmpc_solve_backward_dbas's argument validation before
any device call (fake pointers, never dereferenced), the Python defaults, and diff_ilqr_solve's refusals that need no
device."""
from __future__ import annotations

import ctypes as C
import dataclasses
import inspect
import os
import re

import pytest


@pytest.fixture(scope="module")
def lib():
    from diff_tube_mpc_strict_pt import _lib

    return _lib.load()


def _setup():
    from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config

    return paper_setup_from_config(paper_config())


def _decl(name):
    """(return type, [argument types]) of a prototype in include/dtmpc.h."""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtmpc.h")).read()
    m = re.search(r"^([\w ]+?)\s*\b%s\(([^;]*)\);" % name, hdr, re.M)
    assert m, name
    args = [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in m.group(2).replace("\n", " ").split(",")]
    return m.group(1).strip(), args


def test_dbas_entry_points_are_exported_beside_abi_8(lib):
    from diff_tube_mpc_strict_pt import _abi, core

    assert _abi.ABI_VERSION == 8 and lib.dtmpc_abi_version() == 8
    for name in ("dtmpc_solve_backward_dbas_workspace_bytes", "dtmpc_solve_backward_dbas"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
    # dtmpc_solve_backward_weights' arguments with one more pointer (g_dbas) after g_obs
    old, new = _abi.PROTOTYPES["dtmpc_solve_backward_weights"], _abi.PROTOTYPES["dtmpc_solve_backward_dbas"]
    assert new[0] is old[0] and len(new[1]) == len(old[1]) + 1
    assert new[1][:18] == old[1][:18] and new[1][18] is C.c_void_p and new[1][19:] == old[1][18:]
    rw, pw = _decl("dtmpc_solve_backward_weights")
    rd, pd = _decl("dtmpc_solve_backward_dbas")
    assert rd == rw == "int" and pd == pw[:18] + ["void*"] + pw[18:]
    assert len(pd) == len(new[1])
    assert _decl("dtmpc_solve_backward_dbas_workspace_bytes") == ("size_t", ["int", "int32_t", "int64_t"])
    assert _abi.PROTOTYPES["dtmpc_solve_backward_dbas_workspace_bytes"] == \
        _abi.PROTOTYPES["dtmpc_solve_backward_geom_workspace_bytes"]
    f = {x.name: x for x in dataclasses.fields(core.SolveGradient)}
    assert f["dbas"].default is None and list(f)[-2:] == ["x0", "obstacles"]  # (the geom fields stay the last two)
    assert inspect.signature(core.solve_backward).parameters["want_dbas"].default is False
    ds = inspect.signature(core.diff_ilqr_solve).parameters
    assert ds["dbas_alpha"].default is None and ds["dbas_gamma"].default is None


def test_dbas_workspace_bytes(lib):
    from diff_tube_mpc_strict_pt import _abi

    f = lib.dtmpc_solve_backward_dbas_workspace_bytes
    for N, B in ((50, 65536), (1, 1), (3, 257)):
        assert f(_abi.F32, N, B) == lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, N, B) == N * 100 * B
    assert f(_abi.F64, 50, 4) == 0
    assert f(_abi.F32, 0, 4) == 0
    assert f(_abi.F32, 50, 0) == 0


def test_dbas_refuses_before_any_device_call(lib):
    """Every BAD_ARG condition of dtmpc_solve_backward and the new entry's own (g_dbas NULL, work_bytes below its
    size), with fake pointers; weights, g_x0 and g_obs may each be NULL -- those calls get past the argument rules
    (they are not made here: they would reach the device)."""
    from diff_tube_mpc_strict_pt import _abi

    st = _setup()
    p, c = st.problem, st.nominal_cost
    B, N = 8, p.horizon
    wb = lib.dtmpc_solve_backward_dbas_workspace_bytes(_abi.F32, N, B)
    tgt = dict(dtype=_abi.F32, spec=p.to_c(), cost=c.to_c(), B=B, X=1, U=1, Xref=None, Uref=None, scenes=None,
               weights=None, gX=1, gU=1, g_w=1, g_target=1, g_xref=None, g_uref=None, g_x0=1, g_obs=1, g_dbas=1, work=1,
               work_bytes=wb, status=1)
    trk = dict(tgt, cost=dataclasses.replace(c, kind="track").to_c(), Xref=1, Uref=1, g_target=None, g_xref=1,
               g_uref=1)

    def call(base, **over):
        a = dict(base, **over)
        sp, cc = a["spec"], a["cost"]
        return lib.dtmpc_solve_backward_dbas(a["dtype"], None if sp is None else C.byref(sp),
                                             None if cc is None else C.byref(cc), a["B"], a["X"], a["U"], a["Xref"],
                                             a["Uref"], a["scenes"], a["weights"], a["gX"], a["gU"], a["g_w"],
                                             a["g_target"], a["g_xref"], a["g_uref"], a["g_x0"], a["g_obs"],
                                             a["g_dbas"], a["work"], a["work_bytes"], a["status"], None)

    def refused(base, word, **over):
        rc = call(base, **over)
        assert rc == _abi.ERR_BAD_ARG, (over, rc)
        assert word in lib.dtmpc_last_error(), (over, lib.dtmpc_last_error())

    # the new rules; they hold with and without weights, and whichever of g_x0 / g_obs is passed
    for base in (tgt, trk, dict(tgt, weights=1), dict(tgt, g_x0=None, g_obs=None), dict(trk, g_x0=None)):
        refused(base, b"g_dbas", g_dbas=None)
        refused(base, b"dtmpc_solve_backward_dbas_workspace_bytes", work_bytes=wb - 1)
        refused(base, b"dtmpc_solve_backward_dbas_workspace_bytes",
                work_bytes=lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, N, B))
        refused(base, b"work_bytes", work=None)
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
    # any dbas_gamma is supported: the refusal of a too small workspace is reached, not one of the configuration
    refused(tgt, b"work_bytes", spec=dataclasses.replace(p, dbas_gamma=0.3).to_c(), work_bytes=wb - 1)


def test_diff_ilqr_solve_dbas_refusals_without_a_device():
    import torch

    from diff_tube_mpc_strict_pt.core import diff_ilqr_solve

    st = _setup()
    p = st.problem
    B, N = 3, p.horizon
    w = dict(Q=torch.ones(3), R=torch.ones(2), Qf=torch.ones(3), qb=torch.tensor(1.0), target=torch.zeros(3))
    kw = dict(cfg=st.ilqr_nom, kind="target", x0=torch.zeros(B, 4), V_init=torch.zeros(B, N, 2), **w)
    # per-trajectory DBaS parameters are not built
    for name in ("dbas_alpha", "dbas_gamma"):
        for shape in ((B,), (B, 1), (2,)):
            with pytest.raises(ValueError, match="per-trajectory DBaS parameters are not built"):
                diff_ilqr_solve(problem=p, **kw, **{name: torch.full(shape, 0.1, requires_grad=True)})
        with pytest.raises(ValueError, match="zero-dim or one-element tensor"):
            diff_ilqr_solve(problem=p, **kw, **{name: 0.1})
    # problem.dbas_* as tensors stay refused, and the message names the new arguments
    for name in ("dbas_alpha", "dbas_gamma"):
        with pytest.raises(ValueError, match=f"argument {name}= of diff_ilqr_solve"):
            diff_ilqr_solve(problem=dataclasses.replace(p, **{name: torch.tensor(0.1)}), **kw)
    # eps and beta: no gradient
    for name in ("dbas_eps", "obs_beta"):
        with pytest.raises(ValueError, match="dbas_eps and obs_beta are not provided"):
            diff_ilqr_solve(problem=dataclasses.replace(p, **{name: torch.tensor(0.1)}), **kw)
    # a zero-dim or a one-element tensor is admitted: the next refusal is the device's (these are host tensors)
    for t in (torch.tensor(0.05, requires_grad=True), torch.tensor([0.05])):
        with pytest.raises(ValueError, match="no CPU fallback"):
            diff_ilqr_solve(problem=p, dbas_alpha=t, dbas_gamma=torch.tensor(0.2, requires_grad=True), **kw)
