"""Own theta (per-trajectory ancillary weights), host side (no device): the new entry points beside ABI 8, the
dtmpc_own_theta struct's layout, the dtmpc_own_theta_supported truth table and dtmpc_tube_step_own's argument
validation before any device call."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dtmpc.h")


@pytest.fixture(scope="module")
def lib():
    from diff_tube_mpc_strict_pt import _lib

    return _lib.load()


def _setup():
    from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config

    return paper_setup_from_config(paper_config())


def _tube_cfg(st, ilqr=None):
    from diff_tube_mpc_strict_pt import _abi

    tc = _abi.DtmpcTubeCfg()
    tc.nominal = st.nominal_cost.to_c()
    tc.nom_ilqr = (ilqr or st.ilqr_nom).to_c()
    tc.aux_ilqr = (ilqr or st.ilqr_aux).to_c()
    tc.disturbance = 1
    return tc


def _cases(st):
    """(name, dtype, spec, tube cfg, supported) of the issue's truth table (DTMPC_FAST unset)."""
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core.problem import CircleObstacle, ILQRConfig

    p = st.problem
    nine = tuple(CircleObstacle(center=(20.0 + 3 * j, 20.0), radius=1.0) for j in range(9))
    four = ILQRConfig(horizon=50, line_search_alphas=(1.0, 0.5, 0.25, 0.1))
    tc = _tube_cfg(st)
    return [
        ("f32 paper", _abi.F32, p.to_c(), tc, 1),
        ("f64", _abi.F64, p.to_c(), tc, 0),
        ("gamma 0.3", _abi.F32, dataclasses.replace(p, dbas_gamma=0.3).to_c(), tc, 0),
        ("min aggregation", _abi.F32, dataclasses.replace(p, obs_aggregation="min").to_c(), tc, 0),
        ("log barrier", _abi.F32, dataclasses.replace(p, barrier_type="log").to_c(), tc, 0),
        ("nine obstacles", _abi.F32, dataclasses.replace(p, obstacles=nine).to_c(), tc, 0),
        ("eight obstacles", _abi.F32, dataclasses.replace(p, obstacles=nine[:8]).to_c(), tc, 1),
        ("one obstacle", _abi.F32, dataclasses.replace(p, obstacles=nine[:1]).to_c(), tc, 1),
        ("four alphas", _abi.F32, p.to_c(), _tube_cfg(st, four), 0),
    ]


def test_own_theta_entry_points_are_exported_beside_abi_8(lib):
    from diff_tube_mpc_strict_pt import _abi

    assert _abi.ABI_VERSION == 8 and lib.dtmpc_abi_version() == 8
    for name in ("dtmpc_own_theta_supported", "dtmpc_tube_step_own"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
    # the struct ABI 8 pinned is unchanged: scenes is still its last field
    assert _abi.DtmpcTubeState._fields_[-1] == ("scenes", C.c_void_p)


def test_own_theta_struct_matches_header(tmp_path):
    """tests/test_abi_host.py's mirror pattern: sizeof / offsetof from gcc against the ctypes mirror."""
    from diff_tube_mpc_strict_pt import _abi

    py = _abi.DtmpcOwnTheta
    names = [f for f, _ in py._fields_]
    assert names == ["theta", "vel", "adapt", "update", "pad"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("%zu %d\\n", sizeof(dtmpc_own_theta), DTMPC_ABI_VERSION);']
    lines += [f'printf("%zu\\n", offsetof(dtmpc_own_theta, {f}));' for f in names]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(py) and out[1] == 8
    assert out[2:] == [getattr(py, f).offset for f in names]
    assert C.sizeof(py) == 16 + C.sizeof(_abi.DtmpcAdaptCfg) + 8


def test_own_theta_supported_truth_table(lib, monkeypatch):
    from diff_tube_mpc_strict_pt import _abi

    monkeypatch.delenv("DTMPC_FAST", raising=False)
    st = _setup()
    cases = _cases(st)
    for name, dtype, sp, tc, want in cases:
        assert lib.dtmpc_own_theta_supported(dtype, C.byref(sp), C.byref(tc)) == want, name
    assert lib.dtmpc_own_theta_supported(_abi.F32, None, None) == 0
    monkeypatch.setenv("DTMPC_FAST", "0")
    name, dtype, sp, tc, _ = cases[0]
    assert lib.dtmpc_own_theta_supported(dtype, C.byref(sp), C.byref(tc)) == 0


def _state(lib, dtype, B=8, lanes=1):
    """A tube state of fake (never dereferenced) pointers that passes dtmpc_tube_step's own size checks."""
    from diff_tube_mpc_strict_pt import _abi

    state = _abi.DtmpcTubeState()
    for f in ("x", "b", "xbar", "bbar", "Xnom", "Unom", "Xaux", "Uaux", "work", "partials", "status"):
        setattr(state, f, 1)
    state.lanes = lanes
    state.chunk = lib.dtmpc_tube_chunk(50, lanes)
    state.n_partials = lib.dtmpc_tube_partials_count(B, lanes)
    state.work_bytes = lib.dtmpc_tube_workspace_bytes(dtype, 50, B, lanes, state.chunk)
    return state


def _own(st, theta=1, vel=1):
    from diff_tube_mpc_strict_pt import _abi

    own = _abi.DtmpcOwnTheta()
    own.theta, own.vel = theta, vel
    own.adapt = st.adapt.to_c()
    own.update = 1
    return own


def test_tube_step_own_refuses_before_any_device_call(lib, monkeypatch):
    """Every unsupported configuration, a NULL theta / vel and a split phase: DTMPC_ERR_BAD_ARG, never the shared
    theta (state->theta is NULL throughout: the own-theta step does not need it)."""
    from diff_tube_mpc_strict_pt import _abi

    monkeypatch.delenv("DTMPC_FAST", raising=False)
    st = _setup()
    own = _own(st)

    def step(dtype, sp, tc, own=own, phase=0):
        state = _state(lib, dtype)
        state.phase = phase
        return lib.dtmpc_tube_step_own(dtype, C.byref(sp), C.byref(tc), 8, 0, 0, C.byref(state), None, None,
                                       C.byref(own) if own is not None else None)

    cases = _cases(st)
    for name, dtype, sp, tc, want in cases:
        if not want:
            assert step(dtype, sp, tc) == _abi.ERR_BAD_ARG, name
            assert b"own theta" in lib.dtmpc_last_error(), (name, lib.dtmpc_last_error())
    _, dtype, sp, tc, _ = cases[0]
    monkeypatch.setenv("DTMPC_FAST", "0")
    assert step(dtype, sp, tc) == _abi.ERR_BAD_ARG and b"own theta" in lib.dtmpc_last_error()
    monkeypatch.delenv("DTMPC_FAST")
    assert step(dtype, sp, tc, own=_own(st, theta=None)) == _abi.ERR_BAD_ARG
    assert b"NULL theta or vel" in lib.dtmpc_last_error()
    assert step(dtype, sp, tc, own=_own(st, vel=None)) == _abi.ERR_BAD_ARG
    assert b"NULL theta or vel" in lib.dtmpc_last_error()
    assert step(dtype, sp, tc, own=None) == _abi.ERR_BAD_ARG and b"own theta" in lib.dtmpc_last_error()
    for phase in (1, 2):
        assert step(dtype, sp, tc, phase=phase) == _abi.ERR_BAD_ARG, phase
        assert b"phase" in lib.dtmpc_last_error() and b"own theta" in lib.dtmpc_last_error()
    # the shared entry point still needs state->theta
    state = _state(lib, dtype)
    assert lib.dtmpc_tube_step(dtype, C.byref(sp), C.byref(tc), 8, 0, 0, C.byref(state), None, None) == _abi.ERR_BAD_ARG
    assert b"NULL state array" in lib.dtmpc_last_error()


def test_python_refusals_name_the_support_query():
    """The constructor's argument checks that need no device object."""
    from diff_tube_mpc_strict_pt.core import TubeMPC

    with pytest.raises(ValueError, match="own_theta"):
        TubeMPC(_setup(), batch=4, device="cpu", own_theta=True, overlap=True)
    with pytest.raises(ValueError, match="theta0 goes with own_theta"):
        TubeMPC(_setup(), batch=4, device="cpu", theta0=[1.0] * 6)
