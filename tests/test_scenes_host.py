"""Per-trajectory scenes, host side (no device): ABI 8, the new struct field, the dtmpc_scenes_supported truth table,
argument validation before any device call, and problem.pack_scenes."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest
import torch

from _scenes import scene_table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dtmpc.h")


@pytest.fixture(scope="module")
def lib():
    from diff_tube_mpc_strict_pt import _lib

    return _lib.load()


def _setup():
    from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config

    return paper_setup_from_config(paper_config())


def test_abi_8_exports_the_scene_entry_points(lib):
    from diff_tube_mpc_strict_pt import _abi

    assert _abi.ABI_VERSION == 8 and lib.dtmpc_abi_version() == 8
    for name in ("dtmpc_scenes_supported", "dtmpc_ilqr_solve_scenes", "dtmpc_dbas_init_scenes"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name


def test_tube_state_scenes_field_matches_header(tmp_path):
    """tests/test_abi_host.py's mirror pattern on the new last field: offset and struct size from gcc."""
    from diff_tube_mpc_strict_pt import _abi

    py = _abi.DtmpcTubeState
    assert py._fields_[-1] == ("scenes", C.c_void_p) and py._fields_[-2][0] == "costs"
    src = tmp_path / "layout.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
        'printf("%zu %zu %zu %d\\n", sizeof(dtmpc_tube_state), offsetof(dtmpc_tube_state, scenes),',
        "       offsetof(dtmpc_tube_state, costs), DTMPC_ABI_VERSION);", "return 0;}"]))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    size, off, off_costs, abi = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                  check=True).stdout.split())
    assert (size, off, off_costs, abi) == (C.sizeof(py), py.scenes.offset, py.costs.offset, 8)
    assert off == off_costs + 8 and size == off + 8  # appended: every ABI 7 field keeps its place
    assert _abi.DtmpcTubeState().scenes is None  # NULL by default: the shared spec


def test_scenes_supported_truth_table(lib, monkeypatch):
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core.problem import CircleObstacle, ILQRConfig

    monkeypatch.delenv("DTMPC_FAST", raising=False)
    st = _setup()
    ic = st.ilqr_nom.to_c()

    def ok(dtype, problem, cfg=ic):
        sp = problem.to_c()
        return lib.dtmpc_scenes_supported(dtype, C.byref(sp), C.byref(cfg))

    p = st.problem
    assert ok(_abi.F32, p) == 1
    assert ok(_abi.F64, p) == 0
    assert ok(_abi.F32, dataclasses.replace(p, obs_aggregation="min")) == 0
    nine = tuple(CircleObstacle(center=(20.0 + 3 * j, 20.0), radius=1.0) for j in range(9))
    assert ok(_abi.F32, dataclasses.replace(p, obstacles=nine)) == 0
    assert ok(_abi.F32, dataclasses.replace(p, obstacles=nine[:8])) == 1
    assert ok(_abi.F32, dataclasses.replace(p, obstacles=nine[:1])) == 1
    assert ok(_abi.F32, dataclasses.replace(p, obstacles=())) == 0
    assert ok(_abi.F32, dataclasses.replace(p, dbas_gamma=0.3)) == 0
    assert ok(_abi.F32, dataclasses.replace(p, barrier_type="log")) == 0
    four = ILQRConfig(horizon=50, line_search_alphas=(1.0, 0.5, 0.25, 0.1)).to_c()
    assert ok(_abi.F32, p, four) == 0
    six = ILQRConfig(horizon=50, line_search_alphas=(1.0, 0.5, 0.25, 0.1, 0.05, 0.01)).to_c()
    assert ok(_abi.F32, p, six) == 1
    two_zeros = ILQRConfig(horizon=50, line_search_alphas=(1.0, 0.5, 0.25, 0.1, 0.05, 0.01, 0.0, 0.0)).to_c()
    assert ok(_abi.F32, p, two_zeros) == 0
    tight = p.to_c()
    tight.h_offset = 0.1
    assert lib.dtmpc_scenes_supported(_abi.F32, C.byref(tight), C.byref(ic)) == 0
    monkeypatch.setenv("DTMPC_FAST", "0")
    assert ok(_abi.F32, p) == 0


def test_scenes_on_an_unsupported_configuration_is_a_bad_argument(lib, monkeypatch):
    """Before any device call: a scenes pointer never falls back to the shared table."""
    from diff_tube_mpc_strict_pt import _abi

    monkeypatch.delenv("DTMPC_FAST", raising=False)
    st = _setup()
    spec, cost, ic = st.problem.to_c(), st.nominal_cost.to_c(), st.ilqr_nom.to_c()

    def solve(dtype, sp, scenes=1, lanes=1, cst=cost):
        return lib.dtmpc_ilqr_solve_scenes(dtype, C.byref(sp), C.byref(cst), C.byref(ic), 4, 1, None, None, 1, 1, 1, 1,
                                           None, 1, None, None, lanes, None, 0, scenes, None)

    assert solve(_abi.F64, spec) == _abi.ERR_BAD_ARG and b"f32" in lib.dtmpc_last_error()
    gam = st.problem.to_c()
    gam.dbas_gamma = 0.3
    assert solve(_abi.F32, gam) == _abi.ERR_BAD_ARG and b"gamma" in lib.dtmpc_last_error()
    mn = st.problem.to_c()
    mn.obs_aggregation = _abi.OBS_MIN
    assert solve(_abi.F32, mn) == _abi.ERR_BAD_ARG and b"smooth-min" in lib.dtmpc_last_error()
    wrap = st.nominal_cost.to_c()
    wrap.wrap_angle = 1
    assert solve(_abi.F32, spec, cst=wrap) == _abi.ERR_BAD_ARG and b"wrap" in lib.dtmpc_last_error()
    # a supported configuration reaches the launcher's own checks (no workspace here)
    assert solve(_abi.F32, spec) == _abi.ERR_BAD_ARG and b"work_bytes" in lib.dtmpc_last_error()
    # scenes == NULL is dtmpc_ilqr_solve_ws
    assert solve(_abi.F32, spec, scenes=None, lanes=3) == _abi.ERR_BAD_ARG and b"lanes" in lib.dtmpc_last_error()
    assert lib.dtmpc_dbas_init_scenes(_abi.F32, C.byref(spec), 4, 1, None, 1, None) == _abi.ERR_BAD_ARG
    # the tube step: state->scenes on f64 / gamma != 0
    tc = _abi.DtmpcTubeCfg()
    tc.nominal, tc.nom_ilqr, tc.aux_ilqr = cost, st.ilqr_nom.to_c(), st.ilqr_aux.to_c()
    tc.disturbance = 1
    state = _abi.DtmpcTubeState()
    for f in ("x", "b", "xbar", "bbar", "Xnom", "Unom", "Xaux", "Uaux", "work", "theta", "partials", "status", "scenes"):
        setattr(state, f, 1)
    state.lanes = 1
    state.chunk = lib.dtmpc_tube_chunk(50, 1)
    state.n_partials = lib.dtmpc_tube_partials_count(8, 1)
    for dtype, sp, word in ((_abi.F64, spec, b"f32"), (_abi.F32, gam, b"gamma")):
        state.work_bytes = lib.dtmpc_tube_workspace_bytes(dtype, 50, 8, 1, state.chunk)
        rc = lib.dtmpc_tube_step(dtype, C.byref(sp), C.byref(tc), 8, 0, 0, C.byref(state), None, None)
        assert rc == _abi.ERR_BAD_ARG and word in lib.dtmpc_last_error(), lib.dtmpc_last_error()


def test_pack_scenes_layout_and_errors():
    from diff_tube_mpc_strict_pt.core import pack_scenes

    p = _setup().problem
    obs, tgs = scene_table(5)
    B = 7
    k = np.arange(B) % len(obs)
    sc = pack_scenes(p, obs[k], tgs[k], dtype=torch.float32, device="cpu")
    assert sc.shape == (3 * 5 + 3, B) and sc.dtype == torch.float32 and sc.is_contiguous()
    a = sc.numpy()
    assert np.array_equal(a[0:5], obs[k][:, :, 0].T.astype(np.float32))
    assert np.array_equal(a[5:10], obs[k][:, :, 1].T.astype(np.float32))
    r = obs[k][:, :, 2].T
    assert np.array_equal(a[10:15], np.float32(np.float64(r) * np.float64(r)))
    assert np.array_equal(a[15:18], tgs[k].T.astype(np.float32))
    # r2 is the rounded float64 product, not the product of the rounded radius (they differ for these radii)
    assert not np.array_equal(a[10:15], np.float32(r) * np.float32(r))
    d = pack_scenes(p, obs[k], tgs[k], dtype=torch.float64, device="cpu")
    assert d.dtype == torch.float64 and np.array_equal(d.numpy()[10:15], r * r)
    assert pack_scenes(p, torch.as_tensor(obs[k]), torch.as_tensor(tgs[k])).dtype == torch.float32
    with pytest.raises(ValueError, match=r"\[B, M, 3\]"):
        pack_scenes(p, obs[k][:, :, :2], tgs[k])
    with pytest.raises(ValueError, match="circles per scene"):
        pack_scenes(p, obs[k][:, :4], tgs[k])
    with pytest.raises(ValueError, match="targets"):
        pack_scenes(p, obs[k], tgs[k][:-1])
    with pytest.raises(ValueError, match="targets"):
        pack_scenes(p, obs[k], tgs[k][:, :2])
    bad = obs[k].copy()
    bad[3, 2, 2] = 0.0
    with pytest.raises(ValueError, match="positive"):
        pack_scenes(p, bad, tgs[k])
    bad[3, 2, 2] = -1.0
    with pytest.raises(ValueError, match="positive"):
        pack_scenes(p, bad, tgs[k])
    with pytest.raises(ValueError, match="at least one obstacle"):
        pack_scenes(dataclasses.replace(p, obstacles=()), obs[k][:, :0], tgs[k])
