"""Per-trajectory cost weights, host side (no device): the four exports beside ABI 8, problem.pack_weights /
check_weights, every DTMPC_ERR_BAD_ARG path of the two new entries before any device call, the
dtmpc_weights_supported truth table (dtmpc_scenes_supported's) and diff_ilqr_solve's shape rules."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from _weights import W, assignment, cost_of, nine_of, weight_sets

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dtmpc.h")
NEW = ("dtmpc_weights_supported", "dtmpc_ilqr_solve_weights", "dtmpc_solve_backward_weights_workspace_bytes",
       "dtmpc_solve_backward_weights")


@pytest.fixture(scope="module")
def lib():
    from diff_tube_mpc_strict_pt import _lib

    return _lib.load()


def _setup():
    from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config

    return paper_setup_from_config(paper_config())


def _decl(name):
    """(return type, [parameter types]) of a function declared in include/dtmpc.h, whitespace-normalised."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"([A-Za-z_0-9]+\s*\*?)\s*\b%s\s*\(([^;]*?)\)\s*;" % name, text)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(2).split(",")]
    return m.group(1).strip(), [re.sub(r"\s*[A-Za-z_0-9]+$", "", p).strip() for p in params]


def test_the_four_exports_exist_with_the_stated_signatures(lib):
    from diff_tube_mpc_strict_pt import _abi

    assert _abi.ABI_VERSION == 8 and lib.dtmpc_abi_version() == 8  # beside ABI 8: the version stays
    for name in NEW:
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
    # the solve: dtmpc_ilqr_solve_scenes' arguments with `weights` between scenes and stream
    rs, ps = _decl("dtmpc_ilqr_solve_scenes")
    rw, pw = _decl("dtmpc_ilqr_solve_weights")
    assert rw == rs == "int" and pw == ps[:-1] + ["const void*", "void*"] and ps[-2:] == ["const void*", "void*"]
    a_s, a_w = _abi.PROTOTYPES["dtmpc_ilqr_solve_scenes"][1], _abi.PROTOTYPES["dtmpc_ilqr_solve_weights"][1]
    assert a_w == a_s[:-1] + [C.c_void_p, C.c_void_p]
    # supported: dtmpc_scenes_supported's
    assert _decl("dtmpc_weights_supported") == _decl("dtmpc_scenes_supported")
    assert _abi.PROTOTYPES["dtmpc_weights_supported"] == _abi.PROTOTYPES["dtmpc_scenes_supported"]
    # the backward: dtmpc_solve_backward_geom's arguments with `weights` after scenes
    rg, pg = _decl("dtmpc_solve_backward_geom")
    rb, pb = _decl("dtmpc_solve_backward_weights")
    assert rb == rg == "int" and pb == pg[:9] + ["const void*"] + pg[9:]
    a_g, a_b = _abi.PROTOTYPES["dtmpc_solve_backward_geom"][1], _abi.PROTOTYPES["dtmpc_solve_backward_weights"][1]
    assert a_b == a_g[:9] + [C.c_void_p] + a_g[9:]
    assert _decl("dtmpc_solve_backward_weights_workspace_bytes") == ("size_t", ["int", "int32_t", "int64_t", "int32_t"])
    assert _abi.PROTOTYPES["dtmpc_solve_backward_weights_workspace_bytes"] == \
        (C.c_size_t, [C.c_int, C.c_int32, C.c_int64, C.c_int32])


def test_workspace_bytes_are_the_plain_or_the_geom_record(lib):
    from diff_tube_mpc_strict_pt import _abi

    f = lib.dtmpc_solve_backward_weights_workspace_bytes
    for N, B in ((1, 1), (3, 65), (50, 257)):
        assert f(_abi.F32, N, B, 0) == lib.dtmpc_solve_backward_workspace_bytes(_abi.F32, N, B) == N * 80 * B
        assert f(_abi.F32, N, B, 1) == lib.dtmpc_solve_backward_geom_workspace_bytes(_abi.F32, N, B) == N * 100 * B
    assert f(_abi.F64, 50, 8, 0) == 0 and f(_abi.F32, 0, 8, 0) == 0 and f(_abi.F32, 50, 0, 1) == 0


def test_pack_weights_layout_and_check_weights():
    from diff_tube_mpc_strict_pt.core import pack_weights
    from diff_tube_mpc_strict_pt.core.problem import check_weights

    sets = weight_sets(_setup().nominal_cost)
    assert sets.shape == (W, 9) and np.array_equal(sets[0], nine_of(_setup().nominal_cost))
    assert (sets[:, 2] == 0).all()  # the paper's zero heading weight stays zero
    B = 7
    w = sets[assignment(B)]
    t = pack_weights(w[:, 0:3], w[:, 3:5], w[:, 5:8], w[:, 8], device="cpu")
    assert t.shape == (9, B) and t.dtype == torch.float32 and t.is_contiguous()
    assert np.array_equal(t.numpy(), w.T.astype(np.float32))  # row by row, each value rounded to f32 once
    flat = t.numpy().reshape(-1)
    assert flat[3 * B + 2] == np.float32(w[2, 3])  # element (row, i) at row * B + i
    t2 = pack_weights(torch.as_tensor(w[:, 0:3]), torch.as_tensor(w[:, 3:5]), torch.as_tensor(w[:, 5:8]),
                      torch.as_tensor(w[:, 8]))
    assert torch.equal(t, t2)
    with pytest.raises(ValueError, match=r"Q must be \[B, 3\]"):
        pack_weights(w[:, 0:2], w[:, 3:5], w[:, 5:8], w[:, 8])
    with pytest.raises(ValueError, match="R must be"):
        pack_weights(w[:, 0:3], w[:-1, 3:5], w[:, 5:8], w[:, 8])
    with pytest.raises(ValueError, match="R must be"):
        pack_weights(w[:, 0:3], w[:, 3:5], w[:, 5:8], w[:, 8:9])
    bad = w.copy()
    bad[3, 6] = np.nan
    with pytest.raises(ValueError, match="finite"):
        pack_weights(bad[:, 0:3], bad[:, 3:5], bad[:, 5:8], bad[:, 8])
    cpu = torch.device("cpu")
    check_weights(t, B, cpu)
    with pytest.raises(ValueError, match=r"\[9, 8\]"):
        check_weights(t, B + 1, cpu)
    with pytest.raises(ValueError, match=r"\[9, 7\]"):
        check_weights(t[:8], B, cpu)
    with pytest.raises(ValueError, match="float32"):
        check_weights(t.double(), B, cpu)
    with pytest.raises(ValueError, match="must live on"):
        check_weights(t, B, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="contiguous"):
        check_weights(t.t().contiguous().t(), B, cpu)
    n = t.clone()
    n[4, 2] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        check_weights(n, B, cpu)
    n[4, 2] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        check_weights(n, B, cpu)


def test_weights_supported_has_the_truth_table_of_scenes_supported(lib, monkeypatch):
    from diff_tube_mpc_strict_pt import _abi
    from diff_tube_mpc_strict_pt.core.problem import CircleObstacle, ILQRConfig

    monkeypatch.delenv("DTMPC_FAST", raising=False)
    st = _setup()
    p = st.problem
    nine = tuple(CircleObstacle(center=(20.0 + 3 * j, 20.0), radius=1.0) for j in range(9))
    cfgs = [st.ilqr_nom, ILQRConfig(horizon=50, line_search_alphas=(1.0, 0.5, 0.25, 0.1)),
            ILQRConfig(horizon=50, line_search_alphas=(1.0, 0.5, 0.25, 0.1, 0.05, 0.01)),
            ILQRConfig(horizon=50, line_search_alphas=(1.0, 0.5, 0.25, 0.1, 0.05, 0.01, 0.0, 0.0))]
    probs = [p, dataclasses.replace(p, obs_aggregation="min"), dataclasses.replace(p, obstacles=nine),
             dataclasses.replace(p, obstacles=nine[:8]), dataclasses.replace(p, obstacles=nine[:1]),
             dataclasses.replace(p, obstacles=()), dataclasses.replace(p, dbas_gamma=0.3),
             dataclasses.replace(p, barrier_type="log")]
    specs = [q.to_c() for q in probs]
    tight = p.to_c()
    tight.h_offset = 0.1
    specs.append(tight)
    seen = set()
    for fast in (None, "0"):
        if fast is not None:
            monkeypatch.setenv("DTMPC_FAST", fast)
        for dtype in (_abi.F32, _abi.F64):
            for sp in specs:
                for cf in cfgs:
                    ic = cf.to_c()
                    got = lib.dtmpc_weights_supported(dtype, C.byref(sp), C.byref(ic))
                    assert got == lib.dtmpc_scenes_supported(dtype, C.byref(sp), C.byref(ic))
                    seen.add(got)
    assert seen == {0, 1}
    monkeypatch.delenv("DTMPC_FAST", raising=False)
    ic, sp = st.ilqr_nom.to_c(), p.to_c()
    assert lib.dtmpc_weights_supported(_abi.F32, C.byref(sp), C.byref(ic)) == 1
    assert lib.dtmpc_weights_supported(_abi.F32, None, C.byref(ic)) == 0
    assert lib.dtmpc_weights_supported(_abi.F32, C.byref(sp), None) == 0


def test_solve_weights_bad_arguments_return_before_any_device_call(lib, monkeypatch):
    """Never the shared weights in place of the array.  (No device here: a call that reached one would not return
    DTMPC_ERR_BAD_ARG with these messages.)"""
    from diff_tube_mpc_strict_pt import _abi

    monkeypatch.delenv("DTMPC_FAST", raising=False)
    st = _setup()
    spec, cost, ic = st.problem.to_c(), st.nominal_cost.to_c(), st.ilqr_nom.to_c()

    def solve(dtype, sp, weights=1, scenes=None, lanes=1, cst=cost, x0=1, B=4):
        return lib.dtmpc_ilqr_solve_weights(dtype, C.byref(sp), C.byref(cst), C.byref(ic), B, x0, None, None, 1, 1, 1,
                                            1, None, 1, None, None, lanes, None, 0, scenes, weights, None)

    bad = _abi.ERR_BAD_ARG
    assert solve(_abi.F64, spec) == bad and b"f32" in lib.dtmpc_last_error()
    gam = st.problem.to_c()
    gam.dbas_gamma = 0.3
    assert solve(_abi.F32, gam) == bad and b"gamma" in lib.dtmpc_last_error()
    mn = st.problem.to_c()
    mn.obs_aggregation = _abi.OBS_MIN
    assert solve(_abi.F32, mn) == bad and b"smooth-min" in lib.dtmpc_last_error()
    wrap = st.nominal_cost.to_c()
    wrap.wrap_angle = 1
    assert solve(_abi.F32, spec, cst=wrap) == bad and b"wrap" in lib.dtmpc_last_error()
    assert solve(_abi.F32, spec, lanes=3) == bad and b"lanes" in lib.dtmpc_last_error()
    assert solve(_abi.F32, spec, x0=None) == bad and b"NULL" in lib.dtmpc_last_error()
    assert solve(_abi.F32, spec, B=0) == bad
    # a supported configuration reaches the launcher's own checks (no workspace here), with and without scenes
    assert solve(_abi.F32, spec) == bad and b"work_bytes" in lib.dtmpc_last_error()
    assert solve(_abi.F32, spec, scenes=1) == bad and b"work_bytes" in lib.dtmpc_last_error()
    # weights == NULL is dtmpc_ilqr_solve_scenes (and with scenes == NULL dtmpc_ilqr_solve_ws)
    assert solve(_abi.F64, spec, weights=None, scenes=1) == bad and b"scenes" in lib.dtmpc_last_error()
    assert solve(_abi.F32, spec, weights=None, lanes=3) == bad and b"lanes" in lib.dtmpc_last_error()
    monkeypatch.setenv("DTMPC_FAST", "0")
    assert solve(_abi.F32, spec) == bad and b"DTMPC_FAST" in lib.dtmpc_last_error()


def test_solve_backward_weights_bad_arguments_return_before_any_device_call(lib):
    from diff_tube_mpc_strict_pt import _abi

    st = _setup()
    spec, cost = st.problem.to_c(), st.nominal_cost.to_c()
    track = dataclasses.replace(st.nominal_cost, kind="track").to_c()
    N, B = st.problem.horizon, 4
    plain = lib.dtmpc_solve_backward_weights_workspace_bytes(_abi.F32, N, B, 0)
    geom = lib.dtmpc_solve_backward_weights_workspace_bytes(_abi.F32, N, B, 1)

    def call(dtype=_abi.F32, sp=spec, cst=cost, B=B, X=1, Xref=None, Uref=None, weights=1, gX=1, gw=1, gt=None, gxr=None,
             gur=None, gx0=None, gob=None, work=1, wb=plain, status=1):
        return lib.dtmpc_solve_backward_weights(dtype, C.byref(sp) if sp is not None else None,
                                                C.byref(cst) if cst is not None else None, B, X, 1, Xref, Uref, None,
                                                weights, gX, 1, gw, gt, gxr, gur, gx0, gob, work, wb, status, None)

    bad = _abi.ERR_BAD_ARG
    assert call(weights=None) == bad and b"weights" in lib.dtmpc_last_error()
    assert call(dtype=_abi.F64) == bad and b"f32" in lib.dtmpc_last_error()
    assert call(sp=None) == bad and call(cst=None) == bad
    assert call(B=0) == bad and b"batch" in lib.dtmpc_last_error()
    for k in ("X", "gX", "gw", "status"):
        assert call(**{k: None}) == bad and b"NULL" in lib.dtmpc_last_error(), k
    mn = st.problem.to_c()
    mn.obs_aggregation = _abi.OBS_MIN
    assert call(sp=mn) == bad and b"smooth-min" in lib.dtmpc_last_error()
    lg = dataclasses.replace(st.problem, barrier_type="log").to_c()
    assert call(sp=lg) == bad and b"barrier" in lib.dtmpc_last_error()
    wrap = st.nominal_cost.to_c()
    wrap.wrap_angle = 1
    assert call(cst=wrap) == bad and b"wrapped" in lib.dtmpc_last_error()
    assert call(Xref=1, Uref=1) == bad and b"tracking cost" in lib.dtmpc_last_error()
    assert call(gxr=1) == bad and b"tracking cost" in lib.dtmpc_last_error()
    assert call(cst=track) == bad and b"Xref and Uref" in lib.dtmpc_last_error()
    assert call(cst=track, Xref=1, Uref=1, gt=1) == bad and b"g_target" in lib.dtmpc_last_error()
    # the workspace rule follows the record in use: the plain one without g_x0 / g_obs, the geom one with either
    assert call(work=None) == bad and b"work_bytes" in lib.dtmpc_last_error()
    assert call(wb=plain - 1) == bad and b"dtmpc_solve_backward_weights_workspace_bytes" in lib.dtmpc_last_error()
    for kw in (dict(gx0=1), dict(gob=1), dict(gx0=1, gob=1)):
        assert call(wb=plain, **kw) == bad and b"work_bytes" in lib.dtmpc_last_error(), kw
        assert call(wb=geom - 1, **kw) == bad and b"work_bytes" in lib.dtmpc_last_error(), kw
    # any dbas_gamma is supported by the backward: a gamma = 0.3 spec gets past the configuration checks
    gam = st.problem.to_c()
    gam.dbas_gamma = 0.3
    assert call(sp=gam, wb=plain - 1) == bad and b"work_bytes" in lib.dtmpc_last_error()


def test_python_entries_refuse_weights_where_they_are_not_honoured():
    """Before the device is needed: the closure form of ilqr_solve, and solve_backward's / ilqr_solve's checks."""
    from diff_tube_mpc_strict_pt.core import ilqr_solve

    st = _setup()
    w = torch.ones(9, 4)
    with pytest.raises(TypeError, match="weights go with the typed form"):
        ilqr_solve(cfg=st.ilqr_nom, x0=torch.zeros(4, 4), V_init=torch.zeros(4, 50, 2), f=object(), weights=w)


def test_diff_ilqr_solve_shape_rules():
    """Each of Q, R, Qf [k] or [B, k], qb [] or [B]; anything else is refused by name.  The accepted forms get as far
    as the device check (there is none here), the shared form as before."""
    from diff_tube_mpc_strict_pt.core import diff_ilqr_solve

    st = _setup()
    B, N = 4, st.problem.horizon
    base = dict(problem=st.problem, cfg=st.ilqr_nom, kind="target", x0=torch.zeros(B, 4), V_init=torch.zeros(B, N, 2),
                target=torch.zeros(3))
    sh = dict(Q=torch.ones(3), R=torch.ones(2), Qf=torch.ones(3), qb=torch.tensor(0.5))
    pt = dict(Q=torch.ones(B, 3), R=torch.ones(B, 2), Qf=torch.ones(B, 3), qb=torch.ones(B))
    for k in ("Q", "R", "Qf", "qb"):  # one per trajectory, the others shared; and all four
        with pytest.raises(ValueError, match="no CPU fallback"):
            diff_ilqr_solve(**base, **{**sh, k: pt[k]})
    with pytest.raises(ValueError, match="no CPU fallback"):
        diff_ilqr_solve(**base, **pt)
    with pytest.raises(ValueError, match="no CPU fallback"):
        diff_ilqr_solve(**base, **sh)
    with pytest.raises(ValueError, match="shared weights"):
        diff_ilqr_solve(**base, **{**sh, "Q": torch.ones(4)})
    for k, t, word in (("Q", torch.ones(B + 1, 3), "Q must be"), ("Q", torch.ones(B, 2), "Q must be"),
                       ("R", torch.ones(B, 3), "R must be"), ("Qf", torch.ones(1, 3), "Qf must be"),
                       ("qb", torch.ones(B + 1), "qb must be"), ("Q", torch.ones(B, 3, 1), "Q must be")):
        with pytest.raises(ValueError, match=word):
            diff_ilqr_solve(**base, **{**pt, k: t})
    with pytest.raises(ValueError, match="R must be"):
        diff_ilqr_solve(**base, **{**sh, "Q": pt["Q"], "R": torch.ones(3)})


def test_weight_sets_keep_the_cost_kind_and_target():
    st = _setup()
    sets = weight_sets(st.nominal_cost)
    c = cost_of(st.nominal_cost, sets[3])
    assert c.kind == st.nominal_cost.kind and c.target == st.nominal_cost.target
    assert np.array_equal(nine_of(c), sets[3]) and not np.array_equal(sets[3], sets[0])
    f = sets[1:, [0, 1, 3, 4, 5, 6, 7, 8]] / sets[0, [0, 1, 3, 4, 5, 6, 7, 8]]
    assert (f >= 0.5).all() and (f <= 2.0).all()
    tied = weight_sets(dataclasses.replace(st.nominal_cost, kind="track"), tied_terminal=True)
    assert np.array_equal(tied[1:, 5:8], tied[1:, 0:3])
