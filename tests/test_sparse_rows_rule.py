"""CPU test of the host rule that selects the tube step's sparse-state-rows kernel (csrc/dtmpc_fast.hip tube_fast_xs,
through the diagnostics export dtmpc_diag_tube_sparse_rows, which returns the stride or 0 for dense rows): taken where the
sin / cos cache kernel is taken (tests/test_sincos_cache_rule.py) and both LDS tables fit a CU with 256 lanes on it,
N <= 52.  DTMPC_FAST_XROWS=dense keeps the sin / cos cache kernel with dense rows, DTMPC_FAST_SCC=0 the kernel without
either table; dtmpc_diag_tube_sincos_cache answers as before in every case."""
import ctypes as C

import pytest

F32, F64 = 0, 1
S, CAP = 5, 52


@pytest.fixture(scope="module")
def rule():
    from diff_tube_mpc_strict_pt import _lib

    lib = _lib.load()
    sig = [C.c_int, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_double]
    xs, scc = lib.dtmpc_diag_tube_sparse_rows, lib.dtmpc_diag_tube_sincos_cache
    xs.restype, xs.argtypes = C.c_int, sig
    scc.restype, scc.argtypes = C.c_int, sig
    # the lane slots the library sees (as tests/test_sincos_cache_rule.py finds them)
    lo, hi = 257, 1 << 24
    while lo < hi:
        mid = (lo + hi) // 2
        if lib.dtmpc_tube_partials_count(mid, 1) == (mid + 255) // 256:
            hi = mid
        else:
            lo = mid + 1
    return xs, scc, lo, int(lib.dtmpc_tube_chunk(50, 1))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("DTMPC_FAST_XROWS", "DTMPC_FAST_SCC", "DTMPC_FAST_G0"):
        monkeypatch.delenv(k, raising=False)


def test_rule_selects_sparse_rows(rule):
    xs, scc, slots, chunk = rule
    for B in (slots, slots - 1, 200, 1):  # 256-thread workgroups, 64-thread ones, a partial wave, one lane
        assert xs(F32, 50, B, chunk, 1, 0.0) == S and scc(F32, 50, B, chunk, 1, 0.0) == 1
    for N in (1, 2, 3, S - 1, S, S + 1, 2 * S + 1, CAP):
        assert xs(F32, N, 200, chunk, 1, 0.0) == S and scc(F32, N, 200, chunk, 1, 0.0) == 1
    assert xs(F32, 50, 2 * slots, slots, 1, 0.0) == S  # chunks that are launches that fit


def test_cap_is_the_lds_budget(rule):
    xs, scc, slots, chunk = rule
    lds = lambda N: (8 * N + 4 * (N + 1)) * 256 + 4 * 128  # both tables at 256 lanes, four workgroups' static sums
    assert lds(CAP) <= 160 * 1024 < lds(CAP + 1)
    for N in (CAP + 1, 60, 64):  # up to the sin / cos table's own cap: that kernel, dense rows
        assert xs(F32, N, 200, chunk, 1, 0.0) == 0 and scc(F32, N, 200, chunk, 1, 0.0) == 1
    assert xs(F32, 65, 200, chunk, 1, 0.0) == 0 and scc(F32, 65, 200, chunk, 1, 0.0) == 0


def test_rule_falls_back_with_the_sincos_cache(rule):
    xs, scc, slots, chunk = rule
    for args in ((F32, 50, slots + 1, chunk, 1, 0.0), (F32, 50, 2 * slots, chunk, 1, 0.0),  # the residency rule
                 (F32, 50, 200, chunk, 2, 0.0), (F32, 50, 200, chunk, 4, 0.0),              # two and four lanes
                 (F64, 50, 200, chunk, 1, 0.0),                                             # f64
                 (F32, 50, 200, chunk, 1, 0.5),                                             # gamma != 0
                 (F32, 0, 200, chunk, 1, 0.0), (F32, 50, 0, chunk, 1, 0.0), (F32, 50, 200, 0, 1, 0.0),
                 (F32, 50, 200, chunk, 3, 0.0)):
        assert xs(*args) == 0 and scc(*args) == 0


def test_switches(rule, monkeypatch):
    xs, scc, slots, chunk = rule
    monkeypatch.setenv("DTMPC_FAST_XROWS", "dense")  # form 3
    for B in (slots, 200):
        assert xs(F32, 50, B, chunk, 1, 0.0) == 0 and scc(F32, 50, B, chunk, 1, 0.0) == 1
    monkeypatch.setenv("DTMPC_FAST_XROWS", "sparse")  # any other value: the rule
    assert xs(F32, 50, 200, chunk, 1, 0.0) == S and scc(F32, 50, 200, chunk, 1, 0.0) == 1
    monkeypatch.setenv("DTMPC_FAST_SCC", "0")  # form 2, whatever the other switch says
    assert xs(F32, 50, 200, chunk, 1, 0.0) == 0 and scc(F32, 50, 200, chunk, 1, 0.0) == 0
    monkeypatch.delenv("DTMPC_FAST_XROWS")
    assert xs(F32, 50, slots, chunk, 1, 0.0) == 0 and scc(F32, 50, slots, chunk, 1, 0.0) == 0
    monkeypatch.setenv("DTMPC_FAST_SCC", "1")
    assert xs(F32, 50, 200, chunk, 1, 0.0) == S
    monkeypatch.delenv("DTMPC_FAST_SCC")
    monkeypatch.setenv("DTMPC_FAST_G0", "1")  # the compact records with the general recursion: neither table
    assert xs(F32, 50, 200, chunk, 1, 0.0) == 0 and scc(F32, 50, 200, chunk, 1, 0.0) == 0
