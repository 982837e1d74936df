"""CPU test of the host rule that selects the tube step's sin / cos cache kernel (csrc/dtmpc_fast.hip tube_fast_scc,
through the diagnostics export dtmpc_diag_tube_sincos_cache): f32, one lane per trajectory, gamma = 0 records, a horizon
whose [N][threads] table fits the CU's LDS, and a launch every workgroup of which is resident at once -- no more threads
than the device has lane slots (without a device the library assumes the MI355X's 256 CUs = 65,536 slots; with one, the
batches below scale with its CU count).  Everything else takes the kernel without the table."""
import ctypes as C

import pytest

F32, F64 = 0, 1


@pytest.fixture(scope="module")
def rule():
    from diff_tube_mpc_strict_pt import _lib

    lib = _lib.load()
    f = lib.dtmpc_diag_tube_sincos_cache
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_double]
    # the lane slots the library sees: the smallest one-lane batch whose workgroups are 256 threads (tube_block),
    # i.e. whose partial rows are one per 256 trajectories and no longer one per 64
    lo, hi = 257, 1 << 24
    while lo < hi:
        mid = (lo + hi) // 2
        if lib.dtmpc_tube_partials_count(mid, 1) == (mid + 255) // 256:
            hi = mid
        else:
            lo = mid + 1
    slots = lo
    chunk = int(lib.dtmpc_tube_chunk(50, 1))
    return f, slots, chunk


def test_rule_selects_the_headline_shape(rule, monkeypatch):
    f, slots, chunk = rule
    monkeypatch.delenv("DTMPC_FAST_SCC", raising=False)
    monkeypatch.delenv("DTMPC_FAST_G0", raising=False)
    assert slots % 256 == 0 and slots >= 256
    assert f(F32, 50, slots, chunk, 1, 0.0) == 1      # every lane slot taken: 256-thread workgroups
    assert f(F32, 50, slots - 1, chunk, 1, 0.0) == 1  # 64-thread workgroups
    assert f(F32, 50, 200, chunk, 1, 0.0) == 1
    assert f(F32, 3, 200, chunk, 1, 0.0) == 1
    assert f(F32, 64, 200, chunk, 1, 0.0) == 1        # the table's cap


def test_rule_falls_back(rule, monkeypatch):
    f, slots, chunk = rule
    monkeypatch.delenv("DTMPC_FAST_SCC", raising=False)
    monkeypatch.delenv("DTMPC_FAST_G0", raising=False)
    assert f(F32, 65, 200, chunk, 1, 0.0) == 0          # a horizon above the table's cap
    assert f(F32, 50, slots + 1, chunk, 1, 0.0) == 0    # a batch above the residency rule ...
    assert f(F32, 50, 2 * slots, chunk, 1, 0.0) == 0
    assert f(F32, 50, 2 * slots, slots, 1, 0.0) == 1    # ... unless its chunks are launches that fit
    assert f(F32, 50, 200, chunk, 2, 0.0) == 0          # two and four lanes
    assert f(F32, 50, 200, chunk, 4, 0.0) == 0
    assert f(F64, 50, 200, chunk, 1, 0.0) == 0          # f64
    assert f(F32, 50, 200, chunk, 1, 0.5) == 0          # gamma != 0: the general records
    assert f(F32, 0, 200, chunk, 1, 0.0) == 0 and f(F32, 50, 0, chunk, 1, 0.0) == 0 and f(F32, 50, 200, 0, 1, 0.0) == 0


def test_switch_forces_the_plain_kernel(rule, monkeypatch):
    f, slots, chunk = rule
    monkeypatch.delenv("DTMPC_FAST_G0", raising=False)
    monkeypatch.setenv("DTMPC_FAST_SCC", "0")
    assert f(F32, 50, slots, chunk, 1, 0.0) == 0 and f(F32, 50, 200, chunk, 1, 0.0) == 0
    monkeypatch.setenv("DTMPC_FAST_SCC", "1")
    assert f(F32, 50, 200, chunk, 1, 0.0) == 1
    monkeypatch.delenv("DTMPC_FAST_SCC")
    monkeypatch.setenv("DTMPC_FAST_G0", "1")  # the compact records with the general recursion: not the cached form
    assert f(F32, 50, 200, chunk, 1, 0.0) == 0
