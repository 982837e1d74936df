"""The tape's heading sin / cos cached in LDS (csrc/dtmpc_fast.hip Scc, tube_fast_kernel<M, 1, 3>; f32, one lane per
trajectory, gamma = 0 records): the cached values are the ones the kernel would evaluate again, so the cached kernel
(the default where the host rule selects it) and today's kernel (DTMPC_FAST_SCC=0, read at each call) must agree bit
for bit on every array bench.dump_outputs lists, over two closed-loop steps.

Shapes: B = 200 at one lane is four 64-thread workgroups, the last wave partial (8 of 64 lanes); N = 50 is the paper
horizon, N = 3 the shortest one the four-deep line-search loop and the three-deep commit loop leave with a ragged tail;
the smallest batch with 256-thread workgroups is the device's lane slots (CUs x 256)."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu
NAMES = ("x", "b", "xbar", "bbar", "Xnom", "Unom", "Xaux", "Uaux", "status", "iters", "theta", "vel", "sums")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _setup(N=None):
    import bench

    st = bench.bench_setup("f32")
    if N is not None:
        st = dataclasses.replace(st, problem=dataclasses.replace(st.problem, horizon=N),
                                 ilqr_nom=dataclasses.replace(st.ilqr_nom, horizon=N),
                                 ilqr_aux=dataclasses.replace(st.ilqr_aux, horizon=N))
    return st


def _selected(B, N, chunk):
    """the host rule's answer for this launch shape (diagnostics export, not part of include/dtmpc.h)"""
    import ctypes as C

    from diff_tube_mpc_strict_pt import _lib

    f = _lib.load().dtmpc_diag_tube_sincos_cache
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_double]
    return f(0, N, B, chunk, 1, 0.0)


def _run(dev, monkeypatch, scc, B, N=None, overlap=False, chunk=None):
    import bench

    if scc is None:
        monkeypatch.delenv("DTMPC_FAST_SCC", raising=False)
    else:
        monkeypatch.setenv("DTMPC_FAST_SCC", scc)
    st = _setup(N)
    mpc = bench.TubeMPC(st, batch=B, device=dev, dtype=torch.float32, disturbance="philox", seed=0, overlap=overlap)
    assert mpc.lanes == 1 and mpc.overlap == overlap and (chunk is None or mpc.chunk == chunk)
    # both runs must really differ in the kernel they launch: the rule selects the cache only with the switch unset
    assert _selected(B, st.problem.horizon, mpc.chunk) == (0 if scc == "0" else 1)
    mpc.reset(bench.initial_states(0, B, dev, torch.float32))
    mpc.step()
    mpc.step()
    torch.cuda.synchronize(dev)
    return {k: getattr(mpc, k).cpu().numpy().copy() for k in NAMES}


def _same(a, b):
    assert (a["status"] == 0).mean() > 0.9
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k  # bitwise, NaN included


@pytest.mark.parametrize("N", [50, 3])
def test_cached_equals_uncached_small(dev, monkeypatch, N):
    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    _same(_run(dev, monkeypatch, "0", 200, N), _run(dev, monkeypatch, None, 200, N))


def test_cached_equals_uncached_block256(dev, monkeypatch):
    B = torch.cuda.get_device_properties(dev).multi_processor_count * 256  # tube_block(B, 1) = 256 from here
    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    _same(_run(dev, monkeypatch, "0", B), _run(dev, monkeypatch, None, B))


def test_cached_equals_uncached_split_step(dev, monkeypatch):
    """phase 1 (nominal) then phase 2 (the rest): each launch's solve fills its own table"""
    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    a = _run(dev, monkeypatch, "0", 200, overlap=True)
    _same(a, _run(dev, monkeypatch, None, 200, overlap=True))
    _same(a, _run(dev, monkeypatch, None, 200))  # and the split step is the whole step


def test_cached_equals_uncached_chunked(dev, monkeypatch):
    """chunks of 256, the smallest the library takes (DTMPC_FAST_CHUNK, as test_tube_step_fast_chunked_bitwise forces
    them), so the chunked shape is that test's B = 700 = 256 + 256 + 188: 64-thread workgroups, a partial last wave"""
    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    a = _run(dev, monkeypatch, None, 700)
    monkeypatch.setenv("DTMPC_FAST_CHUNK", "256")
    _same(a, _run(dev, monkeypatch, None, 700, chunk=256))
    _same(a, _run(dev, monkeypatch, "0", 700, chunk=256))
