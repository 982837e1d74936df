"""Sparse state rows between the passes of one iLQR solve (csrc/dtmpc_fast.hip Bt, tube_fast_kernel<M, 1, 4>; f32, one
lane per trajectory, gamma = 0 records): the kernel stores only every S-th X row (and row N), keeps b of every row in an
LDS table and re-rolls x, y, theta of the rows between in the backward pass, by the arithmetic that wrote them.  So the
three forms -- 4 (the default where the host rule selects it), 3 (DTMPC_FAST_XROWS=dense: the sin / cos cache with dense
rows) and 2 (DTMPC_FAST_SCC=0: neither table) -- must agree bit for bit, NaN payloads included, on every array
bench.dump_outputs lists, over two closed-loop steps (the second one warm-started).

Shapes: B = 200 at one lane is four 64-thread workgroups, the last wave partial (8 of 64 lanes).  Horizons: 1, 2, 3 (shorter
than a group, and than the prefetch leads), S - 1, S, S + 1 (one group, ragged and not), 2 S + 1 (a one-step top group), 50
(the paper's), 52 (the cap of the rule); none of them is refused by the plain kernel.  53 is the first horizon that keeps
dense rows.  The smallest batch with 256-thread workgroups is the device's lane slots (CUs x 256)."""
import ctypes as C
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu
NAMES = ("x", "b", "xbar", "bbar", "Xnom", "Unom", "Xaux", "Uaux", "status", "iters", "theta", "vel", "sums")
S = 5      # the shipped stride (kXStride)
CAP = 52   # the longest horizon with sparse rows (kSparseMaxN)
FORMS = {4: {}, 3: {"DTMPC_FAST_XROWS": "dense"}, 2: {"DTMPC_FAST_SCC": "0"}}


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


def _launched(B, N, chunk):
    """the form the host rule gives this launch shape under the current environment (diagnostics exports)"""
    from diff_tube_mpc_strict_pt import _lib

    lib = _lib.load()
    out = []
    for f in (lib.dtmpc_diag_tube_sincos_cache, lib.dtmpc_diag_tube_sparse_rows):
        f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_double]
        out.append(f(0, N, B, chunk, 1, 0.0))
    scc, xs = out
    assert xs in (0, S) and (scc == 1 or xs == 0)
    return 4 if xs else 3 if scc else 2


def _run(dev, monkeypatch, form, B, N=None, overlap=False, chunk=None, fill=None, records=False, expect=None):
    import bench

    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    for k in ("DTMPC_FAST_XROWS", "DTMPC_FAST_SCC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    st = _setup(N)
    mpc = bench.TubeMPC(st, batch=B, device=dev, dtype=torch.float32, disturbance="philox", seed=0, overlap=overlap,
                        record_choices=records, record_costs=records)
    assert mpc.lanes == 1 and mpc.overlap == overlap and (chunk is None or mpc.chunk == chunk)
    # the run must really launch the form it means to
    assert _launched(B, st.problem.horizon, mpc.chunk) == (form if expect is None else expect)
    if fill is not None:
        mpc.work[: mpc.work.numel() // 4 * 4].view(torch.float32).fill_(fill)
    mpc.reset(bench.initial_states(0, B, dev, torch.float32))
    mpc.step()
    mpc.step()
    torch.cuda.synchronize(dev)
    names = NAMES + (("choices", "costs") if records else ())
    return {k: getattr(mpc, k).cpu().numpy().copy() for k in names}


def _same(a, b, healthy=0.9):
    assert (a["status"] == 0).mean() > healthy
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k  # bitwise, NaN included


@pytest.mark.parametrize("N", [1, 2, 3, S - 1, S, S + 1, 2 * S + 1, 50, CAP])
def test_three_forms_agree(dev, monkeypatch, N):
    a = _run(dev, monkeypatch, 2, 200, N)
    _same(a, _run(dev, monkeypatch, 3, 200, N))
    _same(a, _run(dev, monkeypatch, 4, 200, N))


def test_above_the_cap_rows_stay_dense(dev, monkeypatch):
    a = _run(dev, monkeypatch, 2, 200, CAP + 1)
    _same(a, _run(dev, monkeypatch, 4, 200, CAP + 1, expect=3))  # no switch set: the rule itself keeps form 3


def test_decision_records_agree(dev, monkeypatch):
    a = _run(dev, monkeypatch, 2, 200, records=True)
    assert (a["choices"] >= 0).any()
    _same(a, _run(dev, monkeypatch, 3, 200, records=True))
    _same(a, _run(dev, monkeypatch, 4, 200, records=True))


def test_block256(dev, monkeypatch):
    B = torch.cuda.get_device_properties(dev).multi_processor_count * 256  # tube_block(B, 1) = 256 from here
    a = _run(dev, monkeypatch, 2, B)
    _same(a, _run(dev, monkeypatch, 4, B))
    _same(a, _run(dev, monkeypatch, 3, B))


def test_split_step(dev, monkeypatch):
    """phase 1 (nominal) then phase 2 (the rest): the second launch reads the dense nominal rows the first one left"""
    a = _run(dev, monkeypatch, 2, 200, overlap=True)
    _same(a, _run(dev, monkeypatch, 4, 200, overlap=True))
    _same(a, _run(dev, monkeypatch, 4, 200))  # and the split step is the whole step


def test_chunked(dev, monkeypatch):
    """chunks of 256 at B = 700 = 256 + 256 + 188 (DTMPC_FAST_CHUNK, as tests/test_gpu_sincos_cache.py forces them)"""
    a = _run(dev, monkeypatch, 4, 700)
    monkeypatch.setenv("DTMPC_FAST_CHUNK", "256")
    _same(a, _run(dev, monkeypatch, 4, 700, chunk=256))
    _same(a, _run(dev, monkeypatch, 3, 700, chunk=256))
    _same(a, _run(dev, monkeypatch, 2, 700, chunk=256))


def test_reads_only_what_it_wrote(dev, monkeypatch):
    """the X rows the passes leave out are never read: whatever the workspace held before, the outputs are the same"""
    a = _run(dev, monkeypatch, 4, 200, 50, fill=float("nan"))
    _same(a, _run(dev, monkeypatch, 4, 200, 50, fill=3.0e38))
    _same(a, _run(dev, monkeypatch, 2, 200, 50))
