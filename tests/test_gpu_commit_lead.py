"""The sparse-rows commit pass's prefetch ring (csrc/dtmpc_fast.hip commit, the SV::xs > 0 branch; DTMPC_CM_LEAD): the
pass keeps R = (L + S) / S * S step buffers in rotation, each refilled L steps before its step uses it, enters its loop
of whole R-step trips through L preloads (each followed by rewrites of X row 0 in the places of a step's stores) and
finishes the N % R steps left outside it.  Only when the loads are issued
differs from the dense commit loop that forms 3 and 2 keep, so form 4 (sparse rows), form 3 (DTMPC_FAST_XROWS=dense) and
form 2 (DTMPC_FAST_SCC=0) must agree bit for bit, NaN payloads included, on every array bench.dump_outputs lists, over
two closed-loop steps (the second one warm-started).

Horizons: the ones the entry sequence and the ragged end can get wrong -- 1, L - 1, L, L + 1 (shorter than, equal to and
just past the preloads, whose indices are clamped to N - 1), R - 1, R, R + 1 (no trip, exactly one, one and a step),
2 R - 1, 2 R, 2 R + 1 (the longest ragged end, two trips, two and a step).  tests/test_gpu_sparse_rows.py holds 50 and 52.
B = 200 at one lane is four 64-thread workgroups, the last wave partial (8 of 64 lanes).  Every horizon is run plainly,
with the decision records on, with the workspace pre-filled with NaN and with 3e38 (a refill that read a row this solve
never wrote, or a row after its overwrite, would differ) and through the split step."""
import ctypes as C
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu
NAMES = ("x", "b", "xbar", "bbar", "Xnom", "Unom", "Xaux", "Uaux", "status", "iters", "theta", "vel", "sums")
S = 5                      # the shipped stride (kXStride)
L = 3                      # the shipped lead of the sparse commit loop (DTMPC_CM_LEAD's default)
R = (L + S) // S * S       # its ring: the step buffers in rotation, the loop's trip in steps
HORIZONS = sorted({n for n in (1, L - 1, L, L + 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1) if n >= 1})
FORMS = {4: {}, 3: {"DTMPC_FAST_XROWS": "dense"}, 2: {"DTMPC_FAST_SCC": "0"}}
B = 200


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _setup(N):
    import bench

    st = bench.bench_setup("f32")
    return dataclasses.replace(st, problem=dataclasses.replace(st.problem, horizon=N),
                               ilqr_nom=dataclasses.replace(st.ilqr_nom, horizon=N),
                               ilqr_aux=dataclasses.replace(st.ilqr_aux, horizon=N))


def _launched(N, chunk):
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


def _run(dev, monkeypatch, form, N, overlap=False, fill=None, records=False):
    import bench

    monkeypatch.setenv("DTMPC_TUBE_LANES", "1")
    for k in ("DTMPC_FAST_XROWS", "DTMPC_FAST_SCC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    st = _setup(N)
    mpc = bench.TubeMPC(st, batch=B, device=dev, dtype=torch.float32, disturbance="philox", seed=0, overlap=overlap,
                        record_choices=records, record_costs=records)
    assert mpc.lanes == 1 and mpc.overlap == overlap
    assert _launched(N, mpc.chunk) == form  # the run must really launch the form it means to
    if fill is not None:
        mpc.work[: mpc.work.numel() // 4 * 4].view(torch.float32).fill_(fill)
    mpc.reset(bench.initial_states(0, B, dev, torch.float32))
    mpc.step()
    mpc.step()
    torch.cuda.synchronize(dev)
    names = NAMES + (("choices", "costs") if records else ())
    return {k: getattr(mpc, k).cpu().numpy().copy() for k in names}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k  # bitwise, NaN included


_REF = {}


def _ref(dev, monkeypatch, N):
    """form 2 at horizon N (neither table, the dense commit loop): computed once, shared by the tests, never changed"""
    if N not in _REF:
        _REF[N] = _run(dev, monkeypatch, 2, N)
        for v in _REF[N].values():
            v.setflags(write=False)
    return _REF[N]


@pytest.mark.parametrize("N", HORIZONS)
def test_three_forms_agree(dev, monkeypatch, N):
    a = _ref(dev, monkeypatch, N)
    assert (a["status"] == 0).any()  # not a comparison of failed solves alone
    _same(a, _run(dev, monkeypatch, 3, N))
    _same(a, _run(dev, monkeypatch, 4, N))


@pytest.mark.parametrize("N", HORIZONS)
def test_decision_records_agree(dev, monkeypatch, N):
    a = _run(dev, monkeypatch, 2, N, records=True)
    _same(a, _run(dev, monkeypatch, 3, N, records=True))
    _same(a, _run(dev, monkeypatch, 4, N, records=True))
    _same({k: a[k] for k in NAMES}, _ref(dev, monkeypatch, N))  # and recording changes no result


@pytest.mark.parametrize("N", HORIZONS)
def test_reads_only_what_it_wrote(dev, monkeypatch, N):
    """whatever the workspace held before the solve, the outputs are the same"""
    a = _ref(dev, monkeypatch, N)
    _same(a, _run(dev, monkeypatch, 4, N, fill=float("nan")))
    _same(a, _run(dev, monkeypatch, 4, N, fill=3.0e38))


@pytest.mark.parametrize("N", HORIZONS)
def test_split_step(dev, monkeypatch, N):
    """phase 1 (nominal) then phase 2 (the rest), each with its own commit passes: the split step is the whole step"""
    a = _ref(dev, monkeypatch, N)
    _same(a, _run(dev, monkeypatch, 2, N, overlap=True))
    _same(a, _run(dev, monkeypatch, 3, N, overlap=True))
    _same(a, _run(dev, monkeypatch, 4, N, overlap=True))
