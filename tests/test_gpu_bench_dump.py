"""bench.py --dump-outputs (GPU): dump_outputs writes what the last step left in the TubeMPC buffers a caller reads,
in the run's precision, sampled by a fixed index set above DUMP_MAX_TRAJ trajectories, and two runs over the same
inputs write the same files bit for bit (so two builds of the library can be compared output for output).
B = 4,200 is the smallest round batch past DUMP_MAX_TRAJ = 4,096 (the sampled path); B = 300 is written whole."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
PER_TRAJ = ("x", "b", "xbar", "bbar", "Xnom", "Unom", "Xaux", "Uaux", "status", "iters")
SHARED = ("theta", "vel", "sums")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("tag,B", [("f32", 4200), ("f32", 300), ("f64", 300)])
def test_dump_outputs_is_the_last_step_and_repeats(dev, tag, B, tmp_path):
    import bench

    tdt, npdt = (torch.float32, np.float32) if tag == "f32" else (torch.float64, np.float64)
    setup = bench.bench_setup(tag)
    x0 = bench.initial_states(0, B, dev, tdt)
    dumps = []
    for run in ("a", "b"):
        mpc = bench.TubeMPC(setup, batch=B, device=dev, dtype=tdt, disturbance="philox", seed=0, global_offset=0,
                            global_batch=B, process_group=None)
        for _ in range(2):  # the bench's timed step: a fresh episode start every time
            mpc.reset(x0)
            mpc.step()
        shapes = bench.dump_outputs(mpc, str(tmp_path / run))
        dumps.append(_load(str(tmp_path / run)))
        assert set(dumps[-1]) == set(PER_TRAJ + SHARED + ("sample_index",)) == set(shapes)
    a, b = dumps
    n = min(B, bench.DUMP_MAX_TRAJ)
    idx = a["sample_index"].astype(np.int64)
    assert idx.shape == (n,) and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < B
    assert n == B or n == bench.DUMP_MAX_TRAJ
    total = 0
    for k, v in a.items():
        total += v.nbytes
        assert v.dtype == (npdt if k in PER_TRAJ[:8] + SHARED else np.float64), k
        assert v.tobytes() == b[k].tobytes(), k  # bitwise, NaN included
        if k in PER_TRAJ + SHARED:  # the buffers of the second run's TubeMPC, on the sampled trajectories
            want = getattr(mpc, k).cpu().numpy()
            want = want[..., idx] if k in PER_TRAJ else want
            assert v.shape == want.shape and np.array_equal(v, want.astype(v.dtype), equal_nan=True), k
    assert total <= 64 * 2 ** 20
    assert np.isfinite(a["theta"]).all() and (a["status"] == 0).mean() > 0.9
    # at the bench's own batch the sample keeps f64 under the limit as well
    per_traj = sum(int(np.prod(a[k].shape[:-1])) for k in PER_TRAJ) + 1
    assert bench.DUMP_MAX_TRAJ * per_traj * 8 <= 64 * 2 ** 20
