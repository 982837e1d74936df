"""What per-trajectory scenes cost: the fused f32 tube step with UNIFORM scenes (every trajectory the paper's table and
target, so both compute the same numbers) against the shared step, same process, runs interleaved.

  python scripts/scenes_cost.py [--rounds 5] [--steps 100] [--out FILE]

Legs: B = 65,536 at one lane (the headline form) and B = 4,096 at four lanes.  Variants per leg, alternated round by
round: `shared` (the product: at one lane the sin / cos cache form, GM 3), `shared_noscc` (one lane only,
DTMPC_FAST_SCC=0: the GM 2 form the scene kernels are instantiated at -- the like-for-like partner) and `scenes`.
Each figure is the median kernel time of `steps` held-theta steps (device events around the launch, after a warm-up
of 3); the spread of a variant is max - min of its per-round medians.  One JSON line per leg."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "differentiable-tube-mpc_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diff_tube_mpc_strict_pt.core import TubeMPC, pack_scenes  # noqa: E402
from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config  # noqa: E402


def make(st, B, lanes, dev, scenes):
    os.environ["DTMPC_TUBE_LANES"] = str(lanes)  # read once, when the state is built
    sc = None
    if scenes:
        obs = np.array([[o.center[0], o.center[1], o.radius] for o in st.problem.obstacles])
        sc = pack_scenes(st.problem, np.broadcast_to(obs, (B,) + obs.shape),
                         np.broadcast_to(np.array(st.nominal_cost.target), (B, 3)), dtype=torch.float32, device=dev)
    m = TubeMPC(st, batch=B, device=dev, dtype=torch.float32, disturbance="philox", seed=7, scenes=sc)
    assert m.lanes == lanes
    rng = np.random.default_rng(1)
    x0 = np.stack([rng.uniform(0, 1, B), rng.uniform(0, 1, B), rng.uniform(0, np.pi / 2, B)], 1)
    return m, torch.as_tensor(x0, dtype=torch.float32, device=dev)


def timed(m, x0, steps, scc):
    """median kernel ms of `steps` steps of a fresh episode (DTMPC_FAST_SCC is read at each launch)"""
    os.environ["DTMPC_FAST_SCC"] = "1" if scc else "0"
    m.reset(x0)
    for _ in range(3):
        m.step(adapt=False)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e in ev:
        m.step(adapt=False, kernel_events=e)
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev), m.x.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    st = paper_setup_from_config(paper_config())
    lines = []
    for B, lanes in ((65536, 1), (4096, 4)):
        shared, x0 = make(st, B, lanes, dev, False)
        scenes, _ = make(st, B, lanes, dev, True)
        variants = [("shared", shared, True), ("scenes", scenes, True)]
        if lanes == 1:
            variants.insert(1, ("shared_noscc", shared, False))
        ms = {n: [] for n, _, _ in variants}
        ends = {}
        for _ in range(a.rounds):
            for n, m, scc in variants:
                t, ends[n] = timed(m, x0, a.steps, scc)
                ms[n].append(t)
        os.environ.pop("DTMPC_FAST_SCC", None)
        same = all(torch.equal(torch.nan_to_num(ends["shared"]), torch.nan_to_num(v)) for v in ends.values())
        rec = {"B": B, "lanes": lanes, "rounds": a.rounds, "steps": a.steps, "outputs_bitwise_equal": bool(same)}
        for n, v in ms.items():
            rec[n] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                      "ms_max": round(max(v), 4), "spread": round(max(v) - min(v), 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del shared, scenes
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
