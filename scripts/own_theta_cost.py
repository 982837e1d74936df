"""What own theta costs: the fused f32 tube step with per-trajectory ancillary weights (TubeMPC(own_theta=True), uniform
theta0, every trajectory adapting from its own gradient row inside the kernel) against the shared step INCLUDING its
partial-sum reduction and theta-update launches, same process, runs interleaved.

  python scripts/own_theta_cost.py [--rounds 5] [--steps 100] [--out FILE]

Legs: B = 4,096 at four lanes and B = 65,536 at one lane (the headline form).  Variants per leg, alternated round by
round: `shared` (the product: at one lane the sin / cos cache form, GM 3), `shared_noscc` (one lane only,
DTMPC_FAST_SCC=0: the GM 2 form the own-theta kernels are instantiated at -- the like-for-like partner) and `own`.
Each figure is the median time of `steps` adapting steps, device events around the whole step (the fused launch and,
for the shared variants, dtmpc_partials_reduce and dtmpc_theta_update; the own variant's reduction for `sums` is
counted too), after a warm-up of 3; the spread of a variant is max - min of its per-round medians.  The two modes
compute different things once theta moves (batch-mean against per-trajectory gradient: other weights, other
per-lane branches), so each variant also runs with theta HELD (`*_held`, adapt=False: one fused launch each, the same
numbers in both modes -- the end states are compared bitwise), which isolates what the per-lane weights cost in the
loops.  One JSON line per leg."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "differentiable-tube-mpc_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diff_tube_mpc_strict_pt.core import TubeMPC  # noqa: E402
from diff_tube_mpc_strict_pt.core.problem import paper_config, paper_setup_from_config  # noqa: E402


def make(st, B, lanes, dev, own):
    os.environ["DTMPC_TUBE_LANES"] = str(lanes)  # read once, when the state is built
    m = TubeMPC(st, batch=B, device=dev, dtype=torch.float32, disturbance="philox", seed=7, own_theta=own)
    assert m.lanes == lanes and not m.overlap
    rng = np.random.default_rng(1)
    x0 = np.stack([rng.uniform(0, 1, B), rng.uniform(0, 1, B), rng.uniform(0, np.pi / 2, B)], 1)
    return m, torch.as_tensor(x0, dtype=torch.float32, device=dev)


def timed(m, x0, steps, scc, adapt):
    """median ms of `steps` steps of a fresh episode (DTMPC_FAST_SCC is read at each launch), and the end state"""
    os.environ["DTMPC_FAST_SCC"] = "1" if scc else "0"
    m.reset(x0)
    for _ in range(3):
        m.step(adapt=adapt)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        m.step(adapt=adapt)
        b.record()
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
    for B, lanes in ((4096, 4), (65536, 1)):
        shared, x0 = make(st, B, lanes, dev, False)
        own, _ = make(st, B, lanes, dev, True)
        variants = [("shared", shared, True), ("own", own, True)]
        if lanes == 1:
            variants.insert(1, ("shared_noscc", shared, False))
        variants = [(n, m, scc, True) for n, m, scc in variants] + [(n + "_held", m, scc, False) for n, m, scc in variants]
        ms = {n: [] for n, *_ in variants}
        ends = {}
        for _ in range(a.rounds):
            for n, m, scc, adapt in variants:
                t, ends[n] = timed(m, x0, a.steps, scc, adapt)
                ms[n].append(t)
        os.environ.pop("DTMPC_FAST_SCC", None)
        same = all(torch.equal(torch.nan_to_num(ends["shared_held"]), torch.nan_to_num(v))
                   for n, v in ends.items() if n.endswith("_held"))
        rec = {"B": B, "lanes": lanes, "rounds": a.rounds, "steps": a.steps, "held_outputs_bitwise_equal": bool(same)}
        for n, v in ms.items():
            rec[n] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                      "ms_max": round(max(v), 4), "spread": round(max(v) - min(v), 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del shared, own
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
