#!/usr/bin/env python3
"""Measures the constants of tests/_layer_gate.sharp_gate and writes the table profiles/r17/layer_sharp_gate.txt holds.

    python scripts/layer_sharp_gate.py --builds-only          # CPU: the three f32 oracle builds among themselves
    python scripts/layer_sharp_gate.py --out FILE             # GPU: the builds + the composition on the device,
                                                              # and the fused kernels' own ratios under the result

Per case (tests/_layer_cases.ALL_CASES), tape, weights mode and key: the leave-one-out ratio (each reference evaluation
held to the band of the others with k = 1, tests/_layer_gate.leave_one_out) at each floor; per key family the worst over
all of them, the floor and k tests/_layer_gate.choose derives, and -- with a device -- every launch's fused kernel's
worst error / band under those constants.  The fused kernels' figures are printed, they do not enter the choice."""
from __future__ import annotations

import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "differentiable-tube-mpc_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--builds-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from oracle import oracle

    oracle.build()
    import _layer_cases as LC
    import _layer_gate as LG

    dev = None
    if not args.builds_only:
        import torch

        assert torch.cuda.is_available(), "the composition and the fused kernels need a HIP device"
        dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("sharp gate: leave-one-out among the reference evaluations, truth = the f64 oracle on the same f32 inputs")
    say("  builds: the three f32 oracle builds among themselves (tests/test_layer_gate_teeth.py's constants)")
    if dev is not None:
        say("  all:    the builds + the composition on the device (tests/test_gpu_layer_all_m.py's constants)")
    modes = ("builds",) if dev is None else ("builds", "all")
    say(f"worst ratio per (case, tape, weights, key) at the floors {LG.FLOORS}, " + " | ".join(modes))
    worst = {m: {fam: {f: 0.0 for f in LG.FLOORS} for fam in LC.FAMILIES} for m in modes}
    contexts = sorted({(v[2], v[3]) for v in LC.LAUNCHES.values()})
    comp = {}
    for case in LC.ALL_CASES:
        for tape, wts in contexts:
            c = LC.tape_case(case, tape)
            refs, truth = LC.references(tuple(case), tape, wts)
            evals = {"builds": list(refs)}
            if dev is not None:
                comp[(tuple(case), tape, wts)] = LC.composition(case, tape, wts, dev)
                evals["all"] = list(refs) + [comp[(tuple(case), tape, wts)]]
            for key in LC.keys_of(LC.WIDEST[(tape, wts)], c):
                cols = []
                for m in modes:
                    r = {f: float(LG.leave_one_out(evals[m], truth, key, f).max()) for f in LG.FLOORS}
                    for f in LG.FLOORS:
                        worst[m][LC.FAMILY[key]][f] = max(worst[m][LC.FAMILY[key]][f], r[f])
                    cols.append(" ".join(f"{r[f]:9.3g}" for f in LG.FLOORS))
                say(f"  {LC.case_id(case):26s} {tape:5s} {'wts' if wts else '   '} {key:9s} " + " | ".join(cols))
    const = {}
    for m in modes:
        say()
        say(f"{m}: per key family the worst leave-one-out ratio at each floor -> floor, k = 2 x worst")
        for fam in LC.FAMILIES:
            const[fam] = LG.choose(worst[m][fam])
            say(f"  {fam:6s} " + " ".join(f"{worst[m][fam][f]:9.3g}" for f in LG.FLOORS)
                + f"  -> floor {const[fam][0]:g}, k {const[fam][1]:g}")
    if dev is not None:
        say()
        say("fused kernels under these constants: worst error / band per launch and key (1 = the band's edge)")
        for case in LC.ALL_CASES:
            for launch, (fam_k, fl, tape, wts, _) in LC.LAUNCHES.items():
                c = LC.tape_case(case, tape)
                refs, truth = LC.references(tuple(case), tape, wts)
                got = LC.fused(case, launch, dev)
                out = []
                for key in LC.keys_of(launch, c):
                    floor, k = const[LC.FAMILY[key]]
                    try:
                        w = LG.sharp_gate(got, list(refs) + [comp[(tuple(case), tape, wts)]], truth, key, floor, k,
                                          "table")
                        out.append(f"{key} {w:.3g}")
                    except AssertionError as e:
                        out.append(f"{key} FAIL {str(e)[:160]}")
                say(f"  {LC.case_id(case):26s} {launch:14s} {fam_k}{'' if fl is None else ('<1>' if fl else '<0>')}: "
                    + ", ".join(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(ln for ln in lines) + "\n")


if __name__ == "__main__":
    main()
