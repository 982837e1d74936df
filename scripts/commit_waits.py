"""The sparse-rows commit loop's vector-memory operations and wait counts, read from the disassembly (the record
profiles/r11/commit_waits.txt): for one kernel of a unit's object, every innermost loop (backward branch) whose body
holds buffer loads and 64-bit buffer stores is listed; the commit's loop of whole trips is the one with 3 * RB buffer
loads, RB 64-bit stores (U rows) and RB / XS 128-bit stores (X rows), once for the nominal and once for the ancillary
solve.  One line per buffer_* / s_waitcnt / branch in body order, the back edge last.  usage: commit_waits.py OBJECT [KERNEL-SUBSTRING] [--loads N]   (default kernel: tube_fast_kernelILi5ELi1ELi4E;
--loads: print only loops with that many buffer loads)"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "differentiable-tube-mpc_amd"))
import build as B  # noqa: E402


def main(obj, want, loads):
    with tempfile.TemporaryDirectory() as d:
        co = B._code_object(obj, d)
        dis = subprocess.run([f"{B.LLVM}/llvm-objdump", "-d", f"--mcpu={B.ARCH}", "--no-show-raw-insn",
                              "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
    for k, ins in B._listing(dis).items():
        if want not in k:
            continue
        idx = {a: i for i, (_, a, _) in enumerate(ins)}
        for i, (x, a, t) in enumerate(ins):
            if not x.startswith(("s_cbranch", "s_branch")) or t is None or t not in idx or idx[t] > i:
                continue
            body = ins[idx[t]:i + 1]
            ops = [y for y, _, _ in body]
            nl = sum(o.startswith("buffer_load") for o in ops)
            ns2 = sum(o.startswith("buffer_store_dwordx2") for o in ops)
            ns4 = sum(o.startswith("buffer_store_dwordx4") for o in ops)
            if not nl or not ns2 or (loads and nl != loads):
                continue
            if any(y.startswith(("s_cbranch", "s_branch")) and u is not None and u <= b for y, b, u in body[:-1]):
                continue  # an outer loop (the body's forward branches -- the step's range tests -- stay)
            nv = sum(o.startswith("v_") for o in ops)
            print(f"== {k}  loop at +{t:#x}..+{a:#x}: {len(ops)} instructions, {nv} VALU, {nl} buffer loads, "
                  f"{ns2} 64-bit and {ns4} 128-bit buffer stores")
            for j, o in enumerate(ops):
                if o.startswith(("buffer_", "s_waitcnt", "s_cbranch", "s_branch")):
                    print(f"  {j:5d}  {o}")


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if not x.startswith("--")]
    n = int(sys.argv[sys.argv.index("--loads") + 1]) if "--loads" in sys.argv else 0
    if "--loads" in sys.argv:
        a.remove(str(n))
    main(a[0], a[1] if len(a) > 1 else "tube_fast_kernelILi5ELi1ELi4E", n)
