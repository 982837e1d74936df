"""Device-code identity of two builds, kernel by kernel (the method of profiles/r08/isa_identity.txt): per unit the
gfx950 code object is unbundled as build.py's _code_object does, disassembled with llvm-objdump -d --no-show-raw-insn
--no-leading-addr and split per kernel; kernels are compared by their instruction text and by their metadata notes
(register, spill and segment sizes).  Kernels present on one side only are listed, not compared.
--by-content UNIT[,UNIT...]: these units' kernels were renamed, so they are compared as multisets of (instruction text,
resource notes) instead, each kernel's own symbol in its branch targets (<symbol+0x...>) replaced by a placeholder.
usage: isa_identity.py [--by-content UNITS] PARENT_product_objs.txt BRANCH_product_objs.txt
       (build/obj/product_objs.txt of each build)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ProcessPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "differentiable-tube-mpc_amd"))
import build as B  # noqa: E402

NOTE = re.compile(r"\s+\.(name|vgpr_count|sgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|"
                  r"private_segment_fixed_size|group_segment_fixed_size|kernarg_segment_size):\s+(\S+)")


def unit(obj):
    with tempfile.TemporaryDirectory() as d:
        co = B._code_object(obj, d)
        dis = subprocess.run([f"{B.LLVM}/llvm-objdump", "-d", f"--mcpu={B.ARCH}", "--no-show-raw-insn",
                              "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([f"{B.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                               text=True).stdout
    # one entry of amdhsa.kernels per kernel, its keys in alphabetical order (.args ... .name ... .wavefront_size): an
    # entry starts at a "- ." line of the list's own indentation (the entries of .args are indented deeper)
    res, cur, ind = {}, None, None
    for line in notes.splitlines():
        if line.strip() == "amdhsa.kernels:":
            cur, ind = None, None
            continue
        e = re.match(r"(\s*)- \.", line)
        if e and (ind is None or len(e.group(1)) <= ind):
            ind, cur = len(e.group(1)), {}
            line = line.replace("- ", "  ", 1)
        m = NOTE.match(line)
        if m and cur is not None:
            if m.group(1) == "name":
                res[m.group(2)] = cur
            else:
                cur[m.group(1)] = m.group(2)
    code, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<?([_A-Za-z0-9.$]+)>?:\s*$", line)
        if m:
            name = m.group(1) if m.group(1) in res else None
            continue
        if name:
            # without the trailing "// address: encoding" comment: kernels behind a new one move in the code object
            # (and without the "..." / blank lines objdump prints for the padding in front of the next function)
            t = line.split("//")[0].strip()
            if t and t != "...":
                code.setdefault(name, []).append(t)
    return os.path.basename(obj).split(".")[0], {k: ("\n".join(v), res[k]) for k, v in code.items()}


def content(kernels):
    """The sorted multiset of a unit's kernels without their names: (sha256 of the text, resource notes)."""
    return sorted((hashlib.sha256(text.replace(f"<{k}+", "<SELF+").encode()).hexdigest(), tuple(sorted(notes.items())))
                  for k, (text, notes) in kernels.items())


def main(pa, br, by_content=()):
    objs = [open(p).read().split() for p in (pa, br)]
    with ProcessPoolExecutor(max_workers=8) as pool:
        P, Q = (dict(pool.map(unit, o)) for o in objs)
    print("# unit  kernels(parent/branch)  sha256(common kernels' disassembly) parent  branch  resource notes  verdict")
    ok = True
    for tu in sorted(P):
        a, b = P[tu], Q[tu]
        if tu in by_content:
            ca, cb = content(a), content(b)
            ha, hb = (hashlib.sha256(repr([t for t, _ in c]).encode()).hexdigest()[:16] for c in (ca, cb))
            notes = sorted(n for _, n in ca) == sorted(n for _, n in cb)
            same = ca == cb
            ok &= same
            print(f"{tu:22s} {len(a):3d}/{len(b):3d}  {ha}  {hb}  {'equal' if notes else 'DIFFER'}  "
                  f"{'IDENTICAL' if same else 'DIFFERENT'}  (by content)")
            continue
        common = sorted(set(a) & set(b))
        ha, hb = (hashlib.sha256("\n".join(k + "\n" + s[k][0] for k in common).encode()).hexdigest()[:16] for s in (a, b))
        notes = all(a[k][1] == b[k][1] for k in common)
        same = ha == hb and notes
        ok &= same
        print(f"{tu:22s} {len(a):3d}/{len(b):3d}  {ha}  {hb}  {'equal' if notes else 'DIFFER'}  "
              f"{'IDENTICAL' if same else 'DIFFERENT'}")
        for k in sorted(set(b) - set(a)):
            print(f"    new in branch: {k}  {b[k][1]}")
        for k in sorted(set(a) - set(b)):
            ok = False
            print(f"    missing in branch: {k}")
        if not same:
            for k in common:
                if a[k] != b[k]:
                    print(f"    differs: {k}")
    print("ALL COMMON KERNELS IDENTICAL" if ok else "DIFFERENCES")
    return 0 if ok else 1


if __name__ == "__main__":
    argv = sys.argv[1:]
    units = ()
    if argv and argv[0] == "--by-content":
        units, argv = tuple(argv[1].split(",")), argv[2:]
    sys.exit(main(argv[0], argv[1], units))
