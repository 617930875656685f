#!/usr/bin/env python3
"""Compare two directories of gfx950 device assembly, kernel by kernel.

    python scripts/isa_compare.py BEFORE_DIR AFTER_DIR

Each directory holds one .s file per kernel unit of __graft_entry__.hip_units(), compiled with the build's flags plus
`--cuda-device-only -S` (scripts/isa_compare.py --dump DIR does that for the tree it sits in).  Files are not compared
byte by byte: two compiles of one source differ in the random __hip_cuid_ symbol, and deleting dead code may move an
instruction by a line.  Per function symbol (kernels and out-of-line device functions), after dropping comments and
__hip_cuid_ lines:

    SAME     the .amdhsa_* descriptor values (registers, scratch, LDS, accumulator offset, ...) are identical and so is
             the multiset of full instruction lines, operands included
    MNEMONIC the descriptor and the multiset of instruction mnemonics are identical, some operands are not
    DIFF     anything else (a symbol missing on one side included)

Exit status 0 iff no function is DIFF.
"""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(out, jobs=8):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    os.makedirs(out, exist_ok=True)
    cmds = [[ge._hipcc()] + ge.HIP_FLAGS + flags + ["--cuda-device-only", "-S", os.path.join(ge.CSRC, src),
                                                    "-o", os.path.join(out, obj[:-2] + ".s")]
            for obj, src, flags in ge.hip_units() if src == "kernels_tu.hip"]
    running = []
    while cmds or running:
        while cmds and len(running) < jobs:
            running.append(subprocess.Popen(cmds.pop(0)))
        proc = running.pop(0)
        if proc.wait() != 0:
            sys.exit("hipcc failed: " + " ".join(proc.args))


def parse(path):
    """{symbol: (descriptor lines, Counter of instruction lines)} of one .s file"""
    funcs, desc = {}, {}
    known = set()
    cur = body = None
    with open(path, errors="replace") as f:
        for raw in f:
            line = raw.split(";", 1)[0].strip()
            if not line or "__hip_cuid_" in line:
                continue
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                known.add(m.group(1))
                continue
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur, body = m.group(1), None
                desc[cur] = []
                continue
            if line == ".end_amdhsa_kernel":
                cur = None
                continue
            if cur is not None and body is None and line.startswith(".amdhsa_"):
                desc[cur].append(" ".join(line.split()))
                continue
            if line.endswith(":") and line[:-1] in known:
                cur, body = line[:-1], collections.Counter()
                funcs[cur] = body
                continue
            if line.startswith(".Lfunc_end"):
                cur = body = None
                continue
            if body is not None and not line.startswith(".") and not line.endswith(":"):
                body[" ".join(line.split())] += 1
    return {k: (desc.get(k, []), v) for k, v in funcs.items()}


def mnemonics(counter):
    out = collections.Counter()
    for line, n in counter.items():
        out[line.split()[0]] += n
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        return dump(sys.argv[2])
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a_dir, b_dir = sys.argv[1:]
    names = sorted(set(n for d in (a_dir, b_dir) for n in os.listdir(d) if n.endswith(".s")))
    tally = collections.Counter()
    for name in names:
        pa, pb = os.path.join(a_dir, name), os.path.join(b_dir, name)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{name}: DIFF  (file missing on one side)")
            tally["DIFF"] += 1
            continue
        a, b = parse(pa), parse(pb)
        for sym in sorted(set(a) | set(b)):
            if sym not in a or sym not in b:
                verdict, why = "DIFF", "symbol missing " + ("before" if sym not in a else "after")
            else:
                (da, ia), (db, ib) = a[sym], b[sym]
                n = sum(ia.values())
                if da != db:
                    changed = sorted(set(da) ^ set(db))
                    verdict, why = "DIFF", "descriptor: " + "; ".join(changed[:6])
                elif ia == ib:
                    verdict, why = "SAME", f"{n} instructions"
                elif mnemonics(ia) == mnemonics(ib):
                    moved = sum(((ia - ib) + (ib - ia)).values())
                    verdict, why = "MNEMONIC", f"{n} instructions, {moved // 2} differ in operands"
                else:
                    d = (mnemonics(ia) - mnemonics(ib)) + (mnemonics(ib) - mnemonics(ia))
                    verdict, why = "DIFF", f"{n} -> {sum(ib.values())} instructions; mnemonics: " + ", ".join(
                        f"{k} x{v}" for k, v in d.most_common(8))
            tally[verdict] += 1
            print(f"{name}: {verdict:8s} {sym}  ({why})")
    print(f"total: {sum(tally.values())} functions in {len(names)} units: {tally['SAME']} SAME, "
          f"{tally['MNEMONIC']} MNEMONIC, {tally['DIFF']} DIFF")
    return 1 if tally["DIFF"] else 0


if __name__ == "__main__":
    sys.exit(main())
