"""Dependency chains per basic block of one kernel in a hipcc --save-temps assembly file: how many
vector instructions a block has, and how many ADJACENT pairs of them are producer -> consumer (the
second reads a vector register the first wrote).  Such a pair cannot issue back to back: a block
made of them runs at the latency of the pipe, not at its rate, whenever no other wave of the SIMD
has a vector instruction ready.  A sibling of tools/kernel_lanes.py and tools/kernel_regs.py.

    hipcc --offload-arch=gfx950 ... -c --save-temps -o x.o file.hip
    python tools/kernel_chains.py file-hip-amdgcn-amd-amdhsa-gfx950.s [--min N] [--distance] substring ...

The kernel is the first one whose demangled name holds every substring (spaces ignored).  Blocks with
fewer than N vector instructions (default 16) are left out of the list, not of the totals.
--distance adds, per block, the shortest and the mean distance (in vector instructions) from a
consumer back to the nearest producer of one of its operands inside the block.

Only register operands are parsed: the first operand of a vector instruction is what it writes, the
others are what it reads; a multiply-accumulate reads its destination too.  (Compares write a
scalar register and so produce nothing here.)
"""
import re
import subprocess
import sys

from kernel_lanes import blocks, kernels

_REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def vregs(operand):
    """The vector registers an operand names, as a set of register numbers."""
    out = set()
    for m in _REG.finditer(operand):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def split_operands(line):
    """(registers written, registers read) of one vector instruction."""
    body = line.split(";")[0].split(None, 1)
    if len(body) < 2:
        return set(), set()
    ops = [o.strip() for o in body[1].split(",")]
    # a register range holds a comma-free "v[a:b]"; modifiers (neg, abs, op_sel ...) carry no register
    written = vregs(ops[0])
    read = set().union(*[vregs(o) for o in ops[1:]]) if len(ops) > 1 else set()
    if "mac_" in body[0]:  # multiply-accumulate: the destination is the third source, not named again
        read |= written
    return written, read


def analyse(lines):
    """vector instructions, dependent adjacent pairs, list of consumer -> nearest producer distances."""
    vec = [split_operands(s) for s in lines if s.startswith("v_")]
    pairs = sum(1 for (w, _), (_, r) in zip(vec, vec[1:]) if w & r)
    last, dist = {}, []
    for i, (w, r) in enumerate(vec):
        d = [i - last[x] for x in r if x in last]
        if d:
            dist.append(min(d))
        for x in w:
            last[x] = i
    return len(vec), pairs, dist


def main():
    args = sys.argv[1:]
    distance = "--distance" in args
    args = [a for a in args if a != "--distance"]
    least = 16
    if "--min" in args:
        i = args.index("--min")
        least = int(args[i + 1])
        del args[i:i + 2]
    text = open(args[0]).read()
    want = [w.replace(" ", "") for w in args[1:]]
    found = kernels(text)
    dem = subprocess.run(["c++filt"], input="\n".join(n for n, _ in found), capture_output=True, text=True).stdout
    for (name, body), d in zip(found, dem.split("\n")):
        if not all(w in d.replace(" ", "") for w in want):
            continue
        print(d.replace("tfem::", "").split("(")[0])
        tot_v = tot_p = 0
        for label, depth, lines in blocks(body):
            n, pairs, dist = analyse(lines)
            tot_v += n
            tot_p += pairs
            if n < least:
                continue
            row = f"  {label:12s} depth {depth}  valu {n:4d}  dependent adjacent pairs {pairs:4d} of {n - 1:4d}"
            if distance and dist:
                row += f"  nearest producer: min {min(dist)} mean {sum(dist) / len(dist):.1f}"
            print(row)
        print(f"  whole kernel: valu {tot_v}  dependent adjacent pairs {tot_p}")
        return
    sys.exit("no kernel matches " + " ".join(args[1:]))


if __name__ == "__main__":
    main()
