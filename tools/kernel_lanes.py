"""Spill traffic per basic block of one kernel in a hipcc --save-temps assembly file: vector
instructions, v_readlane / v_writelane among them, scalar loads, and the loop depth hipcc's block
comments give.  A sibling of tools/kernel_regs.py (registers, scratch, LDS).

    hipcc --offload-arch=gfx950 ... -c --save-temps -o x.o file.hip
    python tools/kernel_lanes.py file-hip-amdgcn-amd-amdhsa-gfx950.s [--all] substring [substring ...]

The kernel is the first one whose demangled name holds every substring (spaces ignored), e.g.
"k_p1_rings<double,7,false,true,4,false,true,2>".  Without --all only blocks with a lane move are
listed; the totals cover the whole kernel and, separately, the blocks inside a loop.
"""
import re
import subprocess
import sys


def kernels(text):
    """(mangled name, body) of every function in the file."""
    out = []
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        out.append((m.group(1), m.group(2)))
    return out


def blocks(body):
    """(label, depth, lines) per basic block; depth = deepest loop the block's comments name."""
    out, label, depth, lines = [], "entry", 0, []
    for line in body.split("\n"):
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            out.append((label, depth, lines))
            label, depth, lines = m.group(1), 0, []
        s = line.strip()
        if s.startswith(";") or "; " in line and re.match(r"^\.LBB", line):
            for d in re.findall(r"Depth[= ](\d+)", line):
                depth = max(depth, int(d))
        if s and not s.startswith((";", ".")) and not re.match(r"^\.?\w+:", s):
            lines.append(s)
    out.append((label, depth, lines))
    return out


def main():
    args = sys.argv[1:]
    show_all = "--all" in args
    args = [a for a in args if a != "--all"]
    text = open(args[0]).read()
    want = [w.replace(" ", "") for w in args[1:]]
    found = kernels(text)
    dem = subprocess.run(["c++filt"], input="\n".join(n for n, _ in found), capture_output=True, text=True).stdout
    for (name, body), d in zip(found, dem.split("\n")):
        if not all(w in d.replace(" ", "") for w in want):
            continue
        print(d.replace("tfem::", "").split("(")[0])
        tot = [0, 0, 0, 0]
        loop = [0, 0, 0, 0]
        for label, depth, lines in blocks(body):
            valu = sum(1 for s in lines if s.startswith("v_"))
            rd = sum(1 for s in lines if s.startswith("v_readlane"))
            wr = sum(1 for s in lines if s.startswith("v_writelane"))
            sl = sum(1 for s in lines if s.startswith("s_load") or s.startswith("s_buffer_load"))
            for acc in (tot, loop) if depth > 0 else (tot,):
                for i, v in enumerate((valu, rd, wr, sl)):
                    acc[i] += v
            if show_all or rd or wr:
                print(f"  {label:12s} depth {depth}  valu {valu:4d}  readlane {rd:3d}  writelane {wr:3d}  s_load {sl:2d}")
        print(f"  whole kernel: valu {tot[0]}  readlane {tot[1]}  writelane {tot[2]}  s_load {tot[3]}")
        print(f"  inside loops: valu {loop[0]}  readlane {loop[1]}  writelane {loop[2]}  s_load {loop[3]}")
        return
    sys.exit("no kernel matches " + " ".join(args[1:]))


if __name__ == "__main__":
    main()
