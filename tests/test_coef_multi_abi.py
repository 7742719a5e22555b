"""The block launch of the variable-coefficient P1 operator (tfem_p1_apply_rings_coef_multi,
k_p1_coef_rows_multi in csrc/tfem_rings_coef_multi.hip) -- what can be said without a GPU: the
entry point is declared, exported and has its ctypes signature; every built instance of the kernel
keeps its sums and the interpreter in registers."""

import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import REPO

NAME = "tfem_p1_apply_rings_coef_multi"
#: widths of k_p1_coef_rows_multi that are built (kCoefWidths), per record size
WIDTHS = {7: (2, 4, 8), 15: (2, 4)}


def test_header_declares_and_library_exports_the_block_entry_point():
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(tfem_[a-z0-9_]+)\(", header, re.M))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert NAME in declared, f"{NAME} is not declared in tfem_assembly.h"
    assert NAME in _native.SIGNATURES, f"{NAME} has no ctypes signature"
    assert NAME in exported and hasattr(lib, NAME), f"{NAME} is not exported"
    # the arguments of tfem_p1_apply_rings_coef with n_vec in front of the stream
    assert len(_native.SIGNATURES[NAME][1]) == 14
    assert _native.SIGNATURES[NAME][1][:12] == _native.SIGNATURES["tfem_p1_apply_rings_coef"][1][:12]


def test_no_block_coefficient_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_rings_coef_multi.hip, compiled for gfx950 with the build's own
    flags and the file's own: fp64 / fp32 x mass x chunked x Q in {1, 3, 4, 6} = 32 per record size
    and width, no scratch memory, at most 256 VGPRs -- read from the assembly with
    tools/kernel_regs.py."""
    import __graft_entry__ as entry

    name = "tfem_rings_coef_multi.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS[name]
    asm = tmp_path / "coef_multi.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm),
                          "k_p1_coef_rows_multi"], check=True, capture_output=True, text=True).stdout
    rows = [re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)", line) for line in out.splitlines()]
    # 32 instances per width and record size: (3 + 2) widths x 32 = 160
    assert sum(len(w) for w in WIDTHS.values()) * 32 == 160
    assert len(rows) == 160 and all(rows), out[-2000:]
    for slots, widths in WIDTHS.items():
        for real in ("double", "float"):
            for nv in widths:
                mine = [m for m in rows if re.search(rf"<{real}, {slots}, \w+, \w+, \d, {nv}>", m.group(5))]
                assert len(mine) == 16, (real, slots, nv, len(mine))
    bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
    assert not bad, bad
