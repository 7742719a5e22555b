"""tfem_p2_apply_rows_multi (csrc/tfem_p2apply_multi.hip) as far as a machine without a GPU can
tell: the declaration, the export, the refusals decided on the host before any launch, and that no
instance of the block kernels uses scratch memory."""

import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, UNSUPPORTED, INDEX_RANGE = 1, 2, 4  # TFEM_ERR_INVALID_ARGUMENT, _UNSUPPORTED, _INDEX_RANGE


def test_header_declares_and_library_exports_the_p2_block_entry_point():
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(tfem_[a-z0-9_]+)\(", header, re.M))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    name = "tfem_p2_apply_rows_multi"
    assert name in declared, f"{name} is not declared in tfem_assembly.h"
    assert name in exported and hasattr(lib, name), f"{name} is not exported"
    # coords, real_bytes, quad_order, alpha, beta, plan, layout, colind, nnz, u, y, n_dofs, n_vec, stream
    assert len(_native.SIGNATURES[name][1]) == 14
    assert lib.tfem_abi_version() == 2


def test_p2_block_apply_refuses_bad_arguments_without_a_device():
    """n_vec, a NULL u, U and Y overlapping in a later column, an extent beyond the 32-bit offsets,
    real_bytes, an unknown quadrature order, an n_dofs that is not the plan's: all decided on the
    host before any launch (addresses only, nothing is dereferenced)."""
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    layout = np.zeros(24, dtype=np.int64)
    layout[0], layout[1], layout[2], layout[3] = 1, 1, 25, 56  # a launch would follow the checks
    z = ctypes.c_void_p(layout.ctypes.data)
    call = lib.tfem_p2_apply_rows_multi
    u, y = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)

    def refused(status, word, *args):
        assert call(*args) == status
        assert word in lib.tfem_last_error(), lib.tfem_last_error()

    refused(INVALID, b"n_vec", None, 8, 2, 1.0, 0.0, None, z, None, 10, u, y, 81, 0, None)
    refused(INVALID, b"n_vec", None, 8, 2, 1.0, 0.0, None, z, None, 10, u, y, 81, -3, None)
    refused(INVALID, b"u is NULL", None, 8, 2, 1.0, 0.0, None, z, None, 10, None, y, 81, 4, None)
    refused(INVALID, b"u is NULL", None, 8, 2, 1.0, 0.0, None, z, None, 10, None, y, 81, 1, None)
    # Y begins inside the LAST column range of U's block: beyond u + 81 * 8, inside u + 81 * 4 * 8
    late = ctypes.c_void_p((1 << 20) + 8 * (81 * 4 - 1))
    refused(INVALID, b"overlap", None, 8, 2, 1.0, 0.0, None, z, None, 10, u, late, 81, 4, None)
    refused(INVALID, b"overlap", None, 8, 2, 1.0, 0.0, None, z, None, 10, late, u, 81, 4, None)
    refused(INVALID, b"overlap", None, 8, 2, 1.0, 0.0, None, z, None, 10, u, u, 81, 4, None)
    # 81 * n_vec * 8 bytes at and beyond 0xFFFFFF00, and a product that does not fit 64 bits
    refused(INDEX_RANGE, b"32-bit", None, 8, 2, 1.0, 0.0, None, z, None, 10, u, y, 81, (0xFFFFFF00 // (81 * 8)) + 1, None)
    refused(INDEX_RANGE, b"32-bit", None, 8, 2, 1.0, 0.0, None, z, None, 10, u, y, 81, 1 << 62, None)
    refused(INVALID, b"real_bytes", None, 3, 2, 1.0, 0.0, None, z, None, 10, u, y, 81, 4, None)
    refused(INVALID, b"plan_layout_host", None, 8, 2, 1.0, 0.0, None, None, None, 10, u, y, 81, 4, None)
    refused(INVALID, b"negative", None, 8, 2, 1.0, 0.0, None, z, None, -10, u, y, 81, 4, None)
    refused(UNSUPPORTED, b"order", None, 8, 9, 1.0, 0.0, None, z, None, 10, u, y, 81, 4, None)
    refused(UNSUPPORTED, b"order", None, 4, 9, 1.0, 0.0, None, z, None, 10, u, y, 81, 1, None)
    refused(INVALID, b"81 DoFs, not 80", None, 8, 2, 1.0, 0.0, None, z, None, 10, u, y, 80, 4, None)
    refused(INVALID, b"NULL", None, 8, 2, 1.0, 0.0, None, z, None, 10, u, y, 81, 4, None)  # coords, plan, colind
    # an empty plan: nothing to do, for one column and for several
    hold = np.zeros(24, dtype=np.int64)
    empty = ctypes.c_void_p(hold.ctypes.data)
    for n_vec in (1, 4):
        assert call(None, 8, 2, 1.0, 0.0, None, empty, None, 0, None, None, 0, n_vec, None) == 0


def test_no_p2_block_apply_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_p2apply_multi.hip, compiled for gfx950 with the build's own
    flags: no scratch memory, at most 256 VGPRs (tools/kernel_regs.py on the assembly).  mass x 2
    kinds x (fp64: the widths 2 and 4, fp32: the column loop inside the launch), and the long rows."""
    import __graft_entry__ as entry

    name = "tfem_p2apply_multi.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS.get(name, [])
    asm = tmp_path / "p2apply_multi.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    counts = {}
    for kernel in ("k_p2_apply_rows_multi", "k_p2_apply_long_rows_multi"):
        out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm), kernel],
                             check=True, capture_output=True, text=True).stdout
        rows = [re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)", line) for line in out.splitlines()]
        assert rows and all(rows), out[-2000:]
        bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
        assert not bad, bad
        counts[kernel] = len(rows)
    print(counts)
    assert counts["k_p2_apply_rows_multi"] == 2 * 2 * (2 + 1)
    assert counts["k_p2_apply_long_rows_multi"] == 4
