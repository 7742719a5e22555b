"""The coefficient-data launches (tfem_p1_rings_field, tfem_p1_apply_rings_field,
tfem_p1_field_adjoint; csrc/tfem_rings_field.hip) -- what can be said without a GPU: the entry points
are declared, exported and have their ctypes signatures; the refusals that are decided before
anything touches a device; every built instance of the two kernels keeps its state in registers."""

import os
import re
import shutil
import subprocess
import sys
from ctypes import c_double, c_int, c_int64, c_void_p

import numpy as np
import pytest

from conftest import REPO

NAMES = ("tfem_p1_rings_field", "tfem_p1_apply_rings_field", "tfem_p1_field_adjoint")
OK, INVALID, UNSUPPORTED, INDEX_RANGE = 0, 1, 2, 4


def _native():
    from pytorch_fem_solver_amd import _native

    return _native


def test_header_declares_and_library_exports_the_entry_points():
    native = _native()
    lib = native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(tfem_[a-z0-9_]+)\(", header, re.M))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    for name in NAMES:
        assert name in declared, f"{name} is not declared in tfem_assembly.h"
        assert name in native.SIGNATURES, f"{name} has no ctypes signature"
        assert name in exported and hasattr(lib, name), f"{name} is not exported"
    # header, binding and library agree on the whole interface
    assert declared == set(native.SIGNATURES)
    assert declared <= exported
    sig = native.SIGNATURES
    store, apply, adjoint = (sig[name][1] for name in NAMES)
    assert all(sig[name][0] is c_int for name in NAMES)
    # coords, real_bytes, n_verts, quad_order, alpha, beta, kappa, kappa_nq, c, c_nq, n_elems, plan, layout
    head = [c_void_p, c_int, c_int64, c_int, c_double, c_double, c_void_p, c_int, c_void_p, c_int, c_int64,
            c_void_p, c_void_p]
    assert store == head + [c_void_p, c_void_p]             # vals, stream
    assert apply == head + [c_void_p, c_void_p, c_void_p]   # u, y, stream
    assert adjoint == [c_void_p, c_int, c_void_p, c_int64, c_int64, c_int, c_double, c_double, c_void_p, c_void_p,
                       c_int64, c_void_p, c_void_p, c_void_p]


def _layout(**over):
    """The layout of a small, valid 7-slot plan (csrc/tfem_rings_host.cpp: ring_layout)."""
    z = np.zeros(32, dtype=np.int64)
    z[0], z[1], z[2], z[3], z[4], z[5], z[6], z[7] = 2, 300, 400, 220, 150, 7, 7, 4
    z[12], z[14], z[17], z[18] = 1 << 16, 70, 300, 1
    for k, v in over.items():
        z[int(k[1:])] = v
    return z


def test_refusals_that_need_no_device():
    """Every refusal below is decided from the arguments: no pointer is dereferenced (the device
    pointers here are made-up addresses) and nothing is launched."""
    lib = _native().load()
    fake = lambda i: c_void_p(0x1000000 * (i + 1))  # noqa: E731
    z = _layout()

    def store(real_bytes=8, n_verts=300, order=3, kappa=fake(1), knq=4, c=fake(2), cnq=4, n_elems=500, layout=z,
              beta=1.0, vals=fake(4)):
        where = None if layout is None else c_void_p(layout.ctypes.data)
        return lib.tfem_p1_rings_field(fake(0), real_bytes, n_verts, order, 1.0, beta, kappa, knq, c, cnq, n_elems,
                                       fake(3), where, vals, None)

    def apply(u, y, n_verts=300, layout=z, beta=1.0, order=3, knq=4):
        return lib.tfem_p1_apply_rings_field(fake(0), 8, n_verts, order, 1.0, beta, fake(1), knq, None, 0, 500, fake(3),
                                             c_void_p(layout.ctypes.data), u, y, None)

    def said(text):
        return text in lib.tfem_last_error().decode()

    # TFEM_ERR_INVALID_ARGUMENT
    assert store(real_bytes=2) == INVALID and said("real_bytes")
    assert store(layout=None) == INVALID and said("plan_layout_host")
    assert store(n_verts=-1) == INVALID and store(n_elems=-1) == INVALID and said("negative")
    assert store(knq=3) == INVALID and store(cnq=2) == INVALID and said("values per element")
    assert store(order=1, knq=4) == INVALID  # order 1 has one point
    assert store(kappa=None, c=None) == INVALID and said("tfem_p1_assemble_rings / tfem_p1_apply_rings")
    assert apply(fake(5), fake(5)) == INVALID and said("overlap")
    assert apply(fake(5), c_void_p(fake(5).value + 8 * 299)) == INVALID  # the last entry of u is the first of y
    assert store(vals=None) == INVALID and apply(fake(5), None) == INVALID and said("NULL")
    # TFEM_ERR_UNSUPPORTED
    assert store(order=7) == UNSUPPORTED and said("Integration order")
    assert store(layout=_layout(z23=3)) == UNSUPPORTED and said("long rows")
    assert store(layout=_layout(z18=0)) == UNSUPPORTED and store(layout=_layout(z17=769)) == UNSUPPORTED and said("stages")
    # LDS: 1024 vertices and 768 elements per tile, fp64 with mass: 16 KB + 16.4 KB stage + 42 KB > 64 KB
    big = _layout(z3=1024, z4=256, z14=256, z17=768)
    assert store(layout=big) == UNSUPPORTED and said("LDS")
    assert apply(fake(5), fake(6), layout=big) == UNSUPPORTED and said("LDS")
    # TFEM_ERR_INDEX_RANGE: n_elems * Q * real_bytes, the vertices, the CSR bound
    assert store(n_elems=(1 << 32) // 32) == INDEX_RANGE
    assert store(n_elems=(1 << 32) // 8, knq=1, c=None) == INDEX_RANGE
    assert store(n_verts=1 << 29) == INDEX_RANGE
    assert store(layout=_layout(z1=1 << 28, z5=8)) == INDEX_RANGE
    # empty plans succeed and launch nothing (no device is needed to say so)
    assert store(layout=_layout(z0=0)) == OK and store(n_verts=0) == OK
    assert apply(fake(5), fake(6), n_verts=0) == OK


def test_adjoint_refusals_that_need_no_device():
    lib = _native().load()
    fake = lambda i: c_void_p(0x1000000 * (i + 1))  # noqa: E731

    def adjoint(real_bytes=8, n_elems=10, n_verts=8, order=3, n_vec=1, g=fake(2), grad_kappa=fake(4), grad_c=fake(5)):
        return lib.tfem_p1_field_adjoint(fake(0), real_bytes, fake(1), n_elems, n_verts, order, 1.0, 1.0, g, fake(3),
                                         n_vec, grad_kappa, grad_c, None)

    assert adjoint(real_bytes=3) == INVALID
    assert adjoint(n_elems=-1) == INVALID and adjoint(n_verts=-1) == INVALID and adjoint(n_vec=0) == INVALID
    assert adjoint(order=9) == UNSUPPORTED
    assert adjoint(g=None) == INVALID
    assert adjoint(n_elems=0) == OK and adjoint(grad_kappa=None, grad_c=None) == OK


def test_no_field_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_rings_field.hip, compiled for gfx950 with the build's own flags:
    k_p1_field_rows in fp64 / fp32 x 7 / 15 slots x mass x chunked x Q in {1, 3, 4, 6} x apply / diag /
    store = 192, k_p1_field_adjoint in fp64 / fp32 x Q = 8; no scratch memory, at most 256 VGPRs --
    read from the assembly with tools/kernel_regs.py."""
    import __graft_entry__ as entry

    name = "tfem_rings_field.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS.get(name, [])
    asm = tmp_path / "field.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    pattern = r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)"
    for kernel, count in (("k_p1_field_rows", 192), ("k_p1_field_adjoint", 8)):
        out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm), kernel],
                             check=True, capture_output=True, text=True).stdout
        rows = [re.match(pattern, line) for line in out.splitlines()]
        assert len(rows) == count and all(rows), out[-2000:]
        if kernel == "k_p1_field_rows":
            for real in ("double", "float"):
                for slots in (7, 15):
                    for mode in (0, 1, 2):
                        mine = [m for m in rows if re.search(rf"<{real}, {slots}, \w+, \w+, \d, {mode}>", m.group(5))]
                        assert len(mine) == 16, (real, slots, mode, len(mine))
        bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
        assert not bad, bad
