"""The coefficient-data block launch (tfem_p1_apply_rings_field_multi, k_p1_field_rows_multi in
csrc/tfem_rings_field_multi.hip) -- what can be said without a GPU: the entry point is declared,
exported and has its ctypes signature; the refusals that are decided before anything touches a
device, in their order; every built instance of the kernel keeps its state in registers."""

import os
import re
import shutil
import subprocess
import sys
from ctypes import c_int, c_int64, c_void_p

import pytest

from conftest import REPO
from test_field_abi import INDEX_RANGE, INVALID, OK, UNSUPPORTED, _layout, _native

NAME = "tfem_p1_apply_rings_field_multi"
#: the kernel's widths per record size: kFieldWidths / kFieldWide15 of csrc/tfem_rings_field_multi.hip
WIDTHS = {7: (2, 4, 8), 15: (2, 4)}


def test_header_declares_and_library_exports_the_entry_point():
    native = _native()
    lib = native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(tfem_[a-z0-9_]+)\(", header, re.M))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert NAME in declared, f"{NAME} is not declared in tfem_assembly.h"
    assert NAME in native.SIGNATURES, f"{NAME} has no ctypes signature"
    assert NAME in exported and hasattr(lib, NAME), f"{NAME} is not exported"
    restype, args = native.SIGNATURES[NAME]
    single = native.SIGNATURES["tfem_p1_apply_rings_field"][1]
    assert restype is c_int and len(args) == 17 and len(single) == 16
    assert args[:15] == single[:15]                 # coords .. layout, u, y
    assert args[15:] == [c_int64, c_void_p]         # n_vec, stream
    # the widths named in the source are the ones this file expects
    source = open(os.path.join(REPO, "pytorch_fem_solver_amd", "csrc", "tfem_rings_field_multi.hip")).read()
    table = re.search(r"constexpr int kFieldWidths\[\] = \{([0-9, ]+)\};\s*constexpr int kFieldWide15 = (\d+);", source)
    assert table, "the width table of tfem_rings_field_multi.hip"
    built = tuple(int(w) for w in table.group(1).split(","))
    assert built == WIDTHS[7] and tuple(w for w in built if w <= int(table.group(2))) == WIDTHS[15]


def test_refusals_that_need_no_device():
    """Every refusal below is decided from the arguments: no pointer is dereferenced (the device
    pointers here are made-up addresses) and nothing is launched.  Each call also carries the NEXT
    refusal's fault (or a later one of another status), so a check out of order shows."""
    lib = _native().load()
    fake = lambda i: c_void_p(0x1000000 * (i + 1))  # noqa: E731
    z = _layout()
    long_rows = _layout(z23=3)

    def multi(u=fake(5), y=fake(6), n_vec=3, real_bytes=8, n_verts=300, order=3, kappa=fake(1), knq=4, c=fake(2),
              cnq=4, n_elems=500, layout=z, beta=1.0):
        where = None if layout is None else c_void_p(layout.ctypes.data)
        return lib.tfem_p1_apply_rings_field_multi(fake(0), real_bytes, n_verts, order, 1.0, beta, kappa, knq, c, cnq,
                                                   n_elems, fake(3), where, u, y, n_vec, None)

    def said(text):
        return text in lib.tfem_last_error().decode()

    # 1 .. 7: TFEM_ERR_INVALID_ARGUMENT
    assert multi(real_bytes=2, layout=None) == INVALID and said("real_bytes")
    assert multi(layout=None, n_verts=-1) == INVALID and said("plan_layout_host")
    assert multi(n_verts=-1, n_vec=0) == INVALID and multi(n_elems=-1, n_vec=0) == INVALID and said("negative")
    assert multi(n_vec=0, u=None) == INVALID and said("n_vec")
    assert multi(n_vec=-1, u=None) == INVALID and said("n_vec")
    assert multi(u=None, kappa=None, c=None) == INVALID and said("u is NULL") and said("tfem_p1_apply_rings_field")
    assert multi(kappa=None, c=None, knq=3) == INVALID and said("tfem_p1_apply_rings_multi")
    assert multi(knq=3, n_verts=1 << 27, n_vec=4) == INVALID and said("values per element")
    assert multi(cnq=2, n_verts=1 << 27, n_vec=4) == INVALID and said("values per element")
    assert multi(order=1, knq=4, cnq=1) == INVALID  # order 1 has one point
    # 8: TFEM_ERR_INDEX_RANGE, before the overlap is looked at
    assert multi(u=fake(5), y=fake(5), n_verts=1 << 27, n_vec=4) == INDEX_RANGE
    assert multi(u=fake(5), y=fake(5), n_vec=1 << 62) == INDEX_RANGE
    assert multi(u=fake(5), y=fake(5), n_elems=(1 << 32) // 32) == INDEX_RANGE
    assert multi(u=fake(5), y=fake(5), n_elems=(1 << 32) // 8, knq=1, c=None) == INDEX_RANGE
    # 9: overlap over the whole block extent, before the plan is looked at
    assert multi(u=fake(5), y=fake(5), layout=long_rows) == INVALID and said("overlap")
    last = c_void_p(fake(5).value + 8 * (300 * 3 - 1))  # the last entry of U is the first of Y
    assert multi(u=fake(5), y=last, layout=long_rows) == INVALID and said("overlap")
    assert multi(u=last, y=fake(5), layout=long_rows) == INVALID and said("overlap")
    assert multi(u=fake(5), y=c_void_p(last.value + 8), order=9) == UNSUPPORTED and said("Integration order")
    # 10: TFEM_ERR_UNSUPPORTED -- long rows, the element stage, LDS, the order
    assert multi(layout=_layout(z23=3, z18=0)) == UNSUPPORTED and said("long rows")
    assert multi(layout=long_rows, n_vec=1) == UNSUPPORTED and said("long rows")
    assert multi(layout=_layout(z18=0, z3=1024, z17=700)) == UNSUPPORTED and said("stages")
    assert multi(layout=_layout(z17=769, z3=1024)) == UNSUPPORTED and said("stages")
    # 1024 vertices and 700 elements per tile, fp64 with mass: the single launch's 3 * 1024 + 7 * 700
    # reals are 63,776 bytes (it takes the plan up to its launch), two columns' (2 + 2) * 1024 + 7 * 700
    # reals are 71,968
    assert 8 * (3 * 1024 + 7 * 700) == 63776 <= 64 * 1024 < 71968 == 8 * (4 * 1024 + 7 * 700)
    big = _layout(z3=1024, z4=256, z14=256, z17=700)
    assert multi(layout=big, order=9) == UNSUPPORTED and said("LDS") and said("71968")
    assert multi(layout=big, order=9, beta=0.0) == UNSUPPORTED and said("Integration order")  # 38,368 bytes: fits
    assert multi(order=9) == UNSUPPORTED and said("Integration order")
    # empty plans succeed and launch nothing (no device is needed to say so)
    assert multi(layout=_layout(z0=0)) == OK and multi(n_verts=0) == OK
    assert multi(layout=_layout(z0=0), n_vec=1) == OK and multi(n_verts=0, n_vec=1) == OK


def test_no_block_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_rings_field_multi.hip, compiled for gfx950 with the build's own
    flags: k_p1_field_rows_multi in fp64 / fp32 x mass x chunked x Q in {1, 3, 4, 6} = 16 per (real,
    record size, width); no scratch memory, at most 256 VGPRs -- read from the assembly with
    tools/kernel_regs.py."""
    import __graft_entry__ as entry

    name = "tfem_rings_field_multi.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    assert name not in entry.PER_FILE_FLAGS  # the build's plain flags, as tfem_rings_field.hip
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS.get(name, [])
    asm = tmp_path / "field_multi.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    pattern = r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)"
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm), "k_p1_field_rows_multi"],
                         check=True, capture_output=True, text=True).stdout
    rows = [re.match(pattern, line) for line in out.splitlines()]
    assert all(rows), out[-2000:]
    assert len(rows) == 2 * 16 * sum(len(w) for w in WIDTHS.values()), len(rows)
    for real in ("double", "float"):
        for slots, widths in WIDTHS.items():
            for nv in widths:
                mine = [m for m in rows if re.search(rf"<{real}, {slots}, \w+, \w+, \d, {nv}>", m.group(5))]
                assert len(mine) == 16, (real, slots, nv, len(mine))
    bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
    assert not bad, bad
