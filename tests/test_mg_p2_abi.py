"""The tfem_mg_p2_* entry points (csrc/tfem_mg.hip, the P2 kind of its transfers) as far as a machine
without a GPU can tell: the declarations, the exports and the refusals decided on the host before
any launch.  The register report of their kernels is in tests/test_mg_abi.py."""

import ctypes
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, INDEX_RANGE = 1, 4  # TFEM_ERR_INVALID_ARGUMENT, TFEM_ERR_INDEX_RANGE

ENTRY_POINTS = {"tfem_mg_p2_restrict_residual": 11, "tfem_mg_p2_prolong_add": 8}  # arguments


def test_header_declares_and_library_exports_the_p2_entry_points():
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(tfem_[a-z0-9_]+)\(", header, re.M))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    for name, n_args in ENTRY_POINTS.items():
        assert name in declared, f"{name} is not declared in tfem_assembly.h"
        assert name in exported and hasattr(lib, name), f"{name} is not exported"
        assert len(_native.SIGNATURES[name][1]) == n_args
        declaration = re.search(rf"^int {name}\(([^;]*)\);", header, re.M | re.S).group(1)
        assert len(declaration.split(",")) == n_args


def test_p2_multigrid_is_exported_by_the_packages():
    import pytorch_fem_solver_amd
    import torch_fem

    assert torch_fem.P2Multigrid is pytorch_fem_solver_amd.P2Multigrid
    assert "P2Multigrid" in pytorch_fem_solver_amd.__all__ and "P2Multigrid" in torch_fem.__all__


def test_p2_launches_refuse_bad_arguments_without_a_device():
    """real_bytes, negative sizes, n_f < n_v, NULL arrays, an output that overlaps an input, arrays
    of 4 GiB or more: decided on the host before any launch -- no call of this test passes the host
    checks, on a machine with a device neither.  Addresses only, nothing is dereferenced."""
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    # 8 GiB apart: no two arrays of a refusal below that is not about overlap overlap
    a = [ctypes.c_void_p((1 << 40) + (1 << 33) * i) for i in range(8)]

    def args_of(name, real_bytes, n_v, n_f):
        return {
            "tfem_mg_p2_restrict_residual": [a[0], a[1], a[2], a[3], a[4], a[5], a[6], real_bytes, n_v, n_f, None],
            "tfem_mg_p2_prolong_add": [a[0], a[1], a[2], a[3], real_bytes, n_v, n_f, None],
        }[name]

    def refused(status, word, name, args):
        got, message = getattr(lib, name)(*args), lib.tfem_last_error()
        assert got == status, (name, got, message)
        assert word in message, message
        if status == INVALID:  # the extent check names the kernels, not the entry point
            assert name.encode() in message, message

    for name in ENTRY_POINTS:
        refused(INVALID, b"real_bytes", name, args_of(name, 3, 10, 30))
        refused(INVALID, b"real_bytes", name, args_of(name, 0, 10, 30))
        refused(INVALID, b"negative", name, args_of(name, 8, -1, 10))
        refused(INVALID, b"negative", name, args_of(name, 4, 10, -2))
        refused(INVALID, b"n_f < n_v", name, args_of(name, 8, 10, 9))
        refused(INVALID, b"n_f < n_v", name, args_of(name, 4, 1, 0))
        # 4 GiB or more in one array: the fine vectors, the coarse vector with them, the edge tables
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 16, 1 << 29))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 16, 1 << 30))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 16, 1 << 62))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 1 << 29, 1 << 29))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 1 << 61, 1 << 62))
        # 2 n_e int32 of idx / edge_vertices: 2^29 edges are 4 GiB of table, and 2 GiB of float32
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 16, 16 + (1 << 29)))

    # NULL arrays that would be read or written (the masks may be NULL: all ones)
    required = {"tfem_mg_p2_restrict_residual": (0, 1, 4, 5, 6), "tfem_mg_p2_prolong_add": (0, 2, 3)}
    for name, places in required.items():
        for place in places:
            args = args_of(name, 8, 10, 30)
            args[place] = None
            refused(INVALID, b"NULL", name, args)

    # the output overlapping an input, by one entry or by one byte: n_v = 10, n_f = 30, 20 edges
    def length(name, place, real_bytes):
        ints = {"tfem_mg_p2_restrict_residual": {0: 11 * 4, 1: 40 * 4, 2: 10 * real_bytes},
                "tfem_mg_p2_prolong_add": {0: 40 * 4, 2: 10 * real_bytes}}
        return ints[name].get(place, 30 * real_bytes)

    def overlapping(name, out, place, out_entries, real_bytes):
        args = args_of(name, real_bytes, 10, 30)
        args[place] = ctypes.c_void_p(args[out].value + (out_entries - 1) * real_bytes)
        refused(INVALID, b"overlap", name, args)
        args[place] = ctypes.c_void_p(args[out].value - length(name, place, real_bytes) + 1)
        refused(INVALID, b"overlap", name, args)

    for real_bytes in (4, 8):
        for place in (0, 1, 2, 3, 4, 5):
            overlapping("tfem_mg_p2_restrict_residual", 6, place, 10, real_bytes)  # r_c: n_v entries
        for place in (0, 1, 2):
            overlapping("tfem_mg_p2_prolong_add", 3, place, 30, real_bytes)  # x_f: n_f entries

    # nothing to do: no launch, whatever the pointers
    assert lib.tfem_mg_p2_restrict_residual(None, None, None, None, None, None, None, 4, 0, 7, None) == 0
    assert lib.tfem_mg_p2_prolong_add(None, None, None, None, 8, 0, 7, None) == 0
    assert lib.tfem_mg_p2_prolong_add(None, None, None, None, 8, 0, 0, None) == 0
