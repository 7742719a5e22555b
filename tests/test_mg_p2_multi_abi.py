"""The tfem_mg_p2_*_multi entry points (csrc/tfem_mg.hip, the P2 kind of its transfers) as far as a
machine without a GPU can tell, after tests/test_mg_p2_abi.py and tests/test_mg_multi_abi.py: the
declarations, the exports and the refusals decided on the host before any launch.  The register
report of their kernels is in tests/test_mg_abi.py."""

import ctypes
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, INDEX_RANGE = 1, 4  # TFEM_ERR_INVALID_ARGUMENT, TFEM_ERR_INDEX_RANGE

RESTRICT, PROLONG = "tfem_mg_p2_restrict_residual_multi", "tfem_mg_p2_prolong_add_multi"
ENTRY_POINTS = {RESTRICT: 12, PROLONG: 9}  # arguments


def test_header_declares_and_library_exports_the_p2_multi_entry_points():
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
        assert "int64_t n_vec" in declaration
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in integration, f"{name} is not in the entry-point list of INTEGRATION.md"


def test_p2_multi_launches_refuse_bad_arguments_without_a_device():
    """real_bytes, negative sizes, n_f < n_v, n_vec < 1, NULL arrays, an output that overlaps an
    input anywhere in its n x n_vec extent, blocks of 4 GiB or more: decided on the host before any
    launch -- no call of this test passes the host checks, on a machine with a device neither.
    Addresses only, nothing is dereferenced."""
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    # 8 GiB apart: no two arrays of a refusal below that is not about overlap overlap
    a = [ctypes.c_void_p((1 << 40) + (1 << 33) * i) for i in range(8)]

    def args_of(name, real_bytes, n_v, n_f, n_vec):
        return {
            RESTRICT: [a[0], a[1], a[2], a[3], a[4], a[5], a[6], real_bytes, n_v, n_f, n_vec, None],
            PROLONG: [a[0], a[1], a[2], a[3], real_bytes, n_v, n_f, n_vec, None],
        }[name]

    def refused(status, word, name, args):
        got, message = getattr(lib, name)(*args), lib.tfem_last_error()
        assert got == status, (name, got, message)
        assert word in message, message
        if status == INVALID:  # the extent check names the kernels, not the entry point
            assert name.encode() + b":" in message, message

    for name in ENTRY_POINTS:
        for n_vec in (2, 3):
            refused(INVALID, b"real_bytes", name, args_of(name, 3, 10, 30, n_vec))
            refused(INVALID, b"real_bytes", name, args_of(name, 0, 10, 30, n_vec))
            refused(INVALID, b"negative", name, args_of(name, 8, -1, 10, n_vec))
            refused(INVALID, b"negative", name, args_of(name, 4, 10, -2, n_vec))
            refused(INVALID, b"n_f < n_v", name, args_of(name, 8, 10, 9, n_vec))
            refused(INVALID, b"n_f < n_v", name, args_of(name, 4, 1, 0, n_vec))
        for n_vec in (0, -1, -(1 << 40)):
            refused(INVALID, b"n_vec", name, args_of(name, 8, 10, 30, n_vec))
            refused(INVALID, b"n_vec", name, args_of(name, 8, 0, 0, n_vec))
        # 4 GiB or more in one block through the rows alone, as for the single launches ...
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 16, 1 << 29, 2))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 16, 1 << 62, 2))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 1 << 29, 1 << 29, 2))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 1 << 61, 1 << 62, 2))
        # ... the edge tables: 2^29 edges are 4 GiB of idx / edge_vertices ...
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 16, 16 + (1 << 29), 2))
        # ... and reached only through n_vec, n_f * real_bytes small: 2^26 rows of doubles are
        # 512 MiB, of 8 doubles 4 GiB; 48 bytes of a row times 2^32 / 12 + 1 columns
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 16, 1 << 26, 8))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 16, 1 << 26, 16))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 1, 3, (1 << 32) // 12 + 1))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 16, 48, 1 << 62))

    # NULL arrays that would be read or written (the masks may be NULL: all ones)
    required = {RESTRICT: (0, 1, 4, 5, 6), PROLONG: (0, 2, 3)}
    for name, places in required.items():
        for place in places:
            args = args_of(name, 8, 10, 30, 3)
            args[place] = None
            refused(INVALID, b"NULL", name, args)

    # The output overlapping an input by one byte: at the far end of the output's n x n_vec extent
    # (outside the n entries of a single vector) and at its start.  n_v = 10, n_f = 30, 20 edges.
    n_v, n_f, n_vec = 10, 30, 4

    def input_bytes(name, place, real_bytes):
        """The extent of the input at `place`: a table, one entry per DoF, or a block."""
        sizes = {RESTRICT: {0: (n_v + 1) * 4, 1: 2 * (n_f - n_v) * 4, 2: n_v * real_bytes, 3: n_f * real_bytes},
                 PROLONG: {0: 2 * (n_f - n_v) * 4, 1: n_f * real_bytes, 2: n_v * n_vec * real_bytes}}
        return sizes[name].get(place, n_f * n_vec * real_bytes)

    def overlapping(name, out, place, out_rows, real_bytes):
        args = args_of(name, real_bytes, n_v, n_f, n_vec)
        last = (out_rows * n_vec - 1) * real_bytes
        assert last >= out_rows * real_bytes  # beyond what the single launch would call the output
        args[place] = ctypes.c_void_p(args[out].value + last)
        refused(INVALID, b"overlap", name, args)
        args[place] = ctypes.c_void_p(args[out].value - input_bytes(name, place, real_bytes) + 1)
        refused(INVALID, b"overlap", name, args)

    for real_bytes in (4, 8):
        for place in (0, 1, 2, 3, 4, 5):
            overlapping(RESTRICT, 6, place, n_v, real_bytes)  # r_c: n_v rows
        for place in (0, 1, 2):
            overlapping(PROLONG, 3, place, n_f, real_bytes)  # x_f: n_f rows

    # nothing to do: no launch, whatever the pointers (n_vec = 1 forwards to the single launch)
    for n_vec in (1, 3, 8):
        assert lib.tfem_mg_p2_restrict_residual_multi(None, None, None, None, None, None, None, 4, 0, 7, n_vec, None) == 0
        assert lib.tfem_mg_p2_prolong_add_multi(None, None, None, None, 8, 0, 7, n_vec, None) == 0
        assert lib.tfem_mg_p2_prolong_add_multi(None, None, None, None, 8, 0, 0, n_vec, None) == 0
    # n_vec = 1 IS the single launch: its refusals carry the single entry point's name
    assert lib.tfem_mg_p2_prolong_add_multi(a[0], a[1], a[2], a[2], 8, 10, 30, 1, None) == INVALID
    assert b"tfem_mg_p2_prolong_add:" in lib.tfem_last_error()
