"""The tfem_mg_*_multi entry points (csrc/tfem_mg.hip) as far as a machine without a GPU can tell,
after tests/test_mg_abi.py: the declarations, the exports and the refusals decided on the host
before any launch.  The register report of their kernels is in tests/test_mg_abi.py."""

import ctypes
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, INDEX_RANGE = 1, 4  # TFEM_ERR_INVALID_ARGUMENT, TFEM_ERR_INDEX_RANGE

ENTRY_POINTS = {"tfem_mg_smooth_multi": 9, "tfem_mg_restrict_residual_multi": 12,
                "tfem_mg_prolong_add_multi": 9}  # arguments


def test_header_declares_and_library_exports_the_mg_multi_entry_points():
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


def test_mg_multi_launches_refuse_bad_arguments_without_a_device():
    """real_bytes, negative sizes, n_vec < 1, NULL arrays, an output that overlaps an input anywhere
    in its n x n_vec extent, blocks of 4 GiB or more: decided on the host before any launch -- no
    call of this test passes the host checks, on a machine with a device neither.  Addresses only,
    nothing is dereferenced."""
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    # 8 GiB apart: no two arrays of a refusal below that is not about overlap overlap
    a = [ctypes.c_void_p((1 << 40) + (1 << 33) * i) for i in range(8)]

    def args_of(name, real_bytes, n, m, n_vec, first=0):
        """smooth: n rows; restrict: n_c = n, n_f = m; prolong: n_f = n, n_c = m."""
        return {
            "tfem_mg_smooth_multi": [a[0], a[1], a[2], a[3], real_bytes, n, n_vec, first, None],
            "tfem_mg_restrict_residual_multi": [a[0], a[1], a[2], a[3], a[4], a[5], a[6], real_bytes, n, m, n_vec, None],
            "tfem_mg_prolong_add_multi": [a[0], a[1], a[2], a[3], real_bytes, n, m, n_vec, None],
        }[name]

    def refused(status, word, name, args):
        got, message = getattr(lib, name)(*args), lib.tfem_last_error()
        assert got == status, (name, got, message)
        assert word in message, message
        if status == INVALID:  # the extent check names the kernels, not the entry point
            assert name.encode() in message, message

    smooth = "tfem_mg_smooth_multi"
    for name in ENTRY_POINTS:
        for n_vec in (2, 3):
            refused(INVALID, b"real_bytes", name, args_of(name, 3, 10, 10, n_vec))
            refused(INVALID, b"real_bytes", name, args_of(name, 0, 10, 10, n_vec))
            refused(INVALID, b"negative", name, args_of(name, 8, -1, 10, n_vec))
            if name != smooth:
                refused(INVALID, b"negative", name, args_of(name, 4, 10, -2, n_vec))
        for n_vec in (0, -1, -(1 << 40)):
            refused(INVALID, b"n_vec", name, args_of(name, 8, 10, 10, n_vec))
            refused(INVALID, b"n_vec", name, args_of(name, 8, 0, 0, n_vec))
        # 4 GiB or more in one block through the rows alone, as for the single launches ...
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 1 << 29, 16, 2))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 1 << 62, 16, 2))
        # ... and reached only through n_vec: 2^26 rows of doubles are 512 MiB, of 8 doubles 4 GiB
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 1 << 26, 16, 8))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 1 << 26, 16, 16))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 3, 16, (1 << 32) // 12 + 1))
        refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 16, 16, 1 << 62))
        if name != smooth:
            refused(INDEX_RANGE, b"32-bit", name, args_of(name, 8, 16, 1 << 26, 8))
            refused(INDEX_RANGE, b"32-bit", name, args_of(name, 4, 16, 1 << 61, 2))

    # NULL arrays that would be read or written (the masks may be NULL: all ones)
    required = {smooth: (0, 1, 2, 3), "tfem_mg_restrict_residual_multi": (0, 1, 4, 5, 6),
                "tfem_mg_prolong_add_multi": (0, 2, 3)}
    for name, places in required.items():
        for place in places:
            args = args_of(name, 8, 10, 10, 3)
            args[place] = None
            refused(INVALID, b"NULL", name, args)
    # the first sweep does not read ax, but the other arrays
    for place in (0, 1, 3):
        args = args_of(smooth, 8, 10, 0, 2, first=1)
        args[place] = None
        refused(INVALID, b"NULL", smooth, args)

    # The output overlapping an input by one entry, at the far end of the output's n x n_vec extent
    # (outside its first column and outside the n entries of a single vector) and at its start.
    n, n_vec = 10, 4

    def input_bytes(name, place, real_bytes):
        """The extent of the input at `place`: a block, one entry per DoF, or a table."""
        per_dof = {smooth: {3: n}, "tfem_mg_restrict_residual_multi": {2: n, 3: n}, "tfem_mg_prolong_add_multi": {1: n}}
        ints = {"tfem_mg_restrict_residual_multi": {0: (n + 1) * 4, 1: 2 * n * 4}, "tfem_mg_prolong_add_multi": {0: 2 * n * 4}}
        if place in ints.get(name, {}):
            return ints[name][place]
        return per_dof[name].get(place, n * n_vec) * real_bytes

    def overlapping(name, out, place, real_bytes=8):
        args = args_of(name, real_bytes, n, n, n_vec)
        last = (n * n_vec - 1) * real_bytes
        assert last >= n * real_bytes  # beyond what the single launch would call the output
        args[place] = ctypes.c_void_p(args[out].value + last)
        refused(INVALID, b"overlap", name, args)
        args[place] = ctypes.c_void_p(args[out].value - input_bytes(name, place, real_bytes) + 1)
        refused(INVALID, b"overlap", name, args)

    for place in (1, 2, 3):
        overlapping(smooth, 0, place)
    for place in (0, 1, 2, 3, 4, 5):
        overlapping("tfem_mg_restrict_residual_multi", 6, place, 4)
    for place in (0, 1, 2):
        overlapping("tfem_mg_prolong_add_multi", 3, place)
    # the first sweep reads b and w as well: x = b is refused there too
    args = args_of(smooth, 8, 10, 0, 3, first=1)
    args[1] = args[0]
    refused(INVALID, b"overlap", smooth, args)

    # nothing to do: no launch, whatever the pointers (n_vec = 1 forwards to the single launch)
    for n_vec in (1, 3, 8):
        assert lib.tfem_mg_smooth_multi(None, None, None, None, 8, 0, n_vec, 0, None) == 0
        assert lib.tfem_mg_restrict_residual_multi(None, None, None, None, None, None, None, 4, 0, 7, n_vec, None) == 0
        assert lib.tfem_mg_prolong_add_multi(None, None, None, None, 8, 0, 7, n_vec, None) == 0
    # n_vec = 1 IS the single launch: its refusals carry the single entry point's name
    assert lib.tfem_mg_smooth_multi(a[0], a[0], a[2], a[3], 8, 10, 1, 0, None) == INVALID
    assert b"tfem_mg_smooth:" in lib.tfem_last_error()
