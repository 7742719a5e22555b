"""The tfem_pcg_* entry points (csrc/tfem_pcg.hip) as far as a machine without a GPU can tell: the
declarations, the exports, the refusals decided on the host before any launch, and the register
report of the kernels (no instance may use scratch memory).  In the manner of tests/test_cg_abi.py,
whose launches these share their checks, workspace and helpers (csrc/tfem_cg.hpp) with."""

import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, INDEX_RANGE = 1, 4  # TFEM_ERR_INVALID_ARGUMENT, TFEM_ERR_INDEX_RANGE

ENTRY_POINTS = {  # name -> number of arguments
    "tfem_pcg_start": 9, "tfem_pcg_update": 12, "tfem_pcg_rz": 9, "tfem_pcg_direction": 10,
}
#: the positions of the arrays (the workspace included) among the arguments
POINTERS = {"tfem_pcg_start": (0, 1, 2, 3, 7), "tfem_pcg_update": (0, 1, 2, 3, 4, 5, 10),
            "tfem_pcg_rz": (0, 1, 2, 7), "tfem_pcg_direction": (0, 1, 2, 3, 8)}
WITH_STEP = ("tfem_pcg_update", "tfem_pcg_rz", "tfem_pcg_direction")


def test_header_declares_and_library_exports_the_pcg_entry_points():
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
        # the declaration has as many parameters as the binding
        text = re.search(rf"^int {name}\((.*?)\);", header, re.M | re.S).group(1)
        assert len(text.split(",")) == n_args, (name, text)
    # the mask stands where inv_diag stands: the header says so
    assert "mask[i] == 0 marks a HELD DoF" in header


def test_pcg_launches_refuse_bad_arguments_without_a_device():
    """real_bytes, negative sizes and steps, NULL arrays, vectors of 4 GiB or more: decided on the
    host before any launch, with the codes of tfem_cg_*: no call of this test passes the host checks,
    on a machine with a device neither.  Addresses only, nothing is dereferenced."""
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    a = [ctypes.c_void_p((1 << 20) + 4096 * i) for i in range(8)]

    def calls(real_bytes, n, n_vec, step=0, null=None, only=None):
        """The four launches (`only`: those named) with the given sizes; `null`: (launch, argument
        index) to pass as NULL.  Every call made here must be one the host checks stop."""
        table = {
            "tfem_pcg_start": [a[0], a[1], a[2], a[3], real_bytes, n, n_vec, a[7], None],
            "tfem_pcg_update": [a[0], a[1], a[2], a[3], a[4], a[5], real_bytes, n, n_vec, step, a[7], None],
            "tfem_pcg_rz": [a[0], a[1], a[2], real_bytes, n, n_vec, step, a[7], None],
            "tfem_pcg_direction": [a[0], a[1], a[2], a[5], real_bytes, n, n_vec, step, a[7], None],
        }
        for name, args in table.items():
            assert len(args) == ENTRY_POINTS[name]
            if only is not None and name not in only:
                continue
            if null is not None:
                if null[0] != name:
                    continue
                args[null[1]] = None
            yield name, getattr(lib, name)(*args), lib.tfem_last_error()

    def refused(status, word, *args, **kwargs):
        seen = list(calls(*args, **kwargs))
        assert seen
        for name, got, message in seen:
            assert got == status, (name, got, message)
            assert word in message and name.encode() in message, message

    refused(INVALID, b"real_bytes", 3, 10, 1)
    refused(INVALID, b"real_bytes", 0, 10, 1)
    refused(INVALID, b"real_bytes", 16, 10, 1)
    refused(INVALID, b"negative", 8, -1, 1)
    refused(INVALID, b"negative", 4, 10, -2)
    for name, places in POINTERS.items():
        for place in places:
            refused(INVALID, b"NULL", 8, 10, 2, null=(name, place))
    # start takes no step: with valid sizes nothing would stop it, so it is not called
    refused(INVALID, b"step", 8, 10, 2, step=-1, only=WITH_STEP)
    refused(INVALID, b"step", 4, 10, 3, step=-(1 << 40), only=WITH_STEP)
    refused(INDEX_RANGE, b"4 GiB", 8, 1 << 29, 1)
    refused(INDEX_RANGE, b"4 GiB", 4, 1 << 30, 1)
    refused(INDEX_RANGE, b"4 GiB", 4, 1 << 15, 1 << 15)
    refused(INDEX_RANGE, b"4 GiB", 8, 1 << 40, 1 << 40)
    refused(INDEX_RANGE, b"4 GiB", 8, 3, 1 << 33)
    # nothing to do: no launch, whatever the pointers
    for n, n_vec in ((0, 4), (7, 0), (0, 0)):
        for name, got, _ in calls(8, n, n_vec):
            assert got == 0, name
        for name, places in POINTERS.items():
            for _, got, _ in calls(4, n, n_vec, null=(name, places[0])):
                assert got == 0, name


def test_fused_loop_refuses_an_unknown_read(monkeypatch):
    """The form of the host read is checked before anything else is touched: no device needed."""
    from pytorch_fem_solver_amd import multigrid

    assert multigrid._PCG_READ in (None, "drain", "overlap") and multigrid._PCG_OVERLAP_WIDTHS >= 0
    monkeypatch.setattr(multigrid, "_PCG_READ", "poll")
    with pytest.raises(ValueError, match="_PCG_READ"):
        multigrid._fused_cycle_pcg(None, None, None, None, None, None, None, None, None, None, 1e-10, 1)


def test_no_pcg_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_pcg.hip, compiled for gfx950 with the build's own flags: no
    scratch memory, at most 256 VGPRs (tools/kernel_regs.py on the assembly).  Four kernels x two
    types x the widths 1, 2, 4, 8 and the generic passes."""
    import __graft_entry__ as entry

    name = "tfem_pcg.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS.get(name, [])
    asm = tmp_path / "pcg.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    for kernel in ("k_pcg_start", "k_pcg_update", "k_pcg_rz", "k_pcg_direction"):
        out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm), kernel],
                             check=True, capture_output=True, text=True).stdout
        rows = [re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)", line) for line in out.splitlines()]
        assert rows and all(rows), out[-2000:]
        bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
        assert not bad, bad
        assert len(rows) == 10, out
