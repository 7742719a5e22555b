"""The tfem_cg_* entry points (csrc/tfem_cg.hip) as far as a machine without a GPU can tell: the
declarations, the exports, the workspace size, the refusals decided on the host before any launch,
and the register report of the kernels (no instance may use scratch memory)."""

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
    "tfem_cg_workspace_bytes": 2, "tfem_cg_constant": 1, "tfem_cg_start": 8, "tfem_cg_dot": 8,
    "tfem_cg_update": 12, "tfem_cg_direction": 10,
}


def test_header_declares_and_library_exports_the_cg_entry_points():
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    assert re.search(r"#define TFEM_ERR_INVALID_ARGUMENT\s+1\b", header) or re.search(r"TFEM_ERR_INVALID_ARGUMENT\s*=\s*1\b", header)
    assert re.search(r"#define TFEM_ERR_INDEX_RANGE\s+4\b", header) or re.search(r"TFEM_ERR_INDEX_RANGE\s*=\s*4\b", header)
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(tfem_[a-z0-9_]+)\(", header, re.M))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    for name, n_args in ENTRY_POINTS.items():
        assert name in declared, f"{name} is not declared in tfem_assembly.h"
        assert name in exported and hasattr(lib, name), f"{name} is not exported"
        assert len(_native.SIGNATURES[name][1]) == n_args
    # inv_diag doubles as the mask: the header says so
    assert "inv_diag[i] == 0 marks a HELD DoF" in header


def test_workspace_size():
    from pytorch_fem_solver_amd import _native
    from pytorch_fem_solver_amd.sparse import cg_constants

    lib = _native.load()
    block, cap, per_pass = cg_constants()
    assert block == 256 and 256 <= cap <= 8 * 256 and per_pass == 8
    assert lib.tfem_cg_constant(3) == -1
    size = lib.tfem_cg_workspace_bytes
    for n in (0, 1, 65, 10**6):
        sizes = [size(n, k) for k in range(1, 18)]
        assert all(s > 0 for s in sizes), (n, sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, sizes)
        # five buffers of G x n_vec doubles, G a function of n alone and at most the cap
        grids = {s // (40 * k) for k, s in zip(range(1, 18), sizes)}
        assert len(grids) == 1 and all(s % (40 * k) == 0 for k, s in zip(range(1, 18), sizes))
        assert grids.pop() == min(max(-(-n // block), 1), cap)
    assert size(-1, 1) < 0 and size(1, -1) < 0 and size(-5, -5) < 0
    # vectors the launches refuse have no workspace either
    assert size(1 << 31, 1) < 0 and size(1 << 20, 1 << 12) < 0 and size(1, 1 << 40) < 0


def test_cg_launches_refuse_bad_arguments_without_a_device():
    """real_bytes, negative sizes, NULL arrays, vectors of 4 GiB or more: decided on the host before
    any launch: no call of this test passes the host checks, on a machine with a device neither.
    Addresses only, nothing is dereferenced."""
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    a = [ctypes.c_void_p((1 << 20) + 4096 * i) for i in range(8)]

    def calls(real_bytes, n, n_vec, step=0, null=None, only=None):
        """The four launches (`only`: those named) with the given sizes; `null`: (launch, argument
        index) to pass as NULL.  Every call made here must be one the host checks stop."""
        table = {
            "tfem_cg_start": [a[0], a[1], a[2], real_bytes, n, n_vec, a[7], None],
            "tfem_cg_dot": [a[0], a[1], a[2], real_bytes, n, n_vec, a[7], None],
            "tfem_cg_update": [a[0], a[1], a[2], a[3], a[4], a[5], real_bytes, n, n_vec, step, a[7], None],
            "tfem_cg_direction": [a[0], a[1], a[2], a[5], real_bytes, n, n_vec, step, a[7], None],
        }
        for name, args in table.items():
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
    refused(INVALID, b"negative", 8, -1, 1)
    refused(INVALID, b"negative", 4, 10, -2)
    pointers = {"tfem_cg_start": (0, 1, 2, 6), "tfem_cg_dot": (0, 1, 2, 6),
                "tfem_cg_update": (0, 1, 2, 3, 4, 5, 10), "tfem_cg_direction": (0, 1, 2, 3, 8)}
    for name, places in pointers.items():
        for place in places:
            refused(INVALID, b"NULL", 8, 10, 2, null=(name, place))
    # start and dot take no step: with valid sizes nothing would stop them, so they are not called
    refused(INVALID, b"step", 8, 10, 2, step=-1, only=("tfem_cg_update", "tfem_cg_direction"))
    refused(INDEX_RANGE, b"4 GiB", 8, 1 << 29, 1)
    refused(INDEX_RANGE, b"4 GiB", 4, 1 << 30, 1)
    refused(INDEX_RANGE, b"4 GiB", 4, 1 << 15, 1 << 15)
    refused(INDEX_RANGE, b"4 GiB", 8, 1 << 40, 1 << 40)
    refused(INDEX_RANGE, b"4 GiB", 8, 3, 1 << 33)
    # nothing to do: no launch, whatever the pointers
    for n, n_vec in ((0, 4), (7, 0), (0, 0)):
        for name, got, _ in calls(8, n, n_vec):
            assert got == 0, name
        for name, places in pointers.items():
            for _, got, _ in calls(4, n, n_vec, null=(name, places[0])):
                assert got == 0, name


def test_fused_loop_is_refused_on_cpu_tensors():
    import torch

    from pytorch_fem_solver_amd.sparse import CSRMatrix, FormOperator

    crow = torch.tensor([0, 1, 2], dtype=torch.int64)
    K = CSRMatrix(crow, torch.tensor([0, 1], dtype=torch.int32), torch.tensor([2.0, 4.0], dtype=torch.float64), (2, 2))
    b = torch.tensor([2.0, 4.0], dtype=torch.float64)
    for A in (K, FormOperator.from_csr(K, symmetric=True)):
        with pytest.raises(ValueError, match="fused"):
            A.solve_cg(b, loop="fused")
        with pytest.raises(ValueError, match="fused"):
            A.solve_cg_multi(torch.stack([b, b], dim=1), loop="fused")
        with pytest.raises(ValueError, match="loop"):
            A.solve_cg(b, loop="graph")
        # the default on the host is the loop of torch operations (a diagonal system: one iteration)
        x, it, res = A.solve_cg(b, rtol=1e-12, maxiter=1)
        assert torch.allclose(x, torch.ones(2, dtype=torch.float64)) and res <= 1e-12
        x, it, res = A.solve_cg(b, rtol=1e-12, maxiter=1, loop="torch")
        assert torch.allclose(x, torch.ones(2, dtype=torch.float64))


def test_no_cg_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_cg.hip, compiled for gfx950 with the build's own flags: no
    scratch memory, at most 256 VGPRs (tools/kernel_regs.py on the assembly).  Four kernels x two
    types x the widths 1, 2, 4, 8 and the generic passes."""
    import __graft_entry__ as entry

    name = "tfem_cg.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS.get(name, [])
    asm = tmp_path / "cg.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    for kernel in ("k_cg_start", "k_cg_dot", "k_cg_update", "k_cg_direction"):
        out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm), kernel],
                             check=True, capture_output=True, text=True).stdout
        rows = [re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)", line) for line in out.splitlines()]
        assert rows and all(rows), out[-2000:]
        bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
        assert not bad, bad
        assert len(rows) == 10, out
