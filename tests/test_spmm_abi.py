"""tfem_csr_spmm (csrc/tfem_spmm.hip) as far as a machine without a GPU can tell: the declaration,
the export, the refusals decided on the host before any launch, the nothing-to-do cases, and the
register report of the kernels (no instance may use scratch memory)."""

import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = 1  # TFEM_ERR_INVALID_ARGUMENT


def test_header_declares_and_library_exports_the_entry_point():
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    assert re.search(r"TFEM_ERR_INVALID_ARGUMENT\s*=\s*1\b", header)
    declaration = re.search(r"^int tfem_csr_spmm\(([^;]*)\);", header, re.M)
    assert declaration, "tfem_csr_spmm is not declared in tfem_assembly.h"
    assert len(declaration.group(1).split(",")) == 10
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert "tfem_csr_spmm" in exported and hasattr(lib, "tfem_csr_spmm")
    assert len(_native.SIGNATURES["tfem_csr_spmm"][1]) == 10
    # the comment says what the entry point stands for on the reference side and states the rule
    comment = header[:declaration.start()].rsplit("/*", 1)[1]
    assert "abstract_basis.py:177-195" in comment and "bit for bit" in comment


def test_spmm_refuses_bad_arguments_without_a_device():
    """real_bytes, negative sizes, NULL arrays, overlapping x and y: decided on the host before any
    launch: no call of this test passes the host checks, on a machine with a device neither.
    Addresses only, nothing is dereferenced."""
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    base = 1 << 20
    rowptr, colind, vals, x, y = (ctypes.c_void_p(base + (1 << 16) * i) for i in range(5))

    def call(real_bytes=8, n_rows=10, n_cols=12, n_vec=4, **pointers):
        p = dict(rowptr=rowptr, x=x, y=y)
        p.update(pointers)
        status = lib.tfem_csr_spmm(p["rowptr"], colind, vals, real_bytes, n_rows, n_cols, n_vec, p["x"], p["y"], None)
        return status, lib.tfem_last_error()

    def refused(word, **kwargs):
        status, message = call(**kwargs)
        assert status == INVALID, (kwargs, status, message)
        assert word in message and b"tfem_csr_spmm" in message, message

    for real_bytes in (0, 2, 3, 16):
        refused(b"real_bytes", real_bytes=real_bytes)
    refused(b"negative", n_rows=-1)
    refused(b"negative", n_cols=-1)
    refused(b"negative", n_vec=-1)
    refused(b"negative", real_bytes=4, n_rows=-3, n_cols=-3, n_vec=-3)
    for name in ("rowptr", "x", "y"):
        refused(b"NULL", **{name: None})
        refused(b"NULL", real_bytes=4, n_vec=1, **{name: None})
    # extents: x holds n_cols * n_vec reals, y n_rows * n_vec
    at = lambda offset: ctypes.c_void_p(x.value + offset)  # noqa: E731
    refused(b"overlap", y=x)
    refused(b"overlap", y=at(12 * 4 * 8 - 8))               # y starts on the last entry of x
    refused(b"overlap", y=at(-(10 * 4 * 8 - 8)))            # y ends on the first entry of x
    refused(b"overlap", real_bytes=4, n_vec=3, y=at(12 * 3 * 4 - 4))
    refused(b"overlap", n_rows=1000, n_cols=1, n_vec=1, y=at(-800))   # x inside y
    # nothing to do: no launch, whatever the pointers
    for sizes in (dict(n_rows=0), dict(n_vec=0), dict(n_rows=0, n_cols=0, n_vec=0)):
        for real_bytes in (4, 8):
            assert call(real_bytes=real_bytes, **sizes)[0] == 0
            assert call(real_bytes=real_bytes, rowptr=None, x=None, y=None, **sizes)[0] == 0
            assert call(real_bytes=real_bytes, y=x, **sizes)[0] == 0


def test_block_matvec_on_the_host_keeps_the_column_path():
    """CPU tensors: today's path (torch's sparse product column by column), no native launch."""
    import torch

    from pytorch_fem_solver_amd.sparse import CSRMatrix

    crow = torch.tensor([0, 2, 3, 3], dtype=torch.int64)
    K = CSRMatrix(crow, torch.tensor([0, 2, 1], dtype=torch.int32), torch.tensor([2.0, -1.0, 4.0], dtype=torch.float64), (3, 3))
    X = torch.arange(6, dtype=torch.float64).reshape(3, 2)
    assert torch.equal(K.matvec(X), K.to_dense() @ X)
    with pytest.raises(ValueError, match="rows"):
        K.matvec(torch.zeros(4, 2, dtype=torch.float64))


def test_no_spmm_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_spmm.hip, compiled for gfx950 with the build's own flags: no
    scratch memory, at most 256 VGPRs (tools/kernel_regs.py on the assembly).  Two types x the
    widths 2, 4, 8 and the generic passes."""
    import __graft_entry__ as entry

    name = "tfem_spmm.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS.get(name, [])
    asm = tmp_path / "spmm.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm), "k_csr_spmm"],
                         check=True, capture_output=True, text=True).stdout
    rows = [re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)", line) for line in out.splitlines()]
    assert rows and all(rows), out[-2000:]
    bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
    assert not bad, bad
    assert len(rows) == 8, out
