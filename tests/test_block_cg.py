"""conjugate_gradients_multi (sparse.py): Jacobi-preconditioned CG on k columns at once, on CPU
tensors with a dense SPD matvec; and the register report of the multi-vector apply kernels
(csrc/tfem_rings_apply.hip compiled for gfx950: no instance may use scratch memory)."""

import os
import re
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
CHECK = 25  # the residual is checked every 25 iterations: the margin between two CG runs


def _laplacian_2d(m):
    """Dense 5-point Laplacian on an m x m grid plus 0.01 I: SPD, condition ~ m^2."""
    n = m * m
    A = torch.zeros(n, n, dtype=torch.float64)
    idx = torch.arange(n).reshape(m, m)
    A[idx.reshape(-1), idx.reshape(-1)] = 4.01
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        A[a.reshape(-1), b.reshape(-1)] = -1.0
        A[b.reshape(-1), a.reshape(-1)] = -1.0
    # rows scaled differently, so that the Jacobi preconditioner does something
    s = 1.0 + torch.arange(n, dtype=torch.float64) % 7
    return s[:, None] * A * s[None, :]


def _system():
    from pytorch_fem_solver_amd.sparse import conjugate_gradients, conjugate_gradients_multi

    # a 12 x 12 block that nothing couples to the grid: a right-hand side inside it converges
    # within 12 iterations (first check), the grid's columns need several checks
    ns = 12
    small = 3.0 * torch.eye(ns, dtype=torch.float64)
    small[torch.arange(ns - 1), torch.arange(1, ns)] = -1.0
    small[torch.arange(1, ns), torch.arange(ns - 1)] = -1.0
    A = torch.block_diag(small, _laplacian_2d(24))
    n = A.shape[0]
    g = torch.Generator().manual_seed(11)
    smooth = torch.zeros(n, dtype=torch.float64)
    smooth[:ns] = torch.linspace(1.0, 2.0, ns, dtype=torch.float64)
    B = torch.stack([
        smooth,
        torch.randn(n, dtype=torch.float64, generator=g),
        torch.zeros(n, dtype=torch.float64),               # the all-zero column
        1e6 * torch.randn(n, dtype=torch.float64, generator=g),
        torch.eye(n, dtype=torch.float64)[n // 2],         # one point load
    ], dim=1)
    return A, B, conjugate_gradients, conjugate_gradients_multi


def _check_columns(A, B, X, its, res, single, free=None, X0=None):
    n, k = B.shape
    assert X.shape == (n, k) and its.shape == (k,) and res.shape == (k,)
    assert torch.isfinite(X).all() and torch.isfinite(res).all()
    mask = torch.ones(n, dtype=torch.float64)
    if free is not None:
        mask.zero_()
        mask[free] = 1
    for j in range(k):
        b = B[:, j]
        true = torch.linalg.vector_norm(mask * (b - A @ X[:, j]))
        b_norm = torch.linalg.vector_norm(mask * b).clamp_min(torch.finfo(torch.float64).tiny)
        print(f"column {j}: {int(its[j])} iterations, reported {float(res[j]):.3e}, true {float(true / b_norm):.3e}")
        assert float(true / b_norm) <= RTOL
        x0 = None if X0 is None else X0[:, j]
        x1, it1, res1 = single(lambda v: A @ v, A.diagonal(), b, free, x0, RTOL)
        assert abs(int(its[j]) - it1) <= CHECK, (j, int(its[j]), it1)
        assert float(res[j]) <= RTOL
        scale = x1.abs().max().clamp_min(1e-300)
        assert float((X[:, j] - x1).abs().max() / scale) <= 1e-6


def test_columns_with_different_convergence_and_a_zero_column():
    A, B, single, multi = _system()
    X, its, res = multi(lambda V: A @ V, A.diagonal(), B, None, None, RTOL)
    _check_columns(A, B, X, its, res, single)
    assert int(its[2]) == 0 and float(res[2]) == 0.0 and torch.equal(X[:, 2], torch.zeros(A.shape[0], dtype=torch.float64))
    # the columns do converge at different checks: the frozen ones must not move afterwards
    assert len({int(i) for i in its}) >= 3


def test_free_mask_and_nonzero_start():
    A, B, single, multi = _system()
    n = A.shape[0]
    free = torch.arange(n)[torch.arange(n) % 5 != 0]
    g = torch.Generator().manual_seed(5)
    X0 = torch.randn(n, B.shape[1], dtype=torch.float64, generator=g)
    X0[:, 2] = 0.0
    # the masked problem: the DoFs outside `free` keep X0's values
    X, its, res = multi(lambda V: A @ V, A.diagonal(), B, free, X0, RTOL)
    _check_columns(A, B, X, its, res, single, free, X0)
    fixed = torch.ones(n, dtype=torch.bool)
    fixed[free] = False
    assert torch.equal(X[fixed], X0[fixed])
    # a zero right-hand side with a zero start stays zero and reports no iteration
    assert int(its[2]) == 0 and not X[:, 2].any()


def test_single_column_block_and_maxiter():
    A, B, single, multi = _system()
    X, its, res = multi(lambda V: A @ V, A.diagonal(), B[:, :1], None, None, RTOL)
    x1, it1, _ = single(lambda v: A @ v, A.diagonal(), B[:, 0], None, None, RTOL)
    assert X.shape == (A.shape[0], 1) and abs(int(its[0]) - it1) <= CHECK
    # maxiter ends the loop for every column that still runs; nothing becomes NaN
    X, its, res = multi(lambda V: A @ V, A.diagonal(), B, None, None, RTOL, maxiter=7)
    assert torch.isfinite(X).all() and its.tolist() == [7, 7, 0, 7, 7] and float(res[1]) > RTOL
    with pytest.raises(ValueError):
        multi(lambda V: A @ V, A.diagonal(), B[:, 0], None, None, RTOL)


def test_no_apply_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_rings_apply.hip, compiled for gfx950 with the build's own flags:
    no scratch memory, at most 256 VGPRs (tools/kernel_regs.py on the assembly).  The multi-vector
    kernels: 2 types x mass x chunked x (widths 2, 4 for both record sizes, 8 for 7 slots), and the long rows."""
    import __graft_entry__ as entry

    name = "tfem_rings_apply.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS.get(name, [])
    asm = tmp_path / "apply.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    counts = {}
    for kernel in ("k_p1_apply_rows_multi", "k_p1_apply_long_rows_multi", "k_p1_apply_rows", "k_p1_apply_long_rows"):
        out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm), kernel],
                             check=True, capture_output=True, text=True).stdout
        rows = [re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)", line) for line in out.splitlines()]
        assert rows and all(rows), out[-2000:]
        bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
        assert not bad, bad
        counts[kernel] = len(rows)
    print(counts)
    # widths 2 and 4 for both record sizes, 8 for the 7-slot records
    assert counts["k_p1_apply_rows_multi"] == 2 * 2 * 2 * (2 * 2 + 1)
    assert counts["k_p1_apply_long_rows_multi"] == 4
