"""The matrix-free P2 operator on several vectors in one launch (tfem_p2_apply_rows_multi,
csrc/tfem_p2apply_multi.hip) on a real MI355X: every column of K U BIT FOR BIT the single launch
(tfem_p2_apply_rows) on that column, row-wise against the assembled CSR and the oracle, one launch
per block, columns that do not mix, out=, block CG, the gradient, the example."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rowwise_error, scaled_error
from test_hip_p2_operator import FORMS, TOL, _case, _oracle_csr, csr_scale, form, load, p2_basis, tf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 3, 5, 9)  # an odd remainder, a remainder of one column, more columns than the widest pass
CASES = ["p2_global_n4.npz", "mixed70_q2", "mixed70_q4", "delaunay_morton", "renumbered30"]


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def oracle_apply_block(name, alpha, beta, U):
    """(K U, sum_j |K_ij U_jc|) column by column from the oracle's CSR values (assembled once)."""
    rowptr, colind, stiff, mass = _oracle_csr(name)
    n = rowptr.shape[0] - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    vals = alpha * stiff + beta * mass
    want, scale = np.empty(U.shape), np.empty(U.shape)
    for c in range(U.shape[1]):
        prod = vals * U[colind, c]
        want[:, c] = np.bincount(rows, prod, minlength=n)
        scale[:, c] = np.bincount(rows, np.abs(prod), minlength=n)
    return want, scale


def block_error(got, want, scale):
    got, want, scale = (np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float64) for a in (got, want, scale))
    assert got.shape == want.shape == scale.shape, (got.shape, want.shape, scale.shape)
    return max(rowwise_error(got[:, c], want[:, c], scale=scale[:, c]) for c in range(got.shape[1]))


def counted(lib, monkeypatch, names):
    """Counts the calls of the library's entry points; tfem_p2_apply_rows without u (the diagonal)
    is counted under "diagonal"."""
    counts = dict.fromkeys((*names, "diagonal"), 0)

    def wrap(name):
        inner = getattr(lib, name)

        def call(*args):
            if name == "tfem_p2_apply_rows" and args[9] is None:
                counts["diagonal"] += 1
            else:
                counts[name] += 1
            return inner(*args)

        monkeypatch.setattr(lib, name, call, raising=True)

    for name in names:
        wrap(name)
    return counts


SPIED = ("tfem_p2_apply_rows_multi", "tfem_p2_apply_rows", "tfem_p2_assemble_rows", "tfem_csr_spmv", "tfem_csr_spmm")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("which", list(FORMS))
def test_p2_block_is_the_single_launch_per_column_and_matches_the_csr_and_the_oracle(case, which, monkeypatch):
    alpha, beta = FORMS[which]
    mesh_np, order, _ = _case(case)
    if case == "renumbered30":
        monkeypatch.setenv("TFEM_RENUMBER", "1")
    basis = p2_basis(mesh_np, order)
    op = basis.integrate_bilinear_form(form(alpha, beta), layout="matrix_free")
    K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
    eng = basis._engine
    assert op.matrix_free is True and eng.renumbered == (case == "renumbered30")
    if case == "delaunay_morton":
        assert int(eng.p2_plan()["layout"][18]) > 100
    n, kmax = K.shape[0], max(WIDTHS)
    U = torch.tensor(np.random.default_rng(3).standard_normal((n, kmax)))
    single = torch.stack([op.matvec(U[:, j].contiguous()) for j in range(kmax)], dim=1)
    want, oscale = oracle_apply_block(case, alpha, beta, U.cpu().numpy())
    for k in WIDTHS:
        Uk = U[:, :k].contiguous()
        got = op @ Uk
        assert got.shape == (n, k) and got.dtype == torch.float64
        for j in range(k):
            assert torch.equal(got[:, j], single[:, j]), f"k = {k}: column {j} is not the single launch's"
        scale = torch.stack([csr_scale(K, Uk[:, j].contiguous()) for j in range(k)], dim=1)
        e_csr = block_error(got, K.matvec(Uk), scale)
        e_oracle = block_error(got, want[:, :k], oscale[:, :k])
        print(f"{case} {which} k = {k}: against the CSR {e_csr:.2e}, the oracle {e_oracle:.2e}")
        assert e_csr <= TOL and e_oracle <= TOL
        # a non-contiguous block (a column slice of the wider one) gives the same bits
        if k < kmax:
            assert not U[:, :k].is_contiguous() and torch.equal(op.matvec(U[:, :k]), got)


@pytest.mark.parametrize("real", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", ["mixed70_q2", "delaunay_morton"])
def test_raw_entry_point_bit_for_bit_against_the_single_launch(case, real):
    """tfem_p2_apply_rows_multi against tfem_p2_apply_rows on contiguous columns, in the engine's
    numbering, with and without mass, every width; n_vec = 1 is the single launch."""
    from pytorch_fem_solver_amd import _native

    mesh_np, order, _ = _case(case)
    torch.set_default_dtype(real)
    if real == torch.float32:
        mesh_np = {k: v.astype(np.float32) if k == "vertices" else v for k, v in mesh_np.items()}
    basis = p2_basis(mesh_np, order)
    eng = basis._engine
    rows, d = eng.p2_plan(), eng._inputs()
    colind = eng.csr_structure()[1]
    n, nnz, rb = eng.n_dofs, int(colind.shape[0]), eng.real_bytes
    assert rb == (8 if real == torch.float64 else 4) and not eng.renumbered
    lib = eng.lib
    kmax = max(WIDTHS)
    U = torch.tensor(np.random.default_rng(9).standard_normal((n, kmax)), dtype=real)
    for alpha, beta in FORMS.values():
        head = (_native.ptr(d["coords"]), rb, order, alpha, beta, _native.ptr(rows["blob"]),
                ctypes.c_void_p(rows["layout"].ctypes.data), _native.ptr(colind), nnz)
        single = torch.empty(kmax, n, dtype=real)
        for j in range(kmax):
            u = U[:, j].contiguous()
            _native.check(lib.tfem_p2_apply_rows(*head, _native.ptr(u), _native.ptr(single[j]), n, eng._stream()))
        for k in (1, *WIDTHS):
            Uk = U[:, :k].contiguous()
            Y = torch.full((n, k), float("nan"), dtype=real)
            _native.check(lib.tfem_p2_apply_rows_multi(*head, _native.ptr(Uk), _native.ptr(Y), n, k, eng._stream()))
            for j in range(k):
                assert torch.equal(Y[:, j], single[j]), f"({alpha}, {beta}) k = {k}: column {j}"
        assert bool(torch.isfinite(single).all())


def test_raw_entry_point_refusals_leave_y_untouched():
    from pytorch_fem_solver_amd import _native

    mesh_np, order, _ = _case("p2_global_n4.npz")
    basis = p2_basis(mesh_np, order)
    eng = basis._engine
    rows, d = eng.p2_plan(), eng._inputs()
    colind = eng.csr_structure()[1]
    n, nnz = eng.n_dofs, int(colind.shape[0])
    lib = eng.lib
    head = (_native.ptr(d["coords"]), 8, order, 1.0, 0.5, _native.ptr(rows["blob"]),
            ctypes.c_void_p(rows["layout"].ctypes.data))
    buf = torch.rand(2 * 3 * n)
    U, Y = buf[: 3 * n], buf[3 * n:]
    before = Y.clone()

    def call(colind_ptr, u_ptr, y_ptr, n_dofs, n_vec):
        return lib.tfem_p2_apply_rows_multi(*head, colind_ptr, nnz, u_ptr, y_ptr, n_dofs, n_vec, eng._stream())

    assert call(_native.ptr(colind), _native.ptr(U), _native.ptr(Y), n, 0) == 1 and b"n_vec" in lib.tfem_last_error()
    assert call(_native.ptr(colind), None, _native.ptr(Y), n, 3) == 1 and b"u is NULL" in lib.tfem_last_error()
    assert call(None, _native.ptr(U), _native.ptr(Y), n, 3) == 1 and b"NULL" in lib.tfem_last_error()
    # Y begins in the last column of U's block
    assert call(_native.ptr(colind), _native.ptr(U), ctypes.c_void_p(U.data_ptr() + 8 * (3 * n - 1)), n, 3) == 1
    assert b"overlap" in lib.tfem_last_error()
    assert call(_native.ptr(colind), _native.ptr(U), _native.ptr(Y), n - 1, 3) == 1 and b"DoFs" in lib.tfem_last_error()
    assert call(_native.ptr(colind), _native.ptr(U), _native.ptr(Y), n, (0xFFFFFF00 // (8 * n)) + 1) == 4
    torch.cuda.synchronize()
    assert torch.equal(Y, before)  # nothing was launched
    _native.check(call(_native.ptr(colind), _native.ptr(U), _native.ptr(Y), n, 3))  # a valid call still works
    K = basis.integrate_bilinear_form(form(1.0, 0.5), layout="csr")
    assert not eng.renumbered
    Ub = U.view(n, 3)
    scale = torch.stack([csr_scale(K, Ub[:, j].contiguous()) for j in range(3)], dim=1)
    assert block_error(Y.view(n, 3), K.matvec(Ub), scale) <= TOL


def test_a_block_is_one_launch_and_nothing_is_assembled(monkeypatch):
    mesh_np, order, _ = _case("square20")  # counter-clockwise triangles: K is positive definite, CG converges
    basis = p2_basis(mesh_np, order)
    op = basis.integrate_bilinear_form(form(1.0, 0.5), layout="matrix_free")
    n = op.shape[0]
    U = torch.rand(n, 4)
    F = torch.cat([basis.integrate_linear_form(load), 2.0 * basis.integrate_linear_form(load)], dim=1)
    free = basis._basis_parameters["inner_dofs"]
    op.diagonal()
    with monkeypatch.context() as m:
        counts = counted(basis._engine.lib, m, SPIED)
        got = op @ U
        assert got.shape == (n, 4)
        assert counts["tfem_p2_apply_rows_multi"] == 1 and counts["tfem_p2_apply_rows"] == 0, counts
        for single in (U[:, 0].contiguous(), U[:, :1].contiguous()):  # (N,) and (N, 1): the single launch
            before = dict(counts)
            out = op.matvec(single)
            assert out.shape == single.shape and torch.equal(out.reshape(-1), got[:, 0])
            assert counts["tfem_p2_apply_rows"] == before["tfem_p2_apply_rows"] + 1
            assert counts["tfem_p2_apply_rows_multi"] == before["tfem_p2_apply_rows_multi"]
        before = dict(counts)
        _, its, res = op.solve_cg_multi(F, free=free, rtol=1e-8, loop="fused")
        print(counts, its.tolist())
        assert float(res.max()) <= 1e-8
        assert counts["tfem_p2_apply_rows_multi"] - before["tfem_p2_apply_rows_multi"] >= int(its.max())
        assert counts["tfem_p2_apply_rows"] == before["tfem_p2_apply_rows"], "a single-column apply in the block loop"
        assert counts["tfem_p2_assemble_rows"] == 0 and counts["tfem_csr_spmv"] == 0 and counts["tfem_csr_spmm"] == 0
    assert op._csr is None and op.matrix_free is True


def test_columns_do_not_mix():
    """NaN in column 1: every other column keeps the bits of its single launch, column 1 is NaN
    exactly where the single launch is; the rows of vertices without elements stay 0."""
    mesh_np, order, _ = _case("delaunay_morton")
    # three vertices that no triangle uses: empty rows (k = 0)
    lone = dict(mesh_np)
    lone["vertices"] = np.concatenate([mesh_np["vertices"], [[2.0, 2.0], [2.5, 2.0], [2.0, 2.5]]])
    lone["vertex_markers"] = np.concatenate([mesh_np["vertex_markers"], np.zeros((3, 1), dtype=mesh_np["vertex_markers"].dtype)])
    n_vert = lone["vertices"].shape[0]
    basis = p2_basis(lone, order)
    op = basis.integrate_bilinear_form(form(1.0, 0.5), layout="matrix_free")
    n = op.shape[0]
    U = torch.tensor(np.random.default_rng(12).standard_normal((n, 5)))
    U[:, 1] = float("nan")
    got = op @ U
    for j in range(5):
        single = op.matvec(U[:, j].contiguous())
        if j == 1:
            assert torch.equal(torch.isnan(got[:, j]), torch.isnan(single))
            assert int(torch.isnan(single).sum()) >= n - 3
        else:
            assert torch.equal(got[:, j], single), f"column {j}"
            assert bool(torch.isfinite(got[:, j]).all())
    assert bool((got[n_vert - 3:n_vert] == 0).all()), "the rows of vertices without elements"


def test_out_is_written_in_place_and_must_not_be_u():
    mesh_np, order, _ = _case("p2_global_n4.npz")
    basis = p2_basis(mesh_np, order)
    op = basis.integrate_bilinear_form(form(2.0, 0.5), layout="matrix_free")
    eng = basis._engine
    n, k = op.shape[0], 3
    U = torch.rand(n, k)
    out = torch.full((n * k,), float("nan"))
    got = eng.apply(2.0, 0.5, U, out=out)
    assert got.shape == (n, k) and got.data_ptr() == out.data_ptr()
    assert torch.equal(out.view(n, k), op @ U)
    with pytest.raises(ValueError, match="out must not be u"):
        eng._apply_p2_rows(2.0, 0.5, U, out=U.view(-1))


@pytest.fixture(scope="module")
def cg_case():
    """square20: the operator, the CSR, three loads (the last all zero) and the single-column CSR
    solves, computed once."""
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    try:
        mesh_np, order, _ = _case("square20")
        basis = p2_basis(mesh_np, order)
        op = basis.integrate_bilinear_form(form(1.0, 1.0), layout="matrix_free")
        K = basis.integrate_bilinear_form(form(1.0, 1.0), layout="csr")
        free = basis._basis_parameters["inner_dofs"]
        f = basis.integrate_linear_form(load)
        B = torch.cat([f, torch.randn(K.shape[0], 1, generator=torch.Generator(device="cuda").manual_seed(3)),
                       torch.zeros_like(f)], dim=1)
        singles = [K.solve_cg(B[:, c].contiguous(), free=free, rtol=1e-10) for c in (0, 1)]
    finally:
        torch.set_default_device("cpu")
        torch.set_default_dtype(torch.float32)
    return basis, op, K, free, B, singles


@pytest.mark.parametrize("loop", ("fused", "torch"))
def test_block_cg_on_the_p2_operator_against_the_single_csr_solves(cg_case, loop, monkeypatch):
    basis, op, K, free, B, singles = cg_case
    with monkeypatch.context() as m:
        counts = counted(basis._engine.lib, m, SPIED)
        X, its, ress = op.solve_cg_multi(B, free=free, rtol=1e-10, loop=loop)
    print(loop, counts, its.tolist())
    assert counts["tfem_p2_apply_rows"] == 0 and counts["tfem_csr_spmm"] == 0 and counts["tfem_csr_spmv"] == 0
    assert counts["tfem_p2_apply_rows_multi"] >= int(its.max())
    assert X.shape == B.shape and bool(torch.isfinite(X).all())
    assert int(its[2]) == 0 and float(ress[2]) == 0.0 and bool((X[:, 2] == 0).all())
    for c in (0, 1):
        x, it, res = singles[c]
        err = scaled_error(X[:, c].cpu(), x.cpu())
        print(f"{loop}, column {c}: scaled error {err:.3e}, iterations {int(its[c])} / {it}, residual {float(ress[c]):.3e}")
        assert err <= 1e-8 and float(ress[c]) <= 1e-10


def test_gradient_of_a_block_is_k_g(cg_case):
    """(op @ U * G).sum().backward(): dL/dU = K^T G = K G, through the block launch."""
    basis, op, K, free, B, singles = cg_case
    n = op.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(21)
    U = torch.randn(n, 3, generator=gen).requires_grad_(True)
    G = torch.randn(n, 3, generator=gen)
    ((op @ U) * G).sum().backward()
    scale = torch.stack([csr_scale(K, G[:, j].contiguous()) for j in range(3)], dim=1)
    err = block_error(U.grad, K.matvec(G), scale)
    print(f"gradient of the block against K G: {err:.2e}")
    assert err <= TOL


def test_p2_operator_loads_example_runs():
    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_p2_operator_loads.py"), "40"],
                          capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "matrix-free, P2 rows" in done.stdout, "the example prints the operator it solved with"
