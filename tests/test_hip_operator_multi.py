"""The matrix-free P1 operator on several vectors at once (tfem_p1_apply_rings_multi,
k_p1_apply_rows_multi in csrc/tfem_rings_apply.hip) on a real MI355X: every column of K U against
the oracle, the assembled CSR operator and the single-vector launch; the C ABI; the operators that
serve (N, k) by one launch per column; the gradient; block CG."""

import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, mesh_from_golden, rowwise_error, scaled_error
from oracle import assembly_oracle as orc
from test_hip_operator import FORMS, TOL, _case, csr_scale, form, load, tf

pytestmark = pytest.mark.gpu

WIDTHS = (2, 3, 4, 5, 8, 11)  # odd counts and counts above one pass on purpose


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def oracle_apply_block(mesh_np, alpha, beta, U):
    """(K U, sum_j |K_ij U_jc|) column by column from the oracle's CSR values (assembled once)."""
    verts, tris = mesh_np["vertices"], mesh_np["triangles"]
    n = verts.shape[0]
    rowptr, colind, slots = orc.csr_pattern(tris, n)
    vals = np.zeros(colind.shape[0])
    for name, c in (("stiffness", alpha), ("mass", beta)):
        if c:
            local, _ = orc.p1_assemble(verts, tris, 3, name)
            vals += c * orc.assemble_csr_values(local, slots, colind.shape[0])
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    want, scale = np.empty(U.shape), np.empty(U.shape)
    for c in range(U.shape[1]):
        prod = vals * U[colind, c]
        want[:, c] = np.bincount(rows, prod, minlength=n)
        scale[:, c] = np.bincount(rows, np.abs(prod), minlength=n)
    return want, scale


def block_error(got, want, scale):
    """The largest row-wise error over the columns; printed before anything is asserted."""
    got, want, scale = (np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float64) for a in (got, want, scale))
    assert got.shape == want.shape == scale.shape, (got.shape, want.shape, scale.shape)
    return max(rowwise_error(got[:, c], want[:, c], scale=scale[:, c]) for c in range(got.shape[1]))


def check_block(op, K, mesh_np, alpha, beta, tol, widths=WIDTHS, seed=3, oracle_mesh=None):
    n = op.shape[0]
    kmax = max(widths)
    U = torch.tensor(np.random.default_rng(seed).standard_normal((n, kmax)), dtype=op.dtype)
    want, oscale = oracle_apply_block(oracle_mesh or mesh_np, alpha, beta, U.double().cpu().numpy())
    single = torch.stack([op.matvec(U[:, j].contiguous()) for j in range(kmax)], dim=1)
    for k in widths:
        Uk = U[:, :k].contiguous()
        got = op @ Uk
        assert got.shape == (n, k) and got.dtype == op.dtype
        e_oracle = block_error(got, want[:, :k], oscale[:, :k])
        e_single = block_error(got, single[:, :k].double(), oscale[:, :k])
        print(f"k = {k}: against the oracle {e_oracle:.2e}, against the single launch {e_single:.2e}")
        assert e_oracle <= tol and e_single <= tol
        if K is not None:
            scale = torch.stack([csr_scale(K, Uk[:, j].contiguous()) for j in range(k)], dim=1)
            e_csr = block_error(got, K.matvec(Uk), scale)
            print(f"k = {k}: against the assembled CSR {e_csr:.2e}")
            assert e_csr <= tol
        # non-contiguous U: a column slice of the wider block, a transposed view
        if k < kmax:
            assert not U[:, :k].is_contiguous()
            assert torch.equal(op.matvec(U[:, :k]), got)
        Ut = Uk.t().contiguous().t()
        assert not Ut.is_contiguous() and torch.equal(op @ Ut, got)


@pytest.mark.parametrize("case", ["p1_square_n8.npz", "p1_delaunay_170.npz", "p1_square_n5_clockwise.npz",
                                  "mixed", "structured", "delaunay_generator_order"])
@pytest.mark.parametrize("which", list(FORMS))
def test_block_matches_the_oracle_the_assembled_operator_and_the_single_launch(case, which):
    alpha, beta = FORMS[which]
    mesh_np = _case(case)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
    K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
    assert op.matrix_free and op.dtype == torch.float64
    eng = basis._engine
    if case == "structured":
        assert eng.ring_plan()["chunked"]
    if case == "delaunay_generator_order":  # renumbered inside the engine, 15-slot records
        assert eng.renumbered and int(eng.ring_plan()["layout"][6]) == 15
    check_block(op, K, mesh_np, alpha, beta, TOL)


def test_block_float32():
    mesh_np = mesh_from_golden(load_golden("p1_square_n6_float32.npz"))
    mesh64 = {k: v.astype(np.float64) if k == "vertices" else v for k, v in mesh_np.items()}
    torch.set_default_dtype(torch.float32)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    for alpha, beta in FORMS.values():
        op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
        assert op.matrix_free and op.dtype == torch.float32
        check_block(op, None, mesh_np, alpha, beta, 2e-5, seed=4, oracle_mesh=mesh64)


@pytest.mark.parametrize("numbering", ["morton", "native"])
def test_block_on_a_plan_with_long_rows(numbering, monkeypatch):
    """TFEM_RING_LONG=1: the vertices with 8 .. 15 neighbours go through k_p1_apply_long_rows_multi."""
    from pytorch_fem_solver_amd import meshgen

    monkeypatch.setenv("TFEM_RING_LONG", "1")
    mesh_np = meshgen.delaunay_square(7000, 21)
    if numbering == "morton":
        mesh_np = meshgen.permute_mesh(mesh_np, vertex_order=meshgen.morton_order(mesh_np["vertices"]))
    basis = tf().Basis(tf().MeshTri(mesh_np), tf().ElementTri(1, 3))
    for alpha, beta in FORMS.values():
        op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
        assert op.matrix_free and int(basis._engine.ring_plan()["layout"][23]) > 100
        check_block(op, None, mesh_np, alpha, beta, TOL, seed=8)


def test_block_on_a_plan_that_is_not_chunked():
    """Tiles whose vertex ids come from the plan (7-slot records, several tiles)."""
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(40, 0.25, 1)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    rings = basis._engine.ring_plan()
    assert rings is not None and not rings["chunked"] and rings["n_tiles"] > 1 and int(rings["layout"][6]) == 7, \
        "the generator no longer produces a non-chunked 7-slot plan for this mesh: pick another one"
    for alpha, beta in FORMS.values():
        op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
        K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
        check_block(op, K, mesh_np, alpha, beta, TOL, seed=6)


def test_c_abi_single_column_and_refused_arguments():
    from pytorch_fem_solver_amd import _native, meshgen

    mesh_np = meshgen.unit_square(40, 0.25, 4)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    eng = basis._engine
    rings, d, n = eng.ring_plan(), eng._inputs(), eng.n_dofs
    assert not eng.renumbered
    head = (_native.ptr(d["coords"]), 8, n, 3, 2.0, 0.5, _native.ptr(rings["blob"]),
            ctypes.c_void_p(rings["layout"].ctypes.data))
    lib = eng.lib
    u = torch.rand(n)
    y1, ym = torch.empty(n), torch.empty(n)
    _native.check(lib.tfem_p1_apply_rings(*head, _native.ptr(u), _native.ptr(y1), eng._stream()))
    _native.check(lib.tfem_p1_apply_rings_multi(*head, _native.ptr(u), _native.ptr(ym), 1, eng._stream()))
    torch.cuda.synchronize()
    assert torch.equal(y1, ym)  # n_vec = 1 is the single-vector launch
    # three columns through the entry point itself, against the engine's numbering of the same call
    U = torch.rand(n, 3)
    Y = torch.full((n, 3), float("nan"))
    _native.check(lib.tfem_p1_apply_rings_multi(*head, _native.ptr(U), _native.ptr(Y), 3, eng._stream()))
    torch.cuda.synchronize()
    K = basis.integrate_bilinear_form(form(2.0, 0.5), layout="csr")
    scale = torch.stack([csr_scale(K, U[:, j].contiguous()) for j in range(3)], dim=1)
    assert torch.isfinite(Y).all() and block_error(Y, K.matvec(U), scale) <= TOL
    # refused on the host, nothing launched: the output keeps its contents
    Y.fill_(7.0)
    buf = torch.rand(4 * n)
    refused = {
        "overlap": (lib.tfem_p1_apply_rings_multi(*head, _native.ptr(buf), ctypes.c_void_p(buf.data_ptr() + 8 * n), 2,
                                                  eng._stream()), 1),
        "same": (lib.tfem_p1_apply_rings_multi(*head, _native.ptr(buf), _native.ptr(buf), 2, eng._stream()), 1),
        "u NULL": (lib.tfem_p1_apply_rings_multi(*head, None, _native.ptr(Y), 3, eng._stream()), 1),
        "n_vec 0": (lib.tfem_p1_apply_rings_multi(*head, _native.ptr(U), _native.ptr(Y), 0, eng._stream()), 1),
        "n_vec -1": (lib.tfem_p1_apply_rings_multi(*head, _native.ptr(U), _native.ptr(Y), -1, eng._stream()), 1),
        # n_verts * n_vec * 8 bytes = 2^32 and beyond: TFEM_ERR_INDEX_RANGE
        "extent": (lib.tfem_p1_apply_rings_multi(*head, _native.ptr(U), _native.ptr(Y), (1 << 29) // n + 1,
                                                 eng._stream()), 4),
        "extent 2^62": (lib.tfem_p1_apply_rings_multi(*head, _native.ptr(U), _native.ptr(Y), 1 << 62, eng._stream()), 4),
    }
    torch.cuda.synchronize()
    assert {k: v[0] for k, v in refused.items()} == {k: v[1] for k, v in refused.items()}
    assert bool((Y == 7.0).all())
    # the engine refuses out = u and a wrong number of rows
    with pytest.raises(ValueError):
        eng._apply_rings(1.0, 0.0, U, out=U)
    with pytest.raises(ValueError):
        basis.integrate_bilinear_form(form(1.0, 0.0), layout="operator").matvec(torch.rand(n + 1, 3))


def test_operators_without_the_block_launch_take_blocks_column_by_column(monkeypatch):
    """The variable-coefficient operator (tfem_p1_apply_rings_coef) and a CSR-wrapping operator (P2)."""
    import coefficient_reference as cref
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(40, 0.25, 1)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(cref.form(1.0, 0.5, cref.kappa_trig, cref.c_exp), layout="operator")
    assert op.matrix_free and op._programs is not None
    U = torch.rand(op.shape[0], 5)
    got = op @ U
    assert got.shape == U.shape
    for j in range(5):
        assert torch.equal(got[:, j], op.matvec(U[:, j].contiguous()))
    # on a renumbered mesh
    shuffled = meshgen.permute_mesh(mesh_np, vertex_order=np.random.default_rng(7).permutation(mesh_np["vertices"].shape[0]))
    monkeypatch.setenv("TFEM_RENUMBER", "1")
    basis_s = tf().Basis(tf().MeshTri(triangulation=shuffled), tf().ElementTri(1, 3))
    for a in (cref.form(1.0, 0.5, cref.kappa_trig, cref.c_exp), form(1.0, 0.5)):
        op_s = basis_s.integrate_bilinear_form(a, layout="operator")
        got = op_s @ U
        assert basis_s._engine.renumbered and got.shape == U.shape
        for j in range(5):
            want = op_s.matvec(U[:, j].contiguous())
            assert scaled_error(got[:, j].cpu(), want.cpu()) <= 1e-13
    monkeypatch.delenv("TFEM_RENUMBER")
    # P2: the operator wraps the assembled CSR
    basis2 = tf().Basis(tf().MeshTri(triangulation=meshgen.unit_square(20, 0.25, 0)), tf().ElementTri(2, 2))
    op2 = basis2.integrate_bilinear_form(form(1.0, 1.0), layout="operator")
    K2 = basis2.integrate_bilinear_form(form(1.0, 1.0), layout="csr")
    U2 = torch.rand(K2.shape[0], 3)
    got2 = op2 @ U2
    assert op2.matrix_free is False and got2.shape == U2.shape and torch.equal(got2, K2.matvec(U2))
    for j in range(3):
        assert torch.equal(got2[:, j], op2.matvec(U2[:, j].contiguous()))
    # block CG on the CSR-wrapping operator and on the CSRMatrix
    F2 = torch.cat([basis2.integrate_linear_form(load), 2.0 * basis2.integrate_linear_form(load)], dim=1)
    free = basis2._basis_parameters["inner_dofs"]
    X, its, res = op2.solve_cg_multi(F2, free=free, rtol=1e-10)
    x0, _, _ = K2.solve_cg(F2[:, 0], free=free, rtol=1e-10)
    assert X.shape == F2.shape and float(res.max()) <= 1e-10
    assert scaled_error(X[:, 0].cpu(), x0.cpu()) <= 1e-8 and scaled_error(X[:, 1].cpu(), 2.0 * x0.cpu()) <= 1e-8


def test_block_matvec_is_differentiable_in_u():
    from pytorch_fem_solver_amd import meshgen

    basis = tf().Basis(tf().MeshTri(triangulation=meshgen.unit_square(12, 0.25, 3)), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.5), layout="operator")
    assert op.matrix_free
    U = torch.rand(op.shape[0], 3, requires_grad=True)
    # an energy-norm loss over the columns: d/dU trace(U^T K U) = 2 K U
    loss = (U.T @ (op @ U)).trace()
    (g,) = torch.autograd.grad(loss, U)
    assert g.shape == U.shape
    assert scaled_error(g.detach().cpu(), (2.0 * (op @ U.detach())).cpu()) <= 1e-14


def test_block_cg_equals_cg_column_by_column():
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(316, 0.25, 2)  # ~1e5 DoFs
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.0), layout="operator")
    assert op.matrix_free

    def source(i, j):
        def linear(b):
            x, y = torch.split(b.integration_points, 1, dim=-1)
            return np.pi**2 * (i * i + j * j) * torch.sin(i * np.pi * x) * torch.sin(j * np.pi * y) * b.v
        return linear

    F = torch.cat([basis.integrate_linear_form(source(i, j)) for i, j in ((1, 1), (2, 1), (1, 3), (4, 4))], dim=1)
    free = basis._basis_parameters["inner_dofs"]
    X, its, res = op.solve_cg_multi(F, free=free, rtol=1e-10)
    assert X.shape == F.shape and its.shape == (4,) and float(res.max()) <= 1e-10
    for j in range(4):
        x, it, r = op.solve_cg(F[:, j].contiguous(), free=free, rtol=1e-10)
        err = scaled_error(X[:, j].cpu(), x.cpu())
        print(f"column {j}: block {int(its[j])} iterations, single {it}; scaled error {err:.2e}")
        assert abs(int(its[j]) - it) <= 25 and err <= 1e-8
    # Basis.solve with (N, 4): the default tolerance of solve_cg, against Basis.solve per column
    sol = basis.solve(op, torch.zeros_like(F), F)
    assert sol.shape == F.shape
    for j in range(4):
        one = basis.solve(op, basis.solution_tensor(), F[:, [j]])
        assert scaled_error(sol[:, j].cpu(), one.reshape(-1).cpu()) <= 1e-8


def test_block_at_full_size():
    """S(2236), 9,999,392 elements, four vectors: K U against tfem_csr_spmv column by column."""
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(2236, 0.25, 0)
    assert mesh_np["triangles"].shape[0] == 9999392
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.0), layout="operator")
    U = torch.randn(op.shape[0], 4, generator=torch.Generator(device="cuda").manual_seed(7))
    got = op.matvec(U)
    K = op.to_csr()
    assert op.matrix_free and got.shape == U.shape
    for j in range(4):
        u = U[:, j].contiguous()
        err = ((got[:, j] - K.matvec(u)).abs() / csr_scale(K, u)).max().item()
        print(f"column {j}: {err:.2e}")
        assert err <= TOL
