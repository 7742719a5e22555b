"""The matrix-free P1 operator (layout="operator", csrc/tfem_rings_apply.hip) on a real MI355X:
K u and diag(K) against the assembled CSR operator and the oracle, CG on it, the CSR fallback of
the forms and bases the launch does not cover, and its gradient."""

import numpy as np
import pytest
import torch

from conftest import load_golden, mesh_from_golden, rowwise_error, scaled_error
from oracle import assembly_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-12
FORMS = {"stiffness": (1.0, 0.0), "mass": (0.0, 1.0), "both": (2.0, 0.5)}


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def tf():
    import pytorch_fem_solver_amd

    return pytorch_fem_solver_amd


def form(alpha, beta):
    def bilinear(b):
        return alpha * (b.v_grad @ b.v_grad.mT) + beta * (b.v @ b.v.mT)

    return bilinear


def convection_x(basis):
    return basis.v @ basis.v_grad[..., [0]].mT


def load(basis):
    x, y = torch.split(basis.integration_points, 1, dim=-1)
    return 2.0 * np.pi**2 * torch.sin(np.pi * x) * torch.sin(np.pi * y) * basis.v


def oracle_apply(mesh_np, alpha, beta, u):
    """(K u, sum_j |K_ij u_j|) from the oracle's CSR values."""
    verts, tris = mesh_np["vertices"], mesh_np["triangles"]
    n = verts.shape[0]
    rowptr, colind, slots = orc.csr_pattern(tris, n)
    vals = np.zeros(colind.shape[0])
    for name, c in (("stiffness", alpha), ("mass", beta)):
        if c:
            local, _ = orc.p1_assemble(verts, tris, 3, name)
            vals += c * orc.assemble_csr_values(local, slots, colind.shape[0])
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    prod = vals * u[colind]
    return np.bincount(rows, prod, minlength=n), np.bincount(rows, np.abs(prod), minlength=n)


def csr_scale(K, u):
    """sum_j |K_ij u_j| of an assembled operator, on the device."""
    absK = tf().CSRMatrix(K.crow_indices, K.col_indices, K.values.abs(), K.shape, K.perm)
    return absK.matvec(u.abs())


def _mixed_mesh():
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(90, 0.25, 4)
    tri = mesh_np["triangles"].copy()
    flip = np.random.default_rng(5).random(tri.shape[0]) < 0.4
    tri[flip] = tri[flip][:, [0, 2, 1]]
    mesh_np["triangles"] = tri
    return mesh_np


def _case(name):
    from pytorch_fem_solver_amd import meshgen

    if name.endswith(".npz"):
        return mesh_from_golden(load_golden(name))
    if name == "mixed":
        return _mixed_mesh()
    if name == "structured":
        return meshgen.unit_square(300, 0.25, 1)
    if name == "delaunay_generator_order":  # above RENUMBER_MIN_DOFS: the engine renumbers
        return meshgen.delaunay_square(60000, 9)
    raise KeyError(name)


@pytest.mark.parametrize("case", ["p1_square_n8.npz", "p1_delaunay_170.npz", "p1_square_n5_clockwise.npz",
                                  "mixed", "structured", "delaunay_generator_order"])
@pytest.mark.parametrize("which", list(FORMS))
def test_operator_matches_the_assembled_operator_and_the_oracle(case, which):
    alpha, beta = FORMS[which]
    mesh_np = _case(case)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
    K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
    assert op.matrix_free and op.shape == K.shape and op.dtype == torch.float64
    eng = basis._engine
    if case == "structured":
        assert eng.ring_plan()["chunked"]
    if case == "delaunay_generator_order":
        assert eng.renumbered and int(eng.ring_plan()["layout"][6]) == 15
    n = K.shape[0]
    u = torch.tensor(np.random.default_rng(3).standard_normal(n))
    got = op.matvec(u)
    assert got.shape == (n,)
    scale = csr_scale(K, u)
    assert rowwise_error(got.cpu(), K.matvec(u).cpu(), scale=scale.cpu()) <= TOL
    want, oscale = oracle_apply(mesh_np, alpha, beta, u.cpu().numpy())
    assert rowwise_error(got.cpu(), want, scale=oscale) <= TOL
    # (N, 1) and the @ operator
    col = op @ u.reshape(-1, 1)
    assert col.shape == (n, 1) and torch.equal(col.reshape(-1), got)
    # the diagonal (Jacobi): the assembled CSR diagonal, relative to the row's magnitude sum_j |K_ij| (the
    # diagonal is formed from the off-diagonal sum; with mixed orientation the signed determinants of a
    # fan cancel inside it, and the two launches contract their multiply-adds differently)
    d_op, d_csr = op.diagonal(), K.diagonal()
    tol = 1e-14 if case != "mixed" else 1e-12
    assert rowwise_error(d_op.cpu(), d_csr.cpu(), scale=csr_scale(K, torch.ones(n)).cpu()) <= tol


def test_operator_float32():
    mesh_np = mesh_from_golden(load_golden("p1_square_n6_float32.npz"))
    torch.set_default_dtype(torch.float32)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    for alpha, beta in FORMS.values():
        op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
        assert op.matrix_free and op.dtype == torch.float32
        u = torch.tensor(np.random.default_rng(4).standard_normal(op.shape[0]), dtype=torch.float32)
        want, scale = oracle_apply({k: v.astype(np.float64) if k == "vertices" else v for k, v in mesh_np.items()},
                                   alpha, beta, u.double().cpu().numpy())
        assert rowwise_error(op.matvec(u).double().cpu(), want, scale=scale) <= 2e-5
        K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
        assert rowwise_error(op.diagonal().double().cpu(), K.diagonal().double().cpu(),
                             scale=K.diagonal().double().abs().cpu()) <= 1e-6


def test_operator_at_full_size():
    """S(2236), 9,999,392 elements: K u without the CSR values against tfem_csr_spmv on them."""
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(2236, 0.25, 0)
    assert mesh_np["triangles"].shape[0] == 9999392
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.0), layout="operator")
    u = torch.randn(op.shape[0], generator=torch.Generator(device="cuda").manual_seed(7))
    got = op.matvec(u)
    K = op.to_csr()
    assert op.matrix_free and isinstance(K, tf().CSRMatrix)
    err = ((got - K.matvec(u)).abs() / csr_scale(K, u)).max().item()
    assert err <= TOL


def test_cg_on_the_operator_equals_cg_on_the_csr_and_the_dense_solve():
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(316, 0.25, 2)  # ~1e5 DoFs
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.0), layout="operator")
    K = basis.integrate_bilinear_form(form(1.0, 0.0), layout="csr")
    f = basis.integrate_linear_form(load)
    u_op = basis.solve(op, basis.solution_tensor(), f)
    u_csr = basis.solve(K, basis.solution_tensor(), f, method="cg")
    assert op.matrix_free and scaled_error(u_op.cpu(), u_csr.cpu()) <= 1e-9
    # small mesh: the reference's dense reduce + torch.linalg.solve
    small = meshgen.unit_square(24, 0.25, 1)
    basis = tf().Basis(tf().MeshTri(triangulation=small), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.0), layout="operator")
    K = basis.integrate_bilinear_form(form(1.0, 0.0), layout="dense")
    f = basis.integrate_linear_form(load)
    u_op = basis.solve(op, basis.solution_tensor(), f)
    u_dense = basis.solve(K, basis.solution_tensor(), f)
    assert scaled_error(u_op.cpu(), u_dense.cpu()) <= 1e-9
    # FormOperator.solve_cg keeps the contract of CSRMatrix.solve_cg on a renumbered mesh too
    big = meshgen.delaunay_square(60000, 9)
    basis = tf().Basis(tf().MeshTri(triangulation=big), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.5), layout="operator")
    K = basis.integrate_bilinear_form(form(1.0, 0.5), layout="csr")
    assert basis._engine.renumbered
    b = torch.rand(op.shape[0], 1)
    free = basis._basis_parameters["inner_dofs"]
    x_op, it_op, res_op = op.solve_cg(b, free=free, rtol=1e-10)
    x_csr, it_csr, res_csr = K.solve_cg(b, free=free, rtol=1e-10)
    assert x_op.shape == b.shape and res_op <= 1e-10 and abs(it_op - it_csr) <= 25
    assert scaled_error(x_op.cpu(), x_csr.cpu()) <= 1e-8


def test_forms_and_bases_without_the_launch_fall_back_to_the_csr(monkeypatch):
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(20, 0.25, 0)
    n1 = mesh_np["vertices"].shape[0]
    u1 = torch.rand(n1)
    # a generic integrand (not alpha * stiffness + beta * mass)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(convection_x, layout="operator")
    K = basis.integrate_bilinear_form(convection_x, layout="csr")
    assert op.matrix_free is False
    assert scaled_error(op.matvec(u1).cpu(), K.matvec(u1).cpu()) <= 1e-14
    assert scaled_error(op.diagonal().cpu(), K.diagonal().cpu()) <= 1e-14
    # P2
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(2, 2))
    op = basis.integrate_bilinear_form(form(1.0, 1.0), layout="operator")
    K = basis.integrate_bilinear_form(form(1.0, 1.0), layout="csr")
    u2 = torch.rand(K.shape[0])
    assert op.matrix_free is False and scaled_error(op.matvec(u2).cpu(), K.matvec(u2).cpu()) <= 1e-14
    f = basis.integrate_linear_form(load)
    assert scaled_error(basis.solve(op, basis.solution_tensor(), f).cpu(),
                        basis.solve(K, basis.solution_tensor(), f, method="cg").cpu()) <= 1e-12
    # a fracture basis
    d = load_golden("fracture_L4.npz")
    tri = mesh_from_golden(d)
    mesh = tf().FracturesTri(triangulations=[tri, tri], fractures_3d_data=torch.tensor(d["in_fractures_3d"]))
    V = tf().FractureBasis(mesh, tf().ElementTri(polynomial_order=1, integration_order=4))
    op = V.integrate_bilinear_form(form(1.0, 0.0), layout="operator")
    K = V.integrate_bilinear_form(form(1.0, 0.0), layout="csr")
    u3 = torch.rand(K.shape[0])
    assert op.matrix_free is False and scaled_error(op.matvec(u3).cpu(), K.matvec(u3).cpu()) <= 1e-14
    # a forced kernel without the ring plan
    monkeypatch.setenv("TFEM_KERNEL", "tiles")
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.0), layout="operator")
    K = basis.integrate_bilinear_form(form(1.0, 0.0), layout="csr")
    assert op.matrix_free is False and scaled_error(op.matvec(u1).cpu(), K.matvec(u1).cpu()) <= 1e-14


@pytest.mark.parametrize("numbering", ["morton", "native"])
def test_operator_on_a_plan_with_long_rows(numbering, monkeypatch):
    """TFEM_RING_LONG=1: the vertices with 8 .. 15 neighbours go through k_p1_apply_long_rows."""
    from pytorch_fem_solver_amd import meshgen

    monkeypatch.setenv("TFEM_RING_LONG", "1")
    mesh_np = meshgen.delaunay_square(7000, 21)
    if numbering == "morton":
        mesh_np = meshgen.permute_mesh(mesh_np, vertex_order=meshgen.morton_order(mesh_np["vertices"]))
    basis = tf().Basis(tf().MeshTri(mesh_np), tf().ElementTri(1, 3))
    for alpha, beta in FORMS.values():
        op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
        assert op.matrix_free and int(basis._engine.ring_plan()["layout"][23]) > 100
        u = torch.tensor(np.random.default_rng(8).standard_normal(op.shape[0]))
        want, scale = oracle_apply(mesh_np, alpha, beta, u.cpu().numpy())
        assert rowwise_error(op.matvec(u).cpu(), want, scale=scale) <= TOL
        K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
        assert rowwise_error(op.diagonal().cpu(), K.diagonal().cpu(), scale=csr_scale(K, torch.ones(K.shape[0])).cpu()) <= 1e-14


def test_matvec_is_differentiable_in_u():
    from pytorch_fem_solver_amd import meshgen

    basis = tf().Basis(tf().MeshTri(triangulation=meshgen.unit_square(5, 0.25, 3)), tf().ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.5), layout="operator")
    assert op.matrix_free
    u = torch.rand(op.shape[0], requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: op.matvec(v), (u,))
    # an energy-norm loss: d/du (u^T K u / 2) = K u
    loss = 0.5 * torch.dot(u, op.matvec(u))
    (g,) = torch.autograd.grad(loss, u)
    assert scaled_error(g.detach().cpu(), op.matvec(u.detach()).cpu()) <= 1e-14
