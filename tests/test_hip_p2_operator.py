"""The matrix-free P2 operator (layout="matrix_free", csrc/tfem_p2apply.hip) on a real MI355X: K u
and diag(K) over the P2 row plan against the assembled CSR operator and the oracle, blocks, CG,
its gradient, that nothing is assembled behind it, what the strict layout refuses, and the status
codes of tfem_p2_apply_rows."""

import ctypes
import functools

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


def _flipped(mesh_np):
    """40 % of the triangles stored clockwise (seed 5, as test_p2_row_kernels_against_oracle_and_gather)."""
    tri = mesh_np["triangles"].copy()
    flip = np.random.default_rng(5).random(tri.shape[0]) < 0.4
    tri[flip] = tri[flip][:, [0, 2, 1]]
    mesh_np["triangles"] = tri
    return mesh_np


#: name -> (mesh, quadrature order, stored with mixed orientation)
@functools.lru_cache(maxsize=None)
def _case(name):
    from pytorch_fem_solver_amd import meshgen

    if name == "p2_global_n4.npz":  # a single tile, partial waves, boundary fans
        return mesh_from_golden(load_golden(name)), 2, False
    if name == "square20":  # the mesh of the tests that pin layout="operator" on P2 to the CSR
        return meshgen.unit_square(20, 0.25, 0), 2, False
    if name in ("mixed70_q2", "mixed70_q4"):  # several tiles, mixed orientation
        return _flipped(meshgen.unit_square(70, 0.25, 4)), int(name[-1]), True
    if name == "delaunay_morton":  # long rows, and holes in the tile kernel's waves
        native = meshgen.delaunay_square(6000, 7)
        return _flipped(meshgen.permute_mesh(native, vertex_order=meshgen.morton_order(native["vertices"]))), 2, True
    if name == "renumbered30":  # TFEM_RENUMBER=1: the engine renumbers the edge DoFs
        return meshgen.unit_square(30, 0.25, 1), 2, False
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle_csr(name):
    """(rowptr, colind, stiffness values, mass values) of the oracle's P2 assembly, computed once."""
    from pytorch_fem_solver_amd import dofs

    mesh_np, order, _ = _case(name)
    tri = mesh_np["triangles"]
    conn6, xy, _ = dofs.p2_dofs_numpy(mesh_np["vertices"], tri, mesh_np["edges"], mesh_np["edge_markers"],
                                      mesh_np["vertex_markers"])
    geo = orc.geometry(mesh_np["vertices"][tri], 2, order)
    rowptr, colind, slots = orc.csr_pattern(conn6, xy.shape[0])
    vals = [orc.assemble_csr_values(orc.integrate_local(integrand(geo), geo["dx"]), slots, colind.shape[0])
            for integrand in (orc.integrand_stiffness, orc.integrand_mass)]
    return rowptr, colind, np.asarray(vals[0], dtype=np.float64), np.asarray(vals[1], dtype=np.float64)


def oracle_apply(name, alpha, beta, u):
    """(K u, sum_j |K_ij u_j|) from the oracle's CSR values, multiplied on the host."""
    rowptr, colind, stiff, mass = _oracle_csr(name)
    n = rowptr.shape[0] - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    prod = (alpha * stiff + beta * mass) * u[colind]
    return np.bincount(rows, prod, minlength=n), np.bincount(rows, np.abs(prod), minlength=n)


def csr_scale(K, u):
    """sum_j |K_ij u_j| of an assembled operator, on the device."""
    absK = tf().CSRMatrix(K.crow_indices, K.col_indices, K.values.abs(), K.shape, K.perm)
    return absK.matvec(u.abs())


def p2_basis(mesh_np, order=2):
    return tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(2, order))


CASES = ["p2_global_n4.npz", "square20", "mixed70_q2", "mixed70_q4", "delaunay_morton", "renumbered30"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("which", list(FORMS))
def test_p2_operator_matches_the_assembled_operator_and_the_oracle(case, which, monkeypatch):
    alpha, beta = FORMS[which]
    mesh_np, order, mixed = _case(case)
    if case == "renumbered30":
        monkeypatch.setenv("TFEM_RENUMBER", "1")
    basis = p2_basis(mesh_np, order)
    op = basis.integrate_bilinear_form(form(alpha, beta), layout="matrix_free")
    K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
    assert op.matrix_free is True and op.shape == K.shape and op.dtype == torch.float64
    assert "matrix-free, P2 rows" in repr(op)
    eng = basis._engine
    if case == "delaunay_morton":
        assert int(eng.p2_plan()["layout"][18]) > 100
    if case in ("mixed70_q2", "mixed70_q4"):
        assert int(eng.p2_plan()["layout"][0]) > 1 and int(eng.p2_plan()["layout"][1]) > 1
    assert eng.renumbered == (case == "renumbered30")
    n = K.shape[0]
    u = torch.tensor(np.random.default_rng(3).standard_normal(n))
    got = op.matvec(u)
    assert got.shape == (n,)
    err_csr = rowwise_error(got.cpu(), K.matvec(u).cpu(), scale=csr_scale(K, u).cpu())
    want, oscale = oracle_apply(case, alpha, beta, u.cpu().numpy())
    err_oracle = rowwise_error(got.cpu(), want, scale=oscale)
    # (N, 1) and the @ operator
    col = op @ u.reshape(-1, 1)
    assert col.shape == (n, 1) and torch.equal(col.reshape(-1), got)
    # the diagonal against the assembled one, relative to the row's magnitude sum_j |K_ij|
    err_diag = rowwise_error(op.diagonal().cpu(), K.diagonal().cpu(), scale=csr_scale(K, torch.ones(n)).cpu())
    print(f"{case} {which}: K u against the CSR {err_csr:.2e}, the oracle {err_oracle:.2e}; diagonal {err_diag:.2e}")
    assert err_csr <= TOL and err_oracle <= TOL
    assert err_diag <= (1e-12 if mixed else 1e-14)


def test_p2_operator_float32():
    from pytorch_fem_solver_amd import dofs, meshgen

    mesh_np = meshgen.unit_square(24, 0.25, 1)
    torch.set_default_dtype(torch.float32)
    mesh32 = {k: v.astype(np.float32) if k == "vertices" else v for k, v in mesh_np.items()}
    basis = p2_basis(mesh32)
    tri = mesh_np["triangles"]
    conn6, xy, _ = dofs.p2_dofs_numpy(mesh_np["vertices"], tri, mesh_np["edges"], mesh_np["edge_markers"],
                                      mesh_np["vertex_markers"])
    geo = orc.geometry(mesh32["vertices"][tri], 2, 2)
    rowptr, colind, slots = orc.csr_pattern(conn6, xy.shape[0])
    n = xy.shape[0]
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    vals = {name: np.asarray(orc.assemble_csr_values(orc.integrate_local(integrand(geo), geo["dx"]), slots,
                                                     colind.shape[0]), dtype=np.float64)
            for name, integrand in (("stiffness", orc.integrand_stiffness), ("mass", orc.integrand_mass))}
    for alpha, beta in FORMS.values():
        op = basis.integrate_bilinear_form(form(alpha, beta), layout="matrix_free")
        assert op.matrix_free is True and op.dtype == torch.float32
        u = torch.tensor(np.random.default_rng(4).standard_normal(n), dtype=torch.float32)
        prod = (alpha * vals["stiffness"] + beta * vals["mass"]) * u.double().cpu().numpy()[colind]
        want, scale = np.bincount(rows, prod, minlength=n), np.bincount(rows, np.abs(prod), minlength=n)
        assert rowwise_error(op.matvec(u).double().cpu(), want, scale=scale) <= 2e-5
        K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
        assert rowwise_error(op.diagonal().double().cpu(), K.diagonal().double().cpu(),
                             scale=csr_scale(K, torch.ones(n)).double().cpu()) <= 2e-5


def test_p2_operator_on_blocks_and_block_cg():
    mesh_np, order, _ = _case("square20")
    basis = p2_basis(mesh_np, order)
    op = basis.integrate_bilinear_form(form(1.0, 1.0), layout="matrix_free")
    K = basis.integrate_bilinear_form(form(1.0, 1.0), layout="csr")
    U = torch.rand(K.shape[0], 3)
    got = op @ U
    assert op.matrix_free is True and got.shape == U.shape
    for j in range(3):  # the same launch per column
        assert torch.equal(got[:, j], op.matvec(U[:, j].contiguous()))
    scale = torch.stack([csr_scale(K, U[:, j].contiguous()) for j in range(3)], dim=1)
    assert rowwise_error(got.cpu(), K.matvec(U).cpu(), scale=scale.cpu()) <= TOL
    F = torch.cat([basis.integrate_linear_form(load), 2.0 * basis.integrate_linear_form(load)], dim=1)
    free = basis._basis_parameters["inner_dofs"]
    X, its, res = op.solve_cg_multi(F, free=free, rtol=1e-10)
    assert X.shape == F.shape and float(res.max()) <= 1e-10
    for j in range(2):
        x_j, _, _ = K.solve_cg(F[:, j], free=free, rtol=1e-10)
        assert scaled_error(X[:, j].cpu(), x_j.cpu()) <= 1e-8


def test_cg_on_the_p2_operator_equals_cg_on_the_csr():
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(100, 0.25, 2)
    basis = p2_basis(mesh_np)
    op = basis.integrate_bilinear_form(form(1.0, 0.0), layout="matrix_free")
    K = basis.integrate_bilinear_form(form(1.0, 0.0), layout="csr")
    f = basis.integrate_linear_form(load)
    u_op = basis.solve(op, basis.solution_tensor(), f)
    u_csr = basis.solve(K, basis.solution_tensor(), f, method="cg")
    assert op.matrix_free is True and scaled_error(u_op.cpu(), u_csr.cpu()) <= 1e-9
    b = torch.rand(op.shape[0], 1)
    free = basis._basis_parameters["inner_dofs"]
    x_op, it_op, res_op = op.solve_cg(b, free=free, rtol=1e-10)
    x_csr, it_csr, res_csr = K.solve_cg(b, free=free, rtol=1e-10)
    assert x_op.shape == b.shape and res_op <= 1e-10 and abs(it_op - it_csr) <= 25


def test_p2_matvec_is_differentiable_in_u():
    from pytorch_fem_solver_amd import meshgen

    basis = p2_basis(meshgen.unit_square(4, 0.25, 3))
    op = basis.integrate_bilinear_form(form(1.0, 0.5), layout="matrix_free")
    assert op.matrix_free is True
    u = torch.rand(op.shape[0], requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: op.matvec(v), (u,))
    # an energy-norm loss: d/du (u^T K u / 2) = K u
    loss = 0.5 * torch.dot(u, op.matvec(u))
    (g,) = torch.autograd.grad(loss, u)
    assert scaled_error(g.detach().cpu(), op.matvec(u.detach()).cpu()) <= 1e-14


class _Spy:
    """Counts the calls of the library's entry points that go through an engine."""

    NAMES = ("tfem_p2_apply_rows", "tfem_p2_assemble_rows", "tfem_csr_spmv", "tfem_tri_bilinear_csr")

    def __init__(self, monkeypatch, lib):
        self.calls = {name: 0 for name in self.NAMES}
        for name in self.NAMES:
            inner = getattr(lib, name)
            monkeypatch.setattr(lib, name, self._wrap(name, inner))

    def _wrap(self, name, inner):
        def call(*args):
            self.calls[name] += 1
            return inner(*args)

        return call


def test_nothing_is_assembled_behind_the_p2_operator(monkeypatch):
    mesh_np, order, _ = _case("square20")
    basis = p2_basis(mesh_np, order)
    spy = _Spy(monkeypatch, basis._engine.lib)
    op = basis.integrate_bilinear_form(form(1.0, 0.5), layout="matrix_free")
    u = torch.rand(op.shape[0])
    op.matvec(u)
    op.diagonal()
    _, it, _ = op.solve_cg(basis.integrate_linear_form(load), free=basis._basis_parameters["inner_dofs"], rtol=1e-8)
    assert spy.calls["tfem_p2_apply_rows"] >= it + 3
    assert spy.calls["tfem_p2_assemble_rows"] == 0 and spy.calls["tfem_csr_spmv"] == 0
    assert spy.calls["tfem_tri_bilinear_csr"] == 0 and op._csr is None
    K = op.to_csr()
    assert isinstance(K, tf().CSRMatrix) and op.to_csr() is K
    assert spy.calls["tfem_p2_assemble_rows"] == 1


def _hub_mesh(k):
    """One hub vertex joined to k rim vertices."""
    from pytorch_fem_solver_amd import meshgen

    ang = np.linspace(0, 2 * np.pi, k, endpoint=False)
    verts = np.concatenate([[[0.0, 0.0]], np.stack([np.cos(ang), np.sin(ang)], 1)])
    tris = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], dtype=np.int32)
    edges, on_boundary = meshgen._edges_from_triangles(tris)
    markers = np.zeros((k + 1, 1), dtype=np.int32)
    markers[1:] = 1
    return {"vertices": verts, "vertex_markers": markers, "triangles": tris, "edges": edges,
            "edge_markers": on_boundary.reshape(-1, 1).astype(np.int32),
            # neighbour j lies across the edge opposite to vertex j: the rim, the next and the previous triangle
            "neighbors": np.array([[-1, (i + 1) % k, (i - 1) % k] for i in range(k)], dtype=np.int32)}


def test_matrix_free_layout_is_strict(monkeypatch):
    import coefficient_reference as cref
    from pytorch_fem_solver_amd import meshgen

    def refused(basis, a, word):
        with pytest.raises(NotImplementedError, match=word):
            basis.integrate_bilinear_form(a, layout="matrix_free")

    square, _, _ = _case("square20")
    # P2 in a numbering without locality; a vertex with more than 15 neighbours
    refused(p2_basis(meshgen.delaunay_square(8000, 3)), form(1.0, 0.0), "no row plan")
    refused(p2_basis(_hub_mesh(17)), form(1.0, 0.0), "no row plan")
    # an integrand outside the vocabulary, on P2 and on P1
    refused(p2_basis(square), convection_x, "integrand")
    p1 = tf().Basis(tf().MeshTri(triangulation=square), tf().ElementTri(1, 3))
    refused(p1, convection_x, "integrand")
    # a fracture basis
    d = load_golden("fracture_L4.npz")
    tri = mesh_from_golden(d)
    mesh = tf().FracturesTri(triangulations=[tri, tri], fractures_3d_data=torch.tensor(d["in_fractures_3d"]))
    refused(tf().FractureBasis(mesh, tf().ElementTri(polynomial_order=1, integration_order=4)), form(1.0, 0.0), "fracture")
    # P2 with a coefficient field
    refused(p2_basis(square), cref.form(1.0, 0.5, cref.kappa_trig, cref.c_exp), "coefficient")
    # every other layout value behaves as before
    with pytest.raises(ValueError, match="unknown layout"):
        p1.integrate_bilinear_form(form(1.0, 0.0), layout="matrixfree")
    # P1 on a ring-plan mesh: the bits of layout="operator", constant and variable coefficients
    u = torch.rand(p1._engine.n_dofs)
    for a in (form(1.0, 0.5), cref.form(1.0, 0.5, cref.kappa_trig, cref.c_exp)):
        strict = p1.integrate_bilinear_form(a, layout="matrix_free")
        lazy = p1.integrate_bilinear_form(a, layout="operator")
        assert strict.matrix_free is True and strict._matrix_free is True
        assert torch.equal(strict.matvec(u), lazy.matvec(u)) and lazy.matrix_free
    # assemble_system: the two calls
    op, f = p1.assemble_system(form(1.0, 0.0), load, layout="matrix_free")
    # (the load vector's launch sums element shares with atomics: the same numbers up to the order of a fan's sum)
    assert op.matrix_free is True and scaled_error(f.cpu(), p1.integrate_linear_form(load).cpu()) <= 1e-13
    # P1 under a forced kernel without the ring plan
    monkeypatch.setenv("TFEM_KERNEL", "tiles")
    refused(tf().Basis(tf().MeshTri(triangulation=square), tf().ElementTri(1, 3)), form(1.0, 0.0), "TFEM_KERNEL=tiles")


def test_p2_apply_error_codes_on_the_device():
    from pytorch_fem_solver_amd import _native

    mesh_np, order, _ = _case("square20")
    basis = p2_basis(mesh_np, order)
    eng = basis._engine
    rows, d = eng.p2_plan(), eng._inputs()
    colind = eng.csr_structure()[1]
    n, nnz = eng.n_dofs, int(colind.shape[0])
    lib = eng.lib
    buf = torch.rand(2 * n)
    u, y = buf[:n], buf[n:]
    head = (_native.ptr(d["coords"]), 8, order, 1.0, 0.5, _native.ptr(rows["blob"]),
            ctypes.c_void_p(rows["layout"].ctypes.data))

    def call(colind_ptr, u_ptr, y_ptr, n_dofs):
        return lib.tfem_p2_apply_rows(*head, colind_ptr, nnz, u_ptr, y_ptr, n_dofs, eng._stream())

    before = y.clone()
    assert call(_native.ptr(colind), _native.ptr(u), None, n) == 1 and b"NULL" in lib.tfem_last_error()
    assert call(None, _native.ptr(u), _native.ptr(y), n) == 1 and b"NULL" in lib.tfem_last_error()
    assert call(_native.ptr(colind), _native.ptr(u), ctypes.c_void_p(u.data_ptr() + 8 * (n - 1)), n) == 1
    assert b"overlap" in lib.tfem_last_error()
    assert call(_native.ptr(colind), _native.ptr(u), _native.ptr(u), n) == 1
    assert call(_native.ptr(colind), _native.ptr(u), _native.ptr(y), n - 1) == 1 and b"DoFs" in lib.tfem_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y, before)  # nothing was launched
    # a following valid call still gives the right result
    _native.check(call(_native.ptr(colind), _native.ptr(u), _native.ptr(y), n))
    K = basis.integrate_bilinear_form(form(1.0, 0.5), layout="csr")
    assert not eng.renumbered
    assert rowwise_error(y.cpu(), K.matvec(u.contiguous()).cpu(), scale=csr_scale(K, u.contiguous()).cpu()) <= TOL
    _native.check(call(_native.ptr(colind), None, _native.ptr(y), n))  # u NULL: the diagonal
    assert rowwise_error(y.cpu(), K.diagonal().cpu(), scale=csr_scale(K, torch.ones(n)).cpu()) <= 1e-14
