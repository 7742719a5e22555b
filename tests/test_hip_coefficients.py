"""Variable-coefficient P1 forms on a real MI355X: the coefficient launches
(csrc/tfem_rings_coef.hip) through the C ABI, the engine and the public API, every path against ONE
reference (tests/coefficient_reference.py: the oracle's quadrature on long-double coefficient
values, tolerance = the ring kernels' parity tolerance + the coefficient's propagated bound)."""

import ctypes
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import coefficient_reference as cref
import source_reference as sref
from conftest import load_golden, mesh_from_golden

pytestmark = pytest.mark.gpu

RATIOS = []  # max |err| / tol of every comparison of the running test


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    del RATIOS[:]
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)
    # a test that compared against the reference compared real numbers: cref.check asserted
    # |err| <= tol entry by entry, and somewhere the error is not exactly zero
    if RATIOS:
        print(f"{len(RATIOS)} comparisons, max |err| / tol = {max(RATIOS):.3e}")
        assert 0.0 < max(RATIOS) <= 1.0


def tf():
    import pytorch_fem_solver_amd

    return pytorch_fem_solver_amd


#: (alpha, beta, kappa, c): stiffness alone, mass alone, both with one field, both with two
FORMS = {
    "kappa_xy": (1.0, 0.0, cref.kappa_xy, None),
    "c_exp": (0.0, 1.0, None, cref.c_exp),
    "kappa_trig_plain_mass": (2.0, 0.5, cref.kappa_trig, None),
    "plain_stiffness_c_rational": (1.0, 3.0, None, cref.c_rational),
    "kappa_poly_c_exp": (0.5, 2.0, cref.kappa_poly, cref.c_exp),
}


def _holes(mesh_np, seed=11):
    tri = mesh_np["triangles"].copy()
    rng = np.random.default_rng(seed)
    tri = tri[rng.random(tri.shape[0]) >= 0.1]
    flip = rng.random(tri.shape[0]) < 0.4
    tri[flip] = tri[flip][:, [0, 2, 1]]
    return {"vertices": mesh_np["vertices"], "vertex_markers": mesh_np["vertex_markers"], "triangles": tri}


def _mesh(name):
    from pytorch_fem_solver_amd import meshgen

    if name.endswith(".npz"):
        return mesh_from_golden(load_golden(name))
    if name == "square_chunked":  # 4 tiles of consecutive vertices
        return meshgen.unit_square(30, 0.25, 4)
    if name == "square_multi_tile":  # 7 tiles, vertex ids and row offsets from the plan
        return meshgen.unit_square(40, 0.25, 1)
    if name == "delaunay_15_slots":  # 10 tiles, 15-slot records, rows of up to 12 entries
        return meshgen.delaunay_square(2500, 9)
    if name == "mixed_orientation":
        m = meshgen.unit_square(30, 0.25, 4)
        tri = m["triangles"].copy()
        flip = np.random.default_rng(5).random(tri.shape[0]) < 0.4
        tri[flip] = tri[flip][:, [0, 2, 1]]
        m["triangles"] = tri
        return m
    if name == "holes":  # removed elements, mixed orientation: open fans, flags 0 / 2, isolated rows
        return _holes(meshgen.unit_square(30, 0.25, 4))
    if name == "holes_delaunay":  # the same with 15-slot records
        return _holes(meshgen.delaunay_square(1500, 7), 7)
    if name == "shuffled":  # a numbering without locality: renumbered inside the engine (TFEM_RENUMBER=1)
        m = meshgen.unit_square(30, 0.25, 4)
        return meshgen.permute_mesh(m, vertex_order=np.random.default_rng(7).permutation(m["vertices"].shape[0]))
    raise KeyError(name)


def _engine(mesh_np, order, dtype=torch.float64):
    from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

    idx = torch.tensor(np.ascontiguousarray(mesh_np["triangles"], dtype=np.int32))
    verts = torch.tensor(np.ascontiguousarray(mesh_np["vertices"]), dtype=dtype)
    return AssemblyEngine(verts, idx, idx, verts.shape[0], 1, order)


def _program(fn):
    return None if fn is None else sref.to_native(*cref.ops_of(fn))


def _np_dtype(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def _record(ratio):
    RATIOS.append(ratio)


ENGINE_CASES = [
    ("p1_square_n8.npz", torch.float64), ("p1_square_n5_clockwise.npz", torch.float64),
    ("p1_delaunay_170.npz", torch.float64), ("p1_square_n6_float32.npz", torch.float32),
    ("square_chunked", torch.float64), ("square_multi_tile", torch.float64), ("square_multi_tile", torch.float32),
    ("delaunay_15_slots", torch.float64), ("delaunay_15_slots", torch.float32),
    ("mixed_orientation", torch.float64), ("holes", torch.float64), ("holes_delaunay", torch.float64),
    ("holes_delaunay", torch.float32),
]


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("mesh,dtype", ENGINE_CASES)
def test_c_abi_values_apply_and_diagonal_against_the_reference(mesh, dtype, order):
    """(a) tfem_p1_rings_coef and (c) tfem_p1_apply_rings_coef (K u, diag K) on the engine's plan."""
    from pytorch_fem_solver_amd import _native

    mesh_np = _mesh(mesh)
    eng = _engine(mesh_np, order, dtype)
    rings = eng.ring_plan()
    assert rings is not None and not eng.renumbered and int(rings["layout"][23]) == 0
    if mesh == "square_multi_tile":
        assert not rings["chunked"] and rings["n_tiles"] > 1 and int(rings["layout"][6]) == 7
    if mesh == "square_chunked":
        assert rings["chunked"] and rings["n_tiles"] > 1
    if mesh in ("delaunay_15_slots", "holes_delaunay"):
        assert int(rings["layout"][6]) == 15 and rings["n_tiles"] > 1
    d = eng._inputs()
    n = eng.n_dofs
    rng = np.random.default_rng(order)
    u_np = rng.standard_normal(n)
    for name, (alpha, beta, kappa, c) in FORMS.items():
        parts = cref.reference_parts(mesh_np, order, alpha, beta, kappa, c, _np_dtype(dtype))
        rowptr, colind, want, tol = parts[:4]
        crow, ccol = eng.csr_structure()[0].cpu().numpy(), eng.csr_structure()[1].cpu().numpy()
        assert np.array_equal(crow, rowptr) and np.array_equal(ccol, colind)
        pk, pc = _program(kappa), _program(c)
        ref_k = ctypes.byref(pk) if pk is not None else None
        ref_c = ctypes.byref(pc) if pc is not None else None
        head = (_native.ptr(d["coords"]), eng.real_bytes, n, order, alpha, beta, ref_k, ref_c,
                _native.ptr(rings["blob"]), c_void_p(rings["layout"].ctypes.data))
        vals = torch.full((colind.shape[0],), float("nan"), dtype=dtype)
        _native.check(eng.lib.tfem_p1_rings_coef(*head, _native.ptr(vals), eng._stream()))
        torch.cuda.synchronize()
        got = vals.double().cpu().numpy()
        _record(cref.check(got, want, tol, f"{mesh} {dtype} order {order} {name}: values"))
        # K u and diag K, without the values
        u = torch.tensor(u_np, dtype=dtype)
        y = torch.full((n,), float("nan"), dtype=dtype)
        _native.check(eng.lib.tfem_p1_apply_rings_coef(*head, _native.ptr(u), _native.ptr(y), eng._stream()))
        dg = torch.full((n,), float("nan"), dtype=dtype)
        _native.check(eng.lib.tfem_p1_apply_rings_coef(*head, None, _native.ptr(dg), eng._stream()))
        torch.cuda.synchronize()
        has_row = np.diff(rowptr) > 0
        want_y, tol_y = cref.apply_reference(parts, u.double().cpu().numpy())
        got_y = y.double().cpu().numpy()
        assert np.array_equal(got_y[~has_row], np.zeros(int((~has_row).sum())))  # a vertex without elements
        _record(cref.check(got_y[has_row], want_y[has_row], tol_y[has_row], f"{mesh} {name}: K u"))
        diag_at = np.array([rowptr[i] + np.searchsorted(colind[rowptr[i]:rowptr[i + 1]], i) for i in range(n) if has_row[i]])
        _, tol_d = cref.apply_reference(parts, np.ones(n))
        _record(cref.check(dg.double().cpu().numpy()[has_row], want[diag_at], tol_d[has_row], f"{mesh} {name}: diag K"))


def _basis(mesh_np, order):
    return tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, order))


class _Spy:
    """Counts the calls of the library's entry points that go through an engine."""

    NAMES = ("tfem_p1_rings_coef", "tfem_p1_apply_rings_coef", "tfem_p1_assemble_rings", "tfem_p1_apply_rings",
             "tfem_reduce_scatter_bilinear", "tfem_p1_assemble_rings_source", "tfem_p1_assemble_tiles",
             "tfem_tri_bilinear_csr")

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


#: every mesh of the C-ABI sweep and the renumbered one, through the public API
PUBLIC_CASES = ENGINE_CASES + [("shuffled", torch.float64)]


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("mesh,dtype", PUBLIC_CASES)
def test_public_layouts_operator_and_the_torch_path(mesh, dtype, order, monkeypatch):
    """(b) dense / csr / operator layouts, (c) matvec and diagonal, (d) TFEM_KERNEL=gather (the torch
    path) against the same reference, (e) no CSR values behind matvec."""
    mesh_np = _mesh(mesh)
    torch.set_default_dtype(dtype)
    npd = _np_dtype(dtype)

    def env():
        if mesh == "shuffled":
            monkeypatch.setenv("TFEM_RENUMBER", "1")

    def host(t):
        return t.double().cpu().numpy()

    env()
    n = mesh_np["vertices"].shape[0]
    u_np = np.random.default_rng(2).standard_normal(n).astype(npd).astype(np.float64)
    for name in ("kappa_xy", "c_exp", "kappa_poly_c_exp"):
        alpha, beta, kappa, c = FORMS[name]
        parts = cref.reference_parts(mesh_np, order, alpha, beta, kappa, c, npd)
        rowptr, colind, want, tol = parts[:4]
        want_dense, tol_dense = cref.dense(rowptr, colind, want, n), cref.dense(rowptr, colind, tol, n)
        want_y, tol_y = cref.apply_reference(parts, u_np)
        tol_d = cref.apply_reference(parts, np.ones(n))[1]
        a = cref.form(alpha, beta, kappa, c)
        what = f"{mesh} {npd.__name__} order {order} {name}"
        basis = _basis(mesh_np, order)
        assert basis._engine.dtype == dtype and basis._engine.renumbered == (mesh == "shuffled")
        spy = _Spy(monkeypatch, basis._engine.lib)
        K = basis.integrate_bilinear_form(a, layout="csr")
        assert K.dtype == dtype
        assert spy.calls["tfem_p1_rings_coef"] == 1 and spy.calls["tfem_reduce_scatter_bilinear"] == 0
        _record(cref.check(host(K.to_dense()), want_dense, tol_dense, f"{what}: csr"))
        D = basis.integrate_bilinear_form(a, layout="dense")
        assert isinstance(D, torch.Tensor) and D.shape == (n, n)
        _record(cref.check(host(D), want_dense, tol_dense, f"{what}: dense"))
        before = dict(spy.calls)
        op = basis.integrate_bilinear_form(a, layout="operator")
        assert op.matrix_free is True and "matrix-free, variable coefficients" in repr(op) and op.dtype == dtype
        u = torch.tensor(u_np, dtype=dtype)
        y = op.matvec(u)
        dg = op.diagonal()
        _record(cref.check(host(y), want_y, tol_y, f"{what}: op.matvec"))
        _record(cref.check(host(dg), np.diag(want_dense), tol_d, f"{what}: op.diagonal"))
        assert (op @ u.reshape(-1, 1)).shape == (n, 1)
        # (e) nothing was assembled for them
        assert spy.calls["tfem_p1_rings_coef"] == before["tfem_p1_rings_coef"]
        assert spy.calls["tfem_p1_apply_rings_coef"] == before["tfem_p1_apply_rings_coef"] + 3
        assert spy.calls["tfem_p1_assemble_rings"] == 0 and spy.calls["tfem_reduce_scatter_bilinear"] == 0
        assert op._csr is None
        # to_csr(): by the coefficient launch
        _record(cref.check(host(op.to_csr().to_dense()), want_dense, tol_dense, f"{what}: to_csr"))
        assert spy.calls["tfem_p1_rings_coef"] == before["tfem_p1_rings_coef"] + 1
        # the operator stays differentiable in the vector (K symmetric to rounding)
        ug = u.clone().requires_grad_(True)
        (op.matvec(ug) * u).sum().backward()
        _record(cref.check(host(ug.grad), want_y, tol_y, f"{what}: gradient"))
        monkeypatch.undo()
        env()
        # (d) the torch path of the same callable
        monkeypatch.setenv("TFEM_KERNEL", "gather")
        basis_t = _basis(mesh_np, order)
        spy_t = _Spy(monkeypatch, basis_t._engine.lib)
        Kt = basis_t.integrate_bilinear_form(a, layout="csr")
        assert spy_t.calls["tfem_p1_rings_coef"] == 0 and spy_t.calls["tfem_reduce_scatter_bilinear"] == 1
        _record(cref.check(host(Kt.to_dense()), want_dense, tol_dense, f"{what}: torch path"))
        op_t = basis_t.integrate_bilinear_form(a, layout="operator")
        assert op_t.matrix_free is False
        _record(cref.check(host(op_t.matvec(u)), want_y, tol_y, f"{what}: torch path matvec"))
        _record(cref.check(host(op_t.diagonal()), np.diag(want_dense), tol_d, f"{what}: torch path diagonal"))
        monkeypatch.undo()
        env()


@pytest.mark.parametrize("kernel", ["gather", "atomic", "tiles"])
def test_other_kernel_modes_keep_the_torch_path(kernel, monkeypatch):
    monkeypatch.setenv("TFEM_KERNEL", kernel)
    mesh_np = _mesh("square_chunked")
    n = mesh_np["vertices"].shape[0]
    alpha, beta, kappa, c = FORMS["kappa_trig_plain_mass"]
    basis = _basis(mesh_np, 3)
    assert basis._engine.bilinear_coef(alpha, beta, _program(kappa), None) is None
    spy = _Spy(monkeypatch, basis._engine.lib)
    K = basis.integrate_bilinear_form(cref.form(alpha, beta, kappa, c), layout="csr")
    assert spy.calls["tfem_p1_rings_coef"] == 0 and spy.calls["tfem_reduce_scatter_bilinear"] == 1
    rowptr, colind, want, tol = cref.reference(mesh_np, 3, alpha, beta, kappa, c)
    _record(cref.check(K.to_dense().cpu().numpy(), cref.dense(rowptr, colind, want, n),
                       cref.dense(rowptr, colind, tol, n), f"TFEM_KERNEL={kernel}"))


def test_p2_and_long_row_plans_take_the_torch_path(monkeypatch):
    mesh_np = _mesh("square_chunked")
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(2, 3))
    assert not basis._engine.supports_coefficients()
    spy = _Spy(monkeypatch, basis._engine.lib)
    K = basis.integrate_bilinear_form(cref.form(1.0, 0.0, cref.kappa_xy, None), layout="csr")
    assert spy.calls["tfem_p1_rings_coef"] == 0 and spy.calls["tfem_reduce_scatter_bilinear"] == 1
    assert K.shape[0] == basis._engine.n_dofs
    monkeypatch.undo()
    # a ring plan with long rows: the coefficient launch refuses it, the engine does not offer it
    monkeypatch.setenv("TFEM_RING_LONG", "1")
    from pytorch_fem_solver_amd import _native

    long_np = _mesh("delaunay_15_slots")
    eng = _engine(long_np, 3)
    rings = eng.ring_plan()
    assert rings is not None and int(rings["layout"][23]) > 0
    assert not eng.supports_coefficients() and eng.bilinear_coef(1.0, 0.0, _program(cref.kappa_xy), None) is None
    d = eng._inputs()
    pk = _program(cref.kappa_xy)
    vals = torch.zeros(int(eng.csr_structure()[1].shape[0]))
    st = eng.lib.tfem_p1_rings_coef(_native.ptr(d["coords"]), 8, eng.n_dofs, 3, 1.0, 0.0, ctypes.byref(pk), None,
                                    _native.ptr(rings["blob"]), c_void_p(rings["layout"].ctypes.data),
                                    _native.ptr(vals), eng._stream())
    assert st == 2  # TFEM_ERR_UNSUPPORTED
    basis_l = _basis(long_np, 3)
    n = long_np["vertices"].shape[0]
    K = basis_l.integrate_bilinear_form(cref.form(1.0, 0.0, cref.kappa_xy, None), layout="csr")
    rowptr, colind, want, tol = cref.reference(long_np, 3, 1.0, 0.0, cref.kappa_xy, None)
    _record(cref.check(K.to_dense().cpu().numpy(), cref.dense(rowptr, colind, want, n),
                       cref.dense(rowptr, colind, tol, n), "long-row plan: torch path"))


def test_constant_written_as_a_program_routes_to_the_constant_launch(monkeypatch):
    """(f) kappa = 2.5 as a field folds into the scalar: the launches of the constant form."""
    mesh_np = _mesh("square_chunked")
    basis = _basis(mesh_np, 3)
    spy = _Spy(monkeypatch, basis._engine.lib)

    def a(b):
        x, _ = torch.split(b.integration_points, 1, dim=-1)
        return (2.5 * torch.ones_like(x)) * (b.v_grad @ b.v_grad.mT)

    K = basis.integrate_bilinear_form(a, layout="csr")
    assert spy.calls["tfem_p1_assemble_rings"] == 1 and spy.calls["tfem_p1_rings_coef"] == 0
    plain = basis.integrate_bilinear_form(lambda b: 2.5 * (b.v_grad @ b.v_grad.mT), layout="csr")
    assert torch.equal(K.values, plain.values)
    op = basis.integrate_bilinear_form(a, layout="operator")
    op.matvec(torch.ones(op.shape[0]))
    assert spy.calls["tfem_p1_apply_rings"] == 1 and spy.calls["tfem_p1_apply_rings_coef"] == 0


def test_solve_cg_on_the_operator_and_assemble_system(monkeypatch):
    """-div(kappa grad u) + c u = f on the interior DoFs: CG on the matrix-free operator against
    torch.linalg.solve on the dense reference K, residual-based."""
    mesh_np = _mesh("square_multi_tile")
    n = mesh_np["vertices"].shape[0]
    alpha, beta, kappa, c = 1.0, 1.0, cref.kappa_trig, cref.c_exp
    a = cref.form(alpha, beta, kappa, c)

    def l(b):
        x, y = torch.split(b.integration_points, 1, dim=-1)
        return 2.0 * np.pi**2 * torch.sin(np.pi * x) * torch.sin(np.pi * y) * b.v

    runs = {"a": 0, "l": 0}

    def a_counted(b):
        runs["a"] += 1
        return a(b)

    def l_counted(b):
        runs["l"] += 1
        return l(b)

    # building the operator launches nothing and builds no plan (decided on first use)
    fresh = _basis(mesh_np, 3)
    lazy = fresh.integrate_bilinear_form(a, layout="operator")
    assert fresh._engine._rings is None and "unresolved" in repr(lazy)
    assert lazy.matrix_free is True and fresh._engine._rings is not None
    basis = _basis(mesh_np, 3)
    spy = _Spy(monkeypatch, basis._engine.lib)
    K, f = basis.assemble_system(a_counted, l_counted, layout="csr")
    assert runs == {"a": 1, "l": 1}  # every callable runs once
    assert spy.calls["tfem_p1_rings_coef"] == 1 and spy.calls["tfem_p1_assemble_rings_source"] == 1
    op = basis.integrate_bilinear_form(a, layout="operator")
    free = basis._basis_parameters["inner_dofs"]
    before = dict(spy.calls)
    x, it, res = op.solve_cg(f, free=free, rtol=1e-12)
    assert res <= 1e-12 and 0 < it < 10 * n
    assert spy.calls["tfem_p1_rings_coef"] == before["tfem_p1_rings_coef"] and op._csr is None  # (e)
    assert spy.calls["tfem_p1_apply_rings_coef"] >= it + 2
    rowptr, colind, want, _ = cref.reference(mesh_np, 3, alpha, beta, kappa, c)
    Kd = torch.tensor(cref.dense(rowptr, colind, want, n))
    idx = free.to(Kd.device).reshape(-1)
    direct = torch.linalg.solve(Kd[idx][:, idx], f.reshape(-1)[idx])
    # residual-based: ||K (x - direct)|| <= (rtol of both solves) ||f||
    diff = Kd[idx][:, idx] @ (x.reshape(-1)[idx] - direct)
    assert float(torch.linalg.vector_norm(diff) / torch.linalg.vector_norm(f.reshape(-1)[idx])) <= 1e-10
    # Basis.solve takes the operator unchanged
    sol = basis.solve(op, basis.solution_tensor().to(f.device, f.dtype), f)
    assert float((sol.reshape(-1)[idx] - direct).abs().max()) <= 1e-9 * float(direct.abs().max())


def test_error_codes_on_the_device():
    from pytorch_fem_solver_amd import _native

    mesh_np = _mesh("p1_square_n8.npz")
    eng = _engine(mesh_np, 3)
    rings = eng.ring_plan()
    d = eng._inputs()
    vals = torch.full((int(eng.csr_structure()[1].shape[0]),), 7.0)
    bad = _native.SourceProgram()
    bad.n_ops = 1
    bad.ops[0] = 7  # MUL on an empty stack
    good = _program(cref.kappa_xy)

    def call(n_verts, kappa, c):
        return eng.lib.tfem_p1_rings_coef(
            _native.ptr(d["coords"]), 8, n_verts, 3, 1.0, 1.0, kappa, c, _native.ptr(rings["blob"]),
            c_void_p(rings["layout"].ctypes.data), _native.ptr(vals), eng._stream())

    assert call(eng.n_dofs, None, None) == 1
    assert call(eng.n_dofs, ctypes.byref(bad), None) == 1
    assert call(eng.n_dofs, ctypes.byref(good), ctypes.byref(bad)) == 1
    assert call(0, ctypes.byref(good), None) == 0
    torch.cuda.synchronize()
    assert bool((vals == 7.0).all())  # nothing was launched


def test_full_size_row_sums_and_matvec():
    """S(2236), order 3, kappa = 1 + x y: the rows of the assembled stiffness part sum to zero, and
    K u without the values agrees with tfem_csr_spmv on them."""
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(2236, 0.25, 0)
    basis = _basis(mesh_np, 3)
    a = cref.form(1.0, 0.0, cref.kappa_xy, None)
    K = basis.integrate_bilinear_form(a, layout="csr")
    n = K.shape[0]
    kmax = float(K.values.abs().max())
    sums = K.matvec(torch.ones(n))
    print(f"full size: max |row sum| / max |K| = {float(sums.abs().max()) / kmax:.3e}")
    assert float(sums.abs().max()) <= 1e-12 * kmax
    op = basis.integrate_bilinear_form(a, layout="operator")
    assert op.matrix_free is True
    u = torch.tensor(np.random.default_rng(1).standard_normal(n))
    y, want = op.matvec(u), K.matvec(u)
    absK = tf().CSRMatrix(K.crow_indices, K.col_indices, K.values.abs(), K.shape, K.perm)
    scale = absK.matvec(u.abs())
    ratio = float(((y - want).abs() / scale.clamp_min(1e-300)).max())
    print(f"full size: max |K u - spmv| / sum |K_ij u_j| = {ratio:.3e}")
    assert ratio <= 1e-12


def test_example_runs():
    """examples/poisson_variable_coefficient.py: exit code 0, its own assertions are the checks
    (matrix-free operator, h^2 convergence in L2, agreement with the CSR solve)."""
    import os
    import subprocess
    import sys

    from conftest import REPO

    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_variable_coefficient.py"), "32"],
                          capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "variable coefficients" in done.stdout and "error ratio" in done.stdout
