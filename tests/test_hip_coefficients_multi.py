"""The variable-coefficient P1 operator on several vectors in one launch
(tfem_p1_apply_rings_coef_multi, k_p1_coef_rows_multi in csrc/tfem_rings_coef_multi.hip) on a real
MI355X: every column of K U against the reference of tests/coefficient_reference.py (its
tolerance rule, per column) and BIT FOR BIT against the single-vector launch
(tfem_p1_apply_rings_coef) on that column; the C ABI and its refusals; one call per block; the
gradient; block CG; a small sweep over the random meshes of tests/operator_reference.py."""

import ctypes
import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import coefficient_reference as cref
import operator_reference as oref
import source_reference as sref
from conftest import load_golden, mesh_from_golden, scaled_error
from random_meshes import has_elements
from test_hip_operator import _case, tf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: (alpha, beta, kappa, c): both fields, both fields again, stiffness alone (no mass term in the
#: kernel), a plain stiffness beside a field in the mass (has_kappa = 0), the mass alone
FORMS = {
    "trig_exp": (1.0, 0.5, cref.kappa_trig, cref.c_exp),
    "poly_rational": (0.5, 2.0, cref.kappa_poly, cref.c_rational),
    "xy_stiffness_only": (1.0, 0.0, cref.kappa_xy, None),
    "plain_stiffness_exp": (1.0, 1.0, None, cref.c_exp),
    "rational_mass_only": (0.0, 1.0, None, cref.c_rational),
}
#: one pass (2, 4), a pass with a dropped column (3), several passes with a narrow tail (5, 8, 11)
WIDTHS = (2, 3, 4, 5, 8, 11)
#: the two operators of the sweep (tests/test_hip_operator_fuzz.py's COEFFICIENT_FORMS)
COEFFICIENT_FORMS = ((1.0, 0.5, cref.kappa_trig, cref.c_exp), (0.5, 2.0, cref.kappa_poly, cref.c_rational))


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def host(t):
    return t.detach().double().cpu().numpy()


def _basis(mesh_np, order=3):
    return tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, order))


def _program(fn):
    return None if fn is None else sref.to_native(*cref.ops_of(fn))


def _mesh(name):
    from pytorch_fem_solver_amd import meshgen

    if name == "square_multi_tile":
        return meshgen.unit_square(40, 0.25, 1)
    return _case(name)


def check_columns(got, parts, U_np, what):
    """Every column of `got` against K^ref U[:, c] within the tolerance of coefficient_reference."""
    got = host(got)
    has_row = np.diff(parts[0]) > 0
    worst = 0.0
    for c in range(got.shape[1]):
        want, tol = cref.apply_reference(parts, U_np[:, c])
        assert (got[~has_row, c] == 0.0).all(), f"{what}: a row without elements is not exactly zero"
        worst = max(worst, cref.check(got[has_row, c], want[has_row], tol[has_row], f"{what}, column {c}"))
    return worst


def check_block(op, parts, U, widths, what):
    """op @ U[:, :k] for every width: the reference per column, bit identity with the single
    launch per column, non-contiguous blocks."""
    n, kmax = U.shape
    U_np = host(U)
    single = [op.matvec(U[:, j].contiguous()) for j in range(kmax)]
    for k in widths:
        Uk = U[:, :k].contiguous()
        got = op @ Uk
        assert got.shape == (n, k) and got.dtype == op.dtype
        check_columns(got, parts, U_np[:, :k], f"{what}, k = {k}")
        for j in range(k):
            assert torch.equal(got[:, j], single[j]), f"{what}, k = {k}: column {j} differs from the single launch"
        if k < kmax:  # a column slice of the wider block
            assert not U[:, :k].is_contiguous() and torch.equal(op.matvec(U[:, :k]), got)
        Ut = Uk.t().contiguous().t()  # a transposed view
        assert not Ut.is_contiguous() and torch.equal(op @ Ut, got)


@pytest.mark.parametrize("which", list(FORMS))
@pytest.mark.parametrize("mesh", ["square_multi_tile", "structured", "p1_delaunay_170.npz", "delaunay_generator_order"])
def test_block_matches_the_reference_and_the_single_launch_bit_for_bit(mesh, which):
    alpha, beta, kappa, c = FORMS[which]
    mesh_np = _mesh(mesh)
    basis = _basis(mesh_np)
    eng = basis._engine
    op = basis.integrate_bilinear_form(cref.form(alpha, beta, kappa, c), layout="operator")
    assert op.matrix_free is True and op._programs is not None and op.dtype == torch.float64
    rings = eng.ring_plan()
    pick = "the generator no longer produces such a plan for this mesh: pick another one"
    if mesh == "square_multi_tile":
        assert not rings["chunked"] and rings["n_tiles"] > 1 and int(rings["layout"][6]) == 7 and not eng.renumbered, pick
    if mesh == "structured":
        assert rings["chunked"] and rings["n_tiles"] > 1, pick
    if mesh == "delaunay_generator_order":
        assert eng.renumbered and int(rings["layout"][6]) == 15, pick
    n = op.shape[0]
    parts = cref.reference_parts(mesh_np, 3, alpha, beta, kappa, c, np.float64)
    U = torch.tensor(np.random.default_rng(3).standard_normal((n, max(WIDTHS))))
    check_block(op, parts, U, WIDTHS, f"{mesh} {which}")
    if eng.renumbered:  # the launches themselves, in the engine's numbering
        Ue = eng._dofs_in(U).contiguous()
        for k in WIDTHS:
            Y = eng._apply_rings_coef(op.alpha, op.beta, *op._programs, Ue[:, :k].contiguous())
            for j in range(k):
                one = eng._apply_rings_coef(op.alpha, op.beta, *op._programs, Ue[:, j].contiguous())
                assert torch.equal(Y[:, j], one), f"engine numbering, k = {k}, column {j}"


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_block_at_every_quadrature_order(order):
    """Orders 1 .. 4 are the instances with 1, 3, 4 and 6 points."""
    alpha, beta, kappa, c = FORMS["trig_exp"]
    mesh_np = _mesh("square_multi_tile")
    basis = _basis(mesh_np, order)
    op = basis.integrate_bilinear_form(cref.form(alpha, beta, kappa, c), layout="operator")
    assert op.matrix_free is True and op._programs is not None
    parts = cref.reference_parts(mesh_np, order, alpha, beta, kappa, c, np.float64)
    U = torch.tensor(np.random.default_rng(order).standard_normal((op.shape[0], 4)))
    check_block(op, parts, U, (3, 4), f"order {order}")


def test_block_float32():
    mesh_np = mesh_from_golden(load_golden("p1_square_n6_float32.npz"))
    torch.set_default_dtype(torch.float32)
    basis = _basis(mesh_np)
    for which, (alpha, beta, kappa, c) in FORMS.items():
        op = basis.integrate_bilinear_form(cref.form(alpha, beta, kappa, c), layout="operator")
        assert op.matrix_free is True and op.dtype == torch.float32
        parts = cref.reference_parts(mesh_np, 3, alpha, beta, kappa, c, np.float32)
        U = torch.tensor(np.random.default_rng(4).standard_normal((op.shape[0], 5)).astype(np.float32))
        check_block(op, parts, U, (2, 5), f"float32 {which}")


#: a seed of the operator sweep with coefficients, float64, isolated vertices and no renumbering
#: (3310 vertices, 5 of them without elements, 13 tiles of 15-slot records)
ISOLATED_SEED = 12


def _sweep_basis(case, monkeypatch):
    for key, on in (("TFEM_RENUMBER", case["renumber"]), ("TFEM_RING_LONG", case["long_rows"])):
        if on:
            monkeypatch.setenv(key, "1")
        else:
            monkeypatch.delenv(key, raising=False)
    torch.set_default_dtype(torch.float32 if case["single"] else torch.float64)
    verts, tris = case["verts"], case["tris"]
    outer = ((np.abs(verts) <= 1e-12) | (np.abs(verts - 1.0) <= 1e-12)).any(axis=1)
    mesh_np = {"vertices": verts, "triangles": tris.astype(np.int64) if case["int64"] else tris,
               "vertex_markers": outer.astype(np.int32).reshape(-1, 1)}
    return _basis(mesh_np, case["order"])


def test_every_entry_is_written_once_and_no_column_leaks(monkeypatch):
    case = oref.sweep_case(ISOLATED_SEED)
    assert case["coefficients"] and case["isolated"] > 0 and not case["single"] and not case["renumber"], \
        "the sweep's generator changed: pick another seed with isolated vertices"
    basis = _sweep_basis(case, monkeypatch)
    eng = basis._engine
    n = eng.n_dofs
    lone = torch.tensor(~has_elements(case["tris"], n))
    alpha, beta, kappa, c = FORMS["trig_exp"]
    op = basis.integrate_bilinear_form(cref.form(alpha, beta, kappa, c), layout="operator")
    assert op.matrix_free is True and not eng.renumbered
    rng = np.random.default_rng(9)
    for k in (3, 5):
        U = torch.tensor(rng.standard_normal((n, k)))
        want = eng._apply_rings_coef(op.alpha, op.beta, *op._programs, U)
        out = torch.full((n * k,), float("nan"))
        got = eng._apply_rings_coef(op.alpha, op.beta, *op._programs, U, out=out)
        assert got.data_ptr() == out.data_ptr() and bool(torch.isfinite(out).all()), "entries of Y were left unwritten"
        assert torch.equal(got, want)
        assert bool((got[lone] == 0.0).all()) and int(lone.sum()) > 0
        # a column of NaN stays in its column (every pass fetches NV columns, whatever it stores)
        poisoned = U.clone()
        poisoned[:, 2] = float("nan")
        leak = eng._apply_rings_coef(op.alpha, op.beta, *op._programs, poisoned)
        keep = [j for j in range(k) if j != 2]
        assert torch.equal(leak[:, keep], want[:, keep]), f"k = {k}: column 2 leaked into another column"
        assert bool(torch.isnan(leak[~lone][:, 2]).all())


def counted(lib, monkeypatch, names):
    counts = dict.fromkeys(names, 0)

    def wrap(name):
        inner = getattr(lib, name)

        def call(*args):
            counts[name] += 1
            return inner(*args)

        monkeypatch.setattr(lib, name, call, raising=True)

    for name in names:
        wrap(name)
    return counts


def test_a_block_is_one_call_not_k(monkeypatch):
    from test_hip_fused_cg import build_case

    case, basis, free_np = build_case(7, monkeypatch)
    alpha, beta, kappa, c = FORMS["trig_exp"]
    op = basis.integrate_bilinear_form(cref.form(alpha, beta, kappa, c), layout="operator")
    assert op.matrix_free is True and op._programs is not None
    lib = basis._engine.lib
    names = ("tfem_p1_apply_rings_coef_multi", "tfem_p1_apply_rings_coef")
    B, free = torch.tensor(oref.cg_loads(case)), torch.tensor(free_np)
    U = torch.rand(op.shape[0], 5)
    with monkeypatch.context() as m:
        counts = counted(lib, m, names)
        op @ U
        print(counts)
        assert counts == {"tfem_p1_apply_rings_coef_multi": 1, "tfem_p1_apply_rings_coef": 0}
    with monkeypatch.context() as m:
        counts = counted(lib, m, names)
        _, its, _ = op.solve_cg_multi(B[:, :2].contiguous(), free=free, rtol=0.0, maxiter=50, loop="fused")
        print(counts)
        assert its.tolist() == [50, 50]
        # 50 iterations and the residual of the set-up; the diagonal is the single launch without u
        assert counts == {"tfem_p1_apply_rings_coef_multi": 50 + 1, "tfem_p1_apply_rings_coef": 1}


def test_c_abi_single_column_three_columns_and_every_refusal(monkeypatch):
    from pytorch_fem_solver_amd import _native, meshgen
    from test_hip_coefficients import _engine

    IA, UN, IR = 1, 2, 4  # TFEM_ERR_INVALID_ARGUMENT, TFEM_ERR_UNSUPPORTED, TFEM_ERR_INDEX_RANGE
    mesh_np = meshgen.unit_square(40, 0.25, 4)
    basis = _basis(mesh_np)
    eng = basis._engine
    rings, d, n = eng._coef_rings(), eng._inputs(), eng.n_dofs
    assert rings is not None and not eng.renumbered
    lib, stream = eng.lib, eng._stream()
    alpha, beta, kappa, c = FORMS["trig_exp"]
    pk, pc = _program(kappa), _program(c)
    coords, blob, layout = _native.ptr(d["coords"]), _native.ptr(rings["blob"]), c_void_p(rings["layout"].ctypes.data)

    def multi(u, y, n_vec, real_bytes=8, n_verts=n, order=3, kappa=ctypes.byref(pk), c=ctypes.byref(pc), z=layout,
              plan=blob):
        return lib.tfem_p1_apply_rings_coef_multi(coords, real_bytes, n_verts, order, alpha, beta, kappa, c, plan, z,
                                                  u, y, n_vec, stream)

    u = torch.rand(n)
    y1, ym = torch.full((n,), float("nan")), torch.full((n,), float("nan"))
    _native.check(lib.tfem_p1_apply_rings_coef(coords, 8, n, 3, alpha, beta, ctypes.byref(pk), ctypes.byref(pc), blob,
                                               layout, _native.ptr(u), _native.ptr(y1), stream))
    _native.check(multi(_native.ptr(u), _native.ptr(ym), 1))
    torch.cuda.synchronize()
    assert torch.equal(y1, ym)  # n_vec = 1 is the single-vector launch
    U = torch.rand(n, 3)
    Y = torch.full((n, 3), float("nan"))
    _native.check(multi(_native.ptr(U), _native.ptr(Y), 3))
    torch.cuda.synchronize()
    parts = cref.reference_parts(mesh_np, 3, alpha, beta, kappa, c, np.float64)
    check_columns(Y, parts, host(U), "three columns through the entry point")
    # an empty plan and n_verts = 0 succeed and launch nothing
    Y.fill_(7.0)
    empty = np.zeros(32, dtype=np.int64)
    assert multi(_native.ptr(U), _native.ptr(Y), 3, z=c_void_p(empty.ctypes.data)) == 0
    assert multi(_native.ptr(U), _native.ptr(Y), 3, n_verts=0) == 0
    # a plan with long rows
    monkeypatch.setenv("TFEM_RING_LONG", "1")
    long_eng = _engine(meshgen.delaunay_square(7000, 21), 3)
    long_rings = long_eng.ring_plan()
    monkeypatch.delenv("TFEM_RING_LONG")
    assert long_rings is not None and int(long_rings["layout"][23]) > 0
    long_z = c_void_p(long_rings["layout"].ctypes.data)
    long_plan = _native.ptr(long_rings["blob"])
    bad = _native.SourceProgram()
    bad.n_ops = 2
    bad.ops[0], bad.ops[1] = 4, 4  # ADD on an empty stack
    buf = torch.rand(4 * n)
    pu, py = _native.ptr(U), _native.ptr(Y)
    over_u, over_y = _native.ptr(buf), c_void_p(buf.data_ptr() + 8 * n)
    too_many = (1 << 29) // n + 1  # n * n_vec * 8 bytes >= 2^32
    # every refusal in the order of the checks; each call also carries the NEXT refusal's fault (or a
    # later one of another status), so a check out of order shows
    refused = {
        "1 real_bytes": (multi(pu, py, 3, real_bytes=2, z=None), IA),
        "2 NULL layout": (multi(pu, py, 3, z=None, n_verts=-1), IA),
        "3 n_verts < 0": (multi(pu, py, 0, n_verts=-1), IA),
        "4 n_vec 0": (multi(None, py, 0), IA),
        "4 n_vec -1": (multi(pu, py, -1), IA),
        "5 u NULL": (multi(None, py, too_many, kappa=None, c=None), IA),
        "6 both programs NULL": (multi(pu, py, too_many, kappa=None, c=None), IA),
        "7 extent": (multi(over_u, over_y, too_many), IR),
        "7 extent 2^62": (multi(pu, py, 1 << 62, z=long_z, plan=long_plan), IR),
        "8 overlap": (multi(over_u, over_y, 2, z=long_z, plan=long_plan), IA),
        "8 same": (multi(over_u, over_u, 2, order=9), IA),
        "9 invalid kappa": (multi(pu, py, 3, kappa=ctypes.byref(bad), z=long_z, plan=long_plan), IA),
        "9 invalid c": (multi(pu, py, 3, c=ctypes.byref(bad), order=9), IA),
        "10 long rows": (multi(pu, py, 3, z=long_z, plan=long_plan), UN),
        "10 long rows, one column": (multi(pu, py, 1, z=long_z, plan=long_plan), UN),
        "11 unknown order": (multi(pu, py, 3, order=9), UN),
    }
    torch.cuda.synchronize()
    assert {k: v[0] for k, v in refused.items()} == {k: v[1] for k, v in refused.items()}
    assert b"order" in lib.tfem_last_error().lower()
    assert multi(pu, py, 3, z=long_z, plan=long_plan, order=9) == UN and b"long rows" in lib.tfem_last_error()
    torch.cuda.synchronize()
    assert bool((Y == 7.0).all()), "a refused call wrote to Y"
    # the engine refuses out = u and a wrong number of rows
    with pytest.raises(ValueError):
        eng._apply_rings_coef(alpha, beta, pk, pc, U, out=U)
    with pytest.raises(ValueError):
        eng._apply_rings_coef(alpha, beta, pk, pc, torch.rand(n + 1, 3))


def test_block_cg_on_the_coefficient_operator(monkeypatch):
    """The system of test_hip_fused_cg.test_fused_loop_on_the_coefficient_operator for one seed (its
    block solve now takes the block launch), then Basis.solve with an (N, 3) right-hand side."""
    from pytorch_fem_solver_amd import meshgen
    from test_hip_fused_cg import LD, build_case, compare_loops

    seed = 26
    case, basis, free_np = build_case(seed, monkeypatch)
    a, b, kappa, c = FORMS["trig_exp"]
    opc = basis.integrate_bilinear_form(cref.form(a, b, kappa, c), layout="operator")
    assert opc.matrix_free is True and opc._programs is not None
    plain_mesh = {"vertices": case["verts"], "triangles": case["tris"]}
    rowptr, colind, vals = cref.reference_parts(plain_mesh, case["order"], a, b, kappa, c, np.float64)[:3]
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))

    def apply_ld(x):
        y = np.zeros(rowptr.size - 1, dtype=LD)
        np.add.at(y, rows, vals.astype(LD) * np.asarray(x).astype(LD)[colind])
        return y

    with monkeypatch.context() as m:
        counts = counted(basis._engine.lib, m, ("tfem_p1_apply_rings_coef_multi",))
        compare_loops(opc, oref.cg_loads(case), oref.cg_start(case), free_np, apply_ld, f"seed {seed}, coefficients")
        assert counts["tfem_p1_apply_rings_coef_multi"] > 0
    monkeypatch.delenv("TFEM_RENUMBER", raising=False)
    # Basis.solve with (N, 3) against three solve_cg solves
    basis = _basis(meshgen.unit_square(40, 0.25, 1))
    op = basis.integrate_bilinear_form(cref.form(a, b, kappa, c), layout="operator")

    def source(i, j):
        def linear(bb):
            x, y = torch.split(bb.integration_points, 1, dim=-1)
            return np.pi**2 * (i * i + j * j) * torch.sin(i * np.pi * x) * torch.sin(j * np.pi * y) * bb.v
        return linear

    F = torch.cat([basis.integrate_linear_form(source(i, j)) for i, j in ((1, 1), (2, 1), (1, 3))], dim=1)
    free = basis._basis_parameters["inner_dofs"]
    sol = basis.solve(op, torch.zeros_like(F), F)
    assert sol.shape == F.shape
    for j in range(3):
        x, it, res = op.solve_cg(F[:, j].contiguous(), free=free)
        err = scaled_error(sol[:, j].cpu(), x.reshape(-1).cpu())
        print(f"column {j}: Basis.solve against solve_cg ({it} iterations) {err:.2e}")
        assert err <= 1e-8


def test_block_matvec_of_the_coefficient_operator_is_differentiable_in_u():
    from pytorch_fem_solver_amd import meshgen

    basis = _basis(meshgen.unit_square(12, 0.25, 3))
    op = basis.integrate_bilinear_form(cref.form(*FORMS["trig_exp"]), layout="operator")
    assert op.matrix_free is True and op._programs is not None
    U = torch.rand(op.shape[0], 3, requires_grad=True)
    (g,) = torch.autograd.grad((op @ U).sum(), U)
    # d/dU sum(K U) = K^T ones, applied as K ones (the backward's symmetry): the forward launch on ones
    assert g.shape == U.shape and torch.equal(g, op @ torch.ones_like(U))


SWEEP = {}  # seed -> what it met
#: the seeds below 40 whose sweep_case has "coefficients" true (even, not under TFEM_RING_LONG=1),
#: spelled out so that collecting this file draws no mesh
SWEEP_SEEDS = [s for s in range(40) if s % 2 == 0 and s % 10 not in oref.LONG_ROW_SEEDS]


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_small_sweep_of_random_meshes(seed, monkeypatch):
    case = oref.sweep_case(seed)
    assert case["coefficients"]
    basis = _sweep_basis(case, monkeypatch)
    eng = basis._engine
    single = case["single"]
    dtype = torch.float32 if single else torch.float64
    npd = np.float32 if single else np.float64
    n, k, order = case["verts"].shape[0], case["k"], case["order"]
    rings = eng.ring_plan()
    assert eng.dtype == dtype and eng.renumbered == case["renumber"] and rings is not None
    U = torch.tensor(case["U"])
    U_np = case["U"].astype(np.float64)
    plain_mesh = {"vertices": case["verts"], "triangles": case["tris"]}
    for a, b, kappa, c in COEFFICIENT_FORMS:
        what = f"seed {seed}, {kappa.__name__} / {c.__name__}, k = {k}"
        op = basis.integrate_bilinear_form(cref.form(a, b, kappa, c), layout="operator")
        assert op.matrix_free is True and op._programs is not None
        parts = cref.reference_parts(plain_mesh, order, a, b, kappa, c, npd)
        check_columns(op @ U, parts, U_np, what)
        Ue = eng._dofs_in(U).contiguous()
        out = torch.full((n * k,), float("nan"), dtype=dtype)
        Y = eng._apply_rings_coef(op.alpha, op.beta, *op._programs, Ue, out=out)
        assert bool(torch.isfinite(out).all()), f"{what}: entries of Y were left unwritten"
        for j in range(k):
            one = eng._apply_rings_coef(op.alpha, op.beta, *op._programs, Ue[:, j].contiguous())
            assert torch.equal(Y[:, j], one), f"{what}: column {j} differs from the single launch"
    SWEEP[seed] = {"slots": int(rings["layout"][6]), "chunked": bool(rings["chunked"]),
                   "renumbered": bool(eng.renumbered), "float32": single, "k": k}


def test_small_sweep_met_what_it_is_there_for():
    """Runs last.  The plans of these 16 seeds were looked at beforehand on the CPU
    (operator_reference.plan_of): 7-slot records 10, 15-slot 6, chunked 10, renumbered 6, float32 1
    (seed 20), k above 4: 10."""
    if len(SWEEP) < len(SWEEP_SEEDS):
        pytest.skip(f"only {len(SWEEP)} of {len(SWEEP_SEEDS)} seeds ran in this session")
    met = list(SWEEP.values())
    print(f"[coefficient block sweep] {SWEEP}")
    assert len(met) >= 10
    assert any(r["slots"] == 7 for r in met) and any(r["slots"] == 15 for r in met)
    assert any(r["chunked"] for r in met) and any(not r["chunked"] for r in met)
    assert any(r["renumbered"] for r in met) and any(r["float32"] for r in met) and any(r["k"] > 4 for r in met)


def test_variable_coefficient_loads_example_runs():
    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_variable_coefficient_loads.py"), "120"],
                          capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "block solve" in done.stdout, "the example prints what it computed"
