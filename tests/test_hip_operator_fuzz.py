"""Seeded random sweep of the matrix-free P1 operator stack on a real MI355X (-m gpu): the apply
kernels (k_p1_apply_rows, k_p1_apply_long_rows and their _multi forms), the variable-coefficient
apply (csrc/tfem_rings_coef.hip), the operator diagonal, k_csr_spmv, solve_cg and solve_cg_multi,
on the mesh family of tests/test_hip_fuzz.py (tests/random_meshes.py: removed elements, open fans,
isolated vertices, flipped orientation, rotated local numbering, shuffled / Morton vertex order,
shuffled element order), int32 and int64 connectivity, float64 and float32, every third seed
renumbered inside the engine (TFEM_RENUMBER=1), three seeds in ten with long rows
(TFEM_RING_LONG=1).  tests/operator_reference.sweep_case(seed) draws a seed's case; the rng is
default_rng(5000 + seed).

The reference is tests/operator_reference.py: the repository's oracle run in long double (64-bit
mantissa), NOT the float64 oracle, whose own rounding is of the size of the bound.  Every launch
that can be handed a result buffer gets one filled with NaN: "every kernel writes each entry
exactly once, so nothing is cleared" (engine._output) is checked for rows without elements, for
rows the tile launch leaves to the long-row launch, and for every column of every pass of a block.

Tolerances (none of them comes from a kernel's output):

  float64   1e-12 row-scaled (TOL of tests/test_hip_operator.py): K u and SpMV against
            sum_j |K_ij u_j|, diag K, CSR values and dense entries against sum_j |K_ij|.
  float32   8 x the worst row-scaled error of the ORACLE ITSELF run in float32 (coordinates, tables,
            coefficients, values and row sums in float32) against the long-double reference on the
            same float32-rounded coordinates, over the 11 float32 seeds of the sweep.  Measured on
            the CPU by `python tests/operator_reference.py` (measure_float32):
                K u     worst 4.306e-05 (seed 51)  ->  bound 3.445e-04
                diag K  worst 3.622e-05 (seed 51)  ->  bound 2.898e-04
            The factor 8 covers the different summation order of a fan and the reciprocal with one
            Newton step.
  CG        the recurrence residual meets rtol by construction; the TRUE residual ||b - K x|| on
            the free DoFs, from the long-double reference matrix, may exceed it by the drift between
            the two: true <= rtol * (1 + c).  c = 4 x the worst |true - recurrence| / rtol of
            sparse.conjugate_gradients run on the CPU with the float64 oracle's CSR operator
            (torch) over the 36 CG seeds, both non-zero loads, rtol = 1e-10 (measure_cg in the
            same command): worst 2.064e-03 (seed 75), c = 8.256e-03.
  variable coefficients   tests/coefficient_reference.py: its float64 reference, its tolerance rule.
  block CG against CG column by column   scaled error <= 1e-8, iteration counts within 25: the
            bounds of tests/test_hip_operator_multi.py for that comparison.

Where CG runs is decided by operator_reference.cg_free_dofs (its docstring says why: the forms
use the signed determinant, a mesh with clockwise elements has an indefinite operator).

The last test prints what the seeds reached (record widths, long rows, renumbering, isolated
vertices, index and real types, block widths, CG and coefficient seeds) and asserts lower limits
on them.  operator_reference.route_counts() gives for the plans of the 100 default seeds, on the CPU:
    matrix-free 100, 7-slot records 67, 15-slot records 33, chunked 65, isolated vertices 31,
    long rows listed 11, float32 11, int64 52, CG 36, coefficients 40."""

import os

import numpy as np
import pytest
import torch

import coefficient_reference as cref
import operator_reference as oref
from conftest import scaled_error
from random_meshes import has_elements
from test_hip_operator import TOL, form, tf

pytestmark = pytest.mark.gpu

#: TFEM_FUZZ_SEEDS=n shortens or widens the sweep (developer runs), as in tests/test_hip_fuzz.py
N_SEEDS = int(os.environ.get("TFEM_FUZZ_SEEDS", "100"))

TOL32_APPLY = 8 * 4.306e-05
TOL32_DIAG = 8 * 3.622e-05
CG_RTOL = 1e-10
CG_C = 4 * 2.064e-03
#: K.to_dense() is compared on meshes up to this many vertices
DENSE_MAX_VERTS = 1500
#: (alpha, beta, kappa, c) of the two variable-coefficient operators
COEFFICIENT_FORMS = ((1.0, 0.5, cref.kappa_trig, cref.c_exp), (0.5, 2.0, cref.kappa_poly, cref.c_rational))

ROUTES = {}  # seed -> what the seed exercised


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


def poisoned(numel, dtype):
    return torch.full((numel,), float("nan"), dtype=dtype)


def check_rows(got, want, scale, tol, what):
    """Row-scaled error of a vector (or column by column of a block) against the long-double
    reference; printed before it is asserted."""
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    assert np.isfinite(got).all(), f"{what}: not finite"
    if got.ndim == 2:
        err = max(oref.row_error(got[:, c], want[:, c], scale[:, c]) for c in range(got.shape[1]))
    else:
        err = oref.row_error(got, want, scale)
    print(f"{what}: {err:.3e} (bound {tol:.3e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return err


def run_case(case, monkeypatch):
    """One seed of the sweep: every check of this file on the case's mesh."""
    seed = case["seed"]
    for key, on in (("TFEM_RENUMBER", case["renumber"]), ("TFEM_RING_LONG", case["long_rows"])):
        if on:
            monkeypatch.setenv(key, "1")
        else:
            monkeypatch.delenv(key, raising=False)
    single = case["single"]
    dtype = torch.float32 if single else torch.float64
    torch.set_default_dtype(dtype)
    tol_apply, tol_diag = (TOL32_APPLY, TOL32_DIAG) if single else (TOL, TOL)
    verts, tris = case["verts"], case["tris"]
    order, alpha, beta, k = case["order"], case["alpha"], case["beta"], case["k"]
    n = verts.shape[0]
    lone = ~has_elements(tris, n)
    outer = ((np.abs(verts) <= 1e-12) | (np.abs(verts - 1.0) <= 1e-12)).any(axis=1)
    mesh_np = {"vertices": verts, "triangles": tris.astype(np.int64) if case["int64"] else tris,
               "vertex_markers": outer.astype(np.int32).reshape(-1, 1)}
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, order))
    op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
    K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
    eng = basis._engine
    assert eng.dtype == dtype and op.dtype == dtype and K.dtype == dtype
    matrix_free = bool(op.matrix_free)
    rings = eng.ring_plan()
    route = ROUTES[seed] = {
        "matrix_free": matrix_free, "slots": int(rings["layout"][6]) if rings else 0,
        "chunked": bool(rings["chunked"]) if rings else False, "renumbered": bool(eng.renumbered),
        "long_rows": int(rings["layout"][23]) if rings else 0, "long_mode": case["long_rows"],
        "isolated": int(lone.sum()), "int64": case["int64"], "float32": single, "k": k,
        "n": n, "cg": False, "coefficients": False,
    }
    print(f"seed {seed}: {route}")
    assert matrix_free, "no ring plan for a mesh of this family"
    assert eng.renumbered == case["renumber"]

    ref = oref.OperatorReference(verts, tris, order, alpha, beta)
    u = torch.tensor(case["u"])
    assert u.dtype == dtype
    want, scale = ref.apply(case["u"])
    want_d, scale_d = ref.diagonal()
    assert (scale[lone] == 0).all() and (scale_d[lone] == 0).all()

    # ---- y = K u
    got = op.matvec(u)
    assert got.shape == (n,) and got.dtype == dtype
    check_rows(got, want, scale, tol_apply, "op.matvec")
    assert (host(got)[lone] == 0.0).all(), "a row without elements is not exactly zero"
    out = poisoned(n, dtype)
    assert torch.equal(eng.apply(alpha, beta, u, out=out), got) and bool(torch.isfinite(out).all())
    # the launch itself into a poisoned buffer (a renumbered engine's apply() copies into `out`)
    raw = poisoned(n, dtype)
    eng._apply_rings(alpha, beta, eng._dofs_in(u), out=raw)
    assert bool(torch.isfinite(raw).all()), "the apply launch left entries of y unwritten"
    assert torch.equal(eng._dofs_out(raw), got)

    # ---- diag K
    d_op = op.diagonal()
    check_rows(d_op, want_d, scale_d, tol_diag, "op.diagonal")
    assert (host(d_op)[lone] == 0.0).all()
    raw = poisoned(n, dtype)
    eng._apply_rings(alpha, beta, None, out=raw)
    assert bool(torch.isfinite(raw).all()), "the diagonal launch left entries unwritten"
    assert torch.equal(eng._dofs_out(raw), d_op)

    # ---- Y = K U, k columns
    U = torch.tensor(case["U"])
    columns = [ref.apply(case["U"][:, c]) for c in range(k)]
    want_b, scale_b = (np.stack([col[i] for col in columns], axis=1) for i in (0, 1))
    got_b = op @ U
    assert got_b.shape == (n, k) and got_b.dtype == dtype
    check_rows(got_b, want_b, scale_b, tol_apply, f"op @ U, k = {k}")
    assert (host(got_b)[lone] == 0.0).all()
    single_cols = torch.stack([op.matvec(U[:, c].contiguous()) for c in range(k)], dim=1)
    check_rows(got_b, host(single_cols), scale_b, tol_apply, "op @ U against matvec column by column")
    raw = poisoned(n * k, dtype)
    eng._apply_rings(alpha, beta, eng._dofs_in(U), out=raw)
    assert bool(torch.isfinite(raw).all()), "the block launch left entries of Y unwritten"
    assert torch.equal(eng._dofs_out(raw.view(n, k)), got_b)
    out = poisoned(n * k, dtype)
    assert torch.equal(eng.apply(alpha, beta, U, out=out), got_b) and bool(torch.isfinite(out).all())
    # non-contiguous U: a column slice of a wider block, a transposed view
    wide = torch.cat([U, torch.ones(n, 1)], dim=1)
    assert not wide[:, :k].is_contiguous() and torch.equal(op.matvec(wide[:, :k]), got_b)
    Ut = U.t().contiguous().t()
    assert not Ut.is_contiguous() and torch.equal(op @ Ut, got_b)

    # ---- the other routes to the same operator
    check_rows(op.to_csr().matvec(u), want, scale, tol_apply, "op.to_csr().matvec")
    check_rows(K.matvec(u), want, scale, tol_apply, "K.matvec (k_csr_spmv)")
    plain = K.caller_numbering()
    assert np.array_equal(plain.crow_indices.cpu().numpy(), ref.rowptr)
    assert np.array_equal(plain.col_indices.cpu().numpy(), ref.colind)
    check_rows(plain.values, ref.values, scale_d[ref.rows], tol_diag, "CSR values")
    d_csr = K.diagonal()
    check_rows(d_csr, want_d, scale_d, tol_diag, "K.diagonal")
    check_rows(d_csr, host(d_op), scale_d, tol_diag, "K.diagonal against op.diagonal")
    if n <= DENSE_MAX_VERTS:
        dense = host(K.to_dense())
        assert dense.shape == (n, n)
        check_rows(dense.reshape(-1), ref.dense().reshape(-1), np.repeat(scale_d, n), tol_diag, "K.to_dense")

    # ---- variable coefficients
    if case["coefficients"]:
        route["coefficients"] = True
        npd = np.float32 if single else np.float64
        plain_mesh = {"vertices": verts, "triangles": tris}
        u64 = case["u"].astype(np.float64)
        for a, b, kappa, c in COEFFICIENT_FORMS:
            what = f"coefficients {kappa.__name__} / {c.__name__}"
            parts = cref.reference_parts(plain_mesh, order, a, b, kappa, c, npd)
            rowptr, colind, want_v = parts[:3]
            opc = basis.integrate_bilinear_form(cref.form(a, b, kappa, c), layout="operator")
            assert opc.matrix_free is True and opc._programs is not None
            has_row = np.diff(rowptr) > 0
            assert np.array_equal(has_row, ~lone)
            want_y, tol_y = cref.apply_reference(parts, u64)
            rows = np.repeat(np.arange(n), np.diff(rowptr))
            want_dc = np.zeros(n)
            want_dc[rows[colind == rows]] = want_v[colind == rows]
            tol_dc = cref.apply_reference(parts, np.ones(n))[1]
            y = opc.matvec(u)
            raw = poisoned(n, dtype)
            eng._apply_rings_coef(opc.alpha, opc.beta, *opc._programs, eng._dofs_in(u), out=raw)
            assert bool(torch.isfinite(raw).all()), f"{what}: the launch left entries of y unwritten"
            assert torch.equal(eng._dofs_out(raw), y)
            assert (host(y)[lone] == 0.0).all()
            cref.check(host(y)[has_row], want_y[has_row], tol_y[has_row], f"{what}: K u")
            dg = opc.diagonal()
            raw = poisoned(n, dtype)
            eng._apply_rings_coef(opc.alpha, opc.beta, *opc._programs, None, out=raw)
            assert bool(torch.isfinite(raw).all()) and torch.equal(eng._dofs_out(raw), dg)
            assert (host(dg)[lone] == 0.0).all()
            cref.check(host(dg)[has_row], want_dc[has_row], tol_dc[has_row], f"{what}: diag K")

    # ---- CG
    free_np = oref.cg_free_dofs(case)
    if free_np is None:
        return
    route["cg"] = True
    free = torch.tensor(free_np)
    held = torch.tensor(np.setdiff1d(np.arange(n), free_np))
    assert not np.isin(np.flatnonzero(lone), free_np).any()  # isolated vertices stay outside
    B_np, X0_np = oref.cg_loads(case), oref.cg_start(case)
    B, X0 = torch.tensor(B_np), torch.tensor(X0_np)
    bound = CG_RTOL * (1.0 + CG_C)

    def check_solution(x, res, col, what):
        x_np = host(x).reshape(-1)
        assert np.isfinite(x_np).all(), f"{what}: not finite"
        true = oref.true_residual(ref, x_np, B_np[:, col], free_np)
        print(f"{what}: reported residual {float(res):.3e}, true residual {true:.3e} (bound {bound:.3e})")
        assert float(res) <= CG_RTOL and true <= bound, (what, float(res), true)
        assert torch.equal(x.reshape(-1)[held], X0[:, col][held]), f"{what}: an entry outside `free` moved"

    singles = {}
    for col in (0, 1):
        x, it, res = op.solve_cg(B[:, col].contiguous(), free=free, x0=X0[:, col].contiguous(), rtol=CG_RTOL)
        assert x.shape == (n,) and 0 < it
        check_solution(x, res, col, f"op.solve_cg, column {col} ({it} iterations)")
        singles[col] = (x, it)
    x, it, res = K.solve_cg(B[:, 1].contiguous(), free=free, x0=X0[:, 1].contiguous(), rtol=CG_RTOL)
    check_solution(x, res, 1, f"K.solve_cg, column 1 ({it} iterations)")
    X, its, ress = op.solve_cg_multi(B, free=free, X0=X0, rtol=CG_RTOL)
    assert X.shape == (n, 3) and its.shape == (3,) and bool(torch.isfinite(X).all())
    for col in (0, 1):
        check_solution(X[:, col], ress[col], col, f"op.solve_cg_multi, column {col} ({int(its[col])} iterations)")
        err = scaled_error(host(X[:, col]), host(singles[col][0]))
        print(f"block against single, column {col}: scaled error {err:.3e}, iterations {int(its[col])} / {singles[col][1]}")
        assert err <= 1e-8 and abs(int(its[col]) - singles[col][1]) <= 25
    # the zero column: zero load, zero start
    assert int(its[2]) == 0 and float(ress[2]) == 0.0 and bool((X[:, 2] == 0).all())


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_meshes_through_the_operator_stack(seed, monkeypatch):
    run_case(oref.sweep_case(seed), monkeypatch)


def test_sweep_exercised_what_it_is_there_for():
    """Runs last.  What the hundred seeds reached: conditions, not measurements (the counts of the
    plans were checked beforehand with ring_plan_host on the CPU: operator_reference.route_counts)."""
    if N_SEEDS < 100:
        pytest.skip(f"TFEM_FUZZ_SEEDS={N_SEEDS}: the coverage conditions are stated for the 100 default seeds")
    if len(ROUTES) < N_SEEDS:
        pytest.skip(f"only {len(ROUTES)} of {N_SEEDS} seeds ran in this session")
    routes = [ROUTES[s] for s in range(100)]

    def count(pred):
        return sum(1 for r in routes if pred(r))

    counts = {
        "matrix_free": count(lambda r: r["matrix_free"]),
        "slots_7": count(lambda r: r["slots"] == 7), "slots_15": count(lambda r: r["slots"] == 15),
        "chunked": count(lambda r: r["chunked"]), "renumbered": count(lambda r: r["renumbered"]),
        "isolated": count(lambda r: r["isolated"] > 0),
        "long_rows": count(lambda r: r["long_mode"] and r["long_rows"] > 0),
        "int64": count(lambda r: r["int64"]), "int32": count(lambda r: not r["int64"]),
        "float32": count(lambda r: r["float32"]), "cg": count(lambda r: r["cg"]),
        "cg_with_isolated": count(lambda r: r["cg"] and r["isolated"] > 0),
        "coefficients": count(lambda r: r["coefficients"]),
        "k": {k: count(lambda r, k=k: r["k"] == k) for k in oref.BLOCK_WIDTHS},
    }
    print(f"[operator sweep] {counts}")
    assert counts["matrix_free"] == 100
    assert counts["isolated"] >= 15
    assert counts["slots_7"] >= 25 and counts["slots_15"] >= 25
    assert counts["long_rows"] >= 10
    assert counts["renumbered"] >= 20
    assert counts["int64"] >= 1 and counts["int32"] >= 1
    assert counts["float32"] >= 8
    assert all(v >= 1 for v in counts["k"].values()), counts["k"]
    # CG met zero diagonals (isolated vertices outside `free`) and the coefficient launches ran
    assert counts["cg"] >= 20 and counts["cg_with_isolated"] >= 5 and counts["coefficients"] >= 30
