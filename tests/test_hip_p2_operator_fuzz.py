"""Seeded random sweep of the matrix-free P2 operator stack on a real MI355X (-m gpu): the apply
kernels of csrc/tfem_p2apply.hip (k_p2_apply_rows on vertex and edge rows, k_p2_apply_long_rows)
and of csrc/tfem_p2apply_multi.hip (their _multi forms, pass widths 4 and 2 and the fp32 column
loop), the vertex / edge / long-row plan of csrc/tfem_p2rows_host.cpp, engine._apply_p2_rows and
FormOperator on top of it, the CSR route next to it (k_p2_rows, k_csr_spmv, tfem_csr_spmm) and CG
on both -- on the mesh family of the P1 sweep (tests/random_meshes.py: removed elements, open fans,
several fans per vertex, isolated vertices, flipped orientation, rotated local numbering, shuffled /
Morton vertex order, shuffled element order), int32 and int64 connectivity, float64 and float32,
quadrature orders 2 to 4, block widths 2 to 9, every third seed with the edge DoFs renumbered
inside the engine (TFEM_RENUMBER=1), every fourth seed with all block passes of width 2
(TFEM_P2_APPLY_NV=2).  tests/p2_operator_reference.sweep_case(seed) draws a seed's case; the rng is
default_rng(9000 + seed).  Every seed goes through Basis(MeshTri(...), ElementTri(2, order)) and
integrate_bilinear_form.

The reference is tests/p2_operator_reference.py: the repository's oracle run in long double, NOT
the float64 oracle.  Every launch that can be handed a result buffer gets one filled with NaN: the
rows of isolated vertices (empty rows inside a wave, which the CSR start of the rows behind them
must skip), the rows the tile launch leaves to the long-row launch, and every column of every pass
of a block have to be written.

Routing: the plan p2_plan_host builds on the host for the case (p2_operator_reference.plan_of, in
the engine's numbering -- the edge permutation of a renumbered engine is formed on the host) is the
plan the engine holds, layout word for layout word, and where the host is refused the engine has
none: layout="matrix_free" then refuses, layout="operator" serves the assembled CSR.
layout="operator" on a P2 basis is the assembled CSR on every seed (tests/test_hip_operator.py pins
that: matrix_free is False); it is held to the same bounds.

Tolerances (none of them comes from a kernel's output):

  float64   1e-12 row-scaled (TOL of tests/test_hip_p2_operator.py): K u and SpMV against
            sum_j |K_ij u_j|, diag K and CSR values against sum_j |K_ij|.  Float64 arithmetic alone
            stays far below it: the float64 oracle is within 9.6e-15 of the long-double reference
            on the seeds tests/test_p2_operator_reference.py compares, the float64 walk of the row
            plan (tests/p2rows_emulator.py) within 4.1e-14 on the 30 seeds up to 3000 DoFs (seed
            60; that file prints both).
  float32   8 x the worst row-scaled error of the ORACLE ITSELF run in float32 (coordinates, tables,
            coefficients, values and row sums in float32) against the long-double reference on the
            same float32-rounded coordinates, over the 17 float32 seeds of the sweep.  Measured on
            the CPU by `python tests/p2_operator_reference.py` (measure_float32):
                K u     worst 1.375e-05 (seed 60)  ->  bound 1.100e-04
                diag K  worst 1.043e-05 (seed 60)  ->  bound 8.344e-05
            The factor 8 is the P1 sweep's: the kernel's fan order and closed form sum differently
            from the oracle.
  CG        the recurrence residual meets rtol by construction; the TRUE residual ||b - K x|| on
            the free DoFs, from the long-double reference matrix, may exceed it by the drift between
            the two: true <= rtol * (1 + c).  c = 4 x the worst |true - recurrence| / rtol of
            sparse.conjugate_gradients run on the CPU with the float64 oracle's P2 CSR (torch) over
            the 15 CG seeds, both non-zero loads, rtol = 1e-10 (measure_cg in the same command):
            worst 2.337e-03 (seed 45, the smooth load), c = 9.348e-03.
  block CG against CG column by column   scaled error <= 1e-8, iteration counts within 25: the
            bounds of tests/test_hip_p2_operator_multi.py for that comparison.
  block against single launches   bit for bit (torch.equal), fp64 and fp32, also under
            TFEM_P2_APPLY_NV=2: the contract at the top of csrc/tfem_p2apply_multi.hip.

Where CG runs is decided by p2_operator_reference.cg_free_dofs (its docstring says why).

The last test prints what the seeds reached and asserts lower limits on it.  The limits are
conditions, not measurements; p2_operator_reference.route_counts() gives for the 100 default seeds,
from p2_plan_host on the CPU:
    plan 92, refused 8 (7 "a chunk of the vertex numbering alone exceeds the tile capacity", 1 "the
    vertex numbering has no locality"), long rows 45, isolated vertices 33, both 16, more than one
    tile of each kind 75, int64 48, int32 52, float32 17 (16 with a plan), renumbered 34 (33 forced,
    one by its size), TFEM_P2_APPLY_NV=2 with a plan 20, k = 2 .. 9: 12 11 8 14 15 9 12 11 (with a
    plan), CG 15 (13 with a plan, 7 of those with isolated vertices)."""

import os

import numpy as np
import pytest
import torch

import p2_operator_reference as p2ref
from conftest import scaled_error
from test_hip_operator_fuzz import check_rows, host, poisoned
from test_hip_p2_operator import TOL, form, tf

pytestmark = pytest.mark.gpu

#: TFEM_FUZZ_SEEDS=n shortens or widens the sweep (developer runs), as in the sibling sweeps
N_SEEDS = int(os.environ.get("TFEM_FUZZ_SEEDS", "100"))

TOL32_APPLY = 8 * 1.375e-05
TOL32_DIAG = 8 * 1.043e-05
CG_RTOL = 1e-10
CG_C = 4 * 2.337e-03

ROUTES = {}  # seed -> what the seed exercised


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def reference_block(ref, U):
    """(K U, sum_j |K_ij U_jc|) column by column."""
    columns = [ref.apply(U[:, c]) for c in range(U.shape[1])]
    return tuple(np.stack([col[i] for col in columns], axis=1) for i in (0, 1))


def run_case(case, monkeypatch):
    """One seed of the sweep: every check of this file on the case's mesh."""
    seed = case["seed"]
    for key, value in (("TFEM_RENUMBER", "1" if case["renumber_env"] else None),
                       ("TFEM_P2_APPLY_NV", "2" if case["nv_cap"] else None)):
        if value is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, value)
    single = case["single"]
    dtype = torch.float32 if single else torch.float64
    torch.set_default_dtype(dtype)
    tol_apply, tol_diag = (TOL32_APPLY, TOL32_DIAG) if single else (TOL, TOL)
    order, alpha, beta, k = case["order"], case["alpha"], case["beta"], case["k"]
    n, lone = case["n_dofs"], case["lone"]
    basis = tf().Basis(tf().MeshTri(triangulation=case["mesh"]), tf().ElementTri(2, order))
    eng = basis._engine
    assert eng.dtype == dtype and eng.n_dofs == n
    assert np.array_equal(basis._global_dofs4elements.cpu().numpy(), case["conn6"]), "the caller's numbering is conn6"

    # ---- routing: what the host predicts is what the engine does
    host_plan, _, host_perm, _ = p2ref.plan_of(case)
    has_plan = not isinstance(host_plan, str)
    K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
    lazy = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
    rows = eng.p2_plan()
    route = ROUTES[seed] = p2ref.route_of(case, host_plan)
    route.update({"plan": rows is not None, "renumbered": bool(eng.renumbered), "cg": False})
    print(f"seed {seed}: {route}" + ("" if has_plan else f" -- the host's refusal: {host_plan}"))
    assert (rows is not None) == has_plan, "the engine and p2_plan_host on the host disagree about the plan"
    assert eng.renumbered == case["renumber"]
    if eng.renumbered:
        assert np.array_equal(eng.dof_permutation().cpu().numpy(), host_perm), "the edge permutation formed on the host"
    if has_plan:
        assert np.array_equal(rows["layout"], host_plan["layout"]), "the engine's plan is not the host's"
    assert K.dtype == dtype and lazy.dtype == dtype and K.shape == (n, n)
    # layout="operator" on P2: the assembled CSR behind the operator's interface (test_hip_operator.py)
    assert lazy.matrix_free is False

    ref = p2ref.reference_of(case)
    u, U = torch.tensor(case["u"]), torch.tensor(case["U"])
    assert u.dtype == dtype and U.shape == (n, k)
    want, scale = ref.apply(case["u"])
    want_d, scale_d = ref.diagonal()
    want_b, scale_b = reference_block(ref, case["U"])
    assert (scale[lone] == 0).all() and (scale_d[lone] == 0).all() and np.array_equal(ref.has_row, ~lone)

    def check_operator(op, name):
        """matvec, the diagonal and a block of an operator against the reference; the rows of
        isolated vertices exactly zero.  Returns the three results."""
        got = op.matvec(u)
        assert got.shape == (n,) and got.dtype == dtype
        check_rows(got, want, scale, tol_apply, f"{name}.matvec")
        assert (host(got)[lone] == 0.0).all(), f"{name}.matvec: the row of an isolated vertex is not exactly zero"
        d = op.diagonal()
        assert d.shape == (n,) and d.dtype == dtype
        check_rows(d, want_d, scale_d, tol_diag, f"{name}.diagonal")
        assert (host(d)[lone] == 0.0).all(), f"{name}.diagonal: the row of an isolated vertex is not exactly zero"
        got_b = op.matvec(U) if isinstance(op, tf().CSRMatrix) else op @ U  # a CSRMatrix has no @
        assert got_b.shape == (n, k) and got_b.dtype == dtype
        check_rows(got_b, want_b, scale_b, tol_apply, f"{name} @ U, k = {k}")
        assert (host(got_b)[lone] == 0.0).all(), f"{name} @ U: the row of an isolated vertex is not exactly zero"
        return got, d, got_b

    # ---- the CSR route, on every seed
    check_operator(K, "K (CSR)")
    plain = K.caller_numbering()
    assert np.array_equal(plain.crow_indices.cpu().numpy(), ref.rowptr)
    assert np.array_equal(plain.col_indices.cpu().numpy(), ref.colind)
    check_rows(plain.values, ref.values, scale_d[ref.rows], tol_diag, "CSR values")
    check_operator(lazy, 'layout="operator"')

    if not has_plan:
        # ---- no plan: the strict layout and the launch refuse, nothing else changes
        with pytest.raises(NotImplementedError, match="no row plan"):
            basis.integrate_bilinear_form(form(alpha, beta), layout="matrix_free")
        with pytest.raises(NotImplementedError, match="P2 row plan"):
            eng._apply_p2_rows(alpha, beta, eng._dofs_in(u))
        op = lazy
    else:
        op = basis.integrate_bilinear_form(form(alpha, beta), layout="matrix_free")
        assert op.matrix_free is True and op.dtype == dtype and "matrix-free, P2 rows" in repr(op)
        got, d_op, got_b = check_operator(op, "op")

        # ---- y = K u: the launch into poisoned buffers
        out = poisoned(n, dtype)
        assert torch.equal(eng.apply(alpha, beta, u, out=out), got) and bool(torch.isfinite(out).all())
        raw = poisoned(n, dtype)
        eng._apply_p2_rows(alpha, beta, eng._dofs_in(u), out=raw)
        assert bool(torch.isfinite(raw).all()), "the apply launch left entries of y unwritten"
        assert torch.equal(eng._dofs_out(raw), got)
        # ---- diag K
        raw = poisoned(n, dtype)
        eng._apply_p2_rows(alpha, beta, None, out=raw)
        assert bool(torch.isfinite(raw).all()), "the diagonal launch left entries unwritten"
        assert torch.equal(eng._dofs_out(raw), d_op)
        # ---- Y = K U: every column the single launch's bits, fp64 and fp32, whatever the pass widths
        for c in range(k):
            single_c = op.matvec(U[:, c].contiguous())
            assert torch.equal(got_b[:, c], single_c), f"op @ U, k = {k}: column {c} is not the single launch's"
        raw = poisoned(n * k, dtype)
        eng._apply_p2_rows(alpha, beta, eng._dofs_in(U), out=raw)
        assert bool(torch.isfinite(raw).all()), "the block launch left entries of Y unwritten"
        assert torch.equal(eng._dofs_out(raw.view(n, k)), got_b)
        out = poisoned(n * k, dtype)
        assert torch.equal(eng.apply(alpha, beta, U, out=out), got_b) and bool(torch.isfinite(out).all())
        # non-contiguous U: a column slice of a wider block, a transposed view
        wide = torch.cat([U, torch.ones(n, 1)], dim=1)
        assert not wide[:, :k].is_contiguous() and torch.equal(op.matvec(wide[:, :k]), got_b)
        Ut = U.t().contiguous().t()
        assert not Ut.is_contiguous() and torch.equal(op @ Ut, got_b)
        # the assembled operator behind the matrix-free one
        check_rows(op.to_csr().matvec(u), want, scale, tol_apply, "op.to_csr().matvec")

    # ---- CG
    free_np = p2ref.cg_free_dofs(case)
    if free_np is None:
        return
    route["cg"] = True
    free = torch.tensor(free_np)
    held = torch.tensor(np.setdiff1d(np.arange(n), free_np))
    assert not lone[free_np].any()  # isolated vertices stay outside
    B_np, X0_np = p2ref.cg_loads(case), p2ref.cg_start(case)
    B, X0 = torch.tensor(B_np), torch.tensor(X0_np)
    bound = CG_RTOL * (1.0 + CG_C)

    def check_solution(x, res, col, what):
        x_np = host(x).reshape(-1)
        assert np.isfinite(x_np).all(), f"{what}: not finite"
        true = p2ref.true_residual(ref, x_np, B_np[:, col], free_np)
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
    for loop in ("fused", "torch"):
        X, its, ress = op.solve_cg_multi(B, free=free, X0=X0, rtol=CG_RTOL, loop=loop)
        assert X.shape == (n, 3) and its.shape == (3,) and bool(torch.isfinite(X).all())
        for col in (0, 1):
            check_solution(X[:, col], ress[col], col,
                           f"op.solve_cg_multi ({loop}), column {col} ({int(its[col])} iterations)")
            err = scaled_error(host(X[:, col]), host(singles[col][0]))
            print(f"block ({loop}) against single, column {col}: scaled error {err:.3e}, "
                  f"iterations {int(its[col])} / {singles[col][1]}")
            assert err <= 1e-8 and abs(int(its[col]) - singles[col][1]) <= 25
        # the zero column: zero load, zero start
        assert int(its[2]) == 0 and float(ress[2]) == 0.0 and bool((X[:, 2] == 0).all())


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_meshes_through_the_p2_operator_stack(seed, monkeypatch):
    run_case(p2ref.sweep_case(seed), monkeypatch)


def test_sweep_exercised_what_it_is_there_for():
    """Runs last.  What the hundred seeds reached: conditions, not measurements.  The limits stand
    clearly below the counts p2_operator_reference.route_counts() gives on the CPU (this file's
    docstring lists them): plan 92, refused 8, long rows 45, isolated 33, both 16, many tiles 75,
    int64 48, int32 52, float32 with a plan 16, renumbered 34, NV cap 20, every k at least 8,
    CG 15, CG with a plan 13, CG with isolated vertices 7."""
    if N_SEEDS < 100:
        pytest.skip(f"TFEM_FUZZ_SEEDS={N_SEEDS}: the coverage conditions are stated for the 100 default seeds")
    if len(ROUTES) < N_SEEDS:
        pytest.skip(f"only {len(ROUTES)} of {N_SEEDS} seeds ran in this session")
    counts = p2ref.count_routes([ROUTES[s] for s in range(100)])
    print(f"[P2 operator sweep] {counts}")
    assert counts["plan"] >= 85 and counts["refused"] >= 3
    assert counts["long_rows"] >= 30 and counts["isolated"] >= 20 and counts["long_and_isolated"] >= 10
    assert counts["many_tiles"] >= 50
    assert counts["int64"] >= 30 and counts["int32"] >= 30
    assert counts["float32_with_plan"] >= 8
    assert counts["renumbered"] >= 25 and counts["nv_cap"] >= 12
    assert all(v >= 4 for v in counts["k"].values()), counts["k"]
    # CG met zero diagonals (isolated vertices outside `free`) on the matrix-free operator
    assert counts["cg"] >= 10 and counts["cg_with_plan"] >= 8 and counts["cg_with_isolated"] >= 3
