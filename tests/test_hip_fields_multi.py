"""The P1 operator with coefficient DATA on several vectors in one launch
(tfem_p1_apply_rings_field_multi, k_p1_field_rows_multi in csrc/tfem_rings_field_multi.hip) on a real
MI355X: every column of K U against the reference of tests/field_reference.py (its tolerance rule,
per column) and BIT FOR BIT against the single-vector launch (tfem_p1_apply_rings_field) on that
column; the width cap; the C ABI and its refusals; one call per block; the gradient; block CG; a
small sweep over the random meshes of tests/operator_reference.py; the example."""

import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import field_reference as fref
import operator_reference as oref
from conftest import REPO
from test_hip_coefficients_multi import _sweep_basis, counted
from test_hip_fields import (FORMS, _assert_plan, _basis, _data, _dev, _engine, _form, _head, _host, _mesh,
                             _np_dtype)

pytestmark = pytest.mark.gpu

#: one pass (2, 4), a pass with a dropped column (3), several passes with a narrow tail (5, 8, 11)
WIDTHS = (2, 3, 4, 5, 8, 11)
MULTI, SINGLE = "tfem_p1_apply_rings_field_multi", "tfem_p1_apply_rings_field"


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def check_columns(got, parts, U_np, what):
    """Every column of `got` against K^ref U[:, c] within the tolerance of field_reference; the
    largest |err| / tol."""
    got = _host(got)
    has_row = np.diff(parts[0]) > 0
    worst = 0.0
    for c in range(got.shape[1]):
        want, tol = fref.apply_reference(parts, U_np[:, c])
        assert (got[~has_row, c] == 0.0).all(), f"{what}: a row without elements is not exactly zero"
        worst = max(worst, fref.check(got[has_row, c], want[has_row], tol[has_row], f"{what}, column {c}"))
    assert 0.0 < worst <= 1.0
    return worst


def check_block(op, parts, U, widths, what):
    """op @ U[:, :k] for every width: the reference per column, bit identity with the single
    launch per column, non-contiguous blocks."""
    n, kmax = U.shape
    U_np = _host(U)
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


def _operator(mesh_np, order, dtype, alpha, beta, kv, cv):
    """The matrix-free operator of the form with data kv, cv ((E, Q | 1) arrays or None) and its basis."""
    torch.set_default_dtype(dtype)
    basis = _basis(mesh_np, order)
    kq = None if kv is None else basis.coefficient(torch.tensor(kv, dtype=dtype))
    cq = None if cv is None else basis.coefficient(torch.tensor(cv, dtype=dtype))
    op = basis.integrate_bilinear_form(_form(alpha, beta, kq, cq), layout="matrix_free")
    assert op.matrix_free is True and op._fields is not None and op.dtype == dtype
    return basis, op


BLOCK_CASES = [("square_chunked", torch.float64), ("square_multi_tile", torch.float64),
               ("delaunay_15_slots", torch.float64), ("holes", torch.float64), ("rotated_shuffled", torch.float64),
               ("p1_square_n8.npz", torch.float64), ("square_multi_tile", torch.float32),
               ("p1_square_n6_float32.npz", torch.float32)]


@pytest.mark.parametrize("which", list(FORMS))
@pytest.mark.parametrize("mesh,dtype", BLOCK_CASES)
def test_block_matches_the_reference_and_the_single_launch_bit_for_bit(mesh, dtype, which):
    alpha, beta, has_k, has_c = FORMS[which]
    order = 3
    mesh_np = _mesh(mesh)
    kv, cv = _data(mesh_np, order, has_k, 61, dtype), _data(mesh_np, order, has_c, 62, dtype)
    basis, op = _operator(mesh_np, order, dtype, alpha, beta, kv, cv)
    eng = basis._engine
    rings = eng.ring_plan()
    assert rings is not None and not eng.renumbered
    _assert_plan(mesh, rings)
    for k in WIDTHS:  # the block launch takes these plans at every width (it is not the column loop)
        assert eng.field_refusal(beta, "apply", k) is None
    parts = fref.reference_parts(mesh_np, order, alpha, beta, kv, cv, _np_dtype(dtype))
    U = torch.tensor(np.random.default_rng(3).standard_normal((op.shape[0], max(WIDTHS))), dtype=dtype)
    check_block(op, parts, U, WIDTHS, f"{mesh} {dtype} {which}")


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_block_at_every_quadrature_order_and_one_value_per_element(order):
    """Orders 1 .. 4 are the instances with 1, 3, 4 and 6 points; kappa as (E, 1) beside c as (E, Q)."""
    alpha, beta = 0.5, 2.0
    mesh_np = _mesh("square_multi_tile")
    dtype = torch.float64
    for per_element in (False, True):
        kv = _data(mesh_np, order, True, 71, dtype, per_element=per_element)
        cv = _data(mesh_np, order, True, 72, dtype)
        basis, op = _operator(mesh_np, order, dtype, alpha, beta, kv, cv)
        assert op._fields[0].shape[1] == (1 if per_element else basis._engine.n_quad)
        assert op._fields[1].shape[1] == basis._engine.n_quad
        parts = fref.reference_parts(mesh_np, order, alpha, beta, kv, cv)
        U = torch.tensor(np.random.default_rng(order).standard_normal((op.shape[0], 4)))
        check_block(op, parts, U, (3, 4), f"order {order}, kappa per element {per_element}")


def _abi_case(mesh="square_multi_tile", order=3, beta=2.0):
    mesh_np = _mesh(mesh)
    eng = _engine(mesh_np, order)
    rings = eng.ring_plan()
    assert rings is not None and not eng.renumbered
    kd = _dev(fref.data(mesh_np, order, 81), torch.float64)
    cd = _dev(fref.data(mesh_np, order, 82), torch.float64)
    return mesh_np, eng, rings, kd, cd, _head(eng, rings, order, 0.5, beta, kd, cd)


def test_width_cap_gives_the_same_bits(monkeypatch):
    """TFEM_APPLY_NV = 2 and = 4 through the C ABI: narrower passes, the same bits, k = 11."""
    from pytorch_fem_solver_amd import _native

    mesh_np, eng, rings, kd, cd, head = _abi_case()
    n, k = eng.n_dofs, 11
    U = torch.tensor(np.random.default_rng(5).standard_normal((n, k)))

    def run():
        Y = torch.full((n, k), float("nan"))
        _native.check(eng.lib.tfem_p1_apply_rings_field_multi(*head, _native.ptr(U), _native.ptr(Y), k, eng._stream()))
        torch.cuda.synchronize()
        return Y

    monkeypatch.delenv("TFEM_APPLY_NV", raising=False)
    free = run()
    assert bool(torch.isfinite(free).all())
    check_columns(free, fref.reference_parts(mesh_np, 3, 0.5, 2.0, _host(kd), _host(cd)), _host(U), "uncapped")
    for cap in ("2", "4"):
        monkeypatch.setenv("TFEM_APPLY_NV", cap)
        assert torch.equal(run(), free), f"TFEM_APPLY_NV={cap}"


def test_c_abi_single_column_and_every_refusal_leaves_y_untouched(monkeypatch):
    from pytorch_fem_solver_amd import _native

    IA, UN, IR = 1, 2, 4  # TFEM_ERR_INVALID_ARGUMENT, TFEM_ERR_UNSUPPORTED, TFEM_ERR_INDEX_RANGE
    mesh_np, eng, rings, kd, cd, good = _abi_case()
    n, lib, stream = eng.n_dofs, eng.lib, eng._stream()
    names = ("coords", "real_bytes", "n_verts", "order", "alpha", "beta", "kappa", "knq", "c", "cnq", "n_elems",
             "plan", "layout")

    def multi(u, y, n_vec, **change):
        head = dict(zip(names, good))
        head.update(change)
        return lib.tfem_p1_apply_rings_field_multi(*(head[k] for k in names), u, y, n_vec, stream)

    # n_vec = 1 IS the single-vector launch
    u = torch.rand(n)
    y1, ym = torch.full((n,), float("nan")), torch.full((n,), float("nan"))
    _native.check(lib.tfem_p1_apply_rings_field(*good, _native.ptr(u), _native.ptr(y1), stream))
    _native.check(multi(_native.ptr(u), _native.ptr(ym), 1))
    torch.cuda.synchronize()
    assert torch.equal(y1, ym) and bool(torch.isfinite(ym).all())
    # three columns through the entry point
    U, Y = torch.rand(n, 3), torch.full((n, 3), float("nan"))
    _native.check(multi(_native.ptr(U), _native.ptr(Y), 3))
    torch.cuda.synchronize()
    parts = fref.reference_parts(mesh_np, 3, 0.5, 2.0, _host(kd), _host(cd))
    check_columns(Y, parts, _host(U), "three columns through the entry point")
    # every refusal, and the empty plans, leave a poisoned Y as it is
    Y.fill_(7.0)
    z = rings["layout"]

    def layout(**over):
        out = z.copy()
        for key, v in over.items():
            out[int(key[1:])] = v
        return out

    kept = [layout(z23=2), layout(z18=0), layout(z17=769), layout(z3=1024, z17=700), layout(z0=0)]
    where = [c_void_p(t.ctypes.data) for t in kept]
    buf = torch.rand(4 * n)
    pu, py = _native.ptr(U), _native.ptr(Y)
    over_u, over_y = _native.ptr(buf), c_void_p(buf.data_ptr() + 8 * (3 * n - 1))
    too_many = (1 << 29) // n + 1  # n * n_vec * 8 bytes >= 2^32
    refused = {
        "1 real_bytes": (multi(pu, py, 3, real_bytes=3, layout=None), IA),
        "2 NULL layout": (multi(pu, py, 3, layout=None, n_verts=-1), IA),
        "3 negative": (multi(pu, py, 0, n_verts=-1), IA),
        "4 n_vec 0": (multi(None, py, 0), IA),
        "5 u NULL": (multi(None, py, 3, kappa=None, c=None), IA),
        "6 both fields NULL": (multi(pu, py, 3, kappa=None, c=None, knq=3), IA),
        "7 nq": (multi(pu, py, too_many, knq=3), IA),
        "8 extent": (multi(over_u, over_y, too_many), IR),
        "8 extent of the values": (multi(over_u, over_y, 3, n_elems=1 << 29), IR),
        "9 overlap": (multi(over_u, over_y, 3, layout=where[0]), IA),
        "9 same": (multi(py, py, 3, layout=where[0]), IA),
        "10 long rows": (multi(pu, py, 3, layout=where[0], order=9), UN),
        "10 no element stage": (multi(pu, py, 3, layout=where[1], order=9), UN),
        "10 too many elements": (multi(pu, py, 3, layout=where[2], order=9), UN),
        "10 LDS": (multi(pu, py, 3, layout=where[3], order=9), UN),
        "10 unknown order": (multi(pu, py, 3, order=9), UN),
        "empty plan": (multi(pu, py, 3, layout=where[4]), 0),
        "no vertices": (multi(pu, py, 3, n_verts=0), 0),
    }
    torch.cuda.synchronize()
    assert {k: v[0] for k, v in refused.items()} == {k: v[1] for k, v in refused.items()}
    assert multi(pu, py, 3, layout=where[3]) == UN and b"LDS" in lib.tfem_last_error()
    torch.cuda.synchronize()
    assert bool((Y == 7.0).all()), "a refused call wrote to Y"
    # the engine refuses out = u and a wrong number of rows
    with pytest.raises(ValueError):
        eng._apply_rings_field(0.5, 2.0, (kd, cd), U, out=U)
    with pytest.raises(ValueError):
        eng._apply_rings_field(0.5, 2.0, (kd, cd), torch.rand(n + 1, 3))
    # every entry of a given output is written, and a column of NaN stays in its column
    want = eng._apply_rings_field(0.5, 2.0, (kd, cd), U)
    out = torch.full((3 * n,), float("nan"))
    got = eng._apply_rings_field(0.5, 2.0, (kd, cd), U, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want) and bool(torch.isfinite(out).all())
    poisoned = U.clone()
    poisoned[:, 1] = float("nan")
    leak = eng._apply_rings_field(0.5, 2.0, (kd, cd), poisoned)
    assert torch.equal(leak[:, [0, 2]], want[:, [0, 2]]) and bool(torch.isnan(leak[:, 1]).all())


def test_renumbered_engine_in_both_numberings(monkeypatch):
    monkeypatch.setenv("TFEM_RENUMBER", "1")
    order, alpha, beta = 3, 0.5, 2.0
    mesh_np = _mesh("shuffled")
    kv, cv = fref.data(mesh_np, order, 91), fref.data(mesh_np, order, 92, per_element=True)
    basis, op = _operator(mesh_np, order, torch.float64, alpha, beta, kv, cv)
    eng = basis._engine
    assert eng.renumbered
    parts = fref.reference_parts(mesh_np, order, alpha, beta, kv, cv)
    U = torch.tensor(np.random.default_rng(6).standard_normal((op.shape[0], 5)))
    check_block(op, parts, U, (2, 5), "shuffled, the caller's numbering")
    Ue = eng._dofs_in(U).contiguous()
    for k in (2, 5):
        Y = eng._apply_rings_field(op.alpha, op.beta, op._fields, Ue[:, :k].contiguous())
        assert torch.equal(eng._dofs_out(Y), op @ U[:, :k].contiguous())
        for j in range(k):
            one = eng._apply_rings_field(op.alpha, op.beta, op._fields, Ue[:, j].contiguous())
            assert torch.equal(Y[:, j], one), f"engine numbering, k = {k}, column {j}"


def test_a_block_is_one_call_and_block_cg_takes_block_calls_only(monkeypatch):
    """The data of test_hip_fields.test_fused_cg_equals_cg_on_the_assembled_operator (order 4, kappa at
    the integration points, c per element) with four right-hand sides."""
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(40, 0.25, 1)
    order = 4
    basis = _basis(mesh_np, order)
    x, y = torch.split(basis.integration_points, 1, dim=-1)
    kq = basis.coefficient(1.0 + (torch.sin(3.0 * x) * torch.cos(2.0 * y)) ** 2)
    cq = basis.coefficient(torch.tensor(1.0 + np.asarray(mesh_np["vertices"])[mesh_np["triangles"]].mean(1)[:, 0]))
    op = basis.integrate_bilinear_form(_form(1.0, 1.0, kq, cq), layout="matrix_free")
    f = basis.integrate_linear_form(lambda b: torch.sin(np.pi * torch.split(b.integration_points, 1, dim=-1)[0]) * b.v)
    free = basis._basis_parameters["inner_dofs"]
    f = f.reshape(-1, 1)
    B = torch.cat([f, 2.0 * f, f * torch.rand_like(f), torch.zeros_like(f)], 1).contiguous()
    lib = basis._engine.lib
    names = (MULTI, SINGLE, "tfem_csr_spmv", "tfem_p1_rings_field")
    U = torch.rand(op.shape[0], 5)
    with monkeypatch.context() as m:
        counts = counted(lib, m, names)
        op @ U
        print(counts)
        assert counts == {MULTI: 1, SINGLE: 0, "tfem_csr_spmv": 0, "tfem_p1_rings_field": 0}
    with monkeypatch.context() as m:
        counts = counted(lib, m, names)
        _, its, _ = op.solve_cg_multi(B[:, :3].contiguous(), free=free, rtol=0.0, maxiter=50, loop="fused")
        print(counts)
        assert its.tolist() == [50, 50, 50]
        # 50 iterations and the residual of the set-up; the diagonal is the single launch without u
        assert counts == {MULTI: 50 + 1, SINGLE: 1, "tfem_csr_spmv": 0, "tfem_p1_rings_field": 0}
    rtol = 1e-12
    with monkeypatch.context() as m:
        counts = counted(lib, m, names)
        X, its, res = op.solve_cg_multi(B, free=free, rtol=rtol, loop="fused")
        print(counts, its.tolist(), res.tolist())
        assert counts[MULTI] >= int(its.max()) + 1 and counts[SINGLE] == 1
        assert counts["tfem_csr_spmv"] == 0 and counts["tfem_p1_rings_field"] == 0 and op._csr is None
    assert X.shape == B.shape and float(res.max()) <= rtol
    csr = op.to_csr()
    for j in range(B.shape[1]):
        x_c, _, res_c = csr.solve_cg(B[:, j].contiguous(), free=free, rtol=rtol)
        assert res_c <= rtol
        scale = max(float(x_c.abs().max()), 1e-300)
        err = float((X[:, j] - x_c.reshape(-1)).abs().max())
        print(f"column {j}: block solve against CG on the assembled operator {err / scale:.2e}")
        assert err <= 1e-9 * scale


@pytest.mark.parametrize("mesh", ["square_chunked", "delaunay_15_slots"])
def test_gradients_of_a_block_in_kappa_c_and_u(mesh, monkeypatch):
    """(op.matvec(U) * G).sum().backward() for (N, 3) and (N, 5) against the numpy reference."""
    order, alpha, beta = 3, 0.5, 2.0
    mesh_np = _mesh(mesh)
    n = mesh_np["vertices"].shape[0]
    basis = _basis(mesh_np, order)
    lib = basis._engine.lib
    kv, cv = fref.data(mesh_np, order, 51), fref.data(mesh_np, order, 52)
    parts = fref.reference_parts(mesh_np, order, alpha, beta, kv, cv)
    rng = np.random.default_rng(8)
    for cols in (3, 5):
        u_np, g_np = rng.standard_normal((n, cols)), rng.standard_normal((n, cols))
        kt, ct = torch.tensor(kv).requires_grad_(True), torch.tensor(cv).requires_grad_(True)
        op = basis.integrate_bilinear_form(_form(alpha, beta, basis.coefficient(kt), basis.coefficient(ct)),
                                           layout="matrix_free")
        U, G = torch.tensor(u_np).requires_grad_(True), torch.tensor(g_np)
        what = f"{mesh} {cols} columns"
        with monkeypatch.context() as m:
            counts = counted(lib, m, (MULTI, SINGLE, "tfem_p1_field_adjoint"))
            Y = op.matvec(U)
            assert counts == {MULTI: 1, SINGLE: 0, "tfem_p1_field_adjoint": 0}
            (Y * G).sum().backward()
            # the backward: K G by one more block call, the values' gradients by one adjoint call
            assert counts == {MULTI: 2, SINGLE: 0, "tfem_p1_field_adjoint": 1}
        check_columns(Y, parts, u_np, f"{what}: forward")
        want_k, want_c, tol_k, tol_c = fref.adjoint_reference(mesh_np, order, alpha, beta, g_np, u_np)
        assert kt.grad.shape == kt.shape and ct.grad.shape == ct.shape
        assert 0.0 < fref.check(_host(kt.grad), want_k, tol_k, f"{what}: d / d kappa") <= 1.0
        assert 0.0 < fref.check(_host(ct.grad), want_c, tol_c, f"{what}: d / d c") <= 1.0
        check_columns(U.grad, parts, g_np, f"{what}: d / d u = K g")


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
    n, k, order, alpha, beta = case["verts"].shape[0], case["k"], case["order"], case["alpha"], case["beta"]
    rings = eng.ring_plan()
    assert eng.dtype == dtype and eng.renumbered == case["renumber"] and rings is not None
    assert int(rings["layout"][23]) == 0 and int(rings["layout"][18]) == 1
    assert eng.field_refusal(beta, "apply", k) is None
    plain_mesh = {"vertices": case["verts"], "triangles": case["tris"]}
    # kappa data where there is a stiffness term, c data where there is a mass term; one value per
    # element for kappa on every third seed
    per_element = SWEEP_SEEDS.index(seed) % 3 == 0
    kv = fref.data(plain_mesh, order, 100 + seed, npd, per_element) if alpha != 0.0 else None
    cv = fref.data(plain_mesh, order, 200 + seed, npd) if beta != 0.0 else None
    kq = None if kv is None else basis.coefficient(torch.tensor(kv, dtype=dtype))
    cq = None if cv is None else basis.coefficient(torch.tensor(cv, dtype=dtype))
    op = basis.integrate_bilinear_form(_form(alpha, beta, kq, cq), layout="matrix_free")
    assert op.matrix_free is True and op._fields is not None
    what = f"seed {seed}, alpha {alpha:.3g}, beta {beta:.3g}, order {order}, k = {k}"
    U = torch.tensor(case["U"])
    U_np = case["U"].astype(np.float64)
    parts = fref.reference_parts(plain_mesh, order, alpha, beta, kv, cv, npd)
    with monkeypatch.context() as m:
        counts = counted(eng.lib, m, (MULTI, SINGLE))
        got = op @ U
        assert counts == {MULTI: 1, SINGLE: 0}
    check_columns(got, parts, U_np, what)
    Ue = eng._dofs_in(U).contiguous()
    out = torch.full((n * k,), float("nan"), dtype=dtype)
    Y = eng._apply_rings_field(op.alpha, op.beta, op._fields, Ue, out=out)
    assert bool(torch.isfinite(out).all()), f"{what}: entries of Y were left unwritten"
    for j in range(k):
        one = eng._apply_rings_field(op.alpha, op.beta, op._fields, Ue[:, j].contiguous())
        assert torch.equal(Y[:, j], one), f"{what}: column {j} differs from the single launch"
    SWEEP[seed] = {"slots": int(rings["layout"][6]), "chunked": bool(rings["chunked"]),
                   "renumbered": bool(eng.renumbered), "float32": single, "k": k, "isolated": case["isolated"] > 0,
                   "mass": beta != 0.0, "per_element": per_element and kv is not None}


def test_small_sweep_met_what_it_is_there_for():
    """Runs last.  The plans of these 16 seeds were looked at beforehand on the CPU
    (operator_reference.plan_of): 7- and 15-slot records, chunked and not, fp32 (seed 20), isolated
    vertices (seeds 0, 6, 12, 18, 38), k up to 17."""
    if len(SWEEP) < len(SWEEP_SEEDS):
        pytest.skip(f"only {len(SWEEP)} of {len(SWEEP_SEEDS)} seeds ran in this session")
    met = list(SWEEP.values())
    print(f"[coefficient-data block sweep] {SWEEP}")
    assert len(met) == 16
    assert any(r["slots"] == 7 for r in met) and any(r["slots"] == 15 for r in met)
    assert any(r["chunked"] for r in met) and any(not r["chunked"] for r in met)
    assert any(r["renumbered"] for r in met) and any(r["float32"] for r in met) and any(r["k"] > 8 for r in met)
    assert any(r["isolated"] for r in met) and any(r["mass"] for r in met) and any(not r["mass"] for r in met)
    assert any(r["per_element"] for r in met)


def test_coefficient_field_loads_example_runs():
    """examples/poisson_coefficient_field_loads.py at a small size in a fresh process: exit code 0 (its
    own assertions are the checks) and what it prints."""
    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_coefficient_field_loads.py"), "60"],
                          capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "block applications" in done.stdout and "assembled: 0" in done.stdout
