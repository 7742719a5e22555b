"""The fused CG loop on a real MI355X (-m gpu): the tfem_cg_* launches (csrc/tfem_cg.hip) one by
one against numpy, and sparse.fused_conjugate_gradients through solve_cg / solve_cg_multi against
the loop of torch operations and the long-double operator reference.

Kernel level.  Sizes: n = 1 (less than a wave), 63, 64, 65 (wave edges), 257 (workgroup edge) and
cap * block * (rows a lane takes per trip: 1, or the 2 / 4 that fill 16 bytes) + 77 rows, so that in
every instance the capped grid walks the rows a second time and ends in a ragged group;
n_vec = 1, 2, 4, 8 (the 16-byte instances), 3, 5 (the generic pass) and 9 (two passes); float64
and float32.  ap = d * p with d > 0, inv_diag > 0: every term of every sum is positive, so the
reductions have condition 1.  A fifth of inv_diag is exactly 0 (held rows) with ap = NaN there, one
column is inactive, and the workspace starts as NaN (a second test puts every vector one element
off the 16-byte alignment, where the widths 1, 2, 4, 8 fall back to the generic pass): a finite result proves that held rows are
skipped and that every partial sum a launch reads has been written.  Two steps, so both parities
of the workspace are read and written.

Bounds (none comes from a kernel's output), u = 2^-53 -- the sums are accumulated in double for both
types -- and u_T the unit roundoff of the vectors' type:
  any order of summation of n positive terms has relative error <= (n + 2) u, the products add
  2 u: sum r.r read back from the workspace is within ((n + 4) u + 2 u_T) of the long-double sum;
  alpha and beta, quotients of two such sums, are within (2 n + 8) u;
  an updated entry a + s * b (x + alpha p, r - alpha ap, inv_diag r + beta p) is within
  ((2 n + 8) u + 4 u_T) (|a| + |s b|) of the long-double value.
Held rows and the inactive column are bit for bit their input; two identical call sequences give
bit-identical vectors and workspace.

Loop level.  Meshes and loads from tests/operator_reference.py (the drift bound CG_C was measured
on them): seeds 2 (15-slot records, renumbered), 7 (isolated vertices: zero diagonal entries outside
`free`) and 26 (7-slot records, renumbered).  Bounds of the project: reported residual <= rtol =
1e-10, true residual <= rtol (1 + CG_C) with CG_C = 4 x 2.064e-3 (tests/test_hip_operator_fuzz.py),
fused against torch loop scaled error <= 1e-8 and iteration counts within 25
(tests/test_hip_operator_multi.py)."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coefficient_reference as cref
import operator_reference as oref
from conftest import scaled_error
from test_hip_operator import form, tf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U = 2.0 ** -53
CG_RTOL = 1e-10
CG_C = 4 * 2.064e-03
SEEDS = (2, 7, 26)


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def native():
    from pytorch_fem_solver_amd import _native

    return _native, _native.load()


# --------------------------------------------------------------------------- #
# kernel level
# --------------------------------------------------------------------------- #


def rows_per_lane(k, dtype):
    """Rows a lane takes per trip of its walk: the 16-byte instances (k = 1, 2, 4, 8) pack the 2 or
    4 rows that fill 16 bytes, every other width takes one row."""
    per_16_bytes = 16 // torch.empty(0, dtype=dtype).element_size()
    return max(1, per_16_bytes // k) if k in (1, 2, 4, 8) else 1


def kernel_sizes(k, dtype):
    """The last size is one trip of the capped grid for THIS instance plus 77 rows: every lane's walk
    `g += grid * block` takes a second trip, and the rows end in a ragged group."""
    from pytorch_fem_solver_amd.sparse import cg_constants

    block, cap, _ = cg_constants()
    return (1, 63, 64, 65, 257, cap * block * rows_per_lane(k, dtype) + 77)


def host(t):
    return t.detach().cpu().numpy()


class Launches:
    """The four launches on torch tensors."""

    def __init__(self, n, k, dtype):
        self.nat, self.lib = native()
        self.size = (torch.empty(0, dtype=dtype).element_size(), n, k)
        self.stream = self.nat.current_stream(torch.device("cuda"))

    def _go(self, fn, *args):
        self.nat.check(fn(*[self.nat.ptr(a) if torch.is_tensor(a) else a for a in args], self.stream))

    def start(self, r, inv_diag, p, ws):
        self._go(self.lib.tfem_cg_start, r, inv_diag, p, *self.size, ws)

    def dot(self, p, ap, inv_diag, ws):
        self._go(self.lib.tfem_cg_dot, p, ap, inv_diag, *self.size, ws)

    def update(self, x, r, p, ap, inv_diag, active, step, ws):
        self._go(self.lib.tfem_cg_update, x, r, p, ap, inv_diag, active, *self.size, step, ws)

    def direction(self, p, r, inv_diag, active, step, ws):
        self._go(self.lib.tfem_cg_direction, p, r, inv_diag, active, *self.size, step, ws)


def within(got, want, slack, what):
    """|got - want| <= slack entry by entry (want and slack long double); the worst ratio is printed."""
    got = np.asarray(got).astype(LD)
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), f"{what}: not finite"
    diff = np.abs(got - want)
    ratio = float((diff / np.where(slack > 0, slack, LD(1))).max()) if diff.size else 0.0
    print(f"{what}: worst |error| / bound {ratio:.3e}")
    assert (diff <= slack).all(), f"{what}: {ratio:.3e} of the bound"


def shifted(t):
    """The same values in a view that starts one element into its storage: not 16-byte aligned."""
    view = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    assert view.data_ptr() % 16 != 0
    return view.copy_(t)


def run_steps(n, k, dtype, seed, place=lambda t: t):
    """start, then two iterations (dot, update, direction) on synthetic data; every launch checked
    against numpy.  `place` puts every vector where the launches find it (`shifted`: off the 16-byte
    alignment).  Returns the final (x, r, p, ws) for the run-to-run comparison."""
    from pytorch_fem_solver_amd.sparse import cg_workspace

    npt = np.float64 if dtype == torch.float64 else np.float32
    u_t = float(np.finfo(npt).eps) / 2
    rng = np.random.default_rng(seed)
    inv_diag = rng.uniform(0.5, 2.0, n).astype(npt)
    held = rng.random(n) < 0.2
    held[0] = False  # at least one free row: the sums are positive
    inv_diag[held] = 0
    free = ~held
    d = rng.uniform(0.5, 2.0, (n, 1)).astype(npt)
    active_np = np.ones(k, dtype=np.int32)
    if k > 1:
        active_np[k // 2] = 0
    on = active_np != 0
    off_t = torch.tensor(~on)
    x = place(torch.tensor(rng.standard_normal((n, k)).astype(npt)))
    r = place(torch.tensor(rng.standard_normal((n, k)).astype(npt)))
    p = place(torch.tensor(rng.standard_normal((n, k)).astype(npt)))
    p_start = place(torch.full((n, k), float("nan"), dtype=dtype))
    dev_d, dev_held = torch.tensor(d), torch.tensor(held)
    inv_t, active = place(torch.tensor(inv_diag)), torch.tensor(active_np)
    ws = cg_workspace(n, k, x.device)
    assert ws.shape[0] == 5 and ws.shape[2] == k and ws.dtype == torch.float64
    ws.fill_(float("nan"))
    go = Launches(n, k, dtype)
    sum_tol = (n + 4) * U + 2 * u_t
    step_tol = LD((2 * n + 8) * U + 4 * u_t)
    w = inv_diag.astype(LD)[:, None]

    def sums(r_np):
        """(r.z, r.r) over the free rows in long double, z = inv_diag * r rounded to the type."""
        z = (inv_diag[:, None] * r_np).astype(LD)
        rl = r_np.astype(LD)
        return (rl * z)[free].sum(0), (rl * rl)[free].sum(0)

    def check_sums(parity, r_np, what):
        rz, rr = sums(r_np)
        for name, buf, want in (("r.z", ws[1 + 2 * parity], rz), ("r.r", ws[2 + 2 * parity], rr)):
            got = host(buf.sum(0)).astype(LD)
            assert np.isfinite(host(buf)).all(), f"{what}: a partial of {name} was not written"
            within(got, want, sum_tol * want, f"{what}: sum {name}")
        return rz

    # ---- start: p = inv_diag * r (one rounding: bit for bit), the sums into parity 1
    go.start(r, inv_t, p_start, ws)
    r_np = host(r)
    assert np.array_equal(host(p_start), inv_diag[:, None] * r_np), "start: p != inv_diag * r"
    assert bool((p_start[dev_held] == 0).all())
    rz_prev = check_sums(1, r_np, "start")

    for step in (0, 1):
        what = f"n = {n}, k = {k}, {npt.__name__}, step {step}"
        ap = place(dev_d * p)
        ap[dev_held] = float("nan")
        x0, r0, p0 = x.clone(), r.clone(), p.clone()
        x0_np, r0_np, p0_np, ap_np = host(x0).astype(LD), host(r0).astype(LD), host(p0).astype(LD), host(ap).astype(LD)
        # ---- dot
        go.dot(p, ap, inv_t, ws)
        assert np.isfinite(host(ws[0])).all(), f"{what}: a partial of p.Ap was not written (or a held row was read)"
        pap = (p0_np * ap_np)[free].sum(0)
        within(host(ws[0].sum(0)), pap, sum_tol * pap, f"{what}: sum p.Ap")
        # ---- update
        go.update(x, r, p, ap, inv_t, active, step, ws)
        alpha = np.where(on, rz_prev / pap, LD(0))
        moved = free[:, None] & on[None, :]
        want_x = np.where(moved, x0_np + alpha * p0_np, x0_np)
        want_r = np.where(moved, r0_np - alpha * np.where(moved, ap_np, 0), r0_np)
        within(host(x), want_x, step_tol * (np.abs(x0_np) + np.abs(alpha * p0_np)), f"{what}: x")
        within(host(r), want_r, step_tol * (np.abs(r0_np) + np.abs(alpha * np.where(moved, ap_np, 0))), f"{what}: r")
        assert torch.equal(x[dev_held], x0[dev_held]) and torch.equal(r[dev_held], r0[dev_held]), f"{what}: a held row moved"
        assert torch.equal(x[:, off_t], x0[:, off_t]) and torch.equal(r[:, off_t], r0[:, off_t]), f"{what}: the inactive column moved"
        assert torch.equal(p, p0), f"{what}: update wrote p"
        r1_np = host(r)
        rz_new = check_sums(step & 1, r1_np, what)
        # ---- direction
        go.direction(p, r, inv_t, active, step, ws)
        beta = np.where(on, rz_new / rz_prev, LD(0))
        z = w * r1_np.astype(LD)
        want_p = np.where(moved, z + beta * p0_np, p0_np)
        within(host(p), want_p, step_tol * (np.abs(z) + np.abs(beta * p0_np)), f"{what}: p")
        assert torch.equal(p[dev_held], p0[dev_held]), f"{what}: direction wrote a held row"
        assert torch.equal(p[:, off_t], p0[:, off_t]), f"{what}: direction wrote the inactive column"
        rz_prev = rz_new
    assert bool(torch.isfinite(ws).all())
    return x, r, p, ws


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9])
def test_cg_launches_against_numpy(k, dtype):
    sizes = kernel_sizes(k, dtype)
    for n in sizes:
        first = run_steps(n, k, dtype, seed=1000 * k + n % 997)
        if n in (65, sizes[-1]):
            again = run_steps(n, k, dtype, seed=1000 * k + n % 997)
            for a, b, name in zip(first, again, ("x", "r", "p", "workspace")):
                assert torch.equal(a, b), f"n = {n}, k = {k}: {name} differs between two identical runs"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_cg_launches_on_vectors_off_the_16_byte_alignment(k, dtype):
    """Every vector a view that starts one element into its storage: the widths with a 16-byte
    instance take the generic pass instead, each launch deciding from its own arrays.  The same
    checks against numpy, to the same bounds."""
    for n in (1, 65, 257 * 5 + 3):
        run_steps(n, k, dtype, seed=77 * k + n, place=shifted)


# --------------------------------------------------------------------------- #
# loop level
# --------------------------------------------------------------------------- #


def build_case(seed, monkeypatch):
    case = oref.sweep_case(seed)
    assert not case["single"] and not case["long_rows"]
    monkeypatch.delenv("TFEM_RING_LONG", raising=False)
    if case["renumber"]:
        monkeypatch.setenv("TFEM_RENUMBER", "1")
    else:
        monkeypatch.delenv("TFEM_RENUMBER", raising=False)
    verts, tris = case["verts"], case["tris"]
    outer = ((np.abs(verts) <= 1e-12) | (np.abs(verts - 1.0) <= 1e-12)).any(axis=1)
    mesh_np = {"vertices": verts, "triangles": tris.astype(np.int64) if case["int64"] else tris,
               "vertex_markers": outer.astype(np.int32).reshape(-1, 1)}
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, case["order"]))
    free_np = oref.cg_free_dofs(case)
    assert free_np is not None
    return case, basis, free_np


def true_residual_of(apply_ld, x, b, free_np):
    r = (np.asarray(b).astype(LD) - apply_ld(x))[free_np]
    return float(np.sqrt((r * r).sum()) / np.sqrt((np.asarray(b).astype(LD)[free_np] ** 2).sum()))


def compare_loops(A, B_np, X0_np, free_np, apply_ld, what, rtol=CG_RTOL, block=True):
    """solve_cg on columns 0 and 1 and, with `block`, solve_cg_multi on the three columns: the fused
    loop against the torch loop and the reference operator `apply_ld` (None: no true residual)."""
    n = B_np.shape[0]
    B, X0, free = torch.tensor(B_np), torch.tensor(X0_np), torch.tensor(free_np)
    held = torch.tensor(np.setdiff1d(np.arange(n), free_np))
    bound = rtol * (1.0 + CG_C)

    def check(x, res, col, label):
        assert bool(torch.isfinite(x).all()), f"{label}: not finite"
        assert float(res) <= rtol, (label, float(res))
        if apply_ld is not None:
            true = true_residual_of(apply_ld, host(x).reshape(-1), B_np[:, col], free_np)
            print(f"{label}: reported {float(res):.3e}, true {true:.3e} (bound {bound:.3e})")
            assert true <= bound, (label, true)
        assert torch.equal(x.reshape(-1)[held], X0[:, col][held]), f"{label}: an entry outside `free` moved"

    for col in (0, 1):
        b, x0 = B[:, col].contiguous(), X0[:, col].contiguous()
        xf, itf, resf = A.solve_cg(b, free=free, x0=x0, rtol=rtol, loop="fused")
        xt, itt, rest = A.solve_cg(b, free=free, x0=x0, rtol=rtol, loop="torch")
        assert xf.shape == (n,) and itf > 0 and isinstance(itf, int) and isinstance(resf, float)
        check(xf, resf, col, f"{what}, fused, column {col} ({itf} iterations)")
        check(xt, rest, col, f"{what}, torch, column {col} ({itt} iterations)")
        err = scaled_error(host(xf), host(xt))
        print(f"{what}, column {col}: fused against torch {err:.3e}, iterations {itf} / {itt}")
        assert err <= 1e-8 and abs(itf - itt) <= 25
        # the default on the GPU is the fused loop
        xd, itd, resd = A.solve_cg(b, free=free, x0=x0, rtol=rtol)
        assert torch.equal(xd, xf) and itd == itf and resd == resf
    if not block:
        return
    Xf, itsf, ressf = A.solve_cg_multi(B, free=free, X0=X0, rtol=rtol, loop="fused")
    Xt, itst, resst = A.solve_cg_multi(B, free=free, X0=X0, rtol=rtol, loop="torch")
    assert Xf.shape == (n, 3) and itsf.shape == (3,) and itsf.dtype == torch.int64 and not itsf.is_cuda
    assert not ressf.is_cuda and ressf.shape == (3,)
    for col in (0, 1):
        check(Xf[:, col], ressf[col], col, f"{what}, fused block, column {col} ({int(itsf[col])} iterations)")
        err = scaled_error(host(Xf[:, col]), host(Xt[:, col]))
        print(f"{what}, block column {col}: fused against torch {err:.3e}, iterations {int(itsf[col])} / {int(itst[col])}")
        assert err <= 1e-8 and abs(int(itsf[col]) - int(itst[col])) <= 25
    # the zero column: zero load, zero start
    assert int(itsf[2]) == 0 and float(ressf[2]) == 0.0 and bool((Xf[:, 2] == 0).all())
    # maxiter on a block: everything finite, the zero column untouched
    X7, its7, res7 = A.solve_cg_multi(B, free=free, X0=X0, rtol=rtol, maxiter=7, loop="fused")
    assert its7.tolist() == [7, 7, 0] and bool(torch.isfinite(X7).all()) and bool(torch.isfinite(res7).all())
    assert float(res7[2]) == 0.0 and bool((X7[:, 2] == 0).all())


@pytest.mark.parametrize("seed", SEEDS)
def test_fused_loop_on_the_p1_operator_and_the_csr(seed, monkeypatch):
    case, basis, free_np = build_case(seed, monkeypatch)
    alpha, beta = case["alpha"], case["beta"]
    op = basis.integrate_bilinear_form(form(alpha, beta), layout="operator")
    K = basis.integrate_bilinear_form(form(alpha, beta), layout="csr")
    assert op.matrix_free and basis._engine.renumbered == case["renumber"]
    if seed == 2:
        assert int(basis._engine.ring_plan()["layout"][6]) == 15
    ref = oref.OperatorReference(case["verts"], case["tris"], case["order"], alpha, beta)
    B_np, X0_np = oref.cg_loads(case), oref.cg_start(case)
    apply_ld = lambda x: ref.apply(x)[0]  # noqa: E731
    compare_loops(op, B_np, X0_np, free_np, apply_ld, f"seed {seed}, operator")
    compare_loops(K, B_np, X0_np, free_np, apply_ld, f"seed {seed}, CSR")


@pytest.mark.parametrize("seed", SEEDS)
def test_fused_loop_on_the_coefficient_operator(seed, monkeypatch):
    case, basis, free_np = build_case(seed, monkeypatch)
    a, b, kappa, c = 1.0, 0.5, cref.kappa_trig, cref.c_exp
    opc = basis.integrate_bilinear_form(cref.form(a, b, kappa, c), layout="operator")
    assert opc.matrix_free is True and opc._programs is not None
    # the float64 reference values of tests/coefficient_reference.py, applied in long double
    plain_mesh = {"vertices": case["verts"], "triangles": case["tris"]}
    rowptr, colind, vals = cref.reference_parts(plain_mesh, case["order"], a, b, kappa, c, np.float64)[:3]
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))

    def apply_ld(x):
        y = np.zeros(rowptr.size - 1, dtype=LD)
        np.add.at(y, rows, vals.astype(LD) * np.asarray(x).astype(LD)[colind])
        return y

    compare_loops(opc, oref.cg_loads(case), oref.cg_start(case), free_np, apply_ld, f"seed {seed}, coefficients")


def p2_system():
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(12, 0.25, 0)
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(2, 2))
    op = basis.integrate_bilinear_form(form(1.0, 0.0), layout="matrix_free")
    assert op.matrix_free and "P2 rows" in repr(op)
    n = op.shape[0]
    free_np = host(basis._basis_parameters["inner_dofs"]).reshape(-1)
    rng = np.random.default_rng(12)
    B_np = np.zeros((n, 3))
    B_np[:, 0] = 1.0
    B_np[:, 1] = rng.standard_normal(n)
    X0_np = 0.1 * rng.standard_normal((n, 3))
    X0_np[:, 2] = 0.0
    return basis, op, B_np, X0_np, free_np


def test_fused_loop_on_the_p2_operator():
    basis, op, B_np, X0_np, free_np = p2_system()
    Kc = basis.integrate_bilinear_form(form(1.0, 0.0), layout="csr").caller_numbering()
    rowptr, colind, vals = (host(t) for t in (Kc.crow_indices, Kc.col_indices, Kc.values))
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))

    def apply_ld(x):
        y = np.zeros(rowptr.size - 1, dtype=LD)
        np.add.at(y, rows, vals.astype(LD) * np.asarray(x).astype(LD)[colind])
        return y

    compare_loops(op, B_np, X0_np, free_np, apply_ld, "P2 rows")


def test_fused_loop_float32(monkeypatch):
    """float32 vectors (the sums stay in double): both loops reach rtol = 1e-4 within 25 iterations
    of each other."""
    case, _, free_np = build_case(7, monkeypatch)
    torch.set_default_dtype(torch.float32)
    verts = case["verts"].astype(np.float32)
    outer = ((np.abs(verts) <= 1e-12) | (np.abs(verts - 1.0) <= 1e-12)).any(axis=1)
    mesh_np = {"vertices": verts, "triangles": case["tris"], "vertex_markers": outer.astype(np.int32).reshape(-1, 1)}
    basis = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, case["order"]))
    op = basis.integrate_bilinear_form(form(case["alpha"], case["beta"]), layout="operator")
    assert op.matrix_free and op.dtype == torch.float32
    B = torch.tensor(oref.cg_loads(case).astype(np.float32))
    free = torch.tensor(free_np)
    for col in (0, 1):
        xf, itf, resf = op.solve_cg(B[:, col].contiguous(), free=free, rtol=1e-4, loop="fused")
        xt, itt, rest = op.solve_cg(B[:, col].contiguous(), free=free, rtol=1e-4, loop="torch")
        print(f"float32, column {col}: fused {itf} iterations, residual {resf:.3e}; torch {itt}, {rest:.3e}")
        assert xf.dtype == torch.float32 and bool(torch.isfinite(xf).all())
        assert resf <= 1e-4 and rest <= 1e-4 and abs(itf - itt) <= 25
    Xf, itsf, ressf = op.solve_cg_multi(B, free=free, rtol=1e-4, loop="fused")
    assert Xf.dtype == torch.float32 and float(ressf.max()) <= 1e-4 and int(itsf[2]) == 0


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


CG_SYMBOLS = ("tfem_cg_start", "tfem_cg_dot", "tfem_cg_update", "tfem_cg_direction")


def test_launches_per_iteration(monkeypatch):
    """50 iterations: 50 of each of dot / update / direction, 50 + 1 applies (the + 1 is the residual
    of the set-up), one start."""
    case, basis, free_np = build_case(7, monkeypatch)
    op = basis.integrate_bilinear_form(form(case["alpha"], case["beta"]), layout="operator")
    K = basis.integrate_bilinear_form(form(case["alpha"], case["beta"]), layout="csr")
    B, free = torch.tensor(oref.cg_loads(case)), torch.tensor(free_np)
    op.diagonal(), K.diagonal()
    _, lib = native()
    assert basis._engine.lib is lib
    for A, apply_name, block in ((op, "tfem_p1_apply_rings", False), (K, "tfem_csr_spmv", False),
                                 (op, "tfem_p1_apply_rings_multi", True)):
        with monkeypatch.context() as m:
            counts = counted(lib, m, CG_SYMBOLS + (apply_name,))
            diag_launches = 0 if A is K else 1  # the operator's diagonal is the apply launch without u
            if block:
                _, its, _ = A.solve_cg_multi(B[:, :2].contiguous(), free=free, rtol=0.0, maxiter=50, loop="fused")
                assert its.tolist() == [50, 50]
                diag_name = "tfem_p1_apply_rings"
                diag_launches = 0 if diag_name != apply_name else diag_launches
            else:
                _, it, _ = A.solve_cg(B[:, 1].contiguous(), free=free, rtol=0.0, maxiter=50, loop="fused")
                assert it == 50
        print(apply_name, counts)
        assert counts["tfem_cg_start"] == 1
        assert counts["tfem_cg_dot"] == counts["tfem_cg_update"] == counts["tfem_cg_direction"] == 50
        assert counts[apply_name] == 50 + 1 + diag_launches


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, {repo!r})
import pytorch_fem_solver_amd as tf
from pytorch_fem_solver_amd import _native, meshgen, sparse
assert sparse._CG_LOOP == "torch"
torch.set_default_dtype(torch.float64)
torch.set_default_device("cuda")
lib = _native.load()
counts = {{}}
def wrap(name):
    inner = getattr(lib, name)
    def call(*args):
        counts[name] = counts.get(name, 0) + 1
        return inner(*args)
    setattr(lib, name, call)
for name in {names!r} + ("tfem_p1_apply_rings",):
    wrap(name)
basis = tf.Basis(tf.MeshTri(triangulation=meshgen.unit_square(12, 0.25, 0)), tf.ElementTri(1, 3))
op = basis.integrate_bilinear_form(lambda b: b.v_grad @ b.v_grad.mT, layout="operator")
free = basis._basis_parameters["inner_dofs"]
b = torch.ones(op.shape[0])
x, it, res = op.solve_cg(b, free=free, rtol=1e-10)
X, its, ress = op.to_csr().solve_cg_multi(torch.stack([b, 2 * b], dim=1), free=free, rtol=1e-10)
assert res <= 1e-10 and float(ress.max()) <= 1e-10
print("COUNTS", sorted(counts.items()), it)
"""


def test_tfem_cg_torch_keeps_the_torch_loop():
    """TFEM_CG=torch (read at import, hence the child process): no tfem_cg_* launch."""
    env = dict(os.environ, TFEM_CG="torch")
    out = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, names=CG_SYMBOLS)], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [row for row in out.stdout.splitlines() if row.startswith("COUNTS")][-1]
    print(line)
    assert "tfem_cg_" not in line and "tfem_p1_apply_rings" in line


def test_fused_loop_needs_a_device():
    A = tf().CSRMatrix(torch.tensor([0, 1, 2], device="cpu"), torch.tensor([0, 1], dtype=torch.int32, device="cpu"),
                       torch.tensor([2.0, 4.0], device="cpu"), (2, 2))
    with pytest.raises(ValueError):
        A.solve_cg(torch.ones(2, device="cpu"), loop="fused")
