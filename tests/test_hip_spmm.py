"""tfem_csr_spmm on a real MI355X (-m gpu): the C entry point on seeded random CSR matrices, and the
block path on top of it -- CSRMatrix.matvec, the block CG loops on a CSRMatrix, FormOperator.from_csr
with autograd, the example script.

Kernel level.  Matrices from numpy, independent of any mesh: n_rows = 1 (a lone row), 31 (a partial
workgroup of 32 rows), 33 and 257 (a second workgroup and a ragged last one), n_cols != n_rows, row
lengths from {0, 1, 7, 8, 9, 16, 17, 22, 40} (empty rows; one, two, three and more trips of the
eight lanes with ragged ends), n_vec = 1, 3, 5, 7 (one generic pass), 9, 16, 17 (two and three
passes), 2, 4, 8 (the instances with wide accesses), float64 and float32.  y lies inside a larger
buffer filled with NaN.

Two properties, neither taken from the kernel's output:
  column c of the result has the BITS of tfem_csr_spmv on the contiguous copy of column c;
  every entry is within (m + 1) u S of the reference, S = sum_p |vals[p] x[colind[p]][c]|,
  m = ceil(len / 8) + 3, u = 2^-53 (float64) or 2^-24 (float32): an entry is a product (one
  rounding), at most ceil(len / 8) additions in its lane and three in the butterfly, i.e. at most
  m + 1 chained roundings on every term.  The reference is evaluated from the stored data (the
  float32 data for float32) in numpy's long double, whose own error (len 2^-64 S where long double is
  the x87 format, never more than that of float64) is far inside the bound."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_LENGTHS = (0, 1, 7, 8, 9, 16, 17, 22, 40)
N_ROWS = (1, 31, 33, 257)
N_VECS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17)
PAD = 64  # NaN entries on either side of y: a multiple of 16 bytes, so y keeps the allocation's alignment


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


def tf():
    import pytorch_fem_solver_amd

    return pytorch_fem_solver_amd


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def random_csr(n_rows, seed, np_dtype):
    """(rowptr, colind, vals, n_cols) as numpy arrays: every length of ROW_LENGTHS in the first rows
    (as many as there are rows), the rest drawn; ascending distinct columns per row."""
    rng = np.random.default_rng(seed)
    n_cols = 2 * n_rows + 43
    lengths = rng.choice(ROW_LENGTHS, size=n_rows)
    forced = rng.permutation(len(ROW_LENGTHS))[:n_rows]
    lengths[: forced.size] = np.asarray(ROW_LENGTHS)[forced]
    if n_rows == 1:
        lengths[0] = 22  # the lone row: three trips with a ragged end
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lengths)
    colind = np.concatenate([np.sort(rng.choice(n_cols, size=m, replace=False)) for m in lengths] + [np.zeros(0, np.int64)])
    vals = rng.standard_normal(int(rowptr[-1])).astype(np_dtype)
    return rowptr, colind.astype(np.int32), vals, n_cols


def reference(rowptr, colind, vals, x):
    """(sum_p vals[p] x[colind[p]][c], sum_p |...|, row lengths) in long double from the stored data."""
    LD = np.longdouble
    n_rows = rowptr.size - 1
    lengths = np.diff(rowptr)
    row_of = np.repeat(np.arange(n_rows), lengths)
    prod = vals.astype(LD)[:, None] * x.astype(LD)[colind]
    want = np.zeros((n_rows, x.shape[1]), dtype=LD)
    size = np.zeros((n_rows, x.shape[1]), dtype=LD)
    np.add.at(want, row_of, prod)
    np.add.at(size, row_of, np.abs(prod))
    return want, size, lengths


class Csr:
    """A random matrix on the device and the two launches on it."""

    def __init__(self, n_rows, seed, dtype):
        self.nat, self.lib = native()
        self.dtype = dtype
        self.np_dtype = np.float64 if dtype == torch.float64 else np.float32
        self.host = random_csr(n_rows, seed, self.np_dtype)
        rowptr, colind, vals, self.n_cols = self.host
        self.n_rows = n_rows
        self.rowptr, self.colind, self.vals = torch.tensor(rowptr), torch.tensor(colind), torch.tensor(vals)
        self.real_bytes = self.vals.element_size()
        self.stream = self.nat.current_stream(torch.device("cuda"))

    def spmm(self, x, y):
        p = self.nat.ptr
        self.nat.check(self.lib.tfem_csr_spmm(p(self.rowptr), p(self.colind), p(self.vals), self.real_bytes, self.n_rows,
                                              self.n_cols, x.shape[1], p(x), p(y), self.stream))

    def spmv(self, x):
        p = self.nat.ptr
        y = torch.full((self.n_rows,), float("nan"), dtype=self.dtype)
        self.nat.check(self.lib.tfem_csr_spmv(p(self.rowptr), p(self.colind), p(self.vals), self.real_bytes, self.n_rows,
                                              p(x), p(y), self.stream))
        return y

    def guarded(self, n_vec, shift=0):
        """(buffer of NaN, y = its (n_rows, n_vec) view PAD + shift entries in)."""
        buf = torch.full((self.n_rows * n_vec + 2 * PAD + shift,), float("nan"), dtype=self.dtype)
        lo = PAD + shift
        return buf, buf[lo: lo + self.n_rows * n_vec].view(self.n_rows, n_vec)

    def check_guard(self, buf, y, what):
        lo = (y.data_ptr() - buf.data_ptr()) // buf.element_size()
        assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + y.numel():]).all()), f"{what}: wrote outside y"
        assert not bool(torch.isnan(y).any()), f"{what}: an entry of y was not written"


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32), ids=("float64", "float32"))
def test_spmm_against_spmv_bits_and_the_forward_bound(dtype):
    u = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    worst = 0.0
    for n_rows in N_ROWS:
        A = Csr(n_rows, 1000 + n_rows, dtype)
        rowptr, colind, vals, n_cols = A.host
        assert n_cols != n_rows
        for n_vec in N_VECS:
            what = f"{dtype}, {n_rows} rows, n_vec {n_vec}"
            rng = np.random.default_rng(n_rows * 100 + n_vec)
            x_np = rng.standard_normal((n_cols, n_vec)).astype(A.np_dtype)
            x = torch.tensor(x_np)
            buf, y = A.guarded(n_vec)
            assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
            A.spmm(x, y)
            torch.cuda.synchronize()
            A.check_guard(buf, y, what)
            for c in range(n_vec):
                assert same_bits(y[:, c], A.spmv(x[:, c].contiguous())), f"{what}: column {c} differs from tfem_csr_spmv"
            want, size, lengths = reference(rowptr, colind, vals, x_np)
            m = -(-lengths // 8) + 3
            bound = ((m + 1) * u)[:, None] * size
            err = np.abs(y.cpu().numpy().astype(np.longdouble) - want)
            assert bool((err <= bound).all()), f"{what}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}"
            # an empty row: exactly zero
            assert bool((y.cpu().numpy()[lengths == 0] == 0).all())
            nonzero = bound > 0
            if nonzero.any():
                worst = max(worst, float((err[nonzero] / bound[nonzero]).max()))
    print(f"{dtype}: largest error / bound over the sweep {worst:.3f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32), ids=("float64", "float32"))
@pytest.mark.parametrize("n_vec", (2, 4, 8))
def test_spmm_with_bases_off_the_16_byte_alignment(n_vec, dtype):
    """x and y one element into their allocations: the launch takes the scalar passes (chosen by the
    pointers, not assumed) and gives the bits of the aligned launch; so does each base alone."""
    A = Csr(257, 77, dtype)
    rng = np.random.default_rng(n_vec)
    x_np = rng.standard_normal((A.n_cols, n_vec)).astype(A.np_dtype)
    x = torch.tensor(x_np)
    buf, y = A.guarded(n_vec)
    A.spmm(x, y)
    x_store = torch.full((x.numel() + 1,), float("nan"), dtype=dtype)
    x_off = x_store[1:].view(A.n_cols, n_vec)
    x_off.copy_(x)
    assert x_off.data_ptr() % 16 != 0 and x_off.is_contiguous()
    for x_in, shift in ((x_off, 1), (x_off, 0), (x, 1)):
        buf_off, y_off = A.guarded(n_vec, shift=shift)
        assert (y_off.data_ptr() % 16 != 0) == (shift == 1)
        A.spmm(x_in, y_off)
        torch.cuda.synchronize()
        A.check_guard(buf_off, y_off, f"{dtype}, n_vec {n_vec}, shift {shift}")
        assert same_bits(y_off, y)
    assert bool(torch.isnan(x_store[0])) and same_bits(x_off, x)


# --------------------------------------------------------------------------- #
# the block path on top
# --------------------------------------------------------------------------- #

SPIED = ("tfem_csr_spmm", "tfem_csr_spmv")
CG_SYMBOLS = ("tfem_cg_start", "tfem_cg_dot", "tfem_cg_update", "tfem_cg_direction")


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


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def assembled(order, n):
    from pytorch_fem_solver_amd import meshgen

    basis = tf().Basis(tf().MeshTri(triangulation=meshgen.unit_square(n, 0.25, 0)), tf().ElementTri(order, order + 2))
    K = basis.integrate_bilinear_form(stiffness, layout="csr")
    return basis, K


@pytest.mark.parametrize("order,n", ((1, 9), (2, 6)), ids=("P1", "P2"))
@pytest.mark.parametrize("permuted", (False, True), ids=("plain", "perm"))
def test_csrmatrix_matvec_of_a_block_is_one_spmm_launch(order, n, permuted, monkeypatch):
    from pytorch_fem_solver_amd.sparse import CSRMatrix

    _, K = assembled(order, n)
    N = K.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(5)
    if permuted:  # the stored arrays taken as a renumbering of the caller's DoFs
        K = CSRMatrix(K.crow_indices, K.col_indices, K.values, K.shape, perm=torch.randperm(N, generator=gen))
    assert (K.perm is not None) == permuted
    U = torch.randn(N, 3, generator=gen)
    _, lib = native()
    with monkeypatch.context() as m:
        counts = counted(lib, m, SPIED)
        got = K.matvec(U)
        assert counts == {"tfem_csr_spmm": 1, "tfem_csr_spmv": 0} and got.shape == (N, 3)
        turned = K.matvec(torch.randn(3, N, generator=gen).T)
        assert counts == {"tfem_csr_spmm": 2, "tfem_csr_spmv": 0} and turned.shape == (N, 3)
        for single in (U[:, :1].contiguous(), U[:, 0].contiguous()):
            before = dict(counts)
            out = K.matvec(single)
            assert counts["tfem_csr_spmv"] == before["tfem_csr_spmv"] + 1 and counts["tfem_csr_spmm"] == before["tfem_csr_spmm"]
            assert out.shape == single.shape and same_bits(out.reshape(-1), got[:, 0])
    for j in range(3):
        assert same_bits(got[:, j], K.matvec(U[:, j].contiguous())), f"column {j}"
    # a non-contiguous block (a transposed view) gives the same numbers
    Ut = U.T.contiguous().T
    assert not Ut.is_contiguous() and same_bits(K.matvec(Ut), got)
    # and they are K U in the caller's numbering: the dense product sums the same terms (22 per row at
    # most, the rest zeros) in another order; each of the two sums is within N 2^-53 of |K| |U|
    dense, size = K.to_dense() @ U, K.to_dense().abs() @ U.abs()
    assert bool(((got - dense).abs() <= 2 * N * 2.0 ** -53 * size).all())


def test_fused_block_cg_on_the_csr_launches(monkeypatch):
    """50 iterations: 51 tfem_csr_spmm calls (the + 1 is the residual of the set-up), no tfem_csr_spmv
    call, the tfem_cg_* counts of test_hip_fused_cg.test_launches_per_iteration."""
    basis, K = assembled(2, 16)
    free = basis._basis_parameters["inner_dofs"]
    B = torch.randn(K.shape[0], 2, generator=torch.Generator(device="cuda").manual_seed(11))
    K.diagonal()
    _, lib = native()
    with monkeypatch.context() as m:
        counts = counted(lib, m, SPIED + CG_SYMBOLS)
        _, its, _ = K.solve_cg_multi(B, free=free, rtol=0.0, maxiter=50, loop="fused")
    print(counts)
    assert its.tolist() == [50, 50]
    assert counts["tfem_csr_spmm"] == 51 and counts["tfem_csr_spmv"] == 0
    assert counts["tfem_cg_start"] == 1
    assert counts["tfem_cg_dot"] == counts["tfem_cg_update"] == counts["tfem_cg_direction"] == 50


@pytest.fixture(scope="module")
def cg_case():
    """A P2 stiffness CSR, three loads (the last all zero) and the single-column solves, computed once."""
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    try:
        basis, K = assembled(2, 12)
        free = basis._basis_parameters["inner_dofs"]
        B = torch.randn(K.shape[0], 3, generator=torch.Generator(device="cuda").manual_seed(3))
        B[:, 2] = 0
        singles = [K.solve_cg(B[:, c].contiguous(), free=free, rtol=1e-10) for c in (0, 1)]
    finally:
        torch.set_default_device("cpu")
    return K, free, B, singles


@pytest.mark.parametrize("loop", ("fused", "torch"))
def test_block_cg_on_the_csr_against_the_single_solves(cg_case, loop, monkeypatch):
    """The project's block-CG contract (tests/test_hip_operator_fuzz.py): scaled error <= 1e-8 and
    iteration counts within 25 of the single-column solves; a zero column takes no iteration."""
    from conftest import scaled_error

    K, free, B, singles = cg_case
    _, lib = native()
    with monkeypatch.context() as m:
        counts = counted(lib, m, SPIED)
        X, its, ress = K.solve_cg_multi(B, free=free, rtol=1e-10, loop=loop)
    assert counts["tfem_csr_spmv"] == 0 and counts["tfem_csr_spmm"] >= int(its.max()) + 1
    assert X.shape == B.shape and bool(torch.isfinite(X).all())
    assert int(its[2]) == 0 and float(ress[2]) == 0.0 and bool((X[:, 2] == 0).all())
    for c in (0, 1):
        x, it, res = singles[c]
        err = scaled_error(X[:, c].cpu().numpy(), x.cpu().numpy())
        print(f"{loop}, column {c}: scaled error {err:.3e}, iterations {int(its[c])} / {it}, residual {float(ress[c]):.3e}")
        assert res <= 1e-10 and float(ress[c]) <= 1e-10
        assert err <= 1e-8 and abs(int(its[c]) - it) <= 25


def test_form_operator_from_csr_on_a_block(monkeypatch):
    from pytorch_fem_solver_amd.sparse import FormOperator

    _, K = assembled(1, 5)
    N = K.shape[0]
    assert 24 <= N <= 60
    op = FormOperator.from_csr(K, symmetric=True)
    U = torch.randn(N, 3, generator=torch.Generator(device="cuda").manual_seed(2))
    _, lib = native()
    with monkeypatch.context() as m:
        counts = counted(lib, m, SPIED)
        got = op @ U
        assert counts == {"tfem_csr_spmm": 1, "tfem_csr_spmv": 0}
        leaf = U.clone().requires_grad_(True)
        (op.matvec(leaf) * U).sum().backward()
        assert counts == {"tfem_csr_spmm": 3, "tfem_csr_spmv": 0}
    assert same_bits(got, K.matvec(U))
    assert same_bits(leaf.grad, got)  # d/dU sum(U . K V) at V = U is K^T U = K U
    assert torch.autograd.gradcheck(op.matvec, (U.clone().requires_grad_(True),))


def test_p2_multiple_loads_example_runs():
    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_p2_multiple_loads.py"), "24"],
                          capture_output=True, text=True, timeout=300, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "block solve" in done.stdout, "the example prints what it computed"
