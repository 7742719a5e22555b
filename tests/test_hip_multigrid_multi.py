"""Geometric multigrid on blocks of right-hand sides, on a real MI355X: the three tfem_mg_*_multi
kernels (csrc/tfem_mg.hip) bit for bit against the single kernels on every column and against
numpy in extended precision, ``GeometricMultigrid.vcycle_multi`` against the CPU model of
tests/multigrid_reference.py on every column, and ``solve_multi`` against the model's PCG with
columns that freeze at different times.  Tables, hierarchies, models and solvers are those of
tests/test_hip_multigrid.py (imported, so both files build them once)."""

import numpy as np
import pytest
import torch

import multigrid_reference as mgref
import test_hip_multigrid as single

pytestmark = pytest.mark.gpu

LD = np.longdouble
DTYPES = single.DTYPES
WIDTHS = [1, 2, 3, 4, 5, 8, 9]  # forwarded | rows of 24 / 12 and 40 / 20 bytes | a full pass | a second pass
SENTINEL = 12345.0
tf = single.tf


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


# --------------------------------------------------------------------------------- helpers
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    as_int = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(as_int) == b.view(as_int)).all())


def _block(rng, n, n_vec, np_dtype):
    return rng.standard_normal((n, n_vec)).astype(np_dtype)


def _framed(values, lead, fill=None):
    """(flat, view): a copy of the (n, k) array `values` (or `fill` everywhere) on the device with
    `lead` guard entries in front and 16 behind, all SENTINEL.  lead = 16 keeps the 16-byte
    alignment of the allocation, lead = 17 starts the block one element off it."""
    n, k = values.shape
    flat = torch.full((lead + n * k + 16,), SENTINEL,
                      dtype=torch.float64 if values.dtype == np.float64 else torch.float32)
    view = flat[lead:lead + n * k].view(n, k)
    if fill is None:
        view.copy_(torch.tensor(values))
    else:
        view.fill_(fill)
    assert view.data_ptr() % 16 == (0 if lead == 16 else view.element_size())
    return flat, view


def _guards_intact(flat, lead, size):
    head, tail = flat[:lead].cpu().numpy(), flat[lead + size:].cpu().numpy()
    return bool((head == SENTINEL).all() and (tail == SENTINEL).all())


def _dev(v):
    return None if v is None else torch.tensor(v)


# --------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("n_vec", WIDTHS)
@pytest.mark.parametrize("mesh", ["square5", "delaunay300"])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_smooth_multi_kernel(mesh, dtype, np_dtype, n_vec):
    """x = w b and x += w (b - ax) on (n, n_vec) blocks, 16-byte aligned and one element off the
    grid: column j bit for bit the single kernel on the contiguous column j, |err| <= 2 eps (|x| +
    |w b| + |w ax|) per entry against numpy in longdouble, two runs the same bits."""
    n = single._tables(mesh)[1]
    rng = np.random.default_rng(31)
    w = single._random(rng, n, np_dtype)
    wd = torch.tensor(w)
    wl = w.astype(LD)[:, None]
    for lead in (16, 17):
        host = {k: _block(rng, n, n_vec, np_dtype) for k in "xba"}
        frames = {k: _framed(host[k], lead) for k in "ba"}
        x, b, a = (host[k].astype(LD) for k in "xba")
        for first in (1, 0):
            runs = []
            for _ in range(2):
                flat, xd = _framed(host["x"], lead)
                single._call("tfem_mg_smooth_multi", xd, frames["b"][1], None if first else frames["a"][1], wd,
                             xd.element_size(), n, n_vec, first)
                runs.append(xd.cpu().numpy())
                assert _guards_intact(flat, lead, n * n_vec)
            assert _same_bits(runs[0], runs[1]), "two runs differ"
            for j in range(n_vec):
                xs = torch.tensor(host["x"][:, j].copy())
                single._call("tfem_mg_smooth", xs, torch.tensor(host["b"][:, j].copy()),
                             None if first else torch.tensor(host["a"][:, j].copy()), wd, xs.element_size(), n, first)
                assert _same_bits(runs[0][:, j], xs.cpu().numpy()), f"column {j} differs from the single kernel"
            want = wl * b if first else x + wl * (b - a)
            scale = np.abs(wl * b) if first else np.abs(x) + np.abs(wl * b) + np.abs(wl * a)
            single._close(runs[0], want, scale, 2, np_dtype, f"smooth_multi n_vec={n_vec} first={first} lead={lead}")


def _restrict_reference(ptr, idx, m_c, m_f, b, a, n_c, n_f):
    """(want, scale) (n_c, k) in longdouble; an entry of idx outside [0, n_f) contributes 0."""
    rows = np.repeat(np.arange(n_c), np.diff(ptr))
    inside = (idx >= 0) & (idx < n_f)
    safe = np.where(inside, idx, 0)
    weight = (np.ones(n_f, dtype=LD) if m_f is None else m_f.astype(LD))[safe] * inside
    terms = 0.5 * weight[:, None] * (b.astype(LD)[safe] - a.astype(LD)[safe])
    sizes = 0.5 * weight[:, None] * (np.abs(b.astype(LD))[safe] + np.abs(a.astype(LD))[safe])
    want, scale = np.zeros((n_c, b.shape[1]), dtype=LD), np.zeros((n_c, b.shape[1]), dtype=LD)
    np.add.at(want, rows, terms)
    np.add.at(scale, rows, sizes)
    if m_c is not None:
        want, scale = m_c[:, None] * want, m_c[:, None] * scale
    return want, scale


@pytest.mark.parametrize("n_vec", WIDTHS)
@pytest.mark.parametrize("mesh", ["square5", "delaunay300"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_restrict_multi_kernel(mesh, masked, dtype, np_dtype, n_vec):
    """r_c = m_c P^T (m_f (b - ax)) on blocks: column j bit for bit the single kernel, |err| <= 16
    eps sum |terms| per entry, two runs the same bits, the same bits from blocks one element off the
    16-byte grid, guards around the output intact; an entry of idx that is >= n_f contributes 0
    and changes no other row."""
    n_c, n_f, parents, ptr, idx = single._tables(mesh)
    rng = np.random.default_rng(32)
    b, a = _block(rng, n_f, n_vec, np_dtype), _block(rng, n_f, n_vec, np_dtype)
    m_c = single._random(rng, n_c, np_dtype, mask=True) if masked else None
    m_f = single._random(rng, n_f, np_dtype, mask=True) if masked else None
    tables = (_dev(ptr), _dev(idx), _dev(m_c), _dev(m_f))
    blank = np.zeros((n_c, n_vec), dtype=np_dtype)

    def run(lead, tables=tables):
        bd, ad = _framed(b, lead)[1], _framed(a, lead)[1]
        flat, out = _framed(blank, lead, fill=float("nan"))
        single._call("tfem_mg_restrict_residual_multi", *tables, bd, ad, out, out.element_size(), n_c, n_f, n_vec)
        assert _guards_intact(flat, lead, n_c * n_vec)
        return out.cpu().numpy()

    runs = [run(16), run(16)]
    assert _same_bits(runs[0], runs[1]), "two runs differ"
    assert _same_bits(runs[0], run(17)), "blocks off the 16-byte grid give other bits"
    for j in range(n_vec):
        out = torch.full((n_c,), float("nan"), dtype=dtype)
        single._call("tfem_mg_restrict_residual", *tables, torch.tensor(b[:, j].copy()), torch.tensor(a[:, j].copy()),
                     out, out.element_size(), n_c, n_f)
        assert _same_bits(runs[0][:, j], out.cpu().numpy()), f"column {j} differs from the single kernel"
    want, scale = _restrict_reference(ptr, idx, m_c, m_f, b, a, n_c, n_f)
    if m_c is not None:
        assert (runs[0][m_c == 0] == 0).all()
    single._close(runs[0], want, scale, 16, np_dtype, f"restrict_multi {mesh} masked={masked} n_vec={n_vec}")

    # a data-driven index outside the fine array: the first one past it, and the largest int32
    long_rows = np.flatnonzero(np.diff(ptr) >= 3)
    v0, v1 = int(long_rows[0]), int(long_rows[-1])
    assert v0 != v1
    bad = idx.copy()
    bad[ptr[v0] + 1] = n_f
    bad[ptr[v1] + 2] = np.iinfo(np.int32).max
    for lead in (16, 17):
        got = run(lead, (tables[0], _dev(bad), tables[2], tables[3]))
        others = np.ones(n_c, dtype=bool)
        others[[v0, v1]] = False
        assert _same_bits(got[others], runs[0][others]), "a row without the bad entry changed"
        want_bad, scale_bad = _restrict_reference(ptr, bad, m_c, m_f, b, a, n_c, n_f)
        single._close(got, want_bad, scale_bad, 16, np_dtype, f"restrict_multi out-of-range idx lead={lead}")


@pytest.mark.parametrize("n_vec", WIDTHS)
@pytest.mark.parametrize("mesh", ["square5", "delaunay300"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_prolong_multi_kernel(mesh, masked, dtype, np_dtype, n_vec):
    """x_f += m_f P e_c on blocks: column j bit for bit the single kernel, |err| <= 2 eps (|x| +
    0.5 |e_a| + 0.5 |e_b|) per entry, two runs the same bits, the same from blocks off the 16-byte
    grid, guards around x_f intact; a parent that is >= n_c contributes 0 and changes no other
    row."""
    n_c, n_f, parents, ptr, idx = single._tables(mesh)
    rng = np.random.default_rng(33)
    e, x = _block(rng, n_c, n_vec, np_dtype), _block(rng, n_f, n_vec, np_dtype)
    m_f = single._random(rng, n_f, np_dtype, mask=True) if masked else None
    md = _dev(m_f)

    def run(lead, table=parents):
        ed = _framed(e, lead)[1]
        flat, xd = _framed(x, lead)
        single._call("tfem_mg_prolong_add_multi", torch.tensor(table), md, ed, xd, xd.element_size(), n_f, n_c, n_vec)
        assert _guards_intact(flat, lead, n_f * n_vec)
        return xd.cpu().numpy()

    def reference(table):
        inside = (table >= 0) & (table < n_c)
        safe = np.where(inside, table, 0)
        el = e.astype(LD)
        ea, eb = el[safe[:, 0]] * inside[:, :1], el[safe[:, 1]] * inside[:, 1:]
        weight = (np.ones(n_f, dtype=LD) if m_f is None else m_f.astype(LD))[:, None]
        return (x.astype(LD) + weight * 0.5 * (ea + eb),
                np.abs(x.astype(LD)) + weight * 0.5 * (np.abs(ea) + np.abs(eb)))

    runs = [run(16), run(16)]
    assert _same_bits(runs[0], runs[1]), "two runs differ"
    assert _same_bits(runs[0], run(17)), "blocks off the 16-byte grid give other bits"
    par = torch.tensor(parents)
    for j in range(n_vec):
        xs = torch.tensor(x[:, j].copy())
        single._call("tfem_mg_prolong_add", par, md, torch.tensor(e[:, j].copy()), xs, xs.element_size(), n_f, n_c)
        assert _same_bits(runs[0][:, j], xs.cpu().numpy()), f"column {j} differs from the single kernel"
    if m_f is not None:
        assert _same_bits(runs[0][m_f == 0], x[m_f == 0])
    single._close(runs[0], *reference(parents), 2, np_dtype, f"prolong_multi {mesh} masked={masked} n_vec={n_vec}")

    # a data-driven parent outside the coarse array: the first one past it, and the largest int32
    i0, i1 = n_f // 3, n_f - 2
    bad = parents.copy()
    bad[i0, 1] = n_c
    bad[i1, 0] = np.iinfo(np.int32).max
    for lead in (16, 17):
        got = run(lead, bad)
        others = np.ones(n_f, dtype=bool)
        others[[i0, i1]] = False
        assert _same_bits(got[others], runs[0][others]), "a row without the bad parent changed"
        single._close(got, *reference(bad), 2, np_dtype, f"prolong_multi out-of-range parent lead={lead}")


# --------------------------------------------------------------------------------- the cycle
def _check_columns(Z, R, model, bound, what):
    Z = Z.cpu().numpy()
    assert Z.shape == R.shape
    for j in range(R.shape[1]):
        want = model.vcycle(R[:, j].astype(np.float64))
        err = np.abs(Z[:, j] - want).max() / np.abs(want).max()
        print(f"{what}, column {j}: cycle against the model {err:.3e}")
        assert err <= bound
    assert (Z[model.mask[-1] == 0] == 0).all()
    return Z


@pytest.mark.parametrize("name", ["stiffness", "no_mask", "coefficients", "clockwise"])
def test_vcycle_multi_matches_the_model_on_every_column(name):
    """k = 3 standard-normal columns, 2 levels: every column within 1e-10 of |z|_inf of the model's
    cycle (the bound of the single cycle), exactly 0 on the held DoFs; an all-zero column gives an
    all-zero column; k = 1 works; the single cycle's buffers are not disturbed."""
    mg, model = single._solver(name, 2), single._model(name, 2)
    n = model.K[-1].shape[0]
    rng = np.random.default_rng(41)
    R = rng.standard_normal((n, 3))
    r1 = torch.tensor(rng.standard_normal(n))
    before = mg.vcycle(r1).cpu().numpy()
    Z = mg.vcycle_multi(torch.tensor(R))
    assert Z.dtype == torch.float64 and tuple(Z.shape) == (n, 3)
    _check_columns(Z, R, model, 1e-10, f"{name}, k = 3")
    assert _same_bits(mg.vcycle(r1).cpu().numpy(), before), "the block cycle disturbed the single cycle"
    R0 = R.copy()
    R0[:, 1] = 0
    Z0 = mg.vcycle_multi(torch.tensor(R0)).cpu().numpy()
    assert (Z0[:, 1] == 0).all(), "an all-zero column does not give an all-zero column"
    assert np.abs(Z0[:, [0, 2]] - Z.cpu().numpy()[:, [0, 2]]).max() <= 1e-10 * np.abs(Z0).max()
    Z1 = mg.vcycle_multi(torch.tensor(R[:, :1]))
    assert tuple(Z1.shape) == (n, 1)
    _check_columns(Z1, R[:, :1], model, 1e-10, f"{name}, k = 1")
    # more widths than are kept: the oldest is dropped and comes back
    for k in (2, 3, 1, 2):
        _check_columns(mg.vcycle_multi(torch.tensor(R[:, :k])), R[:, :k], model, 1e-10, f"{name}, k = {k} again")
    assert len(mg._blocks) <= mg.BLOCK_WIDTHS_KEPT
    assert _same_bits(mg.vcycle(r1).cpu().numpy(), before)


def test_vcycle_multi_in_float32():
    """dtype=float32, k = 2: the bound of the single float32 cycle, 5e-3 (tests/test_hip_multigrid.py)."""
    mesh, bilinear, order, _ = single.HIERARCHIES["stiffness"]
    mg = tf().GeometricMultigrid(mesh(), 2, bilinear, quadrature_order=order, dtype=torch.float32)
    model = single._model("stiffness", 2)
    R = np.random.default_rng(42).standard_normal((model.K[-1].shape[0], 2)).astype(np.float32)
    Z = mg.vcycle_multi(torch.tensor(R))
    assert Z.dtype == torch.float32
    _check_columns(Z, R, model, 5e-3, "float32, k = 2")


# --------------------------------------------------------------------------------- the solve
_CASES = {}


def _warm_pcg(model, b, x0, rtol):
    """(x, iterations) of the model's PCG started from x0: it solves for the correction d of
    K d = b - K x0 from d = 0 with the tolerance rescaled by |m b| / |m (b - K x0)|, which is the
    recurrence of a start from x0 measured against |m b|."""
    m = model.mask[-1]
    r0 = m * (b - model.K[-1] @ x0)
    if np.linalg.norm(r0) <= rtol * np.linalg.norm(m * b):
        return x0.copy(), 0
    d, it, _ = model.pcg(r0, rtol=rtol * np.linalg.norm(m * b) / np.linalg.norm(r0))
    return x0 + d, it


def _case(name):
    """(B, X0, model solutions, model counts) of the five columns, built once per hierarchy."""
    if name not in _CASES:
        model = single._model(name, 2)
        n = model.K[-1].shape[0]
        b2, b3, b4 = (mgref.masked_rhs(model, seed) for seed in (2, 3, 4))
        free = np.flatnonzero(model.mask[-1])
        direct = np.zeros(n)
        direct[free] = np.linalg.solve(model.K[-1][free][:, free].toarray(), b2[free])
        rough = model.pcg(b3, rtol=1e-5)[0]
        B = np.stack([b2, np.zeros(n), b3, b4, b2], axis=1)
        X0 = np.stack([np.zeros(n), np.zeros(n), rough, np.zeros(n), direct], axis=1)
        xs, counts = [], []
        for j in range(5):
            x, it = _warm_pcg(model, B[:, j], X0[:, j], 1e-10)
            xs.append(x)
            counts.append(it)
        _CASES[name] = (B, X0, np.stack(xs, axis=1), counts)
    return _CASES[name]


@pytest.mark.parametrize("name", ["stiffness", "delaunay"])
def test_solve_multi(name):
    """Five columns that freeze at three different times (the model: 12 / 0 / 6 / 12 / 0 iterations
    on the structured hierarchy, 23 / 0 / 12 / 23 / 0 on the Delaunay one): residuals <= rtol,
    iterations within 2 of the model's, the columns that start converged untouched, X within 1e-9 of
    |x|_inf of the model's solution, exactly 0 on the held DoFs; maxiter = 3 stops the running
    columns at 3."""
    mg, model = single._solver(name, 2), single._model(name, 2)
    B, X0, x_model, counts = _case(name)
    print(f"{name}: the model's iterations {counts}")
    assert counts[1] == 0 and counts[4] == 0 and len(set(counts)) == 3, counts
    X, its, res = mg.solve_multi(torch.tensor(B), X0=torch.tensor(X0), rtol=1e-10)
    print(f"{name}: iterations {its.tolist()}, residuals {[f'{r:.1e}' for r in res.tolist()]}")
    assert tuple(X.shape) == B.shape and X.dtype == torch.float64
    assert its.dtype == torch.int64 and its.device.type == "cpu" and tuple(its.shape) == (5,)
    assert res.device.type == "cpu" and tuple(res.shape) == (5,)
    assert (res <= 1e-10).all()
    Xh = X.cpu().numpy()
    for j in range(5):
        assert abs(int(its[j]) - counts[j]) <= 2, (j, int(its[j]), counts[j])
        err = np.abs(Xh[:, j] - x_model[:, j]).max()
        print(f"  column {j}: |x - model|_inf = {err:.3e}, |x|_inf = {np.abs(x_model[:, j]).max():.3e}")
        assert err <= 1e-9 * np.abs(x_model[:, j]).max()
    assert int(its[1]) == 0 and int(its[4]) == 0
    assert _same_bits(Xh[:, 1], X0[:, 1]) and _same_bits(Xh[:, 4], X0[:, 4])
    assert (Xh[model.mask[-1] == 0] == 0).all()
    # the same from a zero start without X0, on the columns that have one
    X_zero, its_zero, res_zero = mg.solve_multi(torch.tensor(B[:, [0, 1, 3]]), rtol=1e-10)
    assert (res_zero <= 1e-10).all() and int(its_zero[1]) == 0
    assert abs(int(its_zero[0]) - counts[0]) <= 2 and abs(int(its_zero[2]) - counts[3]) <= 2
    assert np.abs(X_zero.cpu().numpy() - x_model[:, [0, 1, 3]]).max() <= 1e-9 * np.abs(x_model).max()
    # maxiter: the running columns stop at 3 above rtol, the others took no iteration
    X3, its3, res3 = mg.solve_multi(torch.tensor(B), X0=torch.tensor(X0), rtol=1e-10, maxiter=3)
    assert its3.tolist() == [3, 0, 3, 3, 0]
    assert (res3[[0, 2, 3]] > 1e-10).all() and (res3[[1, 4]] <= 1e-10).all()
    assert torch.isfinite(X3).all()


def _check_fallback(mg, what):
    model = single._model("stiffness", 2)
    n = model.K[-1].shape[0]
    R = np.random.default_rng(43).standard_normal((n, 2))
    _check_columns(mg.vcycle_multi(torch.tensor(R)), R, model, 1e-10, what)
    B = np.stack([mgref.masked_rhs(model, 2), mgref.masked_rhs(model, 3)], axis=1)
    X, its, res = mg.solve_multi(torch.tensor(B))
    assert (res <= 1e-10).all()
    for j in range(2):
        x_model, it_model, _ = model.pcg(B[:, j])
        assert abs(int(its[j]) - it_model) <= 2
        assert np.abs(X[:, j].cpu().numpy() - x_model).max() <= 1e-9 * np.abs(x_model).max()


def test_renumbered_levels_go_through_matvec_on_blocks(monkeypatch):
    """TFEM_RENUMBER=1: every engine renumbers, the block cycle applies the operators through the
    public matvec on the block, in the caller's numbering."""
    monkeypatch.setenv("TFEM_RENUMBER", "1")
    mesh, bilinear, order, _ = single.HIERARCHIES["stiffness"]
    mg = tf().GeometricMultigrid(mesh(), 2, bilinear, quadrature_order=order)
    assert all(lv.engine.renumbered for lv in mg.levels)
    _check_fallback(mg, "renumbered levels, k = 2")


def test_csr_levels_on_blocks(monkeypatch):
    """TFEM_KERNEL=tiles: no level has a ring plan, the operators wrap their CSR and the block cycle
    applies them with tfem_csr_spmm (CSRMatrix._prepared_spmv)."""
    monkeypatch.setenv("TFEM_KERNEL", "tiles")
    mesh, bilinear, order, _ = single.HIERARCHIES["stiffness"]
    mg = tf().GeometricMultigrid(mesh(), 2, bilinear, quadrature_order=order)
    assert not any(lv.op.matrix_free for lv in mg.levels)
    assert not any(lv.engine.renumbered for lv in mg.levels)
    _check_fallback(mg, "CSR levels, k = 2")


def test_refusals_of_the_block_methods():
    from pytorch_fem_solver_amd import meshgen

    mg = tf().GeometricMultigrid(meshgen.unit_square(4, 0.25, 1), 1, single.stiffness)
    n = mg.operator.shape[0]
    with pytest.raises(ValueError, match="shape"):
        mg.solve_multi(torch.ones(n))
    with pytest.raises(ValueError, match="shape"):
        mg.solve_multi(torch.ones(n + 1, 2))
    with pytest.raises(ValueError, match="shape"):
        mg.solve_multi(torch.ones(n, 2), X0=torch.ones(n, 3))
    with pytest.raises(ValueError, match="shape"):
        mg.vcycle_multi(torch.ones(n + 1, 2))
    with pytest.raises(TypeError):
        mg.solve_multi(torch.ones(n, 2), free=torch.arange(n))
    with pytest.raises(NotImplementedError, match="blocks"):
        mg.solve(torch.ones(n, 2))
    with pytest.raises(NotImplementedError, match="blocks"):
        mg.vcycle(torch.ones(n, 3))
