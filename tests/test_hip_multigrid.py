"""Geometric multigrid on a real MI355X: the three tfem_mg_* kernels (csrc/tfem_mg.hip) against
numpy in extended precision, the V-cycle of GeometricMultigrid against the CPU model of
tests/multigrid_reference.py, and the multigrid-preconditioned CG against a dense solve, the
model's iteration counts and the Jacobi-preconditioned CG of the operator."""

import numpy as np
import pytest
import torch

from conftest import load_golden, mesh_from_golden

import coefficient_reference as cref
import multigrid_reference as mgref

pytestmark = pytest.mark.gpu

LD = np.longdouble


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


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def stiffness_mass(b):
    return b.v_grad @ b.v_grad.mT + b.v @ b.v.mT


# --------------------------------------------------------------------------------- the kernels
_TABLES = {}


def _tables(name):
    """(n_c, n_f, parents, ptr, idx) one level above the named coarse mesh, built once."""
    if name not in _TABLES:
        from pytorch_fem_solver_amd import meshgen
        from pytorch_fem_solver_amd.multigrid import transpose_parents

        coarse = meshgen.unit_square(5, 0.25, 1) if name == "square5" else meshgen.delaunay_square(300, 7)
        fine, parents = meshgen.refine_uniform(coarse)
        n_c, n_f = coarse["vertices"].shape[0], fine["vertices"].shape[0]
        _TABLES[name] = (n_c, n_f, parents, *transpose_parents(parents, n_c))
    return _TABLES[name]


def _call(name, *args):
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    converted = [_native.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
    _native.check(getattr(lib, name)(*converted, _native.current_stream(torch.device("cuda"))))


def _random(rng, n, np_dtype, mask=False):
    if mask:
        return (rng.random(n) < 0.7).astype(np_dtype)
    return rng.standard_normal(n).astype(np_dtype)


def _close(got, want, scale, factor, np_dtype, what):
    err = np.abs(got.astype(LD) - want)
    tol = factor * np.finfo(np_dtype).eps * scale
    worst = float((err / np.maximum(tol, np.finfo(np.float64).tiny)).max())
    print(f"{what}: max |err| / tol = {worst:.3e}")
    assert (err <= tol).all(), f"{what}: max |err| / tol = {worst:.3e}"


DTYPES = [(torch.float64, np.float64), (torch.float32, np.float32)]


@pytest.mark.parametrize("mesh", ["square5", "delaunay300"])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_smooth_kernel(mesh, dtype, np_dtype):
    """x = w b and x += w (b - ax): |err| <= 2 eps (|x| + |w b| + |w ax|) per entry; aligned arrays
    (16 bytes per lane and the tail one by one) and arrays that start off the 16-byte grid."""
    n = _tables(mesh)[1]
    rng = np.random.default_rng(11)
    for offset in (0, 1):
        host = {k: _random(rng, n + offset, np_dtype) for k in "xbaw"}
        dev = {k: torch.tensor(v)[offset:] for k, v in host.items()}
        x, b, a, w = (host[k][offset:].astype(LD) for k in "xbaw")
        assert dev["x"].data_ptr() % 16 == (0 if offset == 0 else dev["x"].element_size())
        for first in (1, 0):
            runs = []
            for _ in range(2):
                xd = torch.tensor(host["x"])[offset:]
                _call("tfem_mg_smooth", xd, dev["b"], None if first else dev["a"], dev["w"], xd.element_size(), n, first)
                runs.append(xd.cpu().numpy())
            assert (runs[0] == runs[1]).all(), "two runs differ"
            want = w * b if first else x + w * (b - a)
            scale = np.abs(w * b) if first else np.abs(x) + np.abs(w * b) + np.abs(w * a)
            _close(runs[0], want, scale, 2, np_dtype, f"smooth first={first} offset={offset}")


@pytest.mark.parametrize("mesh", ["square5", "delaunay300"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_restrict_kernel(mesh, masked, dtype, np_dtype):
    """r_c = m_c P^T (m_f (b - ax)): |err| <= 16 eps sum |terms| per entry (a sum of at most 17
    terms, each a rounded difference, times 0.5)."""
    n_c, n_f, parents, ptr, idx = _tables(mesh)
    if mesh == "delaunay300":
        assert np.diff(ptr).max() > 8, "rows that take more than one entry per lane"
    rng = np.random.default_rng(12)
    b, a = _random(rng, n_f, np_dtype), _random(rng, n_f, np_dtype)
    m_c = _random(rng, n_c, np_dtype, mask=True) if masked else None
    m_f = _random(rng, n_f, np_dtype, mask=True) if masked else None
    dev = lambda v: None if v is None else torch.tensor(v)  # noqa: E731
    args = (dev(ptr), dev(idx), dev(m_c), dev(m_f), dev(b), dev(a))
    runs = []
    for _ in range(2):
        out = torch.full((n_c,), float("nan"), dtype=dtype)
        _call("tfem_mg_restrict_residual", *args, out, out.element_size(), n_c, n_f)
        runs.append(out.cpu().numpy())
    assert (runs[0] == runs[1]).all(), "two runs differ"
    rows = np.repeat(np.arange(n_c), np.diff(ptr))
    weight = np.ones(n_f, dtype=LD) if m_f is None else m_f.astype(LD)
    terms = 0.5 * weight[idx] * (b.astype(LD)[idx] - a.astype(LD)[idx])
    sizes = 0.5 * weight[idx] * (np.abs(b.astype(LD))[idx] + np.abs(a.astype(LD))[idx])
    want, scale = np.zeros(n_c, dtype=LD), np.zeros(n_c, dtype=LD)
    np.add.at(want, rows, terms)
    np.add.at(scale, rows, sizes)
    if m_c is not None:
        want, scale = m_c * want, m_c * scale
        assert (runs[0][m_c == 0] == 0).all()
    _close(runs[0], want, scale, 16, np_dtype, f"restrict {mesh} masked={masked}")


@pytest.mark.parametrize("mesh", ["square5", "delaunay300"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_prolong_kernel(mesh, masked, dtype, np_dtype):
    """x_f += m_f P e_c: |err| <= 2 eps (|x| + 0.5 |e_a| + 0.5 |e_b|) per entry."""
    n_c, n_f, parents, ptr, idx = _tables(mesh)
    rng = np.random.default_rng(13)
    e, x = _random(rng, n_c, np_dtype), _random(rng, n_f, np_dtype)
    m_f = _random(rng, n_f, np_dtype, mask=True) if masked else None
    par, ed = torch.tensor(parents), torch.tensor(e)
    md = None if m_f is None else torch.tensor(m_f)
    runs = []
    for _ in range(2):
        xd = torch.tensor(x)
        _call("tfem_mg_prolong_add", par, md, ed, xd, xd.element_size(), n_f, n_c)
        runs.append(xd.cpu().numpy())
    assert (runs[0] == runs[1]).all(), "two runs differ"
    weight = np.ones(n_f, dtype=LD) if m_f is None else m_f.astype(LD)
    ea, eb = e.astype(LD)[parents[:, 0]], e.astype(LD)[parents[:, 1]]
    want = x.astype(LD) + weight * 0.5 * (ea + eb)
    scale = np.abs(x.astype(LD)) + weight * 0.5 * (np.abs(ea) + np.abs(eb))
    if m_f is not None:
        assert (runs[0][m_f == 0] == x[m_f == 0]).all()
    _close(runs[0], want, scale, 2, np_dtype, f"prolong {mesh} masked={masked}")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_entries_outside_the_arrays_read_zero_and_write_nothing(masked, dtype, np_dtype):
    """An idx entry >= n_f and a parent >= n_c count as 0 -- just behind the array, where memory
    holds other numbers, and at 2^32 / real_bytes + 3, where a 32-bit byte offset would wrap into
    the array again; the outputs end where they are said to end (canaries behind r_c and x_f).  The
    bounds are those of test_restrict_kernel and test_prolong_kernel."""
    n_c, n_f, parents, ptr, idx = _tables("square5")
    wrap = (1 << 32) // np.dtype(np_dtype).itemsize + 3
    assert wrap < 2**31
    rng = np.random.default_rng(14)
    pad = 64
    b, a = _random(rng, n_f + pad, np_dtype), _random(rng, n_f + pad, np_dtype)  # numbers behind the arrays
    m_c = _random(rng, n_c, np_dtype, mask=True) if masked else None
    m_f = np.ones(n_f + pad, dtype=np_dtype)
    m_f[:n_f] = _random(rng, n_f, np_dtype, mask=True)
    m_f[3] = 1  # the entry a wrapped offset would read
    dev = lambda v, n: None if v is None else torch.tensor(v)[:n]  # noqa: E731
    outside = np.array([2, 9, 17, 40])
    bad_idx = idx.copy()
    bad_idx[outside] = [n_f, n_f + 5, wrap, wrap]
    out = torch.full((n_c + pad,), 7.0, dtype=dtype)
    _call("tfem_mg_restrict_residual", torch.tensor(ptr), torch.tensor(bad_idx), dev(m_c, n_c),
          dev(m_f, n_f) if masked else None, dev(b, n_f), dev(a, n_f), out[:n_c], out.element_size(), n_c, n_f)
    got = out.cpu().numpy()
    assert (got[n_c:] == 7.0).all(), "the kernel wrote behind r_c"
    rows = np.repeat(np.arange(n_c), np.diff(ptr))
    weight = m_f[:n_f].astype(LD) if masked else np.ones(n_f, dtype=LD)
    terms = 0.5 * weight[idx] * (b.astype(LD)[idx] - a.astype(LD)[idx])
    sizes = 0.5 * weight[idx] * (np.abs(b.astype(LD))[idx] + np.abs(a.astype(LD))[idx])
    assert (np.abs(b[3] - a[3]) > 0) and (sizes[outside] > 0).any()
    terms[outside], sizes[outside] = 0, 0
    want, scale = np.zeros(n_c, dtype=LD), np.zeros(n_c, dtype=LD)
    np.add.at(want, rows, terms)
    np.add.at(scale, rows, sizes)
    if masked:
        want, scale = m_c * want, m_c * scale
    _close(got[:n_c], want, scale, 16, np_dtype, f"restrict with entries outside masked={masked}")

    e = _random(rng, n_c + pad, np_dtype)
    bad_parents = parents.copy()
    bad_parents[30] = (n_c, parents[30, 1])  # one parent just behind e_c
    bad_parents[41] = (n_c + 7, wrap)  # both outside
    bad_parents[52] = (parents[52, 0], wrap)
    x = _random(rng, n_f + pad, np_dtype)
    xd = torch.tensor(x)
    _call("tfem_mg_prolong_add", torch.tensor(bad_parents), dev(m_f, n_f) if masked else None, dev(e, n_c), xd[:n_f],
          xd.element_size(), n_f, n_c)
    got = xd.cpu().numpy()
    assert (got[n_f:] == x[n_f:]).all(), "the kernel wrote behind x_f"
    assert got[41] == x[41], "a vertex with both parents outside adds 0"
    el = np.concatenate([e[:n_c], np.zeros(1, dtype=np_dtype)]).astype(LD)
    ends = np.where(bad_parents.astype(np.int64) >= n_c, n_c, bad_parents.astype(np.int64))
    ea, eb = el[ends[:, 0]], el[ends[:, 1]]
    want = x[:n_f].astype(LD) + weight * 0.5 * (ea + eb)
    scale = np.abs(x[:n_f].astype(LD)) + weight * 0.5 * (np.abs(ea) + np.abs(eb))
    _close(got[:n_f], want, scale, 2, np_dtype, f"prolong with parents outside masked={masked}")


# --------------------------------------------------------------------------------- the cycle
_MODELS, _SOLVERS = {}, {}

HIERARCHIES = {
    # name: (coarse mesh, bilinear form, quadrature order, model keywords)
    "stiffness": (lambda: _square8(), stiffness, 2, {}),
    "no_mask": (lambda: _square8(), stiffness_mass, 2, {"beta": 1.0, "dirichlet": False}),
    "coefficients": (lambda: _square8(), cref.form(1.0, 0.5, cref.kappa_trig, cref.c_exp), 3,
                     {"beta": 0.5, "kappa": cref.kappa_trig, "c": cref.c_exp}),
    "delaunay": (lambda: _delaunay80(), stiffness, 2, {}),
    "clockwise": (lambda: mesh_from_golden(load_golden("p1_square_n5_clockwise.npz")), stiffness, 2, {}),
}


def _square8():
    from pytorch_fem_solver_amd import meshgen

    return meshgen.unit_square(8, 0.25, 3)


def _delaunay80():
    from pytorch_fem_solver_amd import meshgen

    return meshgen.delaunay_square(80, 7)


def _model(name, levels):
    """The CPU model of a hierarchy, built once and shared (nothing modifies it)."""
    if (name, levels) not in _MODELS:
        mesh, _, order, kw = HIERARCHIES[name]
        _MODELS[name, levels] = mgref.Model(mesh(), levels, order=order, **kw)
    return _MODELS[name, levels]


def _solver(name, levels):
    if (name, levels) not in _SOLVERS:
        mesh, bilinear, order, kw = HIERARCHIES[name]
        _SOLVERS[name, levels] = tf().GeometricMultigrid(mesh(), levels, bilinear, quadrature_order=order,
                                                         dirichlet=kw.get("dirichlet", True))
    return _SOLVERS[name, levels]


def _check_cycle(mg, model, what):
    n = model.K[-1].shape[0]
    rng = np.random.default_rng(21)
    r1, r2 = rng.standard_normal(n), rng.standard_normal(n)
    z1 = mg.vcycle(torch.tensor(r1))
    z2 = mg.vcycle(torch.tensor(r2)).cpu().numpy()
    assert z1.shape == (n,) and z1.dtype == torch.float64
    z1 = z1.cpu().numpy()
    want = model.vcycle(r1)
    err = np.abs(z1 - want).max() / np.abs(want).max()
    asym = abs(z1 @ r2 - r1 @ z2) / (np.linalg.norm(z1) * np.linalg.norm(r2))
    print(f"{what}: cycle against the model {err:.3e}, asymmetry {asym:.3e}")
    assert err <= 1e-10
    assert asym <= 1e-10
    assert (z1[model.mask[-1] == 0] == 0).all()
    # the same cycle again: the same bits (no atomics, nothing left over in the buffers)
    assert (mg.vcycle(torch.tensor(r1)).cpu().numpy() == z1).all()
    # a column vector comes back as a column vector
    assert mg.vcycle(torch.tensor(r1).reshape(-1, 1)).shape == (n, 1)


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("name", ["stiffness", "no_mask"])
def test_vcycle_matches_the_model_on_the_structured_hierarchy(name, levels):
    mg, model = _solver(name, levels), _model(name, levels)
    assert len(mg.levels) == levels + 1 and len(mg.parents) == levels
    assert [lv.n for lv in mg.levels] == [K.shape[0] for K in model.K]
    assert mg.basis is mg.levels[-1].basis and mg.operator is mg.levels[-1].op
    for lv, parents in zip(mg.levels[1:], model.parents):
        assert lv.op.matrix_free and not lv.engine.renumbered
        assert (lv.parents.cpu().numpy() == parents).all()
    assert mg.levels[0].op.matrix_free and not mg.levels[0].engine.renumbered
    _check_cycle(mg, model, f"{name}, {levels} levels")


def test_vcycle_on_the_clockwise_golden_mesh():
    """Triangles stored clockwise enter the forms with a negative determinant: K is not positive
    definite there, the coarse solve is the LU, and the cycle is still the model's."""
    _check_cycle(_solver("clockwise", 2), _model("clockwise", 2), "clockwise golden mesh, 2 levels")


def test_vcycle_in_float32():
    """dtype=float32: the cycle of the float32 kernels against the float64 model.  About 20 operator
    applications per cycle at the float32 operator parity of 5e-5 (tests/coefficient_reference.py),
    with the margin of the float64 bound (1e-10 for 20 x 1e-12): 5e-3."""
    mesh, bilinear, order, _ = HIERARCHIES["stiffness"]
    mg = tf().GeometricMultigrid(mesh(), 2, bilinear, quadrature_order=order, dtype=torch.float32)
    model = _model("stiffness", 2)
    assert mg.dtype == torch.float32 and torch.get_default_dtype() == torch.float64
    r = np.random.default_rng(22).standard_normal(model.K[-1].shape[0]).astype(np.float32)
    z = mg.vcycle(torch.tensor(r))
    assert z.dtype == torch.float32
    want = model.vcycle(r.astype(np.float64))
    err = np.abs(z.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"float32 cycle against the model: {err:.3e}")
    assert err <= 5e-3


# --------------------------------------------------------------------------------- the solve
@pytest.mark.parametrize("name", ["stiffness", "coefficients", "delaunay"])
def test_solve(name):
    """Levels 1 to 3: the iteration count within 2 of the model's on the same right-hand side; at
    level 2 the solution against the dense solve; at level 3 a quarter of the iterations of the
    Jacobi-preconditioned CG at most; on the structured hierarchy at most 2 more per level."""
    counts = []
    for levels in (1, 2, 3):
        mg, model = _solver(name, levels), _model(name, levels)
        b_np = mgref.masked_rhs(model)
        x_model, it_model, _ = model.pcg(b_np)
        b = torch.tensor(b_np)
        x, it, res = mg.solve(b, rtol=1e-10)
        print(f"{name}, {levels} levels, {model.K[-1].shape[0]} DoFs: {it} iterations (model {it_model}), residual {res:.2e}")
        assert res <= 1e-10 and x.shape == b.shape
        assert abs(it - it_model) <= 2
        counts.append(it)
        free = mg.basis._basis_parameters["inner_dofs"].long()
        if levels == 2:
            K = mg.operator.to_csr().to_dense()
            direct = torch.zeros_like(b)
            direct[free] = torch.linalg.solve(K[free][:, free], b[free])
            err = float((x - direct).abs().max() / direct.abs().max())
            print(f"  against the dense solve: {err:.3e}")
            assert err <= 1e-9
            assert float(x[torch.tensor(model.mask[-1] == 0)].abs().max()) == 0
            # a column vector, and a start from the solution: no iteration
            x2, it2, _ = mg.solve(b.reshape(-1, 1), x0=x.reshape(-1, 1), rtol=1e-9)
            assert x2.shape == (b.shape[0], 1) and it2 == 0
        if levels == 3:
            _, it_jacobi, res_jacobi = mg.operator.solve_cg(b, free=free, rtol=1e-10)
            print(f"  Jacobi-preconditioned CG: {it_jacobi} iterations")
            assert res_jacobi <= 1e-10
            assert 4 * it <= it_jacobi
    if name != "delaunay":
        assert counts[1] <= counts[0] + 2 and counts[2] <= counts[1] + 2


def test_renumbered_levels_go_through_matvec(monkeypatch):
    """TFEM_RENUMBER=1: every engine renumbers its mesh, the cycle applies the operators through
    the public matvec in the caller's numbering.  Correctness only."""
    monkeypatch.setenv("TFEM_RENUMBER", "1")
    mesh, bilinear, order, _ = HIERARCHIES["stiffness"]
    mg = tf().GeometricMultigrid(mesh(), 2, bilinear, quadrature_order=order)
    assert all(lv.engine.renumbered for lv in mg.levels)
    model = _model("stiffness", 2)
    r = np.random.default_rng(23).standard_normal(model.K[-1].shape[0])
    want = model.vcycle(r)
    z = mg.vcycle(torch.tensor(r)).cpu().numpy()
    assert np.abs(z - want).max() <= 1e-10 * np.abs(want).max()
    b_np = mgref.masked_rhs(model)
    x, it, res = mg.solve(torch.tensor(b_np))
    x_model, _, _ = model.pcg(b_np)
    assert res <= 1e-10
    assert np.abs(x.cpu().numpy() - x_model).max() <= 1e-9 * np.abs(x_model).max()


def test_refusals(monkeypatch):
    from pytorch_fem_solver_amd import meshgen

    GMG = tf().GeometricMultigrid
    coarse = meshgen.unit_square(4, 0.25, 1)
    with pytest.raises(NotImplementedError, match="P2"):
        GMG(coarse, 1, stiffness, element=tf().ElementTri(polynomial_order=2, integration_order=3))
    d = load_golden("fracture_L4.npz")
    tri = mesh_from_golden(d)
    fractures = tf().FracturesTri(triangulations=[tri, tri], fractures_3d_data=torch.tensor(d["in_fractures_3d"]))
    with pytest.raises(NotImplementedError, match="fracture"):
        GMG(fractures, 1, stiffness)
    with pytest.raises(NotImplementedError, match="fracture"):
        GMG(tf().FractureBasis(fractures, tf().ElementTri(polynomial_order=1, integration_order=4)), 1, stiffness)
    # coefficient data: values that fit the coarse mesh, values that fit the fine mesh
    n_coarse, n_fine = coarse["triangles"].shape[0], 4 * coarse["triangles"].shape[0]
    for n_elems in (n_coarse, n_fine):
        values = torch.ones(n_elems)
        with pytest.raises(NotImplementedError, match="coefficient data"):
            GMG(coarse, 1, lambda b: b.coefficient(values) * (b.v_grad @ b.v_grad.mT))
    mg = GMG(coarse, 1, stiffness)
    n = mg.operator.shape[0]
    with pytest.raises(NotImplementedError, match="free"):
        mg.solve(torch.ones(n), free=torch.arange(n))
    with pytest.raises(NotImplementedError, match="blocks"):
        mg.solve(torch.ones(n, 2))
    with pytest.raises(NotImplementedError, match="blocks"):
        mg.vcycle(torch.ones(n, 3))
    with pytest.raises(ValueError, match="entries"):
        mg.vcycle(torch.ones(n + 1))
    # the coarse solve is dense: a coarse mesh beyond Basis.DENSE_SOLVE_LIMIT is refused
    monkeypatch.setattr(tf().Basis, "DENSE_SOLVE_LIMIT", 5)
    with pytest.raises(NotImplementedError, match="coarse"):
        GMG(coarse, 1, stiffness)
