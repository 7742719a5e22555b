"""P2 multigrid on a real MI355X: the two tfem_mg_p2_* kernels (csrc/tfem_mg.hip) against numpy
in extended precision, the V-cycle of P2Multigrid against the CPU model of
tests/p2_multigrid_reference.py on every route of the P2 operator (matrix-free in the caller's
numbering, matrix-free in the engine's edge numbering, assembled CSR), and the
multigrid-preconditioned CG against a dense solve, the model's iteration counts and the
Jacobi-preconditioned CG of the operator."""

import numpy as np
import pytest
import torch

import p2_multigrid_reference as p2ref

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
    """(n_v, n_f, edge_vertices (n_e, 2) int32, ptr, idx), built once.  "square3": the 16 vertices and
    33 edges of unit_square(3, 0.25, 1), neither a multiple of a wave.  "star": a hub with 19 edges
    (its row takes one, two and three entries per lane), a rim of four edges, one vertex without any
    edge (the last) and one edge stored with its endpoints in descending order."""
    if name not in _TABLES:
        from pytorch_fem_solver_amd import meshgen
        from pytorch_fem_solver_amd.multigrid import transpose_edges

        if name == "square3":
            mesh = meshgen.unit_square(3, 0.25, 1)
            n_v, edges = mesh["vertices"].shape[0], np.asarray(mesh["edges"]).astype(np.int32)
            assert (n_v, edges.shape[0]) == (16, 33)
        else:
            n_v = 21  # hub 0, spokes 1 .. 19, vertex 20 alone
            spokes = [(0, v) for v in range(1, 20)]
            spokes[4] = (5, 0)  # descending
            edges = np.array(spokes + [(1, 2), (2, 3), (7, 6), (18, 19)], dtype=np.int32)
        ptr, idx = transpose_edges(edges, n_v)
        if name == "star":
            assert ptr[1] - ptr[0] == 19 and ptr[21] == ptr[20]
        _TABLES[name] = (n_v, n_v + edges.shape[0], edges, ptr, idx)
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


def _close(got, want, scale, length, np_dtype, what):
    """|err| <= (row length + 3) eps sum |terms| per entry, `length` the entries of the row of P^T
    (restrict) or of P (prolong): the worst case of a floating-point sum, every rounding at most
    eps / 2 of a partial sum that sum |terms| bounds -- one per term (the difference b - ax; the
    halving and the product with a 0 / 1 mask are exact), one per addition of the row, and the
    additions of d(v) or of x_f."""
    err = np.abs(got.astype(LD) - want)
    tol = (length + 3) * np.finfo(np_dtype).eps * scale
    worst = float((err / np.maximum(tol, np.finfo(np.float64).tiny)).max())
    print(f"{what}: max |err| / tol = {worst:.3e}")
    assert (err <= tol).all(), f"{what}: max |err| / tol = {worst:.3e}"


DTYPES = [(torch.float64, np.float64), (torch.float32, np.float32)]


def _restrict_reference(n_v, n_f, ptr, idx, m_c, m_f, b, a):
    weight = np.ones(n_f, dtype=LD) if m_f is None else m_f.astype(LD)
    d = weight * (b.astype(LD) - a.astype(LD))
    size = weight * (np.abs(b.astype(LD)) + np.abs(a.astype(LD)))
    rows = np.repeat(np.arange(n_v), np.diff(ptr))
    want, scale = d[:n_v].copy(), size[:n_v].copy()
    np.add.at(want, rows, 0.5 * d[idx])
    np.add.at(scale, rows, 0.5 * size[idx])
    if m_c is not None:
        want, scale = m_c * want, m_c * scale
    return want, scale, np.diff(ptr)


@pytest.mark.parametrize("tables", ["square3", "star"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_restrict_kernel(tables, masked, dtype, np_dtype):
    """r_c[v] = m_c[v] (d(v) + 0.5 sum d(idx)), d = m_f (b - ax); NULL masks are all ones; a second
    launch gives the same bits."""
    n_v, n_f, _, ptr, idx = _tables(tables)
    rng = np.random.default_rng(41)
    b, a = _random(rng, n_f, np_dtype), _random(rng, n_f, np_dtype)
    m_c = _random(rng, n_v, np_dtype, mask=True) if masked else None
    m_f = _random(rng, n_f, np_dtype, mask=True) if masked else None
    dev = lambda v: None if v is None else torch.tensor(v)  # noqa: E731
    args = (dev(ptr), dev(idx), dev(m_c), dev(m_f), dev(b), dev(a))
    runs = []
    for _ in range(2):
        out = torch.full((n_v,), float("nan"), dtype=dtype)
        _call("tfem_mg_p2_restrict_residual", *args, out, out.element_size(), n_v, n_f)
        runs.append(out.cpu().numpy())
    assert (runs[0] == runs[1]).all(), "two runs differ"
    want, scale, length = _restrict_reference(n_v, n_f, ptr, idx, m_c, m_f, b, a)
    if m_c is not None:
        assert (runs[0][m_c == 0] == 0).all()
    if tables == "star":  # the vertex without edges: its own masked residual, to the bit
        own = (b[20] - a[20]) * (1 if m_f is None else m_f[20]) * (1 if m_c is None else m_c[20])
        assert runs[0][20] == np_dtype(own)
    _close(runs[0], want, scale, length, np_dtype, f"P2 restrict {tables} masked={masked}")


@pytest.mark.parametrize("tables", ["square3", "star"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_prolong_kernel(tables, masked, dtype, np_dtype):
    """x_f[i] += m_f[i] e_c[i] on the vertices, m_f[i] 0.5 (e_c[a] + e_c[b]) on the edges."""
    n_v, n_f, edges, _, _ = _tables(tables)
    rng = np.random.default_rng(42)
    e, x = _random(rng, n_v, np_dtype), _random(rng, n_f, np_dtype)
    m_f = _random(rng, n_f, np_dtype, mask=True) if masked else None
    ev, ed = torch.tensor(edges), torch.tensor(e)
    md = None if m_f is None else torch.tensor(m_f)
    runs = []
    for _ in range(2):
        xd = torch.tensor(x)
        _call("tfem_mg_p2_prolong_add", ev, md, ed, xd, xd.element_size(), n_v, n_f)
        runs.append(xd.cpu().numpy())
    assert (runs[0] == runs[1]).all(), "two runs differ"
    weight = np.ones(n_f, dtype=LD) if m_f is None else m_f.astype(LD)
    el = e.astype(LD)
    add = np.concatenate([el, 0.5 * (el[edges[:, 0]] + el[edges[:, 1]])])
    size = np.concatenate([np.abs(el), 0.5 * (np.abs(el)[edges[:, 0]] + np.abs(el)[edges[:, 1]])])
    want = x.astype(LD) + weight * add
    scale = np.abs(x.astype(LD)) + weight * size
    length = np.concatenate([np.full(n_v, 1), np.full(n_f - n_v, 2)])
    if m_f is not None:
        assert (runs[0][m_f == 0] == x[m_f == 0]).all()
    _close(runs[0], want, scale, length, np_dtype, f"P2 prolong {tables} masked={masked}")


@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_entries_outside_the_arrays_read_zero_and_write_nothing(dtype, np_dtype):
    """An idx entry >= n_f and an endpoint >= n_v count as 0 -- just behind the array, where memory
    holds other numbers, and at 2^32 / real_bytes + 3, where the 32-bit byte offset wraps into the
    array again; the outputs end where they are said to end (canaries behind r_c and x_f)."""
    n_v, n_f, edges, ptr, idx = _tables("star")
    wrap = (1 << 32) // np.dtype(np_dtype).itemsize + 3
    rng = np.random.default_rng(43)
    pad = 64
    b, a = _random(rng, n_f + pad, np_dtype), _random(rng, n_f + pad, np_dtype)  # numbers behind the arrays
    bad_idx = idx.copy()
    bad_idx[[2, 9, 17]] = [n_f, n_f + 5, wrap]  # three entries of the hub's row
    clean = np.concatenate([b[:n_f], [0]]).astype(np_dtype), np.concatenate([a[:n_f], [0]]).astype(np_dtype)
    zero_idx = bad_idx.copy()
    zero_idx[[2, 9, 17]] = n_f  # -> the appended zero of `clean`
    want, scale, length = _restrict_reference(n_v, n_f + 1, ptr, zero_idx, None, None, *clean)
    out = torch.full((n_v + pad,), 7.0, dtype=dtype)
    _call("tfem_mg_p2_restrict_residual", torch.tensor(ptr), torch.tensor(bad_idx), None, None, torch.tensor(b)[:n_f],
          torch.tensor(a)[:n_f], out[:n_v], out.element_size(), n_v, n_f)
    got = out.cpu().numpy()
    assert (got[n_v:] == 7.0).all(), "the kernel wrote behind r_c"
    _close(got[:n_v], want, scale, length, np_dtype, "P2 restrict with entries outside")

    e = _random(rng, n_v + pad, np_dtype)
    bad_edges = edges.copy()
    bad_edges[3] = (n_v, 4)       # one endpoint just behind e_c
    bad_edges[8] = (n_v + 7, wrap)  # both outside
    x = _random(rng, n_f + pad, np_dtype)
    xd = torch.tensor(x)
    _call("tfem_mg_p2_prolong_add", torch.tensor(bad_edges), None, torch.tensor(e)[:n_v], xd[:n_f], xd.element_size(),
          n_v, n_f)
    got = xd.cpu().numpy()
    assert (got[n_f:] == x[n_f:]).all(), "the kernel wrote behind x_f"
    el = np.concatenate([e[:n_v], np.zeros(1, dtype=np_dtype)]).astype(LD)
    ends = np.where(bad_edges.astype(np.int64) >= n_v, n_v, bad_edges.astype(np.int64))
    add = np.concatenate([el[:n_v], 0.5 * (el[ends[:, 0]] + el[ends[:, 1]])])
    size = np.concatenate([np.abs(el[:n_v]), 0.5 * (np.abs(el)[ends[:, 0]] + np.abs(el)[ends[:, 1]])])
    assert got[n_v + 8] == x[n_v + 8], "an edge with both endpoints outside adds 0"
    _close(got[:n_f], x[:n_f].astype(LD) + add, np.abs(x[:n_f].astype(LD)) + size,
           np.concatenate([np.full(n_v, 1), np.full(n_f - n_v, 2)]), np_dtype, "P2 prolong with endpoints outside")


# --------------------------------------------------------------------------------- the cycle
_MODELS, _SOLVERS = {}, {}

HIERARCHIES = {
    # name: (coarse mesh, bilinear form, model keywords)
    "stiffness": (lambda: _square8(), stiffness, {}),
    "no_mask": (lambda: _square8(), stiffness_mass, {"beta": 1.0, "dirichlet": False}),
    "delaunay": (lambda: _delaunay80(), stiffness, {}),
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
        mesh, _, kw = HIERARCHIES[name]
        _MODELS[name, levels] = p2ref.P2Model(mesh(), levels, order=3, **kw)
    return _MODELS[name, levels]


def _solver(name, levels):
    if (name, levels) not in _SOLVERS:
        mesh, bilinear, kw = HIERARCHIES[name]
        _SOLVERS[name, levels] = tf().P2Multigrid(mesh(), levels, bilinear, dirichlet=kw.get("dirichlet", True))
    return _SOLVERS[name, levels]


def _check_cycle(mg, model, what):
    """The bounds of test_hip_multigrid._check_cycle: about 20 applications at the P2 operator's
    1e-12 parity."""
    n = model.n
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
    assert (z1[model.mask2 == 0] == 0).all()
    # the same cycle again: the same bits (no atomics, nothing left over in the buffers)
    assert (mg.vcycle(torch.tensor(r1)).cpu().numpy() == z1).all()
    # a column vector comes back as a column vector
    assert mg.vcycle(torch.tensor(r1).reshape(-1, 1)).shape == (n, 1)


def _check_solve(mg, model, what, against_model=False):
    """(x, iterations, b): residual <= 1e-10, the iterations within 2 of the model's and, where asked,
    the solution within 1e-9 of the model's."""
    b_np = p2ref.masked_rhs(model)
    x_model, it_model, _ = model.pcg(b_np)
    b = torch.tensor(b_np)
    x, it, res = mg.solve(b, rtol=1e-10)
    err = np.abs(x.cpu().numpy() - x_model).max() / np.abs(x_model).max()
    print(f"{what}: {it} iterations (model {it_model}), residual {res:.2e}, against the model's solution {err:.3e}")
    assert res <= 1e-10 and x.shape == b.shape
    assert abs(it - it_model) <= 2
    assert not against_model or err <= 1e-9
    return x, it, b


@pytest.mark.parametrize("name,levels", [("stiffness", 0), ("stiffness", 1), ("stiffness", 2), ("no_mask", 1)])
def test_vcycle_matches_the_model(name, levels):
    mg, model = _solver(name, levels), _model(name, levels)
    assert len(mg.levels) == levels + 2 and mg.levels[:-1] == mg.p1.levels
    assert [lv.n for lv in mg.levels] == [K.shape[0] for K in model.K]
    assert mg.basis is mg.levels[-1].basis and mg.operator is mg.levels[-1].op
    assert mg.operator.matrix_free and not mg.basis._engine.renumbered
    assert mg.dtype == torch.float64 and mg.device.type == "cuda"
    _check_cycle(mg, model, f"{name}, {levels} refinements")


def test_edge_renumbering_runs_the_rows_launch_in_the_engine_numbering(monkeypatch):
    """TFEM_RENUMBER=1: the P2 engine renumbers its edge DoFs (as it does on its own from 50,000 DoFs
    on), the P2 level keeps the matrix-free launch and works in the engine's numbering."""
    monkeypatch.setenv("TFEM_RENUMBER", "1")
    mesh, bilinear, _ = HIERARCHIES["stiffness"]
    mg = tf().P2Multigrid(mesh(), 1, bilinear)
    engine, top = mg.basis._engine, mg.levels[-1]
    assert engine.renumbered and mg.operator.matrix_free and top.crossing
    perm = engine._perm.cpu().numpy()
    assert (perm[:top.n_v] == np.arange(top.n_v)).all() and (perm != np.arange(top.n)).any()
    calls = []
    rows_into = mg.operator._rows_into
    monkeypatch.setattr(mg.operator, "_rows_into", lambda: calls.append("rows") or rows_into())
    monkeypatch.setattr(mg.operator, "matvec", lambda *a, **k: pytest.fail("the P2 level fell back to matvec"))
    model = _model("stiffness", 1)
    _check_cycle(mg, model, "edge renumbering, 1 refinement")
    assert calls == ["rows"]
    _check_solve(mg, model, "edge renumbering, 1 refinement", against_model=True)


def test_csr_route(monkeypatch):
    """TFEM_KERNEL=gather: no P2 row plan, the P2 level applies the assembled CSR."""
    monkeypatch.setenv("TFEM_KERNEL", "gather")
    mesh, bilinear, _ = HIERARCHIES["stiffness"]
    mg = tf().P2Multigrid(mesh(), 1, bilinear)
    assert not mg.operator.matrix_free and not mg.levels[-1].crossing
    model = _model("stiffness", 1)
    _check_cycle(mg, model, "CSR route, 1 refinement")
    _check_solve(mg, model, "CSR route, 1 refinement", against_model=True)


def test_vcycle_in_float32():
    """dtype=float32: the cycle of the float32 kernels against the float64 model.  About 20 operator
    applications per cycle at the float32 parity of the P2 operator (TOL32_APPLY = 8 x 1.375e-5 of
    tests/test_hip_p2_operator_fuzz.py) with a margin of 5, the derivation of
    test_hip_multigrid.test_vcycle_in_float32: 100 x TOL32_APPLY = 1.1e-2."""
    mesh, bilinear, _ = HIERARCHIES["stiffness"]
    mg = tf().P2Multigrid(mesh(), 1, bilinear, dtype=torch.float32)
    model = _model("stiffness", 1)
    assert mg.dtype == torch.float32 and mg.p1.dtype == torch.float32 and torch.get_default_dtype() == torch.float64
    r = np.random.default_rng(22).standard_normal(model.n).astype(np.float32)
    z = mg.vcycle(torch.tensor(r))
    assert z.dtype == torch.float32
    want = model.vcycle(r.astype(np.float64))
    err = np.abs(z.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"float32 cycle against the model: {err:.3e}")
    assert err <= 100 * 8 * 1.375e-05


# --------------------------------------------------------------------------------- the solve
@pytest.mark.parametrize("name,all_levels", [("stiffness", (1, 2, 3)), ("delaunay", (1, 2))])
def test_solve(name, all_levels):
    """The iteration count within 2 of the model's on the same right-hand side; at 2 refinements the
    solution against the dense solve and a start from the solution; at the largest hierarchy a
    quarter of the iterations of the Jacobi-preconditioned CG at most (the model: 16 against 679,
    35 against 385)."""
    for levels in all_levels:
        mg, model = _solver(name, levels), _model(name, levels)
        x, it, b = _check_solve(mg, model, f"{name}, {levels} refinements, {model.n} DoFs")
        free = mg.basis._basis_parameters["inner_dofs"].long()
        if levels == 2:
            K = mg.operator.to_csr().to_dense()
            direct = torch.zeros_like(b)
            direct[free] = torch.linalg.solve(K[free][:, free], b[free])
            err = float((x - direct).abs().max() / direct.abs().max())
            print(f"  against the dense solve: {err:.3e}")
            assert err <= 1e-9
            assert float(x[torch.tensor(model.mask2 == 0)].abs().max()) == 0
            # a column vector, and a start from the solution: no iteration
            x2, it2, _ = mg.solve(b.reshape(-1, 1), x0=x.reshape(-1, 1), rtol=1e-9)
            assert x2.shape == (b.shape[0], 1) and it2 == 0
        if levels == all_levels[-1]:
            _, it_jacobi, res_jacobi = mg.operator.solve_cg(b, free=free, rtol=1e-10)
            print(f"  Jacobi-preconditioned CG: {it_jacobi} iterations")
            assert res_jacobi <= 1e-10
            assert 4 * it <= it_jacobi


def test_refusals():
    from pytorch_fem_solver_amd import meshgen

    P2MG = tf().P2Multigrid
    coarse = meshgen.unit_square(4, 0.25, 1)
    n_coarse, n_fine = coarse["triangles"].shape[0], 4 * coarse["triangles"].shape[0]
    for n_elems in (n_coarse, n_fine):
        values = torch.ones(n_elems)
        with pytest.raises(NotImplementedError, match="coefficient data"):
            P2MG(coarse, 1, lambda b: b.coefficient(values) * (b.v_grad @ b.v_grad.mT))
    mg = _solver("stiffness", 0)
    n = mg.operator.shape[0]
    with pytest.raises(NotImplementedError, match="free"):
        mg.solve(torch.ones(n), free=torch.arange(n))
    for call in (mg.solve, mg.vcycle):
        with pytest.raises(NotImplementedError, match="blocks.*vcycle_multi.*solve_multi.*P2"):
            call(torch.ones(n, 2))
    with pytest.raises(ValueError, match="entries"):
        mg.vcycle(torch.ones(n + 1))
    with pytest.raises(ValueError, match="entries"):
        mg.solve(torch.ones(n - 1))
    with pytest.raises(NotImplementedError, match="P2.*P2Multigrid"):
        tf().GeometricMultigrid(coarse, 1, stiffness, element=tf().ElementTri(polynomial_order=2, integration_order=3))
