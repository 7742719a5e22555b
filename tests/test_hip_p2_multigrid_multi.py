"""P2 multigrid on blocks of right-hand sides, on a real MI355X: the two tfem_mg_p2_*_multi kernels
(csrc/tfem_mg.hip) bit for bit against the single kernels on every column and against numpy
in extended precision, ``P2Multigrid.vcycle_multi`` against the CPU model of
tests/p2_multigrid_reference.py on every column and on every route of the P2 operator, the sequence
of its launches, and ``solve_multi`` against the model's PCG with columns that freeze at different
times.  Tables, hierarchies, models and solvers are those of tests/test_hip_p2_multigrid.py, the
block helpers those of tests/test_hip_multigrid_multi.py (imported, so the files build them once)."""

import numpy as np
import pytest
import torch

import p2_multigrid_reference as p2ref
import test_hip_multigrid_launches as launches
import test_hip_multigrid_multi as multi
import test_hip_p2_multigrid as p2

pytestmark = pytest.mark.gpu

LD = np.longdouble
DTYPES = p2.DTYPES
WIDTHS = [1, 2, 3, 4, 5, 8, 9]  # forwarded | rows of 24 / 12 and 40 / 20 bytes | a full pass | a second pass
RESTRICT, PROLONG = "tfem_mg_p2_restrict_residual", "tfem_mg_p2_prolong_add"
tf = p2.tf
_same_bits, _framed, _guards_intact, _dev = multi._same_bits, multi._framed, multi._guards_intact, multi._dev


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


# --------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("n_vec", WIDTHS)
@pytest.mark.parametrize("tables", ["square3", "star"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_restrict_multi_kernel(tables, masked, dtype, np_dtype, n_vec):
    """r_c = m_c (d(v) + 0.5 sum d(idx)) on blocks: column j bit for bit the single kernel, two runs
    the same bits, the same bits from blocks one element off the 16-byte grid, guards around the
    output intact, rows with m_c = 0 exactly 0, |err| <= (row length + 3) eps sum |terms|."""
    n_v, n_f, _, ptr, idx = p2._tables(tables)
    rng = np.random.default_rng(51)
    b, a = multi._block(rng, n_f, n_vec, np_dtype), multi._block(rng, n_f, n_vec, np_dtype)
    m_c = p2._random(rng, n_v, np_dtype, mask=True) if masked else None
    m_f = p2._random(rng, n_f, np_dtype, mask=True) if masked else None
    head = (_dev(ptr), _dev(idx), _dev(m_c), _dev(m_f))
    blank = np.zeros((n_v, n_vec), dtype=np_dtype)

    def run(lead):
        bd, ad = _framed(b, lead)[1], _framed(a, lead)[1]
        flat, out = _framed(blank, lead, fill=float("nan"))
        p2._call(RESTRICT + "_multi", *head, bd, ad, out, out.element_size(), n_v, n_f, n_vec)
        assert _guards_intact(flat, lead, n_v * n_vec)
        return out.cpu().numpy()

    runs = [run(16), run(16)]
    assert not np.isnan(runs[0]).any()
    assert _same_bits(runs[0], runs[1]), "two runs differ"
    assert _same_bits(runs[0], run(17)), "blocks off the 16-byte grid give other bits"
    for j in range(n_vec):
        out = torch.full((n_v,), float("nan"), dtype=dtype)
        p2._call(RESTRICT, *head, torch.tensor(b[:, j].copy()), torch.tensor(a[:, j].copy()), out,
                 out.element_size(), n_v, n_f)
        assert _same_bits(runs[0][:, j], out.cpu().numpy()), f"column {j} differs from the single kernel"
        want, scale, length = p2._restrict_reference(n_v, n_f, ptr, idx, m_c, m_f, b[:, j], a[:, j])
        p2._close(runs[0][:, j], want, scale, length, np_dtype,
                  f"P2 restrict_multi {tables} masked={masked} n_vec={n_vec} column {j}")
    if m_c is not None:
        assert (runs[0][m_c == 0] == 0).all()


@pytest.mark.parametrize("n_vec", WIDTHS)
@pytest.mark.parametrize("tables", ["square3", "star"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_prolong_multi_kernel(tables, masked, dtype, np_dtype, n_vec):
    """x_f += m_f P e_c on blocks: column j bit for bit the single kernel, two runs the same bits,
    the same from blocks off the 16-byte grid, guards around x_f intact, rows with m_f = 0
    unchanged, |err| <= (row length + 3) eps sum |terms|."""
    n_v, n_f, edges, _, _ = p2._tables(tables)
    rng = np.random.default_rng(52)
    e, x = multi._block(rng, n_v, n_vec, np_dtype), multi._block(rng, n_f, n_vec, np_dtype)
    m_f = p2._random(rng, n_f, np_dtype, mask=True) if masked else None
    ev, md = torch.tensor(edges), _dev(m_f)

    def run(lead):
        ed = _framed(e, lead)[1]
        flat, xd = _framed(x, lead)
        p2._call(PROLONG + "_multi", ev, md, ed, xd, xd.element_size(), n_v, n_f, n_vec)
        assert _guards_intact(flat, lead, n_f * n_vec)
        return xd.cpu().numpy()

    runs = [run(16), run(16)]
    assert _same_bits(runs[0], runs[1]), "two runs differ"
    assert _same_bits(runs[0], run(17)), "blocks off the 16-byte grid give other bits"
    weight = (np.ones(n_f, dtype=LD) if m_f is None else m_f.astype(LD))[:, None]
    el = e.astype(LD)
    add = np.concatenate([el, 0.5 * (el[edges[:, 0]] + el[edges[:, 1]])])
    size = np.concatenate([np.abs(el), 0.5 * (np.abs(el)[edges[:, 0]] + np.abs(el)[edges[:, 1]])])
    want = x.astype(LD) + weight * add
    scale = np.abs(x.astype(LD)) + weight * size
    length = np.concatenate([np.full(n_v, 1), np.full(n_f - n_v, 2)])
    for j in range(n_vec):
        xs = torch.tensor(x[:, j].copy())
        p2._call(PROLONG, ev, md, torch.tensor(e[:, j].copy()), xs, xs.element_size(), n_v, n_f)
        assert _same_bits(runs[0][:, j], xs.cpu().numpy()), f"column {j} differs from the single kernel"
        p2._close(runs[0][:, j], want[:, j], scale[:, j], length, np_dtype,
                  f"P2 prolong_multi {tables} masked={masked} n_vec={n_vec} column {j}")
    if m_f is not None:
        assert _same_bits(runs[0][m_f == 0], x[m_f == 0])


# --------------------------------------------------------------------------------- the cycle
def _columns_match_the_single_cycle(mg, Z, R, what):
    """Within 1e-10 of |z|_inf, not bit-equal: the coarsest level is torch.mm here, torch.mv there."""
    for j in range(R.shape[1]):
        z = mg.vcycle(torch.tensor(R[:, j].copy())).cpu().numpy()
        err = np.abs(Z[:, j] - z).max() / np.abs(z).max()
        print(f"{what}, column {j}: block cycle against the single cycle {err:.3e}")
        assert err <= 1e-10


@pytest.mark.parametrize("name,levels", [("stiffness", 0), ("stiffness", 1), ("stiffness", 2), ("no_mask", 1)])
def test_vcycle_multi_matches_the_model_on_every_column(name, levels):
    """k = 3 standard-normal columns: every column within 1e-10 of |z|_inf of the model's cycle (the
    bound of the single P2 cycle) and of ``vcycle`` on that column, exactly 0 on the held DoFs; a
    second call gives the same bits; more widths than are kept; the single cycle's buffers are not
    disturbed."""
    mg, model = p2._solver(name, levels), p2._model(name, levels)
    n = model.n
    rng = np.random.default_rng(61)
    R = rng.standard_normal((n, 3))
    r1 = torch.tensor(rng.standard_normal(n))
    before = mg.vcycle(r1).cpu().numpy()
    Z = mg.vcycle_multi(torch.tensor(R))
    assert Z.dtype == torch.float64 and tuple(Z.shape) == (n, 3)
    Zh = multi._check_columns(Z, R, model, 1e-10, f"{name}, {levels} refinements, k = 3")
    assert _same_bits(mg.vcycle(r1).cpu().numpy(), before), "the block cycle disturbed the single cycle"
    _columns_match_the_single_cycle(mg, Zh, R, f"{name}, {levels} refinements")
    assert _same_bits(mg.vcycle_multi(torch.tensor(R)).cpu().numpy(), Zh), "two block cycles differ"
    # more widths than are kept: the oldest is dropped and comes back
    for k in (2, 3, 1, 2):
        multi._check_columns(mg.vcycle_multi(torch.tensor(R[:, :k])), R[:, :k], model, 1e-10,
                             f"{name}, {levels} refinements, k = {k} again")
        assert len(mg._blocks) <= mg.BLOCK_WIDTHS_KEPT and len(mg.p1._blocks) <= mg.p1.BLOCK_WIDTHS_KEPT
    assert _same_bits(mg.vcycle(r1).cpu().numpy(), before)


def _check_route(mg, model, what):
    """Cycle (k = 2) and solve (two columns) of a freshly built hierarchy against the model."""
    n = model.n
    R = np.random.default_rng(63).standard_normal((n, 2))
    multi._check_columns(mg.vcycle_multi(torch.tensor(R)), R, model, 1e-10, what)
    B = np.stack([p2ref.masked_rhs(model, 2), p2ref.masked_rhs(model, 3)], axis=1)
    X, its, res = mg.solve_multi(torch.tensor(B))
    assert tuple(X.shape) == B.shape and (res <= 1e-10).all()
    Xh = X.cpu().numpy()
    for j in range(2):
        x_model, it_model, _ = model.pcg(B[:, j])
        err = np.abs(Xh[:, j] - x_model).max() / np.abs(x_model).max()
        print(f"{what}, column {j}: {int(its[j])} iterations (model {it_model}), against the model's solution {err:.3e}")
        assert abs(int(its[j]) - it_model) <= 2
        assert err <= 1e-9
    assert (Xh[model.mask2 == 0] == 0).all()


def test_edge_renumbering_runs_the_block_rows_launch_in_the_engine_numbering(monkeypatch):
    """TFEM_RENUMBER=1: the P2 level is crossing, its block apply is the prepared rows launch (never
    ``matvec``), and blocks cross once at the boundary of vcycle_multi / solve_multi."""
    monkeypatch.setenv("TFEM_RENUMBER", "1")
    mesh, bilinear, _ = p2.HIERARCHIES["stiffness"]
    mg = tf().P2Multigrid(mesh(), 1, bilinear)
    engine, top = mg.basis._engine, mg.levels[-1]
    assert engine.renumbered and mg.operator.matrix_free and top.crossing
    perm = engine._perm.cpu().numpy()
    assert (perm[:top.n_v] == np.arange(top.n_v)).all() and (perm != np.arange(top.n)).any()
    calls = []
    rows_into = mg.operator._rows_into
    monkeypatch.setattr(mg.operator, "_rows_into", lambda: calls.append("rows") or rows_into())
    monkeypatch.setattr(mg.operator, "matvec", lambda *a, **k: pytest.fail("the P2 level fell back to matvec"))
    _check_route(mg, p2._model("stiffness", 1), "edge renumbering, 1 refinement, k = 2")
    assert calls == ["rows"]


def test_csr_route_on_blocks(monkeypatch):
    """TFEM_KERNEL=gather: no P2 row plan, the P2 level applies the assembled CSR to the block
    (tfem_csr_spmm through CSRMatrix._prepared_spmv)."""
    monkeypatch.setenv("TFEM_KERNEL", "gather")
    mesh, bilinear, _ = p2.HIERARCHIES["stiffness"]
    mg = tf().P2Multigrid(mesh(), 1, bilinear)
    assert not mg.operator.matrix_free and not mg.levels[-1].crossing
    _check_route(mg, p2._model("stiffness", 1), "CSR route, 1 refinement, k = 2")


def test_vcycle_multi_in_float32():
    """dtype=float32, k = 3, against the float64 model: the bound of
    test_hip_p2_multigrid.test_vcycle_in_float32, 100 x TOL32_APPLY = 100 x 8 x 1.375e-5."""
    mesh, bilinear, _ = p2.HIERARCHIES["stiffness"]
    mg = tf().P2Multigrid(mesh(), 1, bilinear, dtype=torch.float32)
    model = p2._model("stiffness", 1)
    R = np.random.default_rng(62).standard_normal((model.n, 3)).astype(np.float32)
    Z = mg.vcycle_multi(torch.tensor(R))
    assert Z.dtype == torch.float32 and tuple(Z.shape) == (model.n, 3)
    multi._check_columns(Z, R, model, 100 * 8 * 1.375e-05, "float32, k = 3")


# --------------------------------------------------------------------------------- the launches
@pytest.fixture
def recorder(monkeypatch):
    from pytorch_fem_solver_amd import _native

    proxy = launches.Recorder(_native.load())
    monkeypatch.setattr(_native, "load", lambda: proxy)
    return proxy


#: position of ``n_vec`` among the arguments of the block launches
N_VEC_ARG = {launches.S + "_multi": 6, launches.R + "_multi": 10, launches.P + "_multi": 7,
             RESTRICT + "_multi": 10, PROLONG + "_multi": 7}


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("levels", [0, 2])
def test_p2_block_cycle_launches(recorder, levels, nu):
    """The launches of the single P2 cycle in their block forms, as many for k = 3 as for k = 1."""
    mg = launches._hierarchy("P2Multigrid", levels, nu)
    smooth = launches.S + "_multi"
    lengths = []
    for k in (1, 3):
        calls = launches._cycle_calls(recorder, mg.vcycle_multi, torch.randn(mg.levels[-1].n, k))
        assert [name for name, _ in calls] == (nu * [smooth] + [RESTRICT + "_multi"] + launches.seq(levels, nu, "_multi")
                                               + [PROLONG + "_multi"] + nu * [smooth])
        for name, args in calls:
            assert args[N_VEC_ARG[name]] == k, (name, args[N_VEC_ARG[name]], k)
        launches._check_smooths(calls, mg, nu)
        lengths.append(len(calls))
    assert lengths[0] == lengths[1]


# --------------------------------------------------------------------------------- the solve
_CASES = {}


def _case(name):
    """(B, X0, model solutions, model counts) of the five columns B = [b2, 0, b3, b4, b2] with the
    starts X0 = [0, 0, rough, 0, direct] -- the construction of test_hip_multigrid_multi._case on the
    P2 model with one refinement --, built once per hierarchy."""
    if name not in _CASES:
        model = p2._model(name, 1)
        n = model.n
        b2, b3, b4 = (p2ref.masked_rhs(model, seed) for seed in (2, 3, 4))
        free = np.flatnonzero(model.mask2)
        direct = np.zeros(n)
        direct[free] = np.linalg.solve(model.K2[free][:, free].toarray(), b2[free])
        rough = model.pcg(b3, rtol=1e-5)[0]
        B = np.stack([b2, np.zeros(n), b3, b4, b2], axis=1)
        X0 = np.stack([np.zeros(n), np.zeros(n), rough, np.zeros(n), direct], axis=1)
        xs, counts = [], []
        for j in range(5):
            x, it = multi._warm_pcg(model, B[:, j], X0[:, j], 1e-10)
            xs.append(x)
            counts.append(it)
        _CASES[name] = (B, X0, np.stack(xs, axis=1), counts)
    return _CASES[name]


@pytest.mark.parametrize("name,n_dofs", [("stiffness", 1089), ("delaunay", 1049)])
def test_solve_multi(name, n_dofs):
    """Five columns that freeze at different times (the model: 13 / 0 / 6 / 12 / 0 iterations on the
    structured hierarchy, 23 / 0 / 13 / 23 / 0 on the Delaunay one, one refinement each): residuals
    <= rtol, iterations within 2 of the model's, the columns that start converged untouched, X within
    1e-9 of |x|_inf of the model's solution, exactly 0 on the held DoFs; the same from a zero start
    without X0; maxiter = 3 stops the running columns at 3."""
    mg, model = p2._solver(name, 1), p2._model(name, 1)
    assert model.n == n_dofs
    B, X0, x_model, counts = _case(name)
    print(f"{name}: the model's iterations {counts}")
    assert counts[1] == 0 and counts[4] == 0 and len(set(counts)) >= 3, counts
    X, its, res = mg.solve_multi(torch.tensor(B), X0=torch.tensor(X0), rtol=1e-10)
    print(f"{name}: iterations {its.tolist()}, residuals {[f'{r:.1e}' for r in res.tolist()]}")
    assert tuple(X.shape) == (n_dofs, 5) and X.dtype == torch.float64
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
    assert (Xh[model.mask2 == 0] == 0).all()
    # the same from a zero start without X0, on the columns that have one
    X_zero, its_zero, res_zero = mg.solve_multi(torch.tensor(B[:, [0, 1, 3]]), rtol=1e-10)
    assert (res_zero <= 1e-10).all() and int(its_zero[1]) == 0
    assert abs(int(its_zero[0]) - counts[0]) <= 2 and abs(int(its_zero[2]) - counts[3]) <= 2
    Xz = X_zero.cpu().numpy()
    for col, j in enumerate((0, 1, 3)):
        assert np.abs(Xz[:, col] - x_model[:, j]).max() <= 1e-9 * np.abs(x_model[:, j]).max()
    assert (Xz[model.mask2 == 0] == 0).all()
    # maxiter: the running columns stop at 3 above rtol, the others took no iteration
    X3, its3, res3 = mg.solve_multi(torch.tensor(B), X0=torch.tensor(X0), rtol=1e-10, maxiter=3)
    assert its3.tolist() == [3, 0, 3, 3, 0]
    assert (res3[[0, 2, 3]] > 1e-10).all() and (res3[[1, 4]] <= 1e-10).all()
    assert torch.isfinite(X3).all()


def test_refusals_of_the_block_methods():
    mg = p2._solver("stiffness", 0)
    n = mg.operator.shape[0]
    with pytest.raises(ValueError, match="shape"):
        mg.solve_multi(torch.ones(n))
    with pytest.raises(ValueError, match="shape"):
        mg.solve_multi(torch.ones(n + 1, 2))
    with pytest.raises(ValueError, match="shape"):
        mg.vcycle_multi(torch.ones(n + 1, 2))
    with pytest.raises(ValueError, match="shape"):
        mg.vcycle_multi(torch.ones(n))
    with pytest.raises(ValueError, match="P2Multigrid"):
        mg.solve_multi(torch.ones(n, 2), X0=torch.ones(n, 3))
    with pytest.raises(NotImplementedError, match="blocks.*vcycle_multi.*solve_multi"):
        mg.solve(torch.ones(n, 2))
    with pytest.raises(NotImplementedError, match="blocks.*vcycle_multi.*solve_multi"):
        mg.vcycle(torch.ones(n, 2))
