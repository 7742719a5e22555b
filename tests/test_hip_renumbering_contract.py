"""The boundary of an engine that renumbered its mesh (AssemblyEngine._perm: P1 vertices along the
Morton curve, P2 edge DoFs along the Morton curve of the midpoints), driven the way a pipeline
drives it: with result buffers (``out=``) on every kernel mode, and sharded through the recipe of
INTEGRATION.md (parallel.InterfaceExchange.from_partition on the engine's own pattern).  Runs on a
real MI355X only (-m gpu).

The reference is the numpy oracle (oracle/assembly_oracle.py) on the CALLER's mesh, in float64;
for a float32 engine on the float32-rounded coordinates and source values.  Every case runs with
TFEM_RENUMBER=1 (the engine renumbers, whatever the size of the mesh) and with TFEM_RENUMBER=0 (the
control).  The result buffers are filled with NaN before every call.

Bounds: scaled_error and rowwise_error (tests/conftest.py) at 1e-12 in float64 and 5e-5 in
float32, the project's own.  "With buffers = without buffers": bit for bit wherever the engine sums
an entry's element shares in a fixed order (ring launch with source values, P2 row plan, element
blocks + gather).  The tile launch and TFEM_KERNEL=atomic add the shares of an entry with atomics
(LDS / memory), and the fused ring launch of a source program adds a vertex's load shares in LDS in
the order the waves reach them: two runs of the SAME launch differ there by the reordering of a
sum of n terms t_k, at most 2 (n - 1) u sum_k |t_k| (u the unit roundoff; Higham, Accuracy and
Stability of Numerical Algorithms, (4.4) applied to both orders).  There the comparison uses that
bound entry by entry, with n the largest number of elements at a DoF and sum |t_k| from the oracle's
element blocks -- nothing measured on the device."""

import math

import numpy as np
import pytest
import torch

from conftest import rowwise_error, scaled_error
from oracle import assembly_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-12, torch.float32: 5e-5}
ROUNDOFF = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
ALPHA, BETA = 1.25, 0.75
ORDER = 3
P1_MODES = ("auto", "rings", "tiles", "gather", "atomic")
NON_RING = ("tiles", "gather", "atomic")
#: 2 pi^2 sin(pi x) sin(pi y)
SOURCE = ("mul", ("mul", ("sin", ("mul", ("x",), ("c", math.pi))), ("c", 2.0 * math.pi ** 2)),
          ("sin", ("mul", ("y",), ("c", math.pi))))


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def _note(group, err, bound):
    """Every figure is printed before it is asserted."""
    print(f"[contract] {group}: {err:.3e} (bound {bound:.1e})")
    assert err <= bound, f"{group}: {err:.3e} > {bound:.1e}"


def _host(t):
    return t.detach().double().cpu().numpy().reshape(-1)


def _poisoned(shape, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype)


def _program():
    from pytorch_fem_solver_amd.basis import forms

    program = forms.compile_program(SOURCE)
    n = int(program.n_ops)
    ops, consts = [int(v) for v in program.ops[:n]], [float(v) for v in program.consts[:n]]
    return program, (lambda pts: orc.source_program_eval(ops, consts, pts[..., [0]], pts[..., [1]]))


# ----------------------------------------------------------------------------- meshes, references
_CASES = {}


def _p1_mesh():
    """delaunay_square(700) with a random vertex numbering; 8 % of the elements removed at random
    (open fans, several fans per vertex) and every element around three vertices (isolated
    vertices: empty rows), about 10 % in all."""
    from pytorch_fem_solver_amd import meshgen

    rng = np.random.default_rng(5)
    mesh = meshgen.delaunay_square(700, 5)
    nv = mesh["vertices"].shape[0]
    mesh = meshgen.permute_mesh(mesh, vertex_order=rng.permutation(nv))
    tris = mesh["triangles"]
    keep = rng.random(tris.shape[0]) >= 0.08
    lonely = rng.choice(nv, size=3, replace=False)
    keep &= ~np.isin(tris, lonely).any(axis=1)
    tris = np.ascontiguousarray(tris[keep].astype(np.int32))
    assert 0.85 <= keep.mean() <= 0.93
    assert (np.bincount(tris.reshape(-1), minlength=nv) == 0).sum() >= 3
    return mesh["vertices"], tris, tris


def _p2_mesh(kind):
    from pytorch_fem_solver_amd import dofs, meshgen

    mesh = meshgen.unit_square(9, 0.25, 3) if kind == "p2_square" else meshgen.delaunay_square(300, 3)
    tris = mesh["triangles"]
    edges, on_boundary = meshgen._edges_from_triangles(tris)
    conn6, xy, _ = dofs.p2_dofs_numpy(mesh["vertices"], tris, edges, on_boundary.astype(np.int32).reshape(-1, 1),
                                      mesh["vertex_markers"])
    return mesh["vertices"], np.ascontiguousarray(tris.astype(np.int32)), np.ascontiguousarray(conn6)


def _case(kind, dtype=torch.float64):
    """Mesh and oracle results of one case, computed once: CSR pattern and values of ALPHA * stiffness
    + BETA * mass, the load vectors of random source values and of SOURCE, and per entry the sum of
    the magnitudes of its element shares (the scale of the reordering bound)."""
    key = (kind, dtype)
    if key in _CASES:
        return _CASES[key]
    verts, tris, conn = _p1_mesh() if kind == "p1" else _p2_mesh(kind)
    single = dtype == torch.float32
    if single:
        verts = verts.astype(np.float32)
    poly = 1 if kind == "p1" else 2
    n = int(conn.max()) + 1 if poly == 2 else verts.shape[0]
    geo = orc.geometry(verts.astype(np.float64)[tris], poly, ORDER)
    local = orc.integrate_local(ALPHA * orc.integrand_stiffness(geo) + BETA * orc.integrand_mass(geo), geo["dx"])
    rowptr, colind, slots = orc.csr_pattern(conn, n)
    nnz = colind.shape[0]
    rng = np.random.default_rng(17)
    n_quad = geo["dx"].shape[-3]
    fq = rng.uniform(-1.0, 1.0, (tris.shape[0], n_quad))
    if single:
        fq = fq.astype(np.float32)
    local_f = orc.integrate_local(fq.astype(np.float64).reshape(-1, n_quad, 1, 1) * geo["v"], geo["dx"])
    program, source = _program()
    local_s = orc.integrate_local(orc.integrand_load(geo, source), geo["dx"])
    vector = lambda loc: orc.assemble_linear(loc, conn, n).reshape(-1)  # noqa: E731
    case = {
        "kind": kind, "poly": poly, "dtype": dtype, "verts": verts, "tris": tris, "conn": conn, "n": n,
        "rowptr": rowptr, "colind": colind, "fq": fq, "program": program,
        "k": orc.assemble_csr_values(local, slots, nnz), "k_abs": orc.assemble_csr_values(np.abs(local), slots, nnz),
        "f": {"fq": vector(local_f), "source": vector(local_s)},
        "f_abs": {"fq": vector(np.abs(local_f)), "source": vector(np.abs(local_s))},
        "fan": int(np.bincount(conn.reshape(-1), minlength=n).max()),
    }
    case["dense"] = orc.csr_to_dense(rowptr, colind, case["k"], n)
    _CASES[key] = case
    return case


def _engine(case, kernel="auto"):
    from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

    coords = torch.tensor(case["verts"], dtype=case["dtype"])
    tris = torch.tensor(case["tris"])
    conn = tris if case["poly"] == 1 else torch.tensor(case["conn"])
    eng = AssemblyEngine(coords, tris, conn, case["n"], case["poly"], ORDER)
    eng.kernel = kernel  # after the constructor, as tests/test_hip_fuzz.py: the renumbering is decided there
    return eng


def _renumber(monkeypatch, on):
    monkeypatch.setenv("TFEM_RENUMBER", "1" if on else "0")


# ----------------------------------------------------------------------------- comparisons
def _check_matrix(eng, vals, case, group):
    """CSR values of the engine, read through wrap_csr in the caller's numbering, against the oracle."""
    assert vals is not None and vals.numel() == case["colind"].shape[0]
    assert not torch.isnan(vals).any(), f"{group}: NaN left in the CSR values"
    m = eng.wrap_csr(vals.reshape(-1)).caller_numbering()
    assert np.array_equal(m.crow_indices.cpu().numpy(), case["rowptr"]), group
    assert np.array_equal(m.col_indices.cpu().numpy(), case["colind"]), group
    got, tol = _host(m.values), TOL[case["dtype"]]
    _note(group + " K scaled", scaled_error(got, case["k"]), tol)
    _note(group + " K rowwise", rowwise_error(got, case["k"], case["rowptr"]), tol)


def _check_vector(f, want, case, group):
    """A per-DoF vector of the engine against the oracle's in the caller's numbering."""
    assert f is not None and f.numel() == want.size
    assert not torch.isnan(f).any(), f"{group}: NaN left in the vector"
    _note(group + " scaled", scaled_error(_host(f), want.reshape(-1)), TOL[case["dtype"]])


def _fixed_order(eng, source):
    """(K, f): whether the launches behind assemble_system add the element shares of an entry in a
    fixed order (module docstring)."""
    if eng.kernel == "atomic":
        return False, False
    if eng.poly_order == 2 or eng.kernel == "gather":
        return True, True  # P2 row plan / element blocks + gather
    if eng._use_rings():
        if source and eng._rings_take_source():
            return True, False  # K in row form; f: shares added in LDS in the order of the waves
        if eng.ring_plan()["fq_ok"]:
            return True, True
    planless = eng.tile_plan() is None
    return planless, planless  # the tile launch adds with LDS atomics


def _check_same(got, ref, fixed, abs_scale, case, group):
    """With buffers = without buffers, on the same engine."""
    got, ref = got.reshape(-1), ref.reshape(-1)
    if fixed:
        assert torch.equal(got, ref), f"{group}: differs from the call without buffers"
        return
    slack = 2.0 * (case["fan"] - 1) * ROUNDOFF[case["dtype"]] * abs_scale
    excess = float((np.abs(_host(got) - _host(ref)) - slack).max())
    print(f"[contract] {group} reordering: excess over the bound {excess:.3e}")
    assert excess <= 0.0, f"{group}: differs from the call without buffers by more than a reordering"


def _abs_in_engine_order(eng, case):
    """case['k_abs'] (caller's CSR order) in the order of the engine's CSR values."""
    if not eng.renumbered:
        return case["k_abs"]
    n = case["n"]
    csr = eng.csr_structure()
    rowptr, colind = csr[0], csr[1]
    perm = eng.dof_permutation().cpu().numpy()
    rows = np.repeat(np.arange(n), np.diff(rowptr.cpu().numpy()))
    from pytorch_fem_solver_amd import parallel

    return case["k_abs"][parallel._csr_positions(case["rowptr"], case["colind"], perm[rows], perm[colind.cpu().numpy()])]


def _system_with_every_out(eng, case, source, group):
    """assemble_system with out = None, (vals, f), (vals, None), (None, f).  Raises
    NotImplementedError from the first call when the mode does not apply to the mesh."""
    dtype, n, nnz = case["dtype"], case["n"], case["colind"].shape[0]
    which = "source" if source else "fq"
    kwargs = {"source": case["program"]} if source else {"fq": torch.tensor(case["fq"], dtype=dtype)}
    vals0, f0 = eng.assemble_system(ALPHA, BETA, **kwargs)
    vals0, f0 = vals0.clone(), f0.clone()
    _check_matrix(eng, vals0, case, f"{group} out=None")
    _check_vector(f0, case["f"][which], case, f"{group} out=None f")
    fixed_k, fixed_f = _fixed_order(eng, source)
    k_abs = _abs_in_engine_order(eng, case)
    for give_k, give_f in ((True, True), (True, False), (False, True)):
        tag = f"{group} out=({'vals' if give_k else None}, {'f' if give_f else None})"
        buf_k = _poisoned(nnz, dtype) if give_k else None
        buf_f = _poisoned(n, dtype) if give_f else None
        result = eng.assemble_system(ALPHA, BETA, out=(buf_k, buf_f), **kwargs)
        assert isinstance(result, tuple) and len(result) == 2, tag
        vals, f = result
        assert torch.is_tensor(vals) and torch.is_tensor(f), f"{tag}: returned {type(vals)}, {type(f)}"
        if give_k:
            assert vals.data_ptr() == buf_k.data_ptr(), tag
            assert not torch.isnan(buf_k).any(), f"{tag}: NaN left in the buffer of the CSR values"
        if give_f:
            assert f.data_ptr() == buf_f.data_ptr(), tag
            assert not torch.isnan(buf_f).any(), f"{tag}: NaN left in the buffer of the load vector"
        _check_matrix(eng, vals, case, tag)
        _check_vector(f, case["f"][which], case, tag + " f")
        _check_same(vals, vals0, fixed_k, k_abs, case, tag + " K")
        _check_same(f, f0, fixed_f, case["f_abs"][which], case, tag + " f")


# ----------------------------------------------------------------------------- assemble_system(out=)
def _p1_modes(case, modes, renumber):
    tried = []
    for kernel in modes:
        for source in (False, True):
            eng = _engine(case, kernel)
            assert eng.renumbered == renumber
            if source and not eng.supports_source():
                continue
            group = f"p1 {case['dtype']} renumber={int(renumber)} {kernel} {'source' if source else 'fq'}"
            try:
                _system_with_every_out(eng, case, source, group)
            except NotImplementedError:
                assert kernel in ("rings", "tiles")  # a plan the mesh does not fit
                break
            tried.append((kernel, source, eng.kernel_name()))
    print("[contract] modes that ran:", tried)
    return {kernel for kernel, _, _ in tried}


@pytest.mark.parametrize("renumber", [True, False])
def test_assemble_system_buffers_p1_every_kernel_mode(renumber, monkeypatch):
    _renumber(monkeypatch, renumber)
    ran = _p1_modes(_case("p1"), P1_MODES, renumber)
    assert "auto" in ran and ran & set(NON_RING)


@pytest.mark.parametrize("renumber", [True, False])
def test_assemble_system_buffers_p1_float32(renumber, monkeypatch):
    _renumber(monkeypatch, renumber)
    ran = _p1_modes(_case("p1", torch.float32), ("auto", "gather"), renumber)
    assert ran == {"auto", "gather"}


@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("kernel", ["auto", "gather"])
@pytest.mark.parametrize("kind", ["p2_square", "p2_delaunay"])
def test_assemble_system_buffers_p2(kind, kernel, renumber, monkeypatch):
    _renumber(monkeypatch, renumber)
    case = _case(kind)
    eng = _engine(case, kernel)
    assert eng.renumbered == renumber
    _system_with_every_out(eng, case, False, f"{kind} renumber={int(renumber)} {kernel} fq")


# ----------------------------------------------------------------------------- the other entry points
def _returns_buffer(result, buf, group):
    assert torch.is_tensor(result) and result.data_ptr() == buf.data_ptr(), group
    assert not torch.isnan(buf).any(), f"{group}: NaN left in the buffer"


@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("kind,kernel", [("p1", "auto"), ("p1", "gather"), ("p2_square", "auto"),
                                         ("p2_delaunay", "auto"), ("p2_delaunay", "gather")])
def test_load_apply_and_bilinear_buffers(kind, kernel, renumber, monkeypatch):
    """load(fq, out=), load_source(program, out=), apply(alpha, beta, u, out=) flat and (N, 3): the
    caller's numbering; bilinear(out=): the engine's values, read through wrap_csr."""
    _renumber(monkeypatch, renumber)
    case = _case(kind)
    eng = _engine(case, kernel)
    assert eng.renumbered == renumber
    dtype, n, nnz = case["dtype"], case["n"], case["colind"].shape[0]
    group = f"{kind} renumber={int(renumber)} {kernel}"
    fixed_k, fixed_f = _fixed_order(eng, False)
    fq = torch.tensor(case["fq"], dtype=dtype)

    plain = eng.load(fq).clone()
    _check_vector(plain, case["f"]["fq"], case, group + " load")
    buf = _poisoned(n, dtype)
    _returns_buffer(eng.load(fq, out=buf), buf, group + " load(out=)")
    _check_vector(buf, case["f"]["fq"], case, group + " load(out=)")
    _check_same(buf, plain, fixed_f, case["f_abs"]["fq"], case, group + " load(out=)")

    assert eng.supports_source()
    plain = eng.load_source(case["program"]).clone()
    _check_vector(plain, case["f"]["source"], case, group + " load_source")
    buf = _poisoned(n, dtype)
    _returns_buffer(eng.load_source(case["program"], out=buf), buf, group + " load_source(out=)")
    _check_vector(buf, case["f"]["source"], case, group + " load_source(out=)")
    _check_same(buf, plain, _fixed_order(eng, True)[1], case["f_abs"]["source"], case, group + " load_source(out=)")

    plain = eng.bilinear(ALPHA, BETA).clone()
    _check_matrix(eng, plain, case, group + " bilinear")
    buf = _poisoned(nnz, dtype)
    _returns_buffer(eng.bilinear(ALPHA, BETA, out=buf), buf, group + " bilinear(out=)")
    _check_matrix(eng, buf, case, group + " bilinear(out=)")
    _check_same(buf, plain, fixed_k, _abs_in_engine_order(eng, case), case, group + " bilinear(out=)")

    if kernel != "auto":
        return  # the matrix-free operator launches over the ring plan / the P2 row plan
    rng = np.random.default_rng(23)
    for shape in ((n,), (n, 3)):
        u = rng.uniform(-1.0, 1.0, shape)
        want = case["dense"] @ u
        tag = f"{group} apply {shape}"
        plain = eng.apply(ALPHA, BETA, torch.tensor(u, dtype=dtype)).clone()
        assert tuple(plain.shape) == shape
        _check_vector(plain, want, case, tag)
        buf = _poisoned(shape, dtype)
        result = eng.apply(ALPHA, BETA, torch.tensor(u, dtype=dtype), out=buf)
        assert tuple(result.shape) == shape
        _returns_buffer(result, buf, tag + " out=")
        _check_vector(buf, want, case, tag + " out=")
        assert torch.equal(buf, plain), tag + ": differs from the call without a buffer"


@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("kind,kernel", [("p1", "auto"), ("p1", "gather"), ("p2_square", "auto")])
def test_a_buffer_that_does_not_fit_is_refused(kind, kernel, renumber, monkeypatch):
    """Wrong length, dtype or contiguity: ValueError, on a renumbered engine as on a plain one."""
    _renumber(monkeypatch, renumber)
    case = _case(kind)
    eng = _engine(case, kernel)
    assert eng.renumbered == renumber
    n, nnz = case["n"], case["colind"].shape[0]
    fq = torch.tensor(case["fq"])
    u = torch.ones(n)

    def misfits(numel):
        return {"length": torch.zeros(numel + 1), "dtype": torch.zeros(numel, dtype=torch.float32),
                "contiguity": torch.zeros(2 * numel)[::2]}

    for what, bad in misfits(nnz).items():
        assert bad.numel() == nnz or what == "length"
        with pytest.raises(ValueError, match="out:"):
            eng.assemble_system(ALPHA, BETA, fq, out=(bad, torch.zeros(n)))
        with pytest.raises(ValueError, match="out:"):
            eng.assemble_system(ALPHA, BETA, fq, out=(bad, None))
        with pytest.raises(ValueError, match="out:"):
            eng.bilinear(ALPHA, BETA, out=bad)
    for what, bad in misfits(n).items():
        with pytest.raises(ValueError, match="out:"):
            eng.assemble_system(ALPHA, BETA, fq, out=(torch.zeros(nnz), bad))
        with pytest.raises(ValueError, match="out:"):
            eng.assemble_system(ALPHA, BETA, fq, out=(None, bad))
        with pytest.raises(ValueError, match="out:"):
            eng.load(fq, out=bad)
        with pytest.raises(ValueError, match="out:"):
            eng.load_source(case["program"], out=bad)
        if kernel == "auto":
            with pytest.raises(ValueError, match="out:"):
                eng.apply(ALPHA, BETA, u, out=bad)
    # and the engine still works
    vals, f = eng.assemble_system(ALPHA, BETA, fq)
    _check_matrix(eng, vals, case, f"{kind} renumber={int(renumber)} {kernel} after the refusals")
    _check_vector(f, case["f"]["fq"], case, f"{kind} renumber={int(renumber)} {kernel} after the refusals f")


@pytest.mark.parametrize("kind", ["p1", "p2_square"])
def test_what_a_renumbered_engine_refuses_by_name(kind, monkeypatch):
    _renumber(monkeypatch, True)
    case = _case(kind)
    eng = _engine(case)
    assert eng.renumbered
    n, nnz = case["n"], case["colind"].shape[0]
    fq = torch.tensor(case["fq"])
    pair = (torch.zeros(nnz), torch.zeros(n))
    with pytest.raises(NotImplementedError, match="renumbered"):
        eng.prepared_system(ALPHA, BETA, pair, fq=fq)
    with pytest.raises(NotImplementedError, match="renumbered"):
        eng.set_priority_vertices(np.zeros(n, dtype=bool))
    with pytest.raises(NotImplementedError, match="renumbered"):
        eng.assemble_system(ALPHA, BETA, fq, out=pair, tiles="all")


# ----------------------------------------------------------------------------- the sharded recipe
_WHOLE = {}


def _whole_mesh():
    """delaunay_square(1500) in a random vertex numbering (a shard of it has no locality) and the
    oracle's operator 1.0 * stiffness + 0.5 * mass and load vector of random source values on it."""
    if not _WHOLE:
        from pytorch_fem_solver_amd import meshgen

        rng = np.random.default_rng(29)
        mesh = meshgen.delaunay_square(1500, 9)
        nv = mesh["vertices"].shape[0]
        mesh = meshgen.permute_mesh(mesh, vertex_order=rng.permutation(nv))
        verts, tris = mesh["vertices"], mesh["triangles"]
        geo = orc.geometry(verts[tris], 1, ORDER)
        local = orc.integrate_local(1.0 * orc.integrand_stiffness(geo) + 0.5 * orc.integrand_mass(geo), geo["dx"])
        n_quad = geo["dx"].shape[-3]
        fq = rng.uniform(-1.0, 1.0, (tris.shape[0], n_quad))
        local_f = orc.integrate_local(fq.reshape(-1, n_quad, 1, 1) * geo["v"], geo["dx"])
        _WHOLE.update(mesh=mesh, fq=fq, dense=orc.assemble_dense_bilinear(local, tris, nv),
                      f=orc.assemble_linear(local_f, tris, nv).reshape(-1))
    return _WHOLE


@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_recipe_on_one_process(world, renumber, monkeypatch):
    """The recipe of INTEGRATION.md, one engine per shard in ONE process: assemble, pack, the sum of
    the packed buffers (what the all-reduce computes), unpack; then EVERY entry a shard holds
    against the oracle of the whole mesh (an entry of a shard's pattern that takes shares from
    another shard lies between two shared vertices: tests/sharded/check_sharded_assembly.py)."""
    from pytorch_fem_solver_amd import parallel
    from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

    _renumber(monkeypatch, renumber)
    whole = _whole_mesh()
    mesh = whole["mesh"]
    order, bounds = parallel.partition_elements(mesh["vertices"], mesh["triangles"], world, "morton")
    device = torch.device("cuda", torch.cuda.current_device())
    shards = []
    for rank in range(world):
        mine = order[bounds[rank]:bounds[rank + 1]]
        local, l2g = parallel.extract_shard(mesh, mine)
        tris = torch.tensor(local["triangles"])
        eng = AssemblyEngine(torch.tensor(local["vertices"]), tris, tris, l2g.shape[0], 1, ORDER)
        assert eng.renumbered == renumber
        vals, f = eng.assemble_system(1.0, 0.5, torch.tensor(whole["fq"][mine]))
        csr = eng.csr_structure()
        rowptr, colind = csr[0], csr[1]
        ex = parallel.InterfaceExchange.from_partition(mesh, order, bounds, rank, rowptr.cpu().numpy(),
                                                       colind.cpu().numpy(), l2g, device, torch.float64,
                                                       perm=eng.dof_permutation())
        assert ex.n_matrix > 0 and ex.n_vector > 0 and ex.k_idx.numel() > 0
        shards.append((eng, l2g, vals, f.reshape(-1), ex))
    assert len({(ex.n_matrix, ex.n_vector) for *_, ex in shards}) == 1  # one global interface numbering
    total = torch.zeros_like(shards[0][4].buffer)
    for _, _, vals, f, ex in shards:
        total += ex.pack(vals, f)
    for rank, (eng, l2g, vals, f, ex) in enumerate(shards):
        ex.buffer.copy_(total)
        ex.unpack(vals, f)
        m = eng.wrap_csr(vals).caller_numbering()
        crow, cols = m.crow_indices.cpu().numpy(), m.col_indices.cpu().numpy().astype(np.int64)
        rows = np.repeat(np.arange(l2g.shape[0]), np.diff(crow))
        want = whole["dense"][l2g[rows], l2g[cols]]
        group = f"shards world={world} renumber={int(renumber)} rank={rank}"
        _note(group + " K scaled", scaled_error(_host(m.values), want), 1e-12)
        _note(group + " K rowwise", rowwise_error(_host(m.values), want, crow), 1e-12)
        _note(group + " f scaled", scaled_error(_host(f), whole["f"][l2g]), 1e-12)
    assert any(eng.renumbered for eng, *_ in shards) == renumber


def test_strip_interfaces_refuse_a_renumbered_engine(monkeypatch):
    from pytorch_fem_solver_amd import meshgen, parallel
    from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

    _renumber(monkeypatch, True)
    strip = meshgen.structured_rectangle(8, 8, 0.0, 1.0, 0.0, 1.0, jitter=0.0)
    tris = torch.tensor(strip["triangles"])
    eng = AssemblyEngine(torch.tensor(strip["vertices"]), tris, tris, 81, 1, ORDER)
    assert eng.renumbered
    with pytest.raises(NotImplementedError, match="renumbered"):
        parallel.InterfaceExchange.for_strips(strip, 0, 2, eng)
