"""Generated source programs through every device interpreter (-m gpu), against the longdouble
reference evaluator with its error bound (tests/source_reference.py):
  * pointwise: tfem_source_eval (src_run), f64 and f32, orders 1 - 4
  * load vectors: the ring launch with the program inside (chunked tiles after Morton
    renumbering, Z-order tiles on the native numbering; the wide interpreter for programs of
    depth <= 2, the general one for depth 3 - 4), the tile / gather / atomic kernels and
    TFEM_DETERMINISTIC=1 behind tfem_source_eval, the residual launch, and P2
  * meshes with one element, with holes and shifted to [-3, 5]^2.
TFEM_FUZZ_SEEDS=n widens the sweep (n programs of each kind)."""

import os

import numpy as np
import pytest
import torch

import source_reference as sr

pytestmark = pytest.mark.gpu

N_PROGRAMS = int(os.environ.get("TFEM_FUZZ_SEEDS", "24"))
DTYPES = {torch.float64: np.float64, torch.float32: np.float32}

#: path -> {dtype name: largest |error| / bound seen}; the last test prints it and checks it
RATIOS = {}
#: src_depth classes ("wide" <= 2, "general" 3-4) of the programs the ring launches ran
RING_DEPTHS = set()
#: path -> {(dtype name, ops, peak depth)} of the programs it ran
PROGRAMS = {}


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


_MESHES = {}


def _mesh(name):
    """(vertices float64, triangles int32) of the named test mesh."""
    if name not in _MESHES:
        from pytorch_fem_solver_amd import meshgen

        if name in ("morton", "native"):  # ~10k elements: tiles whose waves run 1, 2 and 3 rounds
            m = meshgen.delaunay_square(5000, 12)
            if name == "morton":
                m = meshgen.permute_mesh(m, vertex_order=meshgen.morton_order(m["vertices"]))
            verts, tris = m["vertices"], m["triangles"]
        elif name == "shifted":  # [-3, 5]^2 with holes: open fans, isolated vertices
            m = meshgen.delaunay_square(1500, 7)
            keep = np.random.default_rng(7).random(m["triangles"].shape[0]) >= 0.12
            verts, tris = m["vertices"] * 8.0 - 3.0, m["triangles"][keep]
        elif name == "single":
            verts, tris = np.array([[0.3, -1.2], [2.5, 0.4], [-0.7, 1.9]]), np.array([[0, 1, 2]])
        else:
            raise KeyError(name)
        _MESHES[name] = (np.ascontiguousarray(verts, dtype=np.float64), np.ascontiguousarray(tris, dtype=np.int32))
    return _MESHES[name]


_ENGINES = {}


def _engine(mesh, kernel, dtype, order):
    key = (mesh, kernel, dtype, order)
    if key not in _ENGINES:
        from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

        verts, tris = _mesh(mesh)
        idx = torch.tensor(tris)
        eng = AssemblyEngine(torch.tensor(verts, dtype=dtype), idx, idx, verts.shape[0], 1, order)
        eng.kernel = kernel
        assert not eng.renumbered
        _ENGINES[key] = eng
    return _ENGINES[key]


def _record(path, dtype, ratio, ops=None):
    name = "f64" if dtype == torch.float64 else "f32"
    if ops is not None:
        PROGRAMS.setdefault(path, set()).add((name, tuple(ops), sr.depth_profile(ops)[0]))
    slot = RATIOS.setdefault(path, {})
    slot[name] = max(slot.get(name, 0.0), ratio)


def _check_values(got, value, bound, decided, what):
    """|got - value| <= bound at the decided finite points, non-finite values matched exactly."""
    got = got.detach().cpu().double().numpy().reshape(value.shape).astype(sr.LD)
    finite = decided & np.isfinite(value)
    nonfinite = decided & ~np.isfinite(value)
    g, v = got[nonfinite], value[nonfinite]
    assert np.array_equal(np.isnan(g), np.isnan(v)), (what, "NaN where the reference has none or misses one")
    assert np.array_equal(g[~np.isnan(v)], v[~np.isnan(v)]), (what, "inf of the wrong sign")
    with np.errstate(all="ignore"):
        err = np.abs(got[finite] - value[finite])
    b = bound[finite]
    assert np.isfinite(err).all(), (what, "non-finite where the reference is finite")
    assert (err[b == 0] == 0).all(), what
    ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    assert ratio <= 1.0, (what, ratio)
    return ratio


def _check_load(got, f, tol, what):
    got = got.detach().cpu().double().numpy().reshape(-1).astype(sr.LD)
    assert got.shape == f.shape, what
    err = np.abs(got - f)
    assert np.isfinite(err).all(), what
    assert (err[tol == 0] == 0).all(), what
    ratio = float((err[tol > 0] / tol[tol > 0]).max())
    assert ratio <= 1.0, (what, ratio)
    return ratio


def _cells(mesh, np_dtype):
    verts, tris = _mesh(mesh)
    return verts.astype(np_dtype)[tris]


def _depth_class(ops):
    return "wide" if sr.depth_profile(ops)[0] <= 2 else "general"


# ------------------------------------------------------------------------------------------
# pointwise: tfem_source_eval
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(N_PROGRAMS))
def test_pointwise_values_within_the_bound(index):
    for order in (1, 2, 3, 4):
        ops, consts = sr.pointwise_program(index, _cells("shifted", np.float64), order)
        program = sr.to_native(ops, consts)
        for dtype, np_dtype in DTYPES.items():
            eng = _engine("shifted", "auto", dtype, order)
            value, bound, decided = sr.evaluate(ops, consts, _cells("shifted", np_dtype), order, np_dtype)
            got = eng.source_values(program)
            assert got.dtype == dtype and tuple(got.shape) == value.shape
            ratio = _check_values(got, value, bound, decided, (index, order, str(dtype), ops, consts))
            _record("pointwise", dtype, ratio, ops)
            # the same away from the points whose bound says little (f32 sin / cos of ~1e9: the bound
            # is the function's range)
            sharp = decided & np.isfinite(value) & (bound <= 1e-6 * np.maximum(np.abs(value), 1))
            if sharp.any():
                _record("pointwise_sharp", dtype, _check_values(got, value, bound, sharp, "sharp"))


# ------------------------------------------------------------------------------------------
# load vectors
# ------------------------------------------------------------------------------------------
def _reference_load(mesh, ops, consts, order, np_dtype):
    verts, tris = _mesh(mesh)
    cells = _cells(mesh, np_dtype)
    value, bound, decided = sr.evaluate(ops, consts, cells, order, np_dtype)
    assert decided.all() and np.isfinite(value).all()
    return sr.load_reference(value, bound, cells, tris, verts.shape[0], 1, order, np_dtype)


def _ring_engine(mesh, dtype, order):
    eng = _engine(mesh, "auto" if mesh == "morton" else "rings", dtype, order)
    assert eng._rings_take_source() and eng.kernel_name() == "k_p1_rings"
    assert eng.ring_plan()["chunked"] == (mesh == "morton")
    return eng


@pytest.mark.parametrize("index", range(N_PROGRAMS))
def test_load_vectors_of_every_path_within_the_tolerance(index, monkeypatch):
    order = 1 + (index // 4) % 4  # the depths cycle with the index: every (depth, order) in 16 programs
    ops, consts = sr.load_program(index, _cells("morton", np.float64), order)
    program = sr.to_native(ops, consts)
    for dtype, np_dtype in DTYPES.items():
        f, tol = _reference_load("morton", ops, consts, order, np_dtype)
        what = (index, order, str(dtype), ops, consts)
        # the ring launch with the program inside: chunked tiles, then Z-order tiles (15-slot records)
        for mesh in ("morton", "native"):
            eng = _ring_engine(mesh, dtype, order)
            if mesh == "native":
                f, tol = _reference_load("native", ops, consts, order, np_dtype)
            got = eng.load_source(program)
            _record(f"rings_{mesh}", dtype, _check_load(got, f, tol, ("rings", mesh) + what), ops)
            vals, f2 = eng.assemble_system(1.0, 0.5, source=program)
            _record(f"rings_{mesh}_fused", dtype, _check_load(f2, f, tol, ("fused", mesh) + what), ops)
            want_k = eng.bilinear(1.0, 0.5)
            if dtype == torch.float64:
                assert torch.equal(vals, want_k), ("fused K", mesh) + what
            else:  # hipcc contracts the two code shapes differently: last-bit differences
                assert float((vals - want_k).abs().max()) <= 3e-7 * float(want_k.abs().max()), ("fused K", mesh) + what
            RING_DEPTHS.add(_depth_class(ops))
        f, tol = _reference_load("morton", ops, consts, order, np_dtype)
        # tfem_source_eval in front of the kernels that read source values
        for kernel, name in (("tiles", "k_p1_tiles_pipe"), ("gather", "k_p1_bilinear_atomic"),
                             ("atomic", "k_p1_bilinear_atomic")):
            eng = _engine("morton", kernel, dtype, order)
            assert not eng._rings_take_source() and eng.kernel_name() == name
            _record(kernel, dtype, _check_load(eng.load_source(program), f, tol, (kernel,) + what), ops)
            _, f2 = eng.assemble_system(1.0, 0.0, source=program)
            _record(kernel, dtype, _check_load(f2, f, tol, (kernel, "system") + what))
        eng = _engine("morton", "auto", dtype, order)
        with monkeypatch.context() as m:
            m.setenv("TFEM_DETERMINISTIC", "1")
            assert not eng._rings_take_source()
            _, f2 = eng.assemble_system(1.0, 0.5, source=program)
            _record("deterministic", dtype, _check_load(f2, f, tol, ("deterministic",) + what), ops)
        # the residual launch (src_run inside tfem_p1_residual_local) + the gather
        got = eng.residual(None, program, None, 1.0)
        _record("residual", dtype, _check_load(got, f, tol, ("residual",) + what), ops)


@pytest.mark.parametrize("index", range(N_PROGRAMS))
def test_load_vectors_on_small_and_shifted_meshes(index):
    """One element; a mesh with holes on [-3, 5]^2: whatever path the engine picks, and the residual."""
    order = 1 + (index // 4 + 2) % 4
    for mesh in ("shifted", "single"):
        ops, consts = sr.load_program(index, _cells(mesh, np.float64), order)
        program = sr.to_native(ops, consts)
        for dtype, np_dtype in DTYPES.items():
            f, tol = _reference_load(mesh, ops, consts, order, np_dtype)
            eng = _engine(mesh, "auto", dtype, order)
            what = (mesh, eng.kernel_name(), index, order, str(dtype), ops, consts)
            _record(f"{mesh}:{eng.kernel_name()}", dtype, _check_load(eng.load_source(program), f, tol, what), ops)
            _, f2 = eng.assemble_system(1.0, 0.0, source=program)
            _check_load(f2, f, tol, what)
            got = eng.residual(None, program, None, 1.0)
        _record("residual", dtype, _check_load(got, f, tol, ("residual",) + what), ops)


_P2 = {}


@pytest.mark.parametrize("index", range(N_PROGRAMS))
def test_p2_load_vector_within_the_tolerance(index):
    from pytorch_fem_solver_amd import dofs, meshgen
    from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

    if not _P2:
        m = meshgen.delaunay_square(1200, 9)
        m = meshgen.permute_mesh(m, vertex_order=meshgen.morton_order(m["vertices"]))
        edges, on_boundary = meshgen._edges_from_triangles(m["triangles"])
        conn6, xy, _ = dofs.p2_dofs_numpy(m["vertices"], m["triangles"], edges,
                                          on_boundary.astype(np.int32).reshape(-1, 1), m["vertex_markers"])
        _P2.update(verts=m["vertices"], tris=m["triangles"].astype(np.int32), conn6=conn6, n=xy.shape[0])
    order = 1 + (index // 4 + 1) % 4
    cells64 = _P2["verts"][_P2["tris"]]
    ops, consts = sr.load_program(index, cells64, order)
    program = sr.to_native(ops, consts)
    for dtype, np_dtype in DTYPES.items():
        cells = _P2["verts"].astype(np_dtype)[_P2["tris"]]
        value, bound, decided = sr.evaluate(ops, consts, cells, order, np_dtype)
        f, tol = sr.load_reference(value, bound, cells, _P2["conn6"], _P2["n"], 2, order, np_dtype)
        eng = AssemblyEngine(torch.tensor(_P2["verts"], dtype=dtype), torch.tensor(_P2["tris"]),
                             torch.tensor(_P2["conn6"]), _P2["n"], 2, order)
        assert not eng.renumbered and eng.kernel_name() == "k_p2_rows"
        got = eng.load_source(program)
        _record("p2_rows", dtype, _check_load(got, f, tol, ("p2", index, order, str(dtype), ops)), ops)


# ------------------------------------------------------------------------------------------
# what the sweep reached
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["morton", "native"])
def test_ring_meshes_have_waves_of_one_two_and_three_rounds(mesh):
    """compute_g: wave w of a tile runs ceil((n_tv - 64 w') / 256) rounds of the interpreter (w' the
    rotated wave): the ring meshes of the sweep must give all of 1, 2 and 3."""
    from pytorch_fem_solver_amd.basis.engine import unpack_ring_plan

    eng = _ring_engine(mesh, torch.float64, 3)
    plan = eng.ring_plan()
    desc = unpack_ring_plan(plan["blob"].cpu().numpy().tobytes(), plan["layout"])["desc"].reshape(-1, 20)
    n_tv = desc[:, 18].astype(np.int64) >> 8
    rounds = {int(r) for w in range(4) for r in -((-(n_tv - 64 * w)) // 256) if r > 0}
    assert {1, 2, 3} <= rounds, rounds


def test_sweep_reached_both_ring_interpreters_and_stayed_inside_the_bounds():
    """Runs last: the ring launches saw depth <= 2 (wide interpreter) and depth 3-4 (general)
    programs; every path's largest |error| / bound is below 1 and above 0 (the check is not vacuous)."""
    if not RATIOS:  # run alone: nothing to look at
        return
    for path, by_type in sorted(RATIOS.items()):
        ran = PROGRAMS.get(path, set())
        depths = sorted({d for _, _, d in ran})
        print(f"[source programs] {path:28s} " + "  ".join(f"{k} {v:.3e}" for k, v in sorted(by_type.items()))
              + (f"  programs {len({o for _, o, _ in ran})} depths {depths}" if ran else ""))
    if any(p.startswith("rings_") for p in RATIOS):
        assert RING_DEPTHS == {"wide", "general"}, RING_DEPTHS
    for path, by_type in RATIOS.items():
        for name, ratio in by_type.items():
            assert ratio <= 1.0, (path, name, ratio)
            if not path.startswith("single"):  # one element: a handful of values may be exact
                assert ratio > 0.0, (path, name)
