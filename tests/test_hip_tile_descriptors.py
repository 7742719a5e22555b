"""The per-tile buffer descriptors of the fused K + f launch's tile loop (-m gpu; kTileDesc in
csrc/tfem_rings_kernel.hpp): the SEP instantiations read a tile's row records, hand-ins, element table and
vertex ids through descriptors whose base is the wave's first entry and whose length is the wave's count, so
a lane past the count gets its zeros from the range check alone.  That can go wrong where a wave has fewer
entries than lanes and where a count is no multiple of 64, so the meshes are those whose plans have such
tiles: one element; the Delaunay mesh with holes and isolated vertices on [-3, 5]^2 and the Morton-numbered
5000-point Delaunay mesh of tests/test_hip_source_programs.py (15-slot records); S(40), S(63), S(64), S(130)
(7-slot records: first, last and partial tiles, chunks of fewer than 64 rows).  TFEM_RING_WGS=8, so that a
workgroup walks several tiles and the loads of the loop -- not only the prologue's -- are the ones checked.

Per mesh, fp64 and fp32 (the fp32 launches run the interpreter kernels, which keep the shared descriptor):
the plan has a tile with fewer than 256 rows (S(63) cannot: 4096 vertices are sixteen full tiles, which is
asserted instead) and one whose evaluated count is no multiple of 64; K of the
fused launch is the matrix-only launch's (fp64: bit for bit; fp32: 3e-7, tests/test_hip_source_programs.py);
f is inside the bound of the numpy model (tests/source_reference.py); fp64: the launch took route 2 and its f
is the interpreter route's (TFEM_RINGS_SEPARABLE=0) at the route-to-route 1e-14 of
tests/test_hip_fused_separable.py.  One plan with flagged vertices is launched over its two tile ranges:
a descriptor at the end of a range is where the clipping matters."""

import ctypes

import numpy as np
import pytest
import torch

import source_reference as sr
from conftest import scaled_error
from oracle import assembly_oracle as orc

pytestmark = pytest.mark.gpu

TOL_ROUTES = 1e-14   # one route against another (tests/test_hip_fused_separable.py)
TOL_K_F32 = 3e-7     # fp32 K, fused against matrix-only (tests/test_hip_source_programs.py)
ORDER = 3            # four points: the rule of the SEP instantiations

MESHES = ("single", "shifted", "morton", "S40", "S63", "S64", "S130")
FULL_TILES_ONLY = "S63"  # the one mesh whose plan cannot have a tile with fewer than 256 rows (below)
DTYPES = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
#: cos(1.2 x) sin(2.5 y): separable, every argument on [-3, 5]^2 inside the proven range
OPS = [orc.SRC_PUSH_X, orc.SRC_COS, orc.SRC_PUSH_Y, orc.SRC_SIN, orc.SRC_MUL]
CONSTS = [1.2, 1.0, 2.5, 1.0, 0.0]


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


_MESHES, _ENGINES, _RUNS, _WANT = {}, {}, {}, {}


def _mesh(name):
    """(vertices float64, triangles int32, the engine's kernel choice)"""
    if name not in _MESHES:
        from pytorch_fem_solver_amd import meshgen

        kernel = "auto"
        if name == "single":
            verts, tris, kernel = np.array([[0.3, -1.2], [2.5, 0.4], [-0.7, 1.9]]), np.array([[0, 1, 2]]), "rings"
        elif name == "shifted":
            m = meshgen.delaunay_square(1500, 7)
            keep = np.random.default_rng(7).random(m["triangles"].shape[0]) >= 0.12
            verts, tris, kernel = m["vertices"] * 8.0 - 3.0, m["triangles"][keep], "rings"
        elif name == "morton":
            m = meshgen.delaunay_square(5000, 12)
            m = meshgen.permute_mesh(m, vertex_order=meshgen.morton_order(m["vertices"]))
            verts, tris = m["vertices"], m["triangles"]
        else:
            m = meshgen.unit_square(int(name[1:]), 0.25, 0)
            verts, tris = m["vertices"], m["triangles"]
        _MESHES[name] = (np.ascontiguousarray(verts, dtype=np.float64), np.ascontiguousarray(tris, dtype=np.int32),
                         kernel)
    return _MESHES[name]


def _engine(mesh, dtype, monkeypatch, flags=None):
    key = (mesh, dtype, flags is not None)
    if key not in _ENGINES:
        from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

        monkeypatch.setenv("TFEM_RING_WGS", "8")
        verts, tris, kernel = _mesh(mesh)
        idx = torch.tensor(tris)
        eng = AssemblyEngine(torch.tensor(verts, dtype=DTYPES[dtype][0]), idx, idx, verts.shape[0], 1, ORDER)
        eng.kernel = kernel
        if flags is not None:
            eng.set_priority_vertices(flags)
        assert not eng.renumbered and eng.ring_plan() is not None
        assert eng._rings_take_source() and eng.kernel_name() == "k_p1_rings"
        _ENGINES[key] = eng
    return _ENGINES[key]


def _tiles(eng):
    """(rows, evaluated elements) per tile of the engine's plan."""
    from pytorch_fem_solver_amd.basis.engine import unpack_ring_plan

    plan = eng.ring_plan()
    desc = unpack_ring_plan(plan["blob"].cpu().numpy().tobytes(), plan["layout"])["desc"].reshape(-1, 20)
    return desc[:, 7].astype(np.int64), desc[:, 18].astype(np.int64) >> 8


def _assert_partial_tiles(eng, what):
    rows, n_tv = _tiles(eng)
    print(f"{what}: {rows.size} tiles, rows {rows.min()}..{rows.max()}, evaluated {n_tv.min()}..{n_tv.max()}, "
          f"{int((rows < 256).sum())} with < 256 rows, {int((n_tv % 64 != 0).sum())} evaluating no multiple of 64")
    assert (n_tv % 64 != 0).any(), (what, "every evaluated count is a multiple of 64")
    if what.startswith(FULL_TILES_ONLY):
        # 64^2 = 4096 vertices in Z-order tiles: sixteen tiles of exactly 256 rows -- there is no partial tile
        # this plan could hold; its counts of evaluated elements (480 .. 576) are what it adds
        assert rows.size == 16 and (rows == 256).all(), what
    else:
        assert (rows < 256).any(), (what, "no tile with fewer than 256 rows")


def _route(eng, program):
    coords = eng._inputs()["coords"]
    layout = eng.ring_plan()["layout"]
    return eng.lib.tfem_p1_rings_source_route(ctypes.c_void_p(coords.data_ptr()), eng.real_bytes, eng.quad_order,
                                              ctypes.c_void_p(layout.ctypes.data), ctypes.byref(program))


def _model(mesh, dtype):
    """(f, tolerance) of the numpy model, once per mesh and type."""
    key = (mesh, dtype)
    if key not in _WANT:
        verts, tris, _ = _mesh(mesh)
        np_dtype = DTYPES[dtype][1]
        cells = verts.astype(np_dtype)[tris]
        value, bound, decided = sr.evaluate(OPS, CONSTS, cells, ORDER, np_dtype)
        assert decided.all() and np.isfinite(value).all()
        _WANT[key] = sr.load_reference(value, bound, cells, tris, verts.shape[0], 1, ORDER, np_dtype)
    return _WANT[key]


def _run(mesh, dtype, monkeypatch):
    """The fused launch, the matrix-only launch and the fused launch on the interpreter route, once per case."""
    key = (mesh, dtype)
    if key not in _RUNS:
        eng = _engine(mesh, dtype, monkeypatch)
        _assert_partial_tiles(eng, f"{mesh} {dtype}")
        program = sr.to_native(OPS, CONSTS)
        vals, f = eng.assemble_system(1.0, 0.0, source=program)
        route = _route(eng, program)  # (behind the first launch: the engine vouches for its coordinates there)
        want_k = eng.bilinear(1.0, 0.0)
        with monkeypatch.context() as m:
            m.setenv("TFEM_RINGS_SEPARABLE", "0")
            route_off = _route(eng, program)
            _, f_interp = eng.assemble_system(1.0, 0.0, source=program)
        torch.cuda.synchronize()
        _RUNS[key] = (route, route_off, vals.clone(), f.reshape(-1).clone(), want_k.clone(),
                      f_interp.reshape(-1).clone())
    return _RUNS[key]


def _model_ratio(f, mesh, dtype):
    want, tol = _model(mesh, dtype)
    got = f.detach().cpu().double().numpy().reshape(-1).astype(sr.LD)
    assert got.shape == want.shape
    err = np.abs(got - want)
    assert np.isfinite(err).all()
    assert (err[tol == 0] == 0).all()
    return float((err[tol > 0] / tol[tol > 0]).max())


CASES = [(mesh, dtype) for mesh in MESHES for dtype in DTYPES]


@pytest.mark.parametrize("mesh", MESHES)
def test_fp64_launch_took_the_separable_route(mesh, monkeypatch):
    route, route_off, *_ = _run(mesh, "f64", monkeypatch)
    assert route == 2 and route_off == 1


@pytest.mark.parametrize("mesh,dtype", CASES)
def test_fused_matrix_is_the_matrix_only_launch(mesh, dtype, monkeypatch):
    _, _, vals, _, want_k, _ = _run(mesh, dtype, monkeypatch)
    if dtype == "f64":
        assert torch.equal(vals, want_k)
    else:  # hipcc contracts the two code shapes differently: last-bit differences
        assert float((vals - want_k).abs().max()) <= TOL_K_F32 * float(want_k.abs().max())


@pytest.mark.parametrize("mesh,dtype", CASES)
def test_load_vector_inside_the_model_bound(mesh, dtype, monkeypatch):
    _, _, _, f, _, _ = _run(mesh, dtype, monkeypatch)
    ratio = _model_ratio(f, mesh, dtype)
    print(f"{mesh} {dtype}: largest |error| / bound {ratio:.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("mesh", MESHES)
def test_load_vector_against_the_interpreter_route(mesh, monkeypatch):
    _, _, _, f, _, f_interp = _run(mesh, "f64", monkeypatch)
    err = scaled_error(f.cpu(), f_interp.cpu())
    print(f"{mesh}: against TFEM_RINGS_SEPARABLE=0 {err:.3e}")
    assert err <= TOL_ROUTES


@pytest.mark.parametrize("mesh", ["S130", "morton"])
def test_two_launches_over_the_tile_ranges(mesh, monkeypatch):
    verts, _, _ = _mesh(mesh)
    eng = _engine(mesh, "f64", monkeypatch, flags=verts[:, 0] < 0.3)
    _assert_partial_tiles(eng, f"{mesh} with flagged vertices")
    _, _, _, f, want_k, _ = _run(mesh, "f64", monkeypatch)
    (_, n_pri), (_, n_rest) = eng.tile_range("priority"), eng.tile_range("rest")
    assert n_pri > 0 and n_rest > 0
    program = sr.to_native(OPS, CONSTS)
    out = (torch.full((want_k.numel(),), float("nan")), torch.full((f.numel(),), float("nan")))
    eng.assemble_system(1.0, 0.0, source=program, out=out, tiles="priority")
    assert _route(eng, program) == 2
    torch.cuda.synchronize()
    assert torch.isnan(out[0]).any() and torch.isnan(out[1]).any()  # the other rows still untouched
    eng.assemble_system(1.0, 0.0, source=program, out=out, tiles="rest")
    assert torch.equal(out[0], want_k.view(-1))
    err, ratio = scaled_error(out[1].cpu(), f.cpu()), _model_ratio(out[1], mesh, "f64")
    print(f"{mesh}: two launches against one {err:.3e}, largest |error| / bound {ratio:.3e}")
    assert err <= TOL_ROUTES and ratio <= 1.0
