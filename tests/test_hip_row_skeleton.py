"""The row, stage and store phases of the straight-line fused K + f launch (-m gpu; the SEP instantiations of
csrc/tfem_rings_kernel.hpp): with consecutive-vertex tiles and 7-slot records a wave's K entries leave through a
descriptor of the run's own (base: the run's first CSR entry, length: its whole pairs of entries, the lone last
entry of an odd run through a second one), the own-row coordinate load and the f store take their offsets from
the tile descriptor's first vertex, a regular wave is recognised by one masked compare and skips the band and
long-row tests, and the accumulators are zeroed by one store per lane.  What can go wrong there shows in the
waves listed under CASES, so every plan is asked -- from its descriptor words and row records -- to hold the
cases it is here for; a plan without them fails instead of passing.

Plans (TFEM_RING_WGS=8, fp64, order 3): the one-element mesh; S(40), S(64), S(130) and S(129) (S(130) has no
all-regular wave with an odd row count, its chunks are 44 rows; S(129) has 43-row ones); S(63) in Z-order
tiles; a vertex-shuffled S(30) (row offsets from memory); the Morton-numbered 5000-point Delaunay mesh (15-slot
records).  Per plan, without and with a mass term, K + f and f alone, every output an out= view into a larger
buffer filled with a sentinel:
  K       bit for bit the matrix-only launch's
  f       inside the bound of the numpy model (tests/source_reference.py); against the interpreter route
          (TFEM_RINGS_SEPARABLE=0) at the route-to-route bound of tests/test_hip_tile_descriptors.py
  padding both sides of vals and f untouched."""

import ctypes

import numpy as np
import pytest
import torch

import source_reference as sr
from conftest import scaled_error
from test_hip_tile_descriptors import CONSTS, OPS, ORDER, TOL_ROUTES

pytestmark = pytest.mark.gpu

PAD = 37          # entries of padding on both sides (odd: the views start on 8 bytes, not on 16)
SENTINEL = -7.25e300
BETAS = (0.0, 0.7)

#: what each plan is here for (asserted from the plan itself)
CASES = {
    "single": {"chunked": True, "slots": 7, "has": ("empty_wave", "run_of_one")},
    "S40": {"chunked": False, "slots": 7, "has": ("mixed_wave", "run_of_one")},
    "S64": {"chunked": True, "slots": 7, "has": ("mixed_wave", "empty_wave", "run_of_five")},
    "S130": {"chunked": True, "slots": 7, "has": ("mixed_wave", "even_regular_wave", "run_of_five")},
    "S129": {"chunked": True, "slots": 7, "has": ("odd_regular_wave", "mixed_wave", "run_of_five")},
    "S63": {"chunked": False, "slots": 7, "has": ("mixed_wave",)},
    "shuffled": {"chunked": False, "slots": 7, "has": ("mixed_wave", "run_of_one")},
    "morton": {"chunked": True, "slots": 15, "has": ("empty_wave",)},
}
MESHES = tuple(CASES)


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
    if name not in _MESHES:
        from pytorch_fem_solver_amd import meshgen

        kernel = "auto"
        if name == "single":
            verts, tris, kernel = np.array([[0.3, -1.2], [2.5, 0.4], [-0.7, 1.9]]), np.array([[0, 1, 2]]), "rings"
        elif name == "shuffled":
            m = meshgen.unit_square(30, 0.25, 0)
            m = meshgen.permute_mesh(m, vertex_order=np.random.default_rng(3).permutation(m["vertices"].shape[0]))
            verts, tris, kernel = m["vertices"], m["triangles"], "rings"
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


def _engine(mesh, monkeypatch):
    if mesh not in _ENGINES:
        from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

        monkeypatch.setenv("TFEM_RING_WGS", "8")
        verts, tris, kernel = _mesh(mesh)
        idx = torch.tensor(tris)
        eng = AssemblyEngine(torch.tensor(verts, dtype=torch.float64), idx, idx, verts.shape[0], 1, ORDER)
        eng.kernel = kernel
        assert not eng.renumbered and eng.ring_plan() is not None
        assert eng._rings_take_source() and eng.kernel_name() == "k_p1_rings"
        _ENGINES[mesh] = eng
    return _ENGINES[mesh]


def _plan_cases(eng):
    """The cases a plan holds, from its tile descriptors (20 ints: [3..7] the waves' row bounds), its 7-slot row
    records (k in the top bits of words 0 and 1, the flags in bits 10..23 of word 2) and its run list."""
    from pytorch_fem_solver_amd.basis.engine import unpack_ring_plan

    plan = eng.ring_plan()
    p = unpack_ring_plan(plan["blob"].cpu().numpy().tobytes(), plan["layout"])
    desc, found = p["desc"].reshape(-1, 20), set()
    rows = p["rows"].reshape(-1, p["words"])
    for t in desc:
        for w in range(4):
            r0, r1 = int(t[3 + w]), int(t[4 + w])
            if r1 == r0:
                if t[7] > 0:
                    found.add("empty_wave")
                continue
            if p["slots"] != 7:
                continue
            rec = rows[t[2] + r0:t[2] + r1]
            regular = (((rec[:, 2] & 0xFFFC00) == (0x555 << 10)) & ((rec[:, 0] >> 30) == 2)
                       & (((rec[:, 1] >> 30) & 1) == 1))
            if regular.all():
                found.add("odd_regular_wave" if (r1 - r0) % 2 else "even_regular_wave")
            elif regular.any():
                found.add("mixed_wave")
    assert p["n_runs"] > 0
    lengths = np.diff(p["runs"])
    if (lengths == 1).any():
        found.add("run_of_one")
    if (lengths >= 5).any():
        found.add("run_of_five")
    return bool(p["chunked"]), int(p["slots"]), found


def _route(eng, program):
    coords = eng._inputs()["coords"]
    layout = eng.ring_plan()["layout"]
    return eng.lib.tfem_p1_rings_source_route(ctypes.c_void_p(coords.data_ptr()), eng.real_bytes, eng.quad_order,
                                              ctypes.c_void_p(layout.ctypes.data), ctypes.byref(program))


def _model(mesh):
    """(f, tolerance) of the numpy model, once per mesh."""
    if mesh not in _WANT:
        verts, tris, _ = _mesh(mesh)
        cells = verts[tris]
        value, bound, decided = sr.evaluate(OPS, CONSTS, cells, ORDER, np.float64)
        assert decided.all() and np.isfinite(value).all()
        _WANT[mesh] = sr.load_reference(value, bound, cells, tris, verts.shape[0], 1, ORDER, np.float64)
    return _WANT[mesh]


def _padded(n):
    """(the whole buffer, the out= view of n entries inside it)"""
    whole = torch.full((n + 2 * PAD,), SENTINEL)
    return whole, whole[PAD:PAD + n]


def _padding_untouched(whole):
    return bool((whole[:PAD] == SENTINEL).all()) and bool((whole[-PAD:] == SENTINEL).all())


def _run(mesh, beta, monkeypatch):
    """The launches of one plan and mass term, once: K + f and f alone into padded buffers, the matrix-only launch,
    K + f on the interpreter route."""
    key = (mesh, beta)
    if key not in _RUNS:
        eng = _engine(mesh, monkeypatch)
        program = sr.to_native(OPS, CONSTS)
        nnz, n = int(eng.csr_structure()[1].shape[0]), eng.n_dofs
        (vals_all, vals), (f_all, f), (g_all, g) = _padded(nnz), _padded(n), _padded(n)
        eng.assemble_system(1.0, beta, source=program, out=(vals, f))
        route = _route(eng, program)  # (behind the first launch: the engine vouches for its coordinates there)
        eng.load_source(program, out=g)
        want_k = eng.bilinear(1.0, beta)
        with monkeypatch.context() as m:
            m.setenv("TFEM_RINGS_SEPARABLE", "0")
            route_off = _route(eng, program)
            _, f_interp = eng.assemble_system(1.0, beta, source=program)
        torch.cuda.synchronize()
        _RUNS[key] = dict(route=route, route_off=route_off, vals_all=vals_all, vals=vals, f_all=f_all, f=f, g_all=g_all,
                          g=g, want_k=want_k.view(-1), f_interp=f_interp.reshape(-1))
    return _RUNS[key]


def _model_ratio(f, mesh):
    want, tol = _model(mesh)
    got = f.detach().cpu().double().numpy().reshape(-1).astype(sr.LD)
    assert got.shape == want.shape
    err = np.abs(got - want)
    assert np.isfinite(err).all()
    assert (err[tol == 0] == 0).all()
    return float((err[tol > 0] / tol[tol > 0]).max())


@pytest.mark.parametrize("mesh", MESHES)
def test_plan_holds_its_cases(mesh, monkeypatch):
    chunked, slots, found = _plan_cases(_engine(mesh, monkeypatch))
    print(f"{mesh}: consecutive-vertex tiles {chunked}, {slots} slots, {sorted(found)}")
    want = CASES[mesh]
    assert chunked == want["chunked"] and slots == want["slots"]
    assert set(want["has"]) <= found, (mesh, sorted(set(want["has"]) - found))


def test_every_case_occurs_with_consecutive_vertex_tiles(monkeypatch):
    """The descriptor stores are those of consecutive-vertex tiles with 7-slot records: all five cases there."""
    found = set()
    for mesh, want in CASES.items():
        if want["chunked"] and want["slots"] == 7:
            found |= _plan_cases(_engine(mesh, monkeypatch))[2]
    assert {"odd_regular_wave", "mixed_wave", "empty_wave", "run_of_one", "run_of_five"} <= found, sorted(found)


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("mesh", MESHES)
def test_matrix_is_the_matrix_only_launch_and_padding_untouched(mesh, beta, monkeypatch):
    r = _run(mesh, beta, monkeypatch)
    assert r["route"] == 2 and r["route_off"] == 1
    assert torch.equal(r["vals"], r["want_k"])
    assert _padding_untouched(r["vals_all"]) and _padding_untouched(r["f_all"]) and _padding_untouched(r["g_all"])


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("mesh", MESHES)
def test_load_vectors_inside_the_model_bound(mesh, beta, monkeypatch):
    r = _run(mesh, beta, monkeypatch)
    fused, alone = _model_ratio(r["f"], mesh), _model_ratio(r["g"], mesh)
    print(f"{mesh} beta {beta}: largest |error| / bound, K + f {fused:.3e}, f alone {alone:.3e}")
    assert fused <= 1.0 and alone <= 1.0


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("mesh", MESHES)
def test_load_vectors_against_the_interpreter_route(mesh, beta, monkeypatch):
    r = _run(mesh, beta, monkeypatch)
    fused = scaled_error(r["f"].cpu(), r["f_interp"].cpu())
    alone = scaled_error(r["g"].cpu(), r["f_interp"].cpu())
    print(f"{mesh} beta {beta}: against TFEM_RINGS_SEPARABLE=0, K + f {fused:.3e}, f alone {alone:.3e}")
    assert fused <= TOL_ROUTES and alone <= TOL_ROUTES
