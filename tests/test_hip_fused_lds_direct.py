"""The fused K + f launch with the next tile's coordinates loaded straight into LDS (-m gpu): the fp64
source-program launches of the wide interpreter issue the coordinate loads of tile k + 1 in front of phase G of tile k, 16
bytes per lane into the other coordinate buffer, with no register and no copy in between.  What can
go wrong there is where a lane's pair lands and whether it has landed when the next tile reads it,
so the meshes are the smallest that reach every shape of a tile: many tiles per workgroup with two-
and three-element passes (7-slot records), the 15-slot records, one tile with fewer than 64 rows
(one partial wave, three waves without a row) and a last tile whose last wave is partial.  Programs:
the bench's sin * sin, x y + 1, the depth-3 program of tests/test_hip_fused_hot_loop.py (general
interpreter), one that pushes y before x and one that pushes a constant onto a non-empty stack;
Q = 1, 3, 4, 6; float32, whose launches keep the register path, as those of the general interpreter do
(depth-3 programs, Q = 6).

K must be bit for bit the matrix-only launch's K; f is held against the numpy oracle at the bounds
of tests/test_hip_fused_hot_loop.py (1e-12 norm-wise and entry-wise) and against the
TFEM_DETERMINISTIC=1 route at that file's 1e-14.

The same launches skip the range test of a sin / cos of a coordinate push when the host proves the
range from the engine's bound on the coordinates (tests/test_source_trig_proof.py has the proof
itself): at the end of the file the mesh is scaled so that the proof holds with arguments of 3e8 and
so that it fails (arguments on both sides of 1e9), both against tests/source_reference.py, and the
engine must withdraw its bound once the coordinate tensor has been written."""

import math

import numpy as np
import pytest
import torch

import source_reference as sr
from conftest import rowwise_error, scaled_error
from oracle import assembly_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-12            # tests/test_hip_fused_hot_loop.py: f against the oracle, norm-wise and entry-wise
TOL_ROUTES = 1e-14     # ... the default route against TFEM_DETERMINISTIC=1
TOL_FLOAT32 = 2e-6     # ... float32 load vectors

SHAPES = ("structured", "delaunay", "one_tile", "partial_wave")
PROGRAMS = ("sin_sin", "xy_plus_1", "depth_3", "y_then_x", "constant_push")


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


_MESHES, _ENGINES, _WANT, _RUNS = {}, {}, {}, {}


def _mesh(shape):
    if shape not in _MESHES:
        from pytorch_fem_solver_amd import meshgen

        if shape == "structured":      # 51 tiles, 15 of them with a three-element pass
            m = meshgen.unit_square(96, 0.25, 0)
        elif shape == "delaunay":      # 15-slot records
            m = meshgen.delaunay_square(4000, 3)
            m = meshgen.permute_mesh(m, vertex_order=meshgen.morton_order(m["vertices"]))
        elif shape == "one_tile":      # 25 vertices: one tile, fewer than 64 rows
            m = meshgen.unit_square(4)
        else:                          # 441 vertices: the last tile ends in a partial wave
            m = meshgen.unit_square(20)
        _MESHES[shape] = m
    return _MESHES[shape]


def _program(name, basis):
    from pytorch_fem_solver_amd.basis import forms

    if name == "sin_sin":  # the bench's source, traced like the bench traces it

        def load(b):
            x, y = torch.split(b.integration_points, 1, dim=-1)
            return 2.0 * math.pi**2 * torch.sin(math.pi * x) * torch.sin(math.pi * y) * b.v

        return forms.trace(load, basis, (), {}).coefficient.program()
    if name == "xy_plus_1":
        return forms.compile_program(("add", ("mul", ("x",), ("y",)), ("c", 1.0)))
    if name == "y_then_x":  # y + 3 x: the first push is y
        return forms.compile_program(("add", ("y",), ("mul", ("x",), ("c", 3.0))))
    if name == "constant_push":  # (x y + 1) / 4: the divisor is pushed on top of the operand
        return forms.compile_program(("div", ("add", ("mul", ("x",), ("y",)), ("c", 1.0)), ("c", 4.0)))
    # the depth-3 program of tests/test_hip_fused_hot_loop.py (positive on the unit square: the
    # entry-wise bound presumes that no element share cancels inside)
    return forms.compile_program(("add", ("mul", ("x",), ("y",)),
                                  ("mul", ("add", ("sin", ("x",)), ("c", 2.0)), ("add", ("y",), ("x",)))))


def _ops(program):
    n = int(program.n_ops)
    return [int(v) for v in program.ops[:n]], [float(v) for v in program.consts[:n]]


def _engine(shape, order, dtype, monkeypatch):
    """The basis and its engine, the ring plan built for eight resident workgroups."""
    key = (shape, order, dtype)
    if key not in _ENGINES:
        import pytorch_fem_solver_amd as tf

        monkeypatch.setenv("TFEM_RING_WGS", "8")
        torch.set_default_dtype(dtype)
        try:
            basis = tf.Basis(tf.MeshTri(_mesh(shape)), tf.ElementTri(1, order))
            eng = basis._engine
            assert eng.ring_plan() is not None and eng._rings_take_source()
        finally:
            torch.set_default_dtype(torch.float64)
        _ENGINES[key] = (basis, eng)
    return _ENGINES[key]


def _oracle_load(shape, order, name, program, np_dtype=np.float64):
    """(f, sum of the magnitudes of the element shares per entry) of the numpy oracle in float64, once,
    on the vertices as a launch of `np_dtype` holds them."""
    key = (shape, order, name, np_dtype)
    if key not in _WANT:
        m = _mesh(shape)
        ops, consts = _ops(program)
        source = lambda pts: orc.source_program_eval(ops, consts, pts[..., [0]], pts[..., [1]])  # noqa: E731
        vertices = m["vertices"].astype(np_dtype).astype(np.float64)
        local, _ = orc.p1_assemble(vertices, m["triangles"], order, "load", source=source)
        n = m["vertices"].shape[0]
        _WANT[key] = (orc.assemble_linear(local, m["triangles"], n).reshape(-1),
                      orc.assemble_linear(np.abs(local), m["triangles"], n).reshape(-1))
    return _WANT[key]


def _run(shape, order, name, dtype, monkeypatch):
    """One fused launch, the matrix-only launch and the deterministic route, once per case."""
    key = (shape, order, name, dtype)
    if key not in _RUNS:
        basis, eng = _engine(shape, order, dtype, monkeypatch)
        program = _program(name, basis)
        depth = sr.depth_profile(_ops(program)[0])[0]
        assert (depth == 3) if name == "depth_3" else (depth <= 2), (name, depth)
        vals, f = eng.assemble_system(1.0, 0.0, source=program)
        want_k = eng.bilinear(1.0, 0.0)
        with monkeypatch.context() as m:
            m.setenv("TFEM_DETERMINISTIC", "1")
            assert not eng._rings_take_source()
            _, f_det = eng.assemble_system(1.0, 0.0, source=program)
        assert eng._rings_take_source() and eng.kernel_name() == "k_p1_rings"
        _RUNS[key] = (program, vals.clone(), f.reshape(-1).clone(), want_k.clone(), f_det.reshape(-1).clone())
    return _RUNS[key]


CASES = ([(shape, 3, name) for shape in SHAPES for name in PROGRAMS]
         + [(shape, order, "sin_sin") for shape in ("structured", "partial_wave") for order in (1, 2, 4)])


def test_the_programs_push_what_their_names_say():
    from pytorch_fem_solver_amd.basis import forms

    names = {v: k for k, v in forms.OPS.items()}
    y_then_x = [names[o] for o in _ops(_program("y_then_x", None))[0]]
    pushes = [n for n in y_then_x if n.startswith("PUSH")]
    assert pushes == ["PUSH_Y", "PUSH_X"], y_then_x
    constant = [names[o] for o in _ops(_program("constant_push", None))[0]]
    at = constant.index("PUSH_C")
    depth = sum(n.startswith("PUSH") for n in constant[:at]) - sum(n in ("ADD", "SUB", "SUB_R", "MUL", "DIV", "DIV_R")
                                                                    for n in constant[:at])
    assert depth == 1, constant  # the constant lands on a non-empty stack


@pytest.mark.parametrize("shape", SHAPES)
def test_the_plans_have_the_tiles_the_cases_are_about(shape, monkeypatch):
    _, eng = _engine(shape, 3, torch.float64, monkeypatch)
    plan = eng.ring_plan()
    layout = [int(v) for v in plan["layout"]]
    tiles = layout[0]
    blob = plan["blob"].cpu().numpy()
    desc = blob[layout[8]:layout[8] + 80 * tiles].view(np.int32).reshape(tiles, 20)
    rows = desc[:, 4:8] - desc[:, 3:7]  # rows of the four waves of every tile
    evaluated = desc[:, 18] >> 8        # elements the tile evaluates itself
    assert plan["chunked"] and layout[6] == (15 if shape == "delaunay" else 7)
    assert int(rows.sum()) == _mesh(shape)["vertices"].shape[0]
    if shape == "structured":
        assert tiles == 51 and int((evaluated > 512).sum()) == 15
    elif shape == "one_tile":
        assert tiles == 1 and 0 < int(rows[0, 0]) < 64 and int(rows[0, 1:].sum()) == 0
    elif shape == "partial_wave":
        assert _mesh(shape)["vertices"].shape[0] == 441
        last = rows[-1]
        assert any(0 < int(r) < 64 for r in last), last


@pytest.mark.parametrize("shape,order,name", CASES)
def test_fused_matrix_is_bit_for_bit_the_matrix_only_launch(shape, order, name, monkeypatch):
    _, vals, _, want_k, _ = _run(shape, order, name, torch.float64, monkeypatch)
    assert torch.equal(vals, want_k)


@pytest.mark.parametrize("shape,order,name", CASES)
def test_fused_load_vector_against_the_oracle(shape, order, name, monkeypatch):
    program, _, f, _, _ = _run(shape, order, name, torch.float64, monkeypatch)
    want, scale = _oracle_load(shape, order, name, program)
    norm_wise, entry_wise = scaled_error(f.cpu(), want), rowwise_error(f.cpu(), want, scale=scale)
    print(f"{shape} order {order} {name}: norm-wise {norm_wise:.3e} entry-wise {entry_wise:.3e}")
    assert norm_wise <= TOL and entry_wise <= TOL


@pytest.mark.parametrize("shape,order,name", CASES)
def test_fused_load_vector_against_the_deterministic_route(shape, order, name, monkeypatch):
    _, _, f, _, f_det = _run(shape, order, name, torch.float64, monkeypatch)
    err = scaled_error(f.cpu(), f_det.cpu())
    print(f"{shape} order {order} {name}: against the deterministic route {err:.3e}")
    assert err <= TOL_ROUTES


@pytest.mark.parametrize("shape,name", [("structured", n) for n in PROGRAMS] + [("one_tile", "sin_sin"),
                                                                                 ("partial_wave", "sin_sin")])
def test_float32_load_vector_against_the_oracle(shape, name, monkeypatch):
    program, vals, f, want_k, f_det = _run(shape, 3, name, torch.float32, monkeypatch)
    assert vals.dtype == torch.float32 and f.dtype == torch.float32
    want, _ = _oracle_load(shape, 3, name, program, np.float32)
    err = scaled_error(f.cpu(), want)
    print(f"float32 {shape} {name}: {err:.3e}, against the deterministic route {scaled_error(f.cpu(), f_det.cpu()):.3e}")
    assert err <= TOL_FLOAT32 and scaled_error(f_det.cpu(), want) <= TOL_FLOAT32
    # float32: hipcc contracts the two code shapes differently (tests/test_hip_source.py)
    assert scaled_error(vals.cpu(), want_k.cpu()) <= 3e-7


# ------------------------------------------------------------------------------------------
# sin / cos of a coordinate push: range proven once per launch from the engine's coordinate bound
# ------------------------------------------------------------------------------------------
def _scaled_basis(scale, monkeypatch):
    import pytorch_fem_solver_amd as tf

    mesh = {k: np.array(v, copy=True) for k, v in _mesh("partial_wave").items()}
    mesh["vertices"] = mesh["vertices"] * scale
    monkeypatch.setenv("TFEM_RING_WGS", "8")
    basis = tf.Basis(tf.MeshTri(mesh), tf.ElementTri(1, 3))
    assert basis._engine.ring_plan() is not None and basis._engine._rings_take_source()
    return mesh, basis


def _launch_ops(eng, program, coords=None):
    """The operation codes a launch of `program` on the engine's plan hands its kernel."""
    import ctypes

    coords = eng._inputs()["coords"] if coords is None else coords
    ops = (ctypes.c_uint8 * 32)()
    layout = eng.ring_plan()["layout"]
    assert eng.lib.tfem_p1_rings_source_ops(ctypes.c_void_p(coords.data_ptr()), eng.real_bytes, eng.quad_order,
                                            ctypes.c_void_p(layout.ctypes.data), ctypes.byref(program), ops) == 0
    return list(ops)


@pytest.mark.parametrize("shape,order,dtype,proven", [("structured", 3, torch.float64, 2), ("delaunay", 3, torch.float64, 2),
                                                      ("structured", 1, torch.float64, 2), ("structured", 4, torch.float64, 0),
                                                      ("structured", 3, torch.float32, 0)])
def test_the_cases_above_ran_the_proven_sines_where_they_apply(shape, order, dtype, proven, monkeypatch):
    program = _run(shape, order, "sin_sin", dtype, monkeypatch)[0]
    _, eng = _engine(shape, order, dtype, monkeypatch)
    assert _launch_ops(eng, program).count(23) == proven and _launch_ops(eng, program).count(17) == 2 - proven


@pytest.mark.parametrize("scale,proven", [(1.0, 2), (1.0e8, 2), (4.0e8, 0)])
def test_scaled_coordinates_take_the_path_the_proof_allows(scale, proven, monkeypatch):
    """pi * 1e8 < 1e9 / 2 <= pi * 4e8: the first mesh runs both sines without range tests, the second --
    arguments on both sides of 1e9 -- with them.  Both against the longdouble reference at its own
    bound, and at the 1e-5 of tests/test_hip_source.py for arguments of this size."""
    import ctypes

    mesh, basis = _scaled_basis(scale, monkeypatch)
    eng = basis._engine
    program = _program("sin_sin", basis)
    vals, f = eng.assemble_system(1.0, 0.0, source=program)
    layout = eng.ring_plan()["layout"]
    bound = float(np.abs(mesh["vertices"]).max())
    coords = eng._inputs()["coords"]
    # what the engine measured and vouched for, and for which array
    assert layout[31:].view(np.float64)[0] == bound and int(layout[29]) == coords.data_ptr()
    fast = (ctypes.c_uint8 * 32)()
    assert eng.lib.tfem_source_trig_proof(ctypes.byref(program), bound, fast) == proven
    # what the launch handed its kernel: the proven sines, or the tested ones
    assert _launch_ops(eng, program).count(23) == proven
    assert _launch_ops(eng, program, coords=coords.clone()).count(23) == 0  # another array: no bound
    assert torch.equal(vals, eng.bilinear(1.0, 0.0))
    ops, consts = _ops(program)
    cells = mesh["vertices"][mesh["triangles"]]
    value, err_bound, decided = sr.evaluate(ops, consts, cells, 3, np.float64)
    assert decided.all() and np.isfinite(value).all()
    want, tol = sr.load_reference(value, err_bound, cells, mesh["triangles"], mesh["vertices"].shape[0], 1, 3, np.float64)
    err = np.abs(f.reshape(-1).cpu().numpy().astype(sr.LD) - want)
    ratio = float((err[tol > 0] / tol[tol > 0]).max())
    loose = float(err.max() / np.abs(want).max())
    print(f"scale {scale:g}: {proven} proven, error / bound {ratio:.3f}, error / max |f| {loose:.3e}")
    assert (err[tol == 0] == 0).all() and ratio <= 1.0 and loose <= 1e-5


def test_the_engine_withdraws_the_bound_once_the_coordinates_are_written(monkeypatch):
    _, basis = _scaled_basis(1.0, monkeypatch)
    eng = basis._engine
    program = _program("sin_sin", basis)
    _, f = eng.assemble_system(1.0, 0.0, source=program)
    f = f.clone()
    layout = eng.ring_plan()["layout"]
    assert layout[29] != 0 and _launch_ops(eng, program).count(23) == 2
    step = eng.prepared_system(1.0, 0.0, eng.assemble_system(1.0, 0.0, source=program), source=program)
    step()
    assert layout[29] != 0
    eng._inputs()["coords"].mul_(1.0)  # the same values: torch's version counter moves all the same
    _, f_prepared = step()
    assert layout[29] == 0 and layout[31] == 0 and _launch_ops(eng, program).count(23) == 0
    _, f_checked = eng.assemble_system(1.0, 0.0, source=program)
    assert layout[29] == 0  # for good
    assert scaled_error(f_checked.reshape(-1).cpu(), f.reshape(-1).cpu()) <= TOL_ROUTES
    assert scaled_error(f_prepared.reshape(-1).cpu(), f.reshape(-1).cpu()) <= TOL_ROUTES
