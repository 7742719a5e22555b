"""The fast sine / cosine of the source programs and the tail of a pass of the fused launch (-m gpu).
csrc/tfem_source.hpp flips the sign of a fast sine by an addition into the high word and lets the
cosine's extra sign ride on the polynomial's factor; csrc/tfem_rings_kernel.hpp reads the coordinates of
ALL elements of a pass from LDS before the determinants and predicates only the adds of the shares (a
lane without a second or third element reads vertex 0 of its tile).  The cases were laid out for
evaluating the values of a stack entry in interleaved groups of four with a shorter last group -- measured
and not kept (profiles/fused_chain_interleave.log) -- and cover what the kept changes can get wrong: a
wrong sign, a share of a missing element that is added after all, a share that lands on another vertex.
So: the meshes of tests/test_hip_fused_lds_direct.py (the smallest that reach two- and three-element
passes, the 15-slot records, one tile with fewer than 64 rows and a partial last wave); orders 1, 2, 3
and 4, which give entries of 2 / 3, 6 / 9 and 8 / 12 values in the wide interpreter and 6 values in the
general one (order 4); the bench's sin * sin, sin x cos y, cos(3 x) + 2 sin y (a cosine, with and
without a factor behind the function) and the depth-3 program with a sine (general interpreter).

K must be bit for bit the matrix-only launch's K; f is held against the numpy oracle at the project's
1e-12, norm-wise and entry-wise against the sum of the share magnitudes, against the
TFEM_DETERMINISTIC=1 route at 1e-14, and in float32 at 2e-6 (sinf / cosf: untouched code, same bound).

The rare branches at the end: coordinates scaled so that the host refuses the proof and every argument
still takes the fast path behind the range test; scaled further, so that part of the waves take the library
function through the wave-uniform branch (both against the longdouble reference of
tests/source_reference.py at its own bound, as tests/test_hip_fused_lds_direct.py does); a program on the
unit mesh whose arguments cross 1e9 (against the numpy oracle at 1e-12); and k_source_eval
(engine.source_values) against the oracle's point values at 1e-15."""

import math

import numpy as np
import pytest
import torch

import source_reference as sr
from conftest import rowwise_error, scaled_error
from oracle import assembly_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-12            # f against the oracle, norm-wise and entry-wise
TOL_ROUTES = 1e-14     # the default route against TFEM_DETERMINISTIC=1
TOL_FLOAT32 = 2e-6     # float32 load vectors
TOL_POINTS = 1e-15     # k_source_eval against the oracle's point values
STRADDLE = 1.0e9 - 0.5  # x + STRADDLE crosses the fast paths' 1e9 (csrc/tfem_source.hpp, kSrcTrigFastMax) at x = 0.5

SHAPES = ("structured", "delaunay", "one_tile", "partial_wave")
ORDERS = (1, 2, 3, 4)
PROGRAMS = ("sin_sin", "sin_cos", "cos3x_2siny", "depth_3")
CASES = [(shape, order, name) for shape in SHAPES for order in ORDERS for name in PROGRAMS]

SIN, COS, SIN_PROVEN, COS_PROVEN = 17, 18, 23, 24  # operation codes (include/tfem_assembly.h; csrc/tfem_source.hpp)


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

        if shape == "structured":      # tiles with a two-element pass and tiles with a three-element pass
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
    if name == "sin_cos":
        return forms.compile_program(("mul", ("sin", ("x",)), ("cos", ("y",))))
    if name == "cos3x_2siny":
        return forms.compile_program(("add", ("cos", ("mul", ("x",), ("c", 3.0))), ("mul", ("c", 2.0), ("sin", ("y",)))))
    if name == "cos_sin_pi":  # the rare branches: a cosine and a sine whose proof fails with the sines of sin_sin
        return forms.compile_program(("mul", ("cos", ("mul", ("x",), ("c", math.pi))),
                                      ("mul", ("c", 3.0), ("sin", ("mul", ("y",), ("c", math.pi))))))
    if name == "straddle":  # arguments of 1e9 - 0.5 .. 1e9 + 0.5 on the unit square: both sides of the fast paths' 1e9
        return forms.compile_program(("mul", ("sin", ("add", ("x",), ("c", STRADDLE))), ("cos", ("add", ("y",), ("c", STRADDLE)))))
    # the depth-3 program of tests/test_hip_fused_hot_loop.py (positive on the unit square)
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


def _launch_ops(eng, program, coords=None):
    """The operation codes a launch of `program` on the engine's plan hands its kernel."""
    import ctypes

    coords = eng._inputs()["coords"] if coords is None else coords
    ops = (ctypes.c_uint8 * 32)()
    layout = eng.ring_plan()["layout"]
    assert eng.lib.tfem_p1_rings_source_ops(ctypes.c_void_p(coords.data_ptr()), eng.real_bytes, eng.quad_order,
                                            ctypes.c_void_p(layout.ctypes.data), ctypes.byref(program), ops) == 0
    return list(ops)


def test_the_programs_hold_the_functions_their_names_say():
    from pytorch_fem_solver_amd.basis import forms

    names = {v: k for k, v in forms.OPS.items()}
    assert (forms.OPS["SIN"], forms.OPS["COS"]) == (SIN, COS)
    listing = lambda name: [(names[o], c) for o, c in zip(*_ops(_program(name, None)))]  # noqa: E731
    assert [n for n, _ in listing("sin_cos") if n in ("SIN", "COS")] == ["SIN", "COS"]
    # a cosine without a factor behind it on a scaled push, a sine with the factor 2
    assert ("PUSH_X", 3.0) in listing("cos3x_2siny") and ("COS", 1.0) in listing("cos3x_2siny")
    assert ("SIN", 2.0) in listing("cos3x_2siny")
    assert "SIN" in [n for n, _ in listing("depth_3")]


def test_the_structured_plan_has_two_and_three_element_passes(monkeypatch):
    _, eng = _engine("structured", 3, torch.float64, monkeypatch)
    plan = eng.ring_plan()
    layout = [int(v) for v in plan["layout"]]
    tiles = layout[0]
    blob = plan["blob"].cpu().numpy()
    desc = blob[layout[8]:layout[8] + 80 * tiles].view(np.int32).reshape(tiles, 20)
    evaluated = desc[:, 18] >> 8  # elements the tile evaluates itself: more than 512 need a three-element pass
    assert plan["chunked"] and layout[6] == 7
    assert tiles > 8 and 0 < int((evaluated > 512).sum()) < tiles, evaluated


@pytest.mark.parametrize("shape,order", [("structured", 1), ("structured", 2), ("structured", 3), ("delaunay", 3),
                                         ("structured", 4)])
def test_which_interpreter_and_which_sines_the_cases_run(shape, order, monkeypatch):
    """Orders 1-3: the wide interpreter with both sines proven; order 4 (six points): the general
    interpreter, which keeps the range test."""
    program = _run(shape, order, "sin_sin", torch.float64, monkeypatch)[0]
    _, eng = _engine(shape, order, torch.float64, monkeypatch)
    proven = 2 if order < 4 else 0
    assert _launch_ops(eng, program).count(SIN_PROVEN) == proven and _launch_ops(eng, program).count(SIN) == 2 - proven
    mixed = _run(shape, order, "sin_cos", torch.float64, monkeypatch)[0]
    got = _launch_ops(eng, mixed)
    assert (got.count(SIN_PROVEN), got.count(COS_PROVEN)) == ((1, 1) if order < 4 else (0, 0)), got


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


@pytest.mark.parametrize("shape,order,name", CASES)
def test_float32_load_vector_against_the_oracle(shape, order, name, monkeypatch):
    program, vals, f, _, f_det = _run(shape, order, name, torch.float32, monkeypatch)
    assert vals.dtype == torch.float32 and f.dtype == torch.float32
    want, _ = _oracle_load(shape, order, name, program, np.float32)
    err = scaled_error(f.cpu(), want)
    print(f"float32 {shape} order {order} {name}: {err:.3e}, deterministic route {scaled_error(f_det.cpu(), want):.3e}")
    assert err <= TOL_FLOAT32 and scaled_error(f_det.cpu(), want) <= TOL_FLOAT32


# ------------------------------------------------------------------------------------------
# the rare branches: the range test in front of the fast path, and the library function behind it
# ------------------------------------------------------------------------------------------
def _against_the_longdouble_reference(mesh, program, f, order):
    ops, consts = _ops(program)
    cells = mesh["vertices"][mesh["triangles"]]
    value, err_bound, decided = sr.evaluate(ops, consts, cells, order, np.float64)
    assert decided.all() and np.isfinite(value).all()
    want, tol = sr.load_reference(value, err_bound, cells, mesh["triangles"], mesh["vertices"].shape[0], 1, order,
                                  np.float64)
    err = np.abs(f.reshape(-1).cpu().numpy().astype(sr.LD) - want)
    assert (err[tol == 0] == 0).all()
    return float((err[tol > 0] / tol[tol > 0]).max()), float(err.max() / np.abs(want).max())


@pytest.mark.parametrize("scale,order,name", [(scale, order, name) for scale in (2.0e8, 4.0e8) for order in (2, 3)
                                              for name in ("sin_sin", "cos_sin_pi")])
def test_scaled_coordinates_take_the_range_test_and_the_library_function(scale, order, name, monkeypatch):
    """pi * 2e8 lies between the proof's 1e9 / 2 and the fast paths' 1e9: the host refuses the proof and every
    value passes the range test (checked fast path).  pi * 4e8 > 1e9: the waves whose arguments pass take
    the fast path, the others the library function."""
    import pytorch_fem_solver_amd as tf

    mesh = {k: np.array(v, copy=True) for k, v in _mesh("partial_wave").items()}
    mesh["vertices"] = mesh["vertices"] * scale
    monkeypatch.setenv("TFEM_RING_WGS", "8")
    basis = tf.Basis(tf.MeshTri(mesh), tf.ElementTri(1, order))
    eng = basis._engine
    assert eng.ring_plan() is not None and eng._rings_take_source()
    program = _program(name, basis)
    vals, f = eng.assemble_system(1.0, 0.0, source=program)
    got = _launch_ops(eng, program)
    assert got.count(SIN_PROVEN) + got.count(COS_PROVEN) == 0 and got.count(SIN) + got.count(COS) == 2, got
    arguments = math.pi * np.abs(mesh["vertices"])
    assert (arguments.max() < 1.0e9) == (scale == 2.0e8) and arguments.min() < 1.0e9
    assert torch.equal(vals, eng.bilinear(1.0, 0.0))
    ratio, loose = _against_the_longdouble_reference(mesh, program, f, order)
    print(f"scale {scale:g} order {order} {name}: error / bound {ratio:.3f}, error / max |f| {loose:.3e}")
    assert ratio <= 1.0 and loose <= 1e-5


@pytest.mark.parametrize("shape,order", [("partial_wave", 2), ("partial_wave", 3), ("structured", 3), ("partial_wave", 4)])
def test_arguments_past_the_fast_range_take_the_library_function_on_part_of_the_mesh(shape, order, monkeypatch):
    """sin(x + 1e9 - 0.5) cos(y + 1e9 - 0.5) on the unit square: the waves that hold a point with x >= 0.5 (or
    y) leave the fast path through the wave-uniform branch, the others pass the range test.  The sum with
    the constant is one rounding on the device and in the oracle alike (a last-bit difference of the point
    would have to cross a rounding boundary 1e-7 wide to show), so the oracle's bound holds as it stands."""
    basis, eng = _engine(shape, order, torch.float64, monkeypatch)
    program = _program("straddle", basis)
    got = _launch_ops(eng, program)
    assert got.count(SIN_PROVEN) + got.count(COS_PROVEN) == 0 and (got.count(SIN), got.count(COS)) == (1, 1)
    vertices = _mesh(shape)["vertices"]
    assert vertices.min() + STRADDLE < 1.0e9 < vertices.max() + STRADDLE
    vals, f = eng.assemble_system(1.0, 0.0, source=program)
    assert torch.equal(vals, eng.bilinear(1.0, 0.0))
    want, scale = _oracle_load(shape, order, "straddle", program)
    norm_wise, entry_wise = scaled_error(f.reshape(-1).cpu(), want), rowwise_error(f.reshape(-1).cpu(), want, scale=scale)
    print(f"{shape} order {order} straddle: norm-wise {norm_wise:.3e} entry-wise {entry_wise:.3e}")
    assert norm_wise <= TOL and entry_wise <= TOL


@pytest.mark.parametrize("shape,order,name", [(shape, order, name) for shape in ("partial_wave", "delaunay")
                                              for order in ORDERS for name in ("sin_sin", "sin_cos", "cos3x_2siny")])
def test_source_values_against_the_oracles_point_values(shape, order, name, monkeypatch):
    """k_source_eval: the general interpreter on entries of 1, 3, 4 and 6 values."""
    basis, eng = _engine(shape, order, torch.float64, monkeypatch)
    program = _program(name, basis)
    got = eng.source_values(program).cpu().numpy()
    points = basis.integration_points.cpu().numpy()
    ops, consts = _ops(program)
    want = np.asarray(orc.source_program_eval(ops, consts, points[..., [0]], points[..., [1]])).reshape(got.shape)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{shape} order {order} {name}: point values {err:.3e}")
    assert err <= TOL_POINTS
