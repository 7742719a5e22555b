"""The fused K + f launch's straight-line phase G for separable sources k U(a x) V(b y) (-m gpu;
csrc/tfem_source.hpp src_separable, the SEP instantiations of csrc/tfem_rings_kernel.hpp), on the meshes of
tests/test_hip_fused_hot_loop.py with TFEM_RING_WGS=8: unit_square(96) -- 51 tiles, 15 of them with the
three-element pass, hand-ins inside runs -- and the Morton-ordered Delaunay mesh of 4000 points with its
15-slot records.  Programs: the bench's traced sin sin; cos(1.2 x) sin(2.5 y), positive on the unit square
(the entry-wise bound presumes shares that do not cancel, tests/test_hip_fused_hot_loop.py); the same with y
pushed first; -3 cos(pi x) cos(pi y), which changes sign.

For every mesh and program the launch's route is 2 (tfem_p1_rings_source_route), K is bit for bit the
matrix-only launch's K, f is held against the numpy oracle at the project's 1e-12 (norm-wise for all,
entry-wise for the positive programs) and against the same launch on the interpreter
(TFEM_RINGS_SEPARABLE=0) at the project's route-to-route 1e-14.  Then: a mass term, the load vector alone,
the two launches of a plan with flagged vertices, and coordinates written in place (the bound is withdrawn:
route 1, same result)."""

import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import rowwise_error, scaled_error
from oracle import assembly_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-12            # f against the oracle (tests/test_hip_source.py)
TOL_ROUTES = 1e-14     # one route against another (tests/test_hip_fused_hot_loop.py)

SHAPES = ("structured", "delaunay")
#: name -> positive on the unit square (entry-wise bound applies)
PROGRAMS = {"sin_sin": True, "cos_sin": True, "cos_sin_y_first": True, "cos_cos_signed": False}
CASES = [(shape, name) for shape in SHAPES for name in PROGRAMS]


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

        if shape == "structured":
            m = meshgen.unit_square(96, 0.25, 0)  # 18,432 elements
        else:  # 7,746 elements, 15-slot records
            m = meshgen.delaunay_square(4000, 3)
            m = meshgen.permute_mesh(m, vertex_order=meshgen.morton_order(m["vertices"]))
        _MESHES[shape] = m
    return _MESHES[shape]


def _program(name, basis):
    from pytorch_fem_solver_amd.basis import forms

    if name == "sin_sin":  # the bench's source, traced like the bench traces it

        def load(b):
            x, y = torch.split(b.integration_points, 1, dim=-1)
            return 2.0 * math.pi**2 * torch.sin(math.pi * x) * torch.sin(math.pi * y) * b.v

        return forms.trace(load, basis, (), {}).coefficient.program()
    cos_x = ("cos", ("mul", ("x",), ("c", 1.2)))
    sin_y = ("sin", ("mul", ("y",), ("c", 2.5)))
    if name == "cos_sin":
        return forms.compile_program(("mul", cos_x, sin_y))
    if name == "cos_sin_y_first":
        return forms.compile_program(("mul", sin_y, cos_x))
    return forms.compile_program(("mul", ("mul", ("cos", ("mul", ("x",), ("c", math.pi))), ("c", -3.0)),
                                  ("cos", ("mul", ("y",), ("c", math.pi)))))


def _ops(program):
    n = int(program.n_ops)
    return [int(v) for v in program.ops[:n]], [float(v) for v in program.consts[:n]]


def _engine(shape, monkeypatch, flags=None):
    """The basis and its engine, the ring plan built for eight resident workgroups (flags: priority
    vertices, set before the plan is built -- the plan then offers tile ranges)."""
    key = (shape, flags is not None)
    if key not in _ENGINES:
        import pytorch_fem_solver_amd as tf

        monkeypatch.setenv("TFEM_RING_WGS", "8")
        basis = tf.Basis(tf.MeshTri(_mesh(shape)), tf.ElementTri(1, 3))
        eng = basis._engine
        if flags is not None:
            eng.set_priority_vertices(flags)
        assert eng.ring_plan() is not None and eng._rings_take_source()
        _ENGINES[key] = (basis, eng)
    return _ENGINES[key]


def _route(eng, program):
    coords = eng._inputs()["coords"]
    layout = eng.ring_plan()["layout"]
    return eng.lib.tfem_p1_rings_source_route(ctypes.c_void_p(coords.data_ptr()), eng.real_bytes, eng.quad_order,
                                              ctypes.c_void_p(layout.ctypes.data), ctypes.byref(program))


def _oracle_load(shape, name, program):
    """(f, sum of the magnitudes of the element shares per entry) of the numpy oracle, once."""
    key = (shape, name)
    if key not in _WANT:
        m = _mesh(shape)
        ops, consts = _ops(program)
        source = lambda pts: orc.source_program_eval(ops, consts, pts[..., [0]], pts[..., [1]])  # noqa: E731
        local, _ = orc.p1_assemble(m["vertices"], m["triangles"], 3, "load", source=source)
        n = m["vertices"].shape[0]
        _WANT[key] = (orc.assemble_linear(local, m["triangles"], n).reshape(-1),
                      orc.assemble_linear(np.abs(local), m["triangles"], n).reshape(-1))
    return _WANT[key]


def _run(shape, name, monkeypatch):
    """One fused launch on route 2, the same on the interpreter and the matrix-only launch, once per case."""
    key = (shape, name)
    if key not in _RUNS:
        basis, eng = _engine(shape, monkeypatch)
        program = _program(name, basis)
        vals, f = eng.assemble_system(1.0, 0.0, source=program)
        route = _route(eng, program)  # (behind the first launch: the engine vouches for its coordinates there)
        want_k = eng.bilinear(1.0, 0.0)
        with monkeypatch.context() as m:
            m.setenv("TFEM_RINGS_SEPARABLE", "0")
            route_off = _route(eng, program)
            _, f_interp = eng.assemble_system(1.0, 0.0, source=program)
        _RUNS[key] = (program, route, route_off, vals.clone(), f.reshape(-1).clone(), want_k.clone(),
                      f_interp.reshape(-1).clone())
    return _RUNS[key]


def test_the_programs_are_what_their_names_say(monkeypatch):
    from pytorch_fem_solver_amd.basis import forms

    basis, _ = _engine("structured", monkeypatch)
    x, y, sin, cos, mul = (forms.OPS[n] for n in ("PUSH_X", "PUSH_Y", "SIN", "COS", "MUL"))
    assert _ops(_program("sin_sin", basis)) == ([x, sin, y, sin, mul], [math.pi, 2.0 * math.pi**2, math.pi, 1.0, 0.0])
    assert _ops(_program("cos_sin", basis)) == ([x, cos, y, sin, mul], [1.2, 1.0, 2.5, 1.0, 0.0])
    assert _ops(_program("cos_sin_y_first", basis)) == ([y, sin, x, cos, mul], [2.5, 1.0, 1.2, 1.0, 0.0])
    assert _ops(_program("cos_cos_signed", basis)) == ([x, cos, y, cos, mul], [math.pi, -3.0, math.pi, 1.0, 0.0])


@pytest.mark.parametrize("shape,name", CASES)
def test_the_launch_took_the_separable_route(shape, name, monkeypatch):
    _, route, route_off, *_ = _run(shape, name, monkeypatch)
    assert route == 2 and route_off == 1


@pytest.mark.parametrize("shape,name", CASES)
def test_fused_matrix_is_bit_for_bit_the_matrix_only_launch(shape, name, monkeypatch):
    _, _, _, vals, _, want_k, _ = _run(shape, name, monkeypatch)
    assert torch.equal(vals, want_k)


@pytest.mark.parametrize("shape,name", CASES)
def test_load_vector_against_the_oracle(shape, name, monkeypatch):
    program, _, _, _, f, _, _ = _run(shape, name, monkeypatch)
    want, scale = _oracle_load(shape, name, program)
    norm_wise, entry_wise = scaled_error(f.cpu(), want), rowwise_error(f.cpu(), want, scale=scale)
    print(f"{shape} {name}: norm-wise {norm_wise:.3e} entry-wise {entry_wise:.3e}")
    assert norm_wise <= TOL
    if PROGRAMS[name]:
        assert entry_wise <= TOL


@pytest.mark.parametrize("shape,name", CASES)
def test_load_vector_against_the_interpreter_route(shape, name, monkeypatch):
    _, _, _, _, f, _, f_interp = _run(shape, name, monkeypatch)
    err = scaled_error(f.cpu(), f_interp.cpu())
    print(f"{shape} {name}: against TFEM_RINGS_SEPARABLE=0 {err:.3e}")
    assert err <= TOL_ROUTES


@pytest.mark.parametrize("shape", SHAPES)
def test_with_a_mass_term(shape, monkeypatch):
    basis, eng = _engine(shape, monkeypatch)
    program, _, _, _, f, _, _ = _run(shape, "cos_sin", monkeypatch)
    vals, f_mass = eng.assemble_system(1.0, 0.5, source=program)
    assert _route(eng, program) == 2
    assert torch.equal(vals, eng.bilinear(1.0, 0.5))
    err = scaled_error(f_mass.reshape(-1).cpu(), f.cpu())
    print(f"{shape}: f of the launch with mass against the one without {err:.3e}")
    assert err <= TOL_ROUTES


@pytest.mark.parametrize("shape", SHAPES)
def test_the_load_vector_alone(shape, monkeypatch):
    basis, eng = _engine(shape, monkeypatch)
    program, _, _, _, f, _, _ = _run(shape, "cos_cos_signed", monkeypatch)
    alone = eng.load_source(program)
    assert _route(eng, program) == 2
    want, _ = _oracle_load(shape, "cos_cos_signed", program)
    err, against = scaled_error(alone.reshape(-1).cpu(), f.cpu()), scaled_error(alone.reshape(-1).cpu(), want)
    print(f"{shape}: f alone against the fused launch {err:.3e}, against the oracle {against:.3e}")
    assert err <= TOL_ROUTES and against <= TOL


def test_the_two_launches_of_a_plan_with_flagged_vertices(monkeypatch):
    m = _mesh("structured")
    flags = m["vertices"][:, 0] < 0.3
    basis, eng = _engine("structured", monkeypatch, flags=flags)
    program, _, _, _, f, want_k, _ = _run("structured", "cos_sin", monkeypatch)
    (_, n_pri), (_, n_rest) = eng.tile_range("priority"), eng.tile_range("rest")
    assert n_pri > 0 and n_rest > 0
    out = (torch.full((want_k.numel(),), float("nan")), torch.full((f.numel(),), float("nan")))
    eng.assemble_system(1.0, 0.0, source=program, out=out, tiles="priority")
    assert _route(eng, program) == 2
    torch.cuda.synchronize()
    assert torch.isnan(out[0]).any() and torch.isnan(out[1]).any()  # the other rows still untouched
    eng.assemble_system(1.0, 0.0, source=program, out=out, tiles="rest")
    assert torch.equal(out[0], want_k.view(-1))
    err = scaled_error(out[1].cpu(), f.cpu())
    print(f"two launches against one {err:.3e}")
    assert err <= TOL_ROUTES


def test_coordinates_written_in_place_fall_back_to_the_interpreter(monkeypatch):
    import pytorch_fem_solver_amd as tf

    monkeypatch.setenv("TFEM_RING_WGS", "8")
    basis = tf.Basis(tf.MeshTri(_mesh("structured")), tf.ElementTri(1, 3))  # an engine of its own: the bound goes for good
    eng = basis._engine
    program, _, _, _, f, want_k, _ = _run("structured", "sin_sin", monkeypatch)
    vals, f_first = eng.assemble_system(1.0, 0.0, source=program)
    assert _route(eng, program) == 2
    f_first = f_first.reshape(-1).clone()
    eng._inputs()["coords"].mul_(1.0)  # the same values: torch's version counter moves all the same
    vals, f_after = eng.assemble_system(1.0, 0.0, source=program)
    assert _route(eng, program) == 1 and eng.ring_plan()["layout"][29] == 0
    assert torch.equal(vals, want_k)
    want, scale = _oracle_load("structured", "sin_sin", program)
    f_after = f_after.reshape(-1)
    err = scaled_error(f_after.cpu(), f_first.cpu())
    print(f"after the write against before {err:.3e}")
    assert err <= TOL_ROUTES
    assert scaled_error(f_after.cpu(), want) <= TOL and rowwise_error(f_after.cpu(), want, scale=scale) <= TOL
