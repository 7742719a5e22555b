"""The separable phase G of the fused K + f launch with the functions' factors on the share constants
(-m gpu; csrc/tfem_source.hpp src_separable evaluates the two bare functions, the host folds k = c1 c3 into
RingArgs::qsym[3..5]).  The small shapes of tests/test_hip_fused_separable.py, TFEM_RING_WGS=8:
unit_square(96) -- 51 tiles, 15 of them with the three-element pass --, the Morton-ordered Delaunay mesh of
4000 points with its 15-slot records; unit_square(3) -- one tile with most lanes empty, whose zero-filled
codes read vertex 0 --; and the structured mesh with every triangle's last two vertices swapped (negative
determinants).

Programs: the four sine / cosine pairs with push constants that keep them positive on the unit square (the
entry-wise bound presumes shares that do not cancel), one of them with y pushed first, one with the factors
c1 = -3, c3 = 0.25 (one sign everywhere: the entry-wise bound applies), the same factors on a pair that
changes sign, and push constants up to 8 in magnitude.

For every mesh and program: the launch's route is 2, K is bit for bit the matrix-only launch's K, f is held
against the numpy oracle at the project's 1e-12 (norm-wise for all, entry-wise for the programs of one sign)
and against the same launch on the interpreter (TFEM_RINGS_SEPARABLE=0) at the project's route-to-route
1e-14: the two routes form the same points and the same sines, and differ by the roundings of
k (sin X sin Y) against (c1 sin X)(c3 sin Y), a few 1e-16 relative to each value.  Then a mass term and
the load vector alone (KMAT = false).

The integration points themselves keep the reference's form l^T X on both routes: formed from the order-3
rule's symmetry they leave the entry-wise 1e-12 of the full-size comparison with the oracle
(tests/test_hip_source.py::test_full_size_traced_system_against_c_oracle; profiles/fused_rule_points.log,
section 6), which meshes of this size cannot show -- measured here: norm-wise <= 4.9e-16 against the oracle,
1.0e-16 .. 3.8e-16 between the routes."""

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

SHAPES = ("structured", "delaunay", "tiny", "clockwise")


def _fn(fn, coord, inner, outer=1.0):
    node = (fn, ("mul", (coord,), ("c", inner)))
    return node if outer == 1.0 else ("mul", node, ("c", outer))


#: name -> (expression, one sign on the unit square: the entry-wise bound applies)
PROGRAMS = {
    "sin_sin": (("mul", _fn("sin", "x", 1.5), _fn("sin", "y", 2.5)), True),
    "sin_cos": (("mul", _fn("sin", "x", 2.0), _fn("cos", "y", 1.2)), True),
    "cos_sin_y_first": (("mul", _fn("sin", "y", 2.5), _fn("cos", "x", 1.2)), True),
    "cos_cos": (("mul", _fn("cos", "x", 1.2), _fn("cos", "y", 0.9)), True),
    "factors": (("mul", _fn("sin", "x", 1.5, -3.0), _fn("cos", "y", 1.2, 0.25)), True),
    "factors_signed": (("mul", _fn("cos", "x", math.pi, -3.0), _fn("sin", "y", math.pi, 0.25)), False),
    "push_8": (("mul", _fn("sin", "x", 8.0), _fn("cos", "y", -7.5)), False),
}
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
        elif shape == "tiny":
            m = meshgen.unit_square(3, 0.25, 0)  # 18 elements, 16 vertices
        elif shape == "clockwise":
            m = {k: v.copy() for k, v in _mesh("structured").items()}
            m["triangles"] = np.ascontiguousarray(m["triangles"][:, [0, 2, 1]])
        else:  # 7,746 elements, 15-slot records
            m = meshgen.delaunay_square(4000, 3)
            m = meshgen.permute_mesh(m, vertex_order=meshgen.morton_order(m["vertices"]))
        _MESHES[shape] = m
    return _MESHES[shape]


def _program(name):
    from pytorch_fem_solver_amd.basis import forms

    return forms.compile_program(PROGRAMS[name][0])


def _ops(program):
    n = int(program.n_ops)
    return [int(v) for v in program.ops[:n]], [float(v) for v in program.consts[:n]]


def _engine(shape, monkeypatch):
    if shape not in _ENGINES:
        import pytorch_fem_solver_amd as tf

        monkeypatch.setenv("TFEM_RING_WGS", "8")
        basis = tf.Basis(tf.MeshTri(_mesh(shape)), tf.ElementTri(1, 3))
        eng = basis._engine
        assert eng.ring_plan() is not None and eng._rings_take_source()
        _ENGINES[shape] = (basis, eng)
    return _ENGINES[shape]


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
        _, eng = _engine(shape, monkeypatch)
        program = _program(name)
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


def test_the_shapes_and_programs_are_what_the_docstring_says(monkeypatch):
    from pytorch_fem_solver_amd.basis import forms

    x, y, sin, cos, mul = (forms.OPS[n] for n in ("PUSH_X", "PUSH_Y", "SIN", "COS", "MUL"))
    assert _ops(_program("cos_sin_y_first")) == ([y, sin, x, cos, mul], [2.5, 1.0, 1.2, 1.0, 0.0])
    assert _ops(_program("factors")) == ([x, sin, y, cos, mul], [1.5, -3.0, 1.2, 0.25, 0.0])
    assert _ops(_program("factors_signed")) == ([x, cos, y, sin, mul], [math.pi, -3.0, math.pi, 0.25, 0.0])
    assert _ops(_program("push_8")) == ([x, sin, y, cos, mul], [8.0, 1.0, -7.5, 1.0, 0.0])
    assert _mesh("tiny")["triangles"].shape[0] == 18
    for shape, sign in (("structured", 1.0), ("clockwise", -1.0)):
        m = _mesh(shape)
        v = m["vertices"][m["triangles"].astype(np.int64)]
        det = ((v[:, 1, 0] - v[:, 0, 0]) * (v[:, 2, 1] - v[:, 0, 1])
               - (v[:, 2, 0] - v[:, 0, 0]) * (v[:, 1, 1] - v[:, 0, 1]))
        assert (sign * det > 0).all()
    # the programs of one sign: their shares do not cancel in the oracle either
    for name, (_, one_sign) in PROGRAMS.items():
        want, scale = _oracle_load("structured", name, _program(name))
        assert bool(np.allclose(np.abs(want), scale, rtol=1e-9, atol=0.0)) == one_sign, name


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
    if PROGRAMS[name][1]:
        assert entry_wise <= TOL


@pytest.mark.parametrize("shape,name", CASES)
def test_load_vector_against_the_interpreter_route(shape, name, monkeypatch):
    _, _, _, _, f, _, f_interp = _run(shape, name, monkeypatch)
    err = scaled_error(f.cpu(), f_interp.cpu())
    print(f"{shape} {name}: against TFEM_RINGS_SEPARABLE=0 {err:.3e}")
    assert err <= TOL_ROUTES


@pytest.mark.parametrize("shape", SHAPES)
def test_with_a_mass_term(shape, monkeypatch):
    _, eng = _engine(shape, monkeypatch)
    program, _, _, _, f, _, _ = _run(shape, "factors", monkeypatch)
    vals, f_mass = eng.assemble_system(1.0, 0.5, source=program)
    assert _route(eng, program) == 2
    assert torch.equal(vals, eng.bilinear(1.0, 0.5))
    want, scale = _oracle_load(shape, "factors", program)
    f_mass = f_mass.reshape(-1)
    err = scaled_error(f_mass.cpu(), f.cpu())
    print(f"{shape}: f of the launch with mass against the one without {err:.3e}")
    assert err <= TOL_ROUTES
    assert scaled_error(f_mass.cpu(), want) <= TOL and rowwise_error(f_mass.cpu(), want, scale=scale) <= TOL


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["factors", "push_8"])
def test_the_load_vector_alone(shape, name, monkeypatch):
    _, eng = _engine(shape, monkeypatch)
    program, _, _, _, f, _, f_interp = _run(shape, name, monkeypatch)
    alone = eng.load_source(program).reshape(-1)
    assert _route(eng, program) == 2
    want, scale = _oracle_load(shape, name, program)
    err, routes = scaled_error(alone.cpu(), f.cpu()), scaled_error(alone.cpu(), f_interp.cpu())
    against = scaled_error(alone.cpu(), want)
    print(f"{shape} {name}: f alone against the fused launch {err:.3e}, the interpreter {routes:.3e}, the oracle {against:.3e}")
    assert err <= TOL_ROUTES and routes <= TOL_ROUTES and against <= TOL
    if PROGRAMS[name][1]:
        assert rowwise_error(alone.cpu(), want, scale=scale) <= TOL
