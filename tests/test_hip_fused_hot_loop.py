"""The fused K + f launch's hot loop (-m gpu) on the smallest meshes that reach every path of it:
the two- and the three-element pass of the wide interpreter, the general interpreter, a hand-in
between consecutive tiles of a run, the 7- and the 15-slot records, every width of the
integration-point table (Q = 1, 3, 4, 6: the kernels read it by scalar loads from the
kernel-argument segment) and float32.  With TFEM_RING_WGS=8 the plan has eight runs of several
tiles each, as a full-size mesh has on a whole card.

K must be bit for bit the matrix-only launch's K; f is held against the numpy oracle at the
bounds of tests/test_hip_source.py (1e-12 norm-wise and entry-wise) and against the
TFEM_DETERMINISTIC=1 route at that test's 1e-14."""

import math

import numpy as np
import pytest
import torch

import source_reference as sr
from conftest import rowwise_error, scaled_error
from oracle import assembly_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-12            # tests/test_hip_source.py: f against the oracle, norm-wise and entry-wise
TOL_ROUTES = 1e-14     # ... the default route against TFEM_DETERMINISTIC=1
TOL_FLOAT32 = 2e-6     # ... float32 load vectors

#: shape -> (tiles, tiles that evaluate more than 512 elements: the three-element pass)
SHAPES = {"structured": (51, 15), "delaunay": (16, 10)}
PROGRAMS = ("sin_sin", "xy_plus_1", "depth_3")


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
    if name == "xy_plus_1":
        return forms.compile_program(("add", ("mul", ("x",), ("y",)), ("c", 1.0)))
    # three values at once: the general (one element per pass) interpreter.  x y + (sin x + 2)(y + x),
    # positive on the unit square like the other two: the entry-wise bound measures an entry against
    # the sum of the magnitudes of its element shares, which presumes that no share cancels inside
    # (with sin x (y - x) in its place, elements across the zero line of f left 1e-12: 2.8e-12)
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
    on the vertices as a launch of `np_dtype` holds them: a float32 launch is given the coordinates
    rounded to float32, and on a grid of 96 cells that rounding alone moves the determinants by 3e-6."""
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


CASES = [(shape, 3, name) for shape in SHAPES for name in PROGRAMS] + [("structured", order, "sin_sin") for order in (1, 2, 4)]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_plans_have_tiles_of_the_two_and_of_the_three_element_pass(shape, monkeypatch):
    _, eng = _engine(shape, 3, torch.float64, monkeypatch)
    plan = eng.ring_plan()
    layout = [int(v) for v in plan["layout"]]
    tiles, three = SHAPES[shape]
    assert layout[0] == tiles and layout[28] == 8, (layout[0], layout[28])
    assert plan["chunked"] and layout[6] == (7 if shape == "structured" else 15)
    blob = plan["blob"].cpu().numpy()
    desc = blob[layout[8]:layout[8] + 80 * tiles].view(np.int32).reshape(tiles, 20)
    evaluated = desc[:, 18] >> 8  # elements the tile evaluates itself
    assert int((evaluated > 512).sum()) == three and int((evaluated > 768).sum()) == 0
    assert int(((evaluated > 0) & (evaluated <= 512)).sum()) == tiles - three


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


@pytest.mark.parametrize("name", PROGRAMS)
def test_float32_load_vector_against_the_oracle(name, monkeypatch):
    program, vals, f, want_k, f_det = _run("structured", 3, name, torch.float32, monkeypatch)
    assert vals.dtype == torch.float32 and f.dtype == torch.float32
    want, _ = _oracle_load("structured", 3, name, program, np.float32)
    err = scaled_error(f.cpu(), want)
    print(f"float32 {name}: {err:.3e}, against the deterministic route {scaled_error(f.cpu(), f_det.cpu()):.3e}")
    assert err <= TOL_FLOAT32 and scaled_error(f_det.cpu(), want) <= TOL_FLOAT32
    # float32: hipcc contracts the two code shapes differently (tests/test_hip_source.py)
    assert scaled_error(vals.cpu(), want_k.cpu()) <= 3e-7
