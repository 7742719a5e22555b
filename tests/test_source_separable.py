"""Which evaluator a fused launch picks for a source program (tfem_p1_rings_source_route, no GPU):
0 the general interpreter, 1 the wide interpreter, 2 straight-line code for a separable program.
Route 2 is taken only by an fp64 launch with the 4-point rule (order 3) whose program is, after the
proof of tests/test_source_trig_proof.py for the vouched coordinate array, exactly
    PUSH_a(c0) F(c1) PUSH_b(c2) G(c3) MUL,   {a, b} = {X, Y},   F, G proven SIN / COS;
everything else keeps the interpreters, and TFEM_RINGS_SEPARABLE=0 keeps them for every program."""

import ctypes
import math

import numpy as np
import pytest

ARRAY, OTHER = 0x7F0000001000, 0x7F0000002000  # addresses only: nothing is read through them


@pytest.fixture(scope="module")
def lib():
    from pytorch_fem_solver_amd import _native

    return _native.load()


def _program(node):
    from pytorch_fem_solver_amd.basis import forms

    program = forms.compile_program(node)
    names = {v: k for k, v in forms.OPS.items()}
    return program, [names[int(o)] for o in program.ops[: program.n_ops]]


def _layout(lib, bound=1.0, array=ARRAY):
    layout = np.zeros(32, dtype=np.int64)
    if bound is not None:
        assert lib.tfem_ring_plan_vouch_coords(ctypes.c_void_p(layout.ctypes.data), ctypes.c_void_p(array), bound) == 0
    return layout


def _route(lib, layout, program, array=ARRAY, real_bytes=8, order=3):
    return lib.tfem_p1_rings_source_route(ctypes.c_void_p(array), real_bytes, order,
                                          ctypes.c_void_p(layout.ctypes.data), ctypes.byref(program))


def _factor(fn, coord, inner=1.0, outer=1.0):
    node = (coord,) if inner == 1.0 else ("mul", (coord,), ("c", inner))
    node = (fn, node)
    return node if outer == 1.0 else ("mul", node, ("c", outer))


SIN_SIN = ("mul", _factor("sin", "x", math.pi, 2.0 * math.pi**2), _factor("sin", "y", math.pi))


def test_the_bench_source_is_separable(lib):
    program, names = _program(SIN_SIN)
    assert names == ["PUSH_X", "SIN", "PUSH_Y", "SIN", "MUL"]
    assert [float(c) for c in program.consts[:4]] == [math.pi, 2.0 * math.pi**2, math.pi, 1.0]
    assert _route(lib, _layout(lib), program) == 2


@pytest.mark.parametrize("first", ["x", "y"])
@pytest.mark.parametrize("f", ["sin", "cos"])
@pytest.mark.parametrize("g", ["sin", "cos"])
@pytest.mark.parametrize("factors", [(1.0, 1.0, 1.0, 1.0), (-1.0, -1.0, -1.0, -1.0), (1.2, -3.0, 2.5, 0.75)])
def test_the_accepted_family(lib, first, f, g, factors):
    second = "y" if first == "x" else "x"
    program, names = _program(("mul", _factor(f, first, factors[0], factors[1]), _factor(g, second, factors[2], factors[3])))
    assert names == ["PUSH_" + first.upper(), f.upper(), "PUSH_" + second.upper(), g.upper(), "MUL"], names
    assert [float(c) for c in program.consts[:4]] == list(factors)
    assert _route(lib, _layout(lib, 3.0), program) == 2


@pytest.mark.parametrize("node,route", [
    (("mul", ("sin", ("x",)), ("sin", ("x",))), 1),                               # sin x sin x: one coordinate
    (("mul", ("cos", ("y",)), ("sin", ("y",))), 1),
    (("add", ("sin", ("x",)), ("sin", ("y",))), 1),                               # a sum
    (("sub", ("sin", ("x",)), ("cos", ("y",))), 1),
    (("sin", ("mul", ("x",), ("y",))), 1),                                        # sin(x y): not a push in front
    (("mul", ("sin", ("x",)), ("y",)), 1),                                        # four operations
    (("mul", ("sin", ("x",)), ("exp", ("y",))), 1),                               # another function
    (("mul", ("sin", ("x",)), ("sin", ("c", 2.0))), 1),                           # a constant push
    (("mul", ("sin", ("x",)), ("sin", ("add", ("y",), ("c", 1.0)))), 1),          # six operations
    (("neg", ("mul", ("sin", ("x",)), ("sin", ("y",)))), 1),                      # six operations, product inside
    (("mul", ("mul", ("sin", ("x",)), ("cos", ("y",))), ("sin", ("x",))), 1),     # a third factor
    (("add", ("mul", ("x",), ("y",)), ("mul", ("add", ("sin", ("x",)), ("c", 2.0)), ("add", ("y",), ("x",)))), 0),
])
def test_the_near_misses_keep_the_interpreters(lib, node, route):
    program, names = _program(node)
    assert _route(lib, _layout(lib), program) == route, names


def test_a_separable_shape_that_folds_to_more_than_five_operations_is_refused(lib):
    for node in (("mul", ("sin", ("x",)), ("sin", ("add", ("y",), ("c", 1.0)))),
                 ("neg", ("mul", ("sin", ("x",)), ("sin", ("y",))))):
        program, names = _program(node)
        assert len(names) >= 6 and _route(lib, _layout(lib), program) == 1, names


def test_without_a_proof_the_interpreter_stays(lib):
    program, _ = _program(SIN_SIN)
    assert _route(lib, _layout(lib, None), program) == 1                 # no bound
    assert _route(lib, _layout(lib, 1.0, OTHER), program) == 1           # a bound about another array
    assert _route(lib, _layout(lib, 1.0), program, array=OTHER) == 1
    assert _route(lib, _layout(lib, 4.0e8), program) == 1                # pi * 4e8 >= 1e9 / 2: not proven
    assert _route(lib, _layout(lib, 1.0e8), program) == 2
    assert _route(lib, _layout(lib, 0.0), program) == 2                  # a bound of zero is a bound
    layout = _layout(lib)
    assert lib.tfem_ring_plan_vouch_coords(ctypes.c_void_p(layout.ctypes.data), None, -1.0) == 0  # withdrawn
    assert _route(lib, layout, program) == 1
    # one of the two proven is not enough: sin(x) sin(1e3 y) at a bound of 1e6
    half, _ = _program(("mul", ("sin", ("x",)), _factor("sin", "y", 1.0e3)))
    assert _route(lib, _layout(lib, 1.0e6), half) == 1 and _route(lib, _layout(lib, 1.0e5), half) == 2


def test_float32_and_the_other_orders(lib):
    program, _ = _program(SIN_SIN)
    layout = _layout(lib)
    assert _route(lib, layout, program, real_bytes=4) == 1
    assert [_route(lib, layout, program, order=o) for o in (1, 2, 3, 4)] == [1, 1, 2, 0]  # Q = 1, 3, 4, 6
    assert [_route(lib, layout, program, real_bytes=4, order=o) for o in (1, 2, 3, 4)] == [1, 1, 1, 0]


def test_the_kernel_is_handed_the_same_operations_on_routes_1_and_2(lib, monkeypatch):
    program, _ = _program(SIN_SIN)
    layout = _layout(lib)

    def ops():
        out = (ctypes.c_uint8 * 32)()
        assert lib.tfem_p1_rings_source_ops(ctypes.c_void_p(ARRAY), 8, 3, ctypes.c_void_p(layout.ctypes.data),
                                            ctypes.byref(program), out) == 0
        return list(out)

    default = ops()
    assert _route(lib, layout, program) == 2 and default[:5] == [int(program.ops[0]), 23, int(program.ops[2]), 23, int(program.ops[4])]
    monkeypatch.setenv("TFEM_RINGS_SEPARABLE", "0")
    assert _route(lib, layout, program) == 1 and ops() == default


def test_the_switch_and_refused_calls(lib, monkeypatch):
    program, _ = _program(SIN_SIN)
    layout = _layout(lib)
    monkeypatch.setenv("TFEM_RINGS_SEPARABLE", "0")
    assert _route(lib, layout, program) == 1
    monkeypatch.setenv("TFEM_RINGS_SEPARABLE", "1")
    assert _route(lib, layout, program) == 2
    monkeypatch.delenv("TFEM_RINGS_SEPARABLE")
    assert _route(lib, layout, program) == 2
    assert _route(lib, layout, program, real_bytes=2) < 0 and _route(lib, layout, program, order=9) < 0
    assert lib.tfem_p1_rings_source_route(ctypes.c_void_p(ARRAY), 8, 3, None, ctypes.byref(program)) < 0
    bad, _ = _program(SIN_SIN)
    bad.n_ops = 3  # PUSH_X SIN PUSH_Y leaves two values
    assert _route(lib, layout, bad) < 0
