"""The host-side proof that a source program's sin / cos stay on the kernels' fast path
(tfem_source_trig_proof, no GPU): an fp64 launch that is given a bound on the coordinates
(tfem_ring_plan_vouch_coords) skips the range test of every value of a SIN / COS whose operand is the
coordinate push directly in front of it, with constant c, when
    |c| * max|coordinate| * (1 + 1e-9) < 1e9 / 2.
Everything else keeps the tested path, so the proof may say no too often but never yes wrongly."""

import ctypes
import math

import numpy as np
import pytest

import source_reference as sr

LIMIT = sr.TRIG_FAST_MAX / 2
MARGIN = 1.0 + 1e-9


@pytest.fixture(scope="module")
def lib():
    from pytorch_fem_solver_amd import _native

    return _native.load()


def _program(node):
    from pytorch_fem_solver_amd.basis import forms

    program = forms.compile_program(node)
    names = {v: k for k, v in forms.OPS.items()}
    return program, [names[int(o)] for o in program.ops[: program.n_ops]]


def _proof(lib, program, bound):
    fast = (ctypes.c_uint8 * 32)(*([7] * 32))
    count = lib.tfem_source_trig_proof(ctypes.byref(program), float(bound), fast)
    flags = list(fast)
    assert count == sum(flags) and set(flags) <= {0, 1}
    return flags[: program.n_ops], flags[program.n_ops:]


SIN_SIN = ("mul", ("mul", ("sin", ("mul", ("x",), ("c", math.pi))), ("c", 2.0 * math.pi**2)),
           ("sin", ("mul", ("y",), ("c", math.pi))))


def test_the_bench_source_on_the_unit_square_is_proven(lib):
    program, names = _program(SIN_SIN)
    assert names.count("SIN") == 2 and names.count("PUSH_X") == 1 and names.count("PUSH_Y") == 1
    flags, rest = _proof(lib, program, 1.0)
    assert flags == [int(n == "SIN") for n in names] and not any(rest)
    for i, n in enumerate(names):  # the operand of both is the push in front
        if n == "SIN":
            assert names[i - 1] in ("PUSH_X", "PUSH_Y") and float(program.consts[i - 1]) == math.pi


def test_cos_and_a_negative_constant_are_proven_by_magnitude(lib):
    program, names = _program(("add", ("cos", ("mul", ("y",), ("c", -3.0e7))), ("sin", ("x",))))
    flags, _ = _proof(lib, program, 10.0)
    assert flags == [int(n in ("SIN", "COS")) for n in names] and sum(flags) == 2


def test_coordinates_too_large_are_not_proven(lib):
    program, names = _program(SIN_SIN)
    assert not any(_proof(lib, program, 4.0e8)[0])           # pi * 4e8 > 5e8
    assert sum(_proof(lib, program, 1.0e8)[0]) == 2          # pi * 1e8 < 5e8
    # one of two: sin(x) is proven at a bound where sin(1e3 y) is not
    program, names = _program(("add", ("sin", ("x",)), ("sin", ("mul", ("y",), ("c", 1.0e3)))))
    flags, _ = _proof(lib, program, 1.0e6)
    proven = [names[i - 1] for i, f in enumerate(flags) if f]
    assert proven == ["PUSH_X"]


def test_a_bound_exactly_at_the_limit_is_not_proven(lib):
    program, names = _program(("sin", ("x",)))
    assert names == ["PUSH_X", "SIN"] and float(program.consts[0]) == 1.0
    # the doubles around LIMIT / MARGIN: the first whose product reaches the limit, and one that hits it
    m = LIMIT / MARGIN
    while m * MARGIN >= LIMIT:
        m = np.nextafter(m, 0.0)
    while m * MARGIN < LIMIT:
        below, m = m, np.nextafter(m, np.inf)
    assert below * MARGIN < LIMIT <= m * MARGIN
    assert _proof(lib, program, below)[0] == [0, 1]
    assert _proof(lib, program, m)[0] == [0, 0]
    exact = [v for v in (np.nextafter(m, np.inf), m) if v * MARGIN == LIMIT]
    assert exact, "no double whose product is the limit itself"
    assert _proof(lib, program, exact[0])[0] == [0, 0]
    # the same limit through the constant: c = LIMIT on the unit square
    scaled, _ = _program(("sin", ("mul", ("x",), ("c", LIMIT))))
    assert float(scaled.consts[0]) == LIMIT and _proof(lib, scaled, 1.0)[0] == [0, 0]


def test_a_trig_operation_whose_operand_is_not_a_push_keeps_the_tested_path(lib):
    for node in (("sin", ("mul", ("x",), ("y",))),                 # behind MUL
                 ("cos", ("add", ("x",), ("c", 1.0))),             # behind ADD_C
                 ("sin", ("sin", ("x",))),                         # the outer sine behind SIN
                 ("add", ("x",), ("sin", ("c", 2.0)))):            # a constant push
        program, names = _program(node)
        flags, _ = _proof(lib, program, 1.0)
        for i, f in enumerate(flags):
            assert f == int(names[i] in ("SIN", "COS") and names[i - 1] in ("PUSH_X", "PUSH_Y")), (names, flags)
    program, names = _program(("sin", ("sin", ("x",))))
    assert _proof(lib, program, 1.0)[0] == [0, 1, 0]


def test_no_bound_no_proof(lib):
    program, _ = _program(SIN_SIN)
    for bound in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert not any(_proof(lib, program, bound)[0])
    assert sum(_proof(lib, program, 0.0)[0]) == 2  # every coordinate zero
    bad, _ = _program(SIN_SIN)
    bad.n_ops = 3  # PUSH_X SIN PUSH_Y leaves two values: not a valid program
    assert lib.tfem_source_validate(ctypes.byref(bad)) != 0 and not any(_proof(lib, bad, 1.0)[0])


def test_the_bound_travels_in_the_plan_layout_with_the_array_it_is_about(lib):
    layout = np.zeros(32, dtype=np.int64)
    at = ctypes.c_void_p(layout.ctypes.data)
    array = ctypes.c_void_p(0x7F0000001000)  # an address only: nothing is read through it
    assert lib.tfem_ring_plan_vouch_coords(at, array, 2.5) == 0
    assert layout[31:].view(np.float64)[0] == 2.5 and layout[29] == 0x7F0000001000
    assert not layout[:29].any() and layout[30] == 0
    assert lib.tfem_ring_plan_vouch_coords(at, array, 0.0) == 0  # every coordinate zero: a bound like any other
    assert layout[29] == 0x7F0000001000 and layout[31] == 0
    for withdrawn in (-1.0, float("nan"), float("inf")):
        layout[29] = layout[31] = 1
        assert lib.tfem_ring_plan_vouch_coords(at, array, withdrawn) == 0 and layout[29] == 0 and layout[31] == 0
    layout[29] = layout[31] = 1
    assert lib.tfem_ring_plan_vouch_coords(at, None, 1.0) == 0 and layout[29] == 0 and layout[31] == 0
    assert lib.tfem_ring_plan_vouch_coords(None, array, 1.0) != 0


def _launch_ops(lib, layout, array, program, real_bytes=8, order=3):
    ops = (ctypes.c_uint8 * 32)(*([7] * 32))
    at = ctypes.c_void_p(layout.ctypes.data)
    assert lib.tfem_p1_rings_source_ops(ctypes.c_void_p(array), real_bytes, order, at, ctypes.byref(program), ops) == 0
    return list(ops)


def test_what_a_launch_hands_its_kernel(lib):
    """tfem_p1_rings_source_ops: the proven operations (TFEM_SRC_OP_COUNT, + 1) appear for an fp64 launch of the
    wide interpreter that is given the vouched array, and nowhere else."""
    from pytorch_fem_solver_amd.basis import forms

    sin_proven, cos_proven = 23, 24
    program, names = _program(SIN_SIN)
    plain = [forms.OPS[n] for n in names] + [0] * (32 - len(names))
    proven = [sin_proven if n == "SIN" else o for n, o in zip(names, plain)] + [0] * (32 - len(names))
    layout = np.zeros(32, dtype=np.int64)
    at = ctypes.c_void_p(layout.ctypes.data)
    array, other = 0x7F0000001000, 0x7F0000002000
    assert _launch_ops(lib, layout, array, program) == plain           # no bound
    assert lib.tfem_ring_plan_vouch_coords(at, ctypes.c_void_p(array), 1.0) == 0
    assert _launch_ops(lib, layout, array, program) == proven
    assert _launch_ops(lib, layout, other, program) == plain           # another coordinate array
    assert _launch_ops(lib, layout, array, program, real_bytes=4) == plain
    assert _launch_ops(lib, layout, array, program, order=4) == plain  # Q = 6: the general interpreter
    for order in (1, 2):
        assert _launch_ops(lib, layout, array, program, order=order) == proven
    deep, deep_names = _program(("add", ("mul", ("x",), ("y",)),
                                 ("mul", ("add", ("sin", ("x",)), ("c", 2.0)), ("add", ("y",), ("x",)))))
    assert _launch_ops(lib, layout, array, deep)[: len(deep_names)] == [forms.OPS[n] for n in deep_names]  # depth 3
    cosine, cos_names = _program(("cos", ("mul", ("y",), ("c", 2.0))))
    assert _launch_ops(lib, layout, array, cosine)[:2] == [forms.OPS["PUSH_Y"], cos_proven]
    assert lib.tfem_ring_plan_vouch_coords(at, ctypes.c_void_p(array), 4.0e8) == 0
    assert _launch_ops(lib, layout, array, program) == plain           # pi * 4e8: not proven
    assert lib.tfem_ring_plan_vouch_coords(at, ctypes.c_void_p(array), 0.0) == 0
    assert _launch_ops(lib, layout, array, program) == proven          # a bound of zero is a bound
    assert lib.tfem_ring_plan_vouch_coords(at, None, -1.0) == 0
    assert _launch_ops(lib, layout, array, program) == plain
