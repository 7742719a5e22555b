"""Variable-coefficient bilinear forms in the tracer (basis/forms.py) and the C ABI's two entry
points for them -- no GPU needed."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import coefficient_reference as cref
from conftest import REPO


class _FakeBasis:
    def __init__(self):
        self.integration_points = torch.rand(5, 4, 1, 2, dtype=torch.float64)
        self.v = torch.rand(4, 3, 1, dtype=torch.float64)
        self.v_grad = torch.rand(5, 1, 3, 2, dtype=torch.float64)
        self.mesh = "mesh"


def _forms():
    from pytorch_fem_solver_amd.basis import forms

    return forms


def _xy(basis):
    return torch.split(basis.integration_points, 1, dim=-1)


def _stiff(basis):
    return basis.v_grad @ basis.v_grad.mT


def _mass(basis):
    return basis.v @ basis.v.mT


def issue_form(basis):
    x, y = _xy(basis)
    return (1.0 + 0.5 * torch.sin(3 * x) * y) * (basis.v_grad @ basis.v_grad.mT) \
        + torch.exp(-x) * (basis.v @ basis.v.mT)


def test_the_issues_form_traces_to_two_coefficient_programs():
    forms = _forms()
    b = _FakeBasis()
    e = forms.trace(issue_form, b, (), {})
    assert isinstance(e, forms.BilinearExpr) and e.has_coefficients
    assert (e.alpha, e.beta) == (1.0, 1.0)
    assert isinstance(e.kappa, forms.SourceExpr) and isinstance(e.c, forms.SourceExpr)
    kappa, c = e.kappa.program(), e.c.program()
    assert kappa is not None and c is not None and kappa.n_ops > 0 and c.n_ops > 0
    assert [name for name, _ in forms.compile_ops(e.c.node)] == ["PUSH_X", "NEG", "EXP"]
    # the operation order is the caller's: coefficient * form, term + term
    assert torch.equal(e.materialize(), issue_form(b))
    # constant-coefficient forms carry no fields
    plain = forms.trace(lambda basis: 2.0 * _stiff(basis) + _mass(basis), b, (), {})
    assert plain.kappa is None and plain.c is None and not plain.has_coefficients


CASES = {
    "field_times_stiffness": lambda b: cref.kappa_xy(*_xy(b)) * _stiff(b),
    "stiffness_times_field": lambda b: _stiff(b) * cref.kappa_trig(*_xy(b)),
    "torch_mul": lambda b: torch.mul(cref.kappa_poly(*_xy(b)), _stiff(b)),
    "torch_mul_reversed": lambda b: torch.mul(_mass(b), cref.c_exp(*_xy(b))),
    "mass_over_field": lambda b: _mass(b) / (1 + _xy(b)[0] * _xy(b)[0]),
    "stiffness_over_field": lambda b: _stiff(b) / cref.kappa_poly(*_xy(b)),
    "scalar_factors": lambda b: 2.0 * (cref.kappa_xy(*_xy(b)) * _stiff(b)) + (cref.c_exp(*_xy(b)) * _mass(b)) * 0.5,
    "negated": lambda b: -(cref.kappa_xy(*_xy(b)) * _stiff(b)),
    "sum_of_two_fields": lambda b: cref.kappa_xy(*_xy(b)) * _stiff(b) + 3.0 * (cref.kappa_trig(*_xy(b)) * _stiff(b)),
    "difference_of_two_fields": lambda b: cref.c_exp(*_xy(b)) * _mass(b) - cref.c_rational(*_xy(b)) * _mass(b),
    "field_plus_constant_term": lambda b: cref.kappa_xy(*_xy(b)) * _stiff(b) + 2.0 * _stiff(b) + _mass(b),
    "two_fields_on_one_term": lambda b: cref.kappa_xy(*_xy(b)) * (cref.kappa_poly(*_xy(b)) * _stiff(b)),
    "difference_with_mass": lambda b: cref.kappa_trig(*_xy(b)) * _stiff(b) - cref.c_exp(*_xy(b)) * _mass(b),
}


#: the cases whose materialised form associates differently from the callable (see the test)
REASSOCIATED = {"mass_over_field", "stiffness_over_field", "sum_of_two_fields", "difference_of_two_fields",
                "field_plus_constant_term", "two_fields_on_one_term"}


@pytest.mark.parametrize("name", list(CASES))
def test_coefficient_forms_stay_symbolic_and_materialise_to_the_callable(name):
    forms = _forms()
    b = _FakeBasis()
    e = forms.trace(CASES[name], b, (), {})
    assert isinstance(e, forms.BilinearExpr) and e.has_coefficients, name
    assert all(field is None or field.program() is not None for field in (e.kappa, e.c))
    want = CASES[name](b)
    got = e.materialize()
    assert got.shape == want.shape
    if name in REASSOCIATED:
        # fields of one term are summed / multiplied BEFORE the product with the form, a quotient
        # becomes a product with the reciprocal: one or two roundings of difference per entry, so the
        # bound is 1e-15 relative to the entries' magnitude (|want| reaches ~10 here, where one ulp
        # is 1.8e-15: a plain atol = 1e-15 is below the spacing of the numbers compared)
        assert torch.allclose(got, want, rtol=0, atol=1e-15 * max(1.0, float(want.abs().max()))), name
    else:  # the operation order is the caller's
        assert torch.equal(got, want), name


def test_a_constant_written_as_a_field_folds_into_the_scalar():
    forms = _forms()
    b = _FakeBasis()
    e = forms.trace(lambda basis: (2.5 * torch.ones_like(_xy(basis)[0])) * _stiff(basis), b, (), {})
    assert isinstance(e, forms.BilinearExpr) and not e.has_coefficients
    assert (e.alpha, e.beta) == (2.5, 0.0)
    assert torch.equal(e.materialize(), 2.5 * _stiff(b))


REFUSED = {
    "tensor_coefficient": lambda b: _stiff(b) * torch.ones(5, 4, 1, 1, dtype=torch.float64),
    "tensor_coefficient_left": lambda b: torch.full((5, 4, 1, 1), 2.0, dtype=torch.float64) * _mass(b),
    "field_times_mixed_sum": lambda b: cref.kappa_xy(*_xy(b)) * (_stiff(b) + _mass(b)),
    "mixed_sum_over_field": lambda b: (_stiff(b) + 2.0 * _mass(b)) / cref.kappa_poly(*_xy(b)),
    "anisotropic": lambda b: (b.v_grad @ torch.tensor([[2.0, 0.5], [0.5, 1.0]], dtype=torch.float64)) @ b.v_grad.mT,
    "field_on_the_other_term_then_product": lambda b: cref.kappa_xy(*_xy(b)) * (cref.c_exp(*_xy(b)) * _mass(b) + _stiff(b)),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_shapes_outside_the_vocabulary_come_back_as_tensors(name):
    forms = _forms()
    b = _FakeBasis()
    out = forms.trace(REFUSED[name], b, (), {})
    assert isinstance(out, torch.Tensor) and not isinstance(out, forms._Symbol), name
    assert torch.equal(out, REFUSED[name](b)), name


def test_a_field_that_fits_no_program_is_reported():
    forms = _forms()
    b = _FakeBasis()

    def long_field(basis):
        x, y = _xy(basis)
        k = x
        for i in range(40):
            k = torch.sin(k) + (i + 1.5)
        return k * _stiff(basis)

    e = forms.trace(long_field, b, (), {})
    assert isinstance(e, forms.BilinearExpr) and e.kappa is not None
    assert e.kappa.program() is None
    assert torch.equal(e.materialize(), long_field(b))


def test_reference_coefficients_are_decided_everywhere():
    """The fixed coefficients of the GPU tests on their meshes: every point decided, positive --
    a bad choice fails here, on the CPU, before anything is launched."""
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(12, 0.25, 3)
    for order in (1, 2, 3, 4):
        for dtype in (np.float64, np.float32):
            for fn in cref.COEFFICIENTS.values():
                cells = mesh_np["vertices"].astype(dtype)[mesh_np["triangles"]]
                value, bound = cref.coefficient_values(fn, cells, order, dtype)
                assert value.shape == bound.shape == (cells.shape[0], {1: 1, 2: 3, 3: 4, 4: 6}[order])
    _, _, want, tol = cref.reference(mesh_np, 3, 1.0, 0.5, cref.kappa_trig, cref.c_exp)
    base = 1e-12 * np.abs(want).max()
    assert (tol >= base).all() and (tol > base).any() and tol.max() < 2 * base
    # with constant coefficients the reference is the oracle's own assembly
    _, _, plain, _ = cref.reference(mesh_np, 3, 2.0, 0.5, None, None)
    local, _ = orc_local(mesh_np)
    assert np.allclose(plain, local, rtol=0, atol=1e-14 * np.abs(local).max())


def orc_local(mesh_np):
    from oracle import assembly_oracle as orc

    verts, tris = mesh_np["vertices"], mesh_np["triangles"]
    rowptr, colind, slots = orc.csr_pattern(tris, verts.shape[0])
    vals = np.zeros(colind.shape[0])
    for name, factor in (("stiffness", 2.0), ("mass", 0.5)):
        local, _ = orc.p1_assemble(verts, tris, 3, name)
        vals += factor * orc.assemble_csr_values(local, slots, colind.shape[0])
    return vals, rowptr


def test_header_declares_and_library_exports_the_coefficient_entry_points():
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(tfem_[a-z0-9_]+)\(", header, re.M))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    for name in ("tfem_p1_rings_coef", "tfem_p1_apply_rings_coef"):
        assert name in declared, f"{name} is not declared in tfem_assembly.h"
        assert name in exported and hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES, f"{name} has no ctypes signature"
    # both take the two programs behind (alpha, beta) and the plan behind them
    assert len(_native.SIGNATURES["tfem_p1_rings_coef"][1]) == 12
    assert len(_native.SIGNATURES["tfem_p1_apply_rings_coef"][1]) == 13


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Both programs NULL, an invalid program, n_verts = 0: decided on the host, before any
    launch (no GPU is touched: this runs on a machine without one)."""
    import ctypes

    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    layout = np.zeros(32, dtype=np.int64)
    layout[0] = 1  # one tile: a launch would follow if the checks let it through
    z = ctypes.c_void_p(layout.ctypes.data)
    good = cref_program(cref.kappa_xy)
    bad = _native.SourceProgram()
    bad.n_ops = 2
    bad.ops[0], bad.ops[1] = 4, 4  # ADD on an empty stack
    for call, tail in ((lib.tfem_p1_rings_coef, (None, None)), (lib.tfem_p1_apply_rings_coef, (None, None, None))):
        assert call(None, 8, 10, 3, 1.0, 0.0, None, None, None, z, *tail) == 1  # TFEM_ERR_INVALID_ARGUMENT
        assert b"coefficient" in lib.tfem_last_error()
        assert call(None, 8, 10, 3, 1.0, 1.0, ctypes.byref(bad), None, None, z, *tail) == 1
        assert call(None, 8, 10, 3, 1.0, 1.0, ctypes.byref(good), ctypes.byref(bad), None, z, *tail) == 1
        assert call(None, 8, 0, 3, 1.0, 0.0, ctypes.byref(good), None, None, z, *tail) == 0  # nothing to do
        assert call(None, 8, -1, 3, 1.0, 0.0, ctypes.byref(good), None, None, z, *tail) == 1
        assert call(None, 2, 10, 3, 1.0, 0.0, ctypes.byref(good), None, None, z, *tail) == 1
        assert call(None, 8, 10, 9, 1.0, 0.0, ctypes.byref(good), None, None, z, *tail) == 2  # TFEM_ERR_UNSUPPORTED
        assert call(None, 8, 10, 3, 1.0, 0.0, ctypes.byref(good), None, None, z, *tail) == 1  # NULL pointers


def cref_program(fn):
    import source_reference as ref

    return ref.to_native(*cref.ops_of(fn))


def test_no_coefficient_kernel_uses_scratch_memory(tmp_path):
    """Every instance of csrc/tfem_rings_coef.hip, compiled for gfx950 with the build's own flags:
    no scratch memory (the interpreter's arrays keep static indices), at most 256 VGPRs -- read from
    the assembly with tools/kernel_regs.py."""
    import sys

    import __graft_entry__ as entry

    name = "tfem_rings_coef.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the kernels cannot be compiled")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS[name]
    asm = tmp_path / "coef.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(REPO, "include"),
                    "-o", str(asm), os.path.join(entry.CSRC, name)], check=True, capture_output=True)
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), str(asm), "k_p1_coef_rows"],
                         check=True, capture_output=True, text=True).stdout
    rows = [re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)", line) for line in out.splitlines()]
    assert len(rows) == 192 and all(rows), out[-2000:]
    bad = [m.group(5) for m in rows if int(m.group(3)) != 0 or int(m.group(1)) > 256]
    assert not bad, bad
