"""Reference for variable-coefficient P1 forms alpha * kappa * stiffness + beta * c * mass -- test
infrastructure.

The coefficients are fixed, written once as functions of the coordinate columns that run on
torch tensors AND on the tracer's symbols, and chosen so that every integration point is
`decided` in tests/source_reference.evaluate: strictly positive, no divisor / log / sqrt
argument near zero.  `reference` integrates with oracle.assembly_oracle (any integrand) on
coefficient values from source_reference.evaluate (long double, with its per-point bound) and
returns (want, tol) per CSR entry:

    tol = base * max |K^ref|  +  sum_e sum_q |dx_q integrand_ij(e, q)| bound_q

base = 1e-12 (float64) / 5e-5 (float32), the ring kernels' parity tolerances of
tests/test_hip_fuzz.py; the second term is the coefficient's own error bound propagated through
the (linear) quadrature sum, the way source_reference.load_reference builds the tolerance of a
load vector.
"""

from __future__ import annotations

import numpy as np
import torch

import source_reference as ref
from oracle import assembly_oracle as orc

BASE_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 5e-5}


def kappa_xy(x, y):
    return 1.0 + x * y


def kappa_trig(x, y):
    return 1.0 + 0.5 * torch.sin(3 * x) * torch.cos(2 * y)


def c_exp(x, y):
    return torch.exp(-x)


def kappa_poly(x, y):
    return 2 + x ** 2 + y


def c_rational(x, y):
    return 1 / (1 + x * x + y * y)


COEFFICIENTS = {"xy": kappa_xy, "trig": kappa_trig, "exp": c_exp, "poly": kappa_poly, "rational": c_rational}


def ops_of(fn):
    """(op codes, constants) of the program the tracer compiles for fn(x, y)."""
    from pytorch_fem_solver_amd.basis import forms

    field = fn(forms.SourceExpr(None, ("x",)), forms.SourceExpr(None, ("y",)))
    assert isinstance(field, forms.SourceExpr), "the coefficient left the tracer's vocabulary"
    ops = forms.compile_ops(field.node)
    assert ops is not None
    return [forms.OPS[name] for name, _ in ops], [float(c) for _, c in ops]


def form(alpha, beta, kappa, c):
    """The bilinear-form callable alpha * kappa * stiffness + beta * c * mass (kappa / c: a function
    of (x, y) or None)."""
    def bilinear(basis):
        x, y = torch.split(basis.integration_points, 1, dim=-1)
        out = None
        if alpha != 0.0:
            s = basis.v_grad @ basis.v_grad.mT
            s = kappa(x, y) * s if kappa is not None else s
            out = s if alpha == 1.0 else alpha * s
        if beta != 0.0:
            m = basis.v @ basis.v.mT
            m = c(x, y) * m if c is not None else m
            m = m if beta == 1.0 else beta * m
            out = m if out is None else out + m
        return out

    return bilinear


def coefficient_values(fn, cells, order, dtype):
    """(value, bound) (E, Q) of fn at the integration points, every point decided (asserted)."""
    if fn is None:
        shape = (cells.shape[0], ref.rule(order)[0].shape[0])
        return np.ones(shape, dtype=ref.LD), np.zeros(shape, dtype=ref.LD)
    ops, consts = ops_of(fn)
    value, bound, decided = ref.evaluate(ops, consts, cells, order, dtype)
    assert decided.all() and np.isfinite(value).all(), "a coefficient of these tests must be decided everywhere"
    assert (value > 0).all()
    return value, bound


def reference(mesh_np, order, alpha, beta, kappa, c, dtype=np.float64):
    """(rowptr, colind, want (nnz,), tol (nnz,)) of the form on the mesh, in the caller's vertex
    numbering and the sorted-column CSR pattern of oracle.csr_pattern."""
    return reference_parts(mesh_np, order, alpha, beta, kappa, c, dtype)[:4]


def reference_parts(mesh_np, order, alpha, beta, kappa, c, dtype=np.float64):
    """reference(...) + (spread (nnz,), base): the coefficient bound's share of tol per entry and
    the parity tolerance of the real type."""
    dtype = np.dtype(dtype)
    verts = np.asarray(mesh_np["vertices"]).astype(dtype)  # what a kernel in T sees
    tris = np.asarray(mesh_np["triangles"]).astype(np.int64)
    n = verts.shape[0]
    cells = verts[tris]
    geo = orc.geometry(cells.astype(np.float64), 1, order)
    kv, kb = coefficient_values(kappa, cells, order, dtype)
    cv, cb = coefficient_values(c, cells, order, dtype)
    stiff, mass, dx = orc.integrand_stiffness(geo), orc.integrand_mass(geo), geo["dx"]

    def at_points(a):  # (E, Q) -> (E, Q, 1, 1)
        return np.asarray(a, dtype=np.float64)[:, :, None, None]

    local = orc.integrate_local(alpha * at_points(kv) * stiff + beta * at_points(cv) * mass, dx)
    spread = orc.integrate_local(abs(alpha) * at_points(kb) * np.abs(stiff) + abs(beta) * at_points(cb) * np.abs(mass),
                                 np.abs(dx))
    rowptr, colind, slots = orc.csr_pattern(tris, n)
    nnz = colind.shape[0]
    want = orc.assemble_csr_values(local, slots, nnz)
    spread = orc.assemble_csr_values(spread, slots, nnz)
    tol = BASE_TOL[dtype] * np.abs(want).max() + spread
    return rowptr, colind, want, tol, spread, BASE_TOL[dtype]


def apply_reference(parts, u):
    """(K^ref u, tolerance (n,)) for a vector u: base * sum_j |K_ij| |u_j| + sum_j spread_ij |u_j|.
    u = ones gives the tolerance of the diagonal, which the launches form from the row's other entries."""
    rowptr, colind, want, _, spread, base = parts
    n = rowptr.shape[0] - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    y = np.bincount(rows, want * u[colind], minlength=n)
    tol = base * np.bincount(rows, np.abs(want * u[colind]), minlength=n) \
        + np.bincount(rows, spread * np.abs(u[colind]), minlength=n)
    return y, tol


def dense(rowptr, colind, vals, n):
    return orc.csr_to_dense(rowptr, colind, vals, n)


def check(got, want, tol, what):
    """Asserts |got - want| <= tol entry by entry; returns max |err| / tol."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - np.asarray(want, dtype=np.float64))
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), err.shape)
    assert (err[tol == 0] == 0).all(), f"{what}: an entry outside the pattern is not zero"
    ratio = float((err[tol > 0] / tol[tol > 0]).max())
    print(f"{what}: max |err| / tol = {ratio:.3e}")
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), f"{what}: max |err| / tol = {ratio:.3e}"
    return ratio
