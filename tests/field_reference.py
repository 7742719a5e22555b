"""Reference for P1 forms with coefficient DATA, alpha * kappa * stiffness + beta * c * mass with
kappa and c given as (E, Q) values at the integration points -- test infrastructure.

`reference_parts` integrates with oracle.assembly_oracle the way coefficient_reference.reference_parts
does (geometry, integrand_stiffness / integrand_mass, integrate_local, csr_pattern,
assemble_csr_values), on the caller's arrays.  The data are exact (what the kernel reads is what the
oracle reads), so the coefficient's spread term is zero and per CSR entry

    tol = base * max |K^ref|,        base = 1e-12 (float64) / 5e-5 (float32)

the ring kernels' parity tolerances (coefficient_reference.BASE_TOL).  K u and diag K take
coefficient_reference.apply_reference's row-wise bound, base * sum_j |K_ij| |u_j|.

`adjoint_reference` is the derivative of sum_cols g^T K u in the values, with numpy from the oracle's dx and
integrands: grad_kappa[e][q] = alpha * dx[e][q] * sum_cols g_e^T S[e][q] u_e, grad_c with the mass
integrand; tolerance base * max |reference gradient|.
"""

from __future__ import annotations

import numpy as np

import coefficient_reference as cref
from oracle import assembly_oracle as orc

BASE_TOL = cref.BASE_TOL
apply_reference = cref.apply_reference
dense = cref.dense
check = cref.check


def data(mesh_np, order, seed, dtype=np.float64, per_element=False):
    """(E, Q) (or (E, 1)) values, seeded, uniform in [0.5, 1.5], independent per (e, q), rounded to
    `dtype` (the values the kernel reads) and returned in that dtype."""
    n_elems = np.asarray(mesh_np["triangles"]).shape[0]
    nq = 1 if per_element else orc.gauss_rule(order)[0].shape[0]
    return np.random.default_rng(seed).uniform(0.5, 1.5, size=(n_elems, nq)).astype(dtype)


def _geometry(mesh_np, order, dtype):
    verts = np.asarray(mesh_np["vertices"]).astype(np.dtype(dtype))  # what a kernel in T sees
    tris = np.asarray(mesh_np["triangles"]).astype(np.int64)
    geo = orc.geometry(verts[tris].astype(np.float64), 1, order)
    return verts.shape[0], tris, geo


def _at_points(values, n_elems, nq):  # None | (E, Q) | (E, 1) -> (E, Q, 1, 1)
    if values is None:
        return np.ones((n_elems, nq, 1, 1))
    values = np.asarray(values, dtype=np.float64).reshape(n_elems, -1)
    return np.broadcast_to(values, (n_elems, nq))[:, :, None, None]


def reference_parts(mesh_np, order, alpha, beta, kappa, c, dtype=np.float64):
    """(rowptr, colind, want (nnz,), tol (nnz,), spread = 0 (nnz,), base) of the form with data kappa,
    c ((E, Q), (E, 1) or None = 1), in the caller's vertex numbering and oracle.csr_pattern's CSR."""
    dtype = np.dtype(dtype)
    n, tris, geo = _geometry(mesh_np, order, dtype)
    stiff, mass, dx = orc.integrand_stiffness(geo), orc.integrand_mass(geo), geo["dx"]
    n_elems, nq = tris.shape[0], dx.shape[-3]
    local = orc.integrate_local(alpha * _at_points(kappa, n_elems, nq) * stiff
                                + beta * _at_points(c, n_elems, nq) * mass, dx)
    rowptr, colind, slots = orc.csr_pattern(tris, n)
    nnz = colind.shape[0]
    want = orc.assemble_csr_values(local, slots, nnz)
    tol = np.full(nnz, BASE_TOL[dtype] * np.abs(want).max())
    return rowptr, colind, want, tol, np.zeros(nnz), BASE_TOL[dtype]


def adjoint_reference(mesh_np, order, alpha, beta, g, u, dtype=np.float64):
    """(grad_kappa (E, Q), grad_c (E, Q), tol_kappa, tol_c) of sum_cols g^T K u for g, u of shape (N,)
    or (N, k) in the caller's numbering."""
    dtype = np.dtype(dtype)
    n, tris, geo = _geometry(mesh_np, order, dtype)
    dx = np.asarray(geo["dx"])
    n_elems, nq = tris.shape[0], dx.shape[-3]
    dx = np.broadcast_to(dx, (n_elems, nq, 1, 1))[:, :, 0, 0]
    stiff = np.broadcast_to(orc.integrand_stiffness(geo), (n_elems, nq, 3, 3))
    mass = np.broadcast_to(orc.integrand_mass(geo), (n_elems, nq, 3, 3))
    g = np.asarray(g, dtype=np.float64).reshape(n, -1)[tris]  # (E, 3, k)
    u = np.asarray(u, dtype=np.float64).reshape(n, -1)[tris]
    grad_kappa = alpha * dx * np.einsum("eik,eqij,ejk->eq", g, stiff, u)
    grad_c = beta * dx * np.einsum("eik,eqij,ejk->eq", g, mass, u)
    base = BASE_TOL[dtype]
    return grad_kappa, grad_c, base * np.abs(grad_kappa).max(), base * np.abs(grad_c).max()
