"""CPU model of the geometric multigrid (pytorch_fem_solver_amd/multigrid.py) -- test
infrastructure: numpy / scipy only, K per level from oracle.assembly_oracle (with coefficients from
coefficient_reference.reference), P from the parent tables of meshgen.refine_uniform.

    l = 0:  z[free] = K0[free, free]^-1 r[free], 0 elsewhere
    else:   x = w r;  (nu - 1) x  x += w (r - K x)            w = omega * m / diag K
            x += m P vcycle_{l-1}( m_c P^T( m (r - K x) ) )
            nu x  x += w (r - K x)

and conjugate gradients preconditioned by it, the relative residual |r| / |m b| checked every
iteration."""

from __future__ import annotations

import numpy as np
import scipy.linalg
import scipy.sparse as sp

from oracle import assembly_oracle as orc


def refine(coarse, levels):
    """(meshes (levels + 1), parents (levels)) of the hierarchy above `coarse`."""
    from pytorch_fem_solver_amd import meshgen

    meshes, parents = [coarse], []
    for _ in range(levels):
        fine, par = meshgen.refine_uniform(meshes[-1])
        meshes.append(fine)
        parents.append(par)
    return meshes, parents


def prolongation(parents, n_coarse):
    """P (n_fine, n_coarse) as a scipy CSR: 0.5 at (i, parents[i, 0]) and at (i, parents[i, 1]),
    summed to 1 for a kept vertex."""
    n_fine = parents.shape[0]
    rows = np.repeat(np.arange(n_fine), 2)
    P = sp.coo_matrix((np.full(2 * n_fine, 0.5), (rows, parents.reshape(-1).astype(np.int64))),
                      shape=(n_fine, n_coarse))
    return P.tocsr()


def operator(mesh, order=2, alpha=1.0, beta=0.0, kappa=None, c=None):
    """alpha * kappa * stiffness + beta * c * mass on `mesh` as a scipy CSR (float64)."""
    verts = np.asarray(mesh["vertices"], dtype=np.float64)
    tris = np.asarray(mesh["triangles"]).astype(np.int64)
    n = verts.shape[0]
    if kappa is not None or c is not None:
        import coefficient_reference as cref

        rowptr, colind, vals, _ = cref.reference(mesh, order, alpha, beta, kappa, c)
    else:
        rowptr, colind, slots = orc.csr_pattern(tris, n)
        vals = np.zeros(colind.shape[0])
        for name, scale in (("stiffness", alpha), ("mass", beta)):
            if scale:
                local, _ = orc.p1_assemble(verts, tris, order, name)
                vals += scale * orc.assemble_csr_values(local, slots, colind.shape[0])
    return sp.csr_matrix((vals, colind, rowptr), shape=(n, n))


def interior_mask(mesh, dirichlet=True):
    """1 on the DoFs Basis calls inner_dofs (vertex marker != 1), all ones without Dirichlet."""
    markers = np.asarray(mesh["vertex_markers"]).reshape(-1)
    return (markers != 1).astype(np.float64) if dirichlet else np.ones(markers.shape[0])


class Model:
    def __init__(self, coarse, levels, order=2, alpha=1.0, beta=0.0, kappa=None, c=None, dirichlet=True, nu=2,
                 omega=2.0 / 3.0):
        self.meshes, self.parents = refine(coarse, levels)
        self.K = [operator(m, order, alpha, beta, kappa, c) for m in self.meshes]
        self.P = [None] + [prolongation(p, self.K[l].shape[0]) for l, p in enumerate(self.parents)]
        self.mask = [interior_mask(m, dirichlet) for m in self.meshes]
        self.w = [omega * m / K.diagonal() for m, K in zip(self.mask, self.K)]
        self.nu = nu
        free = np.flatnonzero(self.mask[0])
        self.free0 = free
        dense = self.K[0][free][:, free].toarray()
        try:
            factor = scipy.linalg.cho_factor(dense)
            self.solve0 = lambda r: scipy.linalg.cho_solve(factor, r)
        except np.linalg.LinAlgError:
            # the forms carry the signed determinant: with triangles stored clockwise K0 is not
            # positive definite, and the coarse solve is an LU
            lu = scipy.linalg.lu_factor(dense)
            self.solve0 = lambda r: scipy.linalg.lu_solve(lu, r)

    @property
    def top(self):
        return len(self.K) - 1

    def vcycle(self, r, l=None):
        l = self.top if l is None else l
        if l == 0:
            z = np.zeros_like(r)
            z[self.free0] = self.solve0(r[self.free0])
            return z
        K, w, m = self.K[l], self.w[l], self.mask[l]
        x = w * r
        for _ in range(self.nu - 1):
            x = x + w * (r - K @ x)
        coarse = self.mask[l - 1] * (self.P[l].T @ (m * (r - K @ x)))
        x = x + m * (self.P[l] @ self.vcycle(coarse, l - 1))
        for _ in range(self.nu):
            x = x + w * (r - K @ x)
        return x

    def pcg(self, b, rtol=1e-10, maxiter=100):
        """(x, iterations, relative residual) of CG preconditioned by the cycle, from x = 0."""
        return _pcg(self.K[-1], self.mask[-1], self.vcycle, b, rtol, maxiter)

    def jacobi_cg(self, b, rtol=1e-10, maxiter=100000):
        inv = self.mask[-1] / self.K[-1].diagonal()
        return _pcg(self.K[-1], self.mask[-1], lambda r: inv * r, b, rtol, maxiter)


def _pcg(K, m, precondition, b, rtol, maxiter):
    x = np.zeros_like(b)
    r = m * b
    b_norm = max(np.linalg.norm(m * b), np.finfo(np.float64).tiny)
    it, res = 0, np.linalg.norm(r) / b_norm
    if res <= rtol or maxiter <= 0:
        return x, it, res
    p = precondition(r)
    rz = r @ p
    while True:
        ap = m * (K @ p)
        alpha = rz / (p @ ap)
        x = x + alpha * p
        r = r - alpha * ap
        it += 1
        res = np.linalg.norm(r) / b_norm
        if res <= rtol or it >= maxiter:
            return x, it, res
        z = precondition(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new


def masked_rhs(model, seed=2):
    """The right-hand side of the model's measurements: masked standard normal."""
    n = model.K[-1].shape[0]
    return model.mask[-1] * np.random.default_rng(seed).standard_normal(n)
