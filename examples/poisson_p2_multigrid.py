"""-Laplace(u) = 2 pi^2 sin(pi x) sin(pi y) on the unit square, u = 0 on the border, with P2 elements,
solved by conjugate gradients preconditioned with the P2 multigrid V-cycle (P2Multigrid): a P2 level
on the finest mesh of a P1 hierarchy -- the P2 residual is restricted to the P1 space of the same
mesh, the P1 V-cycle of GeometricMultigrid corrects it, and the P2 operator is applied matrix-free.
The number of iterations does not grow with the mesh, where the Jacobi-preconditioned CG doubles
its count with every refinement.

    python examples/poisson_p2_multigrid.py [n] [levels]

prints, for 1 .. levels refinements of the n x n coarse mesh, the P2 DoFs, the iterations of the
solve and the maximal nodal error (vertices and edge midpoints) against the exact solution
sin(pi x) sin(pi y).
"""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_fem import P2Multigrid  # noqa: E402  (the MI355X-native package)
from pytorch_fem_solver_amd import meshgen  # noqa: E402

torch.set_default_device("cuda")
torch.set_default_dtype(torch.float64)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
levels = int(sys.argv[2]) if len(sys.argv) > 2 else 3
coarse = meshgen.unit_square(n, 0.0, 0)


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def load(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return 2.0 * math.pi**2 * torch.sin(math.pi * x) * torch.sin(math.pi * y) * b.v


for level in range(1, levels + 1):
    mg = P2Multigrid(coarse, level, stiffness, quadrature_order=3)
    f = mg.basis.integrate_linear_form(load)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u, iterations, residual = mg.solve(f, rtol=1e-10)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    # the P2 DoFs: the vertices, then the midpoints of the mesh's edges
    mesh = mg.levels[-1].triangulation
    vertices = torch.as_tensor(mesh["vertices"])
    midpoints = vertices[torch.as_tensor(mesh["edges"]).long()].mean(dim=1)
    pts = torch.cat([vertices, midpoints])
    exact = (torch.sin(math.pi * pts[:, 0]) * torch.sin(math.pi * pts[:, 1])).reshape(u.shape)
    error = float((u - exact).abs().max())
    print(f"level {level}: {mg.operator.shape[0]} DoFs, {iterations} iterations, residual {residual:.1e}, "
          f"max nodal error {error:.3e}, {seconds * 1e3:.1f} ms")
    assert residual <= 1e-10 and iterations <= 20
