"""-Laplace(u) = 2 pi^2 sin(pi x) sin(pi y) on the unit square, u = 0 on the border, solved by
conjugate gradients preconditioned with a geometric multigrid V-cycle (GeometricMultigrid): the
coarse mesh is refined uniformly, every level applies its operator matrix-free, and the number of
iterations does not grow with the mesh -- where the Jacobi-preconditioned CG of
poisson_operator_cg.py doubles its count with every refinement.

    python examples/poisson_multigrid.py [n] [levels]

prints, for 1 .. levels refinements of the n x n coarse mesh, the iterations of the solve and the
maximal nodal error against the exact solution sin(pi x) sin(pi y), which falls by about 4 per
level (P1, h^2).
"""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_fem import GeometricMultigrid  # noqa: E402  (the MI355X-native package)
from pytorch_fem_solver_amd import meshgen  # noqa: E402

torch.set_default_device("cuda")
torch.set_default_dtype(torch.float64)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
levels = int(sys.argv[2]) if len(sys.argv) > 2 else 4
coarse = meshgen.unit_square(n, 0.0, 0)


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def load(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return 2.0 * math.pi**2 * torch.sin(math.pi * x) * torch.sin(math.pi * y) * b.v


for level in range(1, levels + 1):
    mg = GeometricMultigrid(coarse, level, stiffness, quadrature_order=3)
    f = mg.basis.integrate_linear_form(load)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u, iterations, residual = mg.solve(f, rtol=1e-10)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    pts = torch.as_tensor(mg.levels[-1].triangulation["vertices"])
    exact = (torch.sin(math.pi * pts[:, 0]) * torch.sin(math.pi * pts[:, 1])).reshape(u.shape)
    error = float((u - exact).abs().max())
    print(f"level {level}: {mg.operator.shape[0]} DoFs, {iterations} iterations, residual {residual:.1e}, "
          f"max nodal error {error:.3e}, {seconds * 1e3:.1f} ms")
    assert residual <= 1e-10 and iterations <= 20
