"""Four load cases of -Laplace(u) = f on the unit square, u = 0 on the border, with P2 elements on the
hierarchy of poisson_p2_multigrid.py, solved by ONE multigrid-preconditioned block CG
(P2Multigrid.solve_multi): every launch of the V-cycle -- the P2 level's sweeps, its matrix-free
apply and its two transfers, and the P1 cycle below -- carries the four columns, the columns
converge -- and are frozen -- independently.

    python examples/poisson_p2_multigrid_loads.py [n] [levels]

prints the iterations of every column and the difference to four calls of P2Multigrid.solve.
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


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def load(i, j):
    """The load of the exact solution sin(i pi x) sin(j pi y)."""
    def linear(b):
        x, y = torch.split(b.integration_points, 1, dim=-1)
        return math.pi**2 * (i * i + j * j) * torch.sin(i * math.pi * x) * torch.sin(j * math.pi * y) * b.v

    linear.__name__ = f"mode ({i}, {j})"
    return linear


mg = P2Multigrid(meshgen.unit_square(n, 0.0, 0), levels, stiffness, quadrature_order=3)
loads = [load(i, j) for i, j in ((1, 1), (2, 1), (1, 3), (3, 2))]
B = torch.cat([mg.basis.integrate_linear_form(load).reshape(-1, 1) for load in loads], dim=1)

mg.solve_multi(B, rtol=1e-10)  # warm-up: block buffers, prepared launches
torch.cuda.synchronize()
t0 = time.perf_counter()
U, iterations, residuals = mg.solve_multi(B, rtol=1e-10)
torch.cuda.synchronize()
t_block = time.perf_counter() - t0

mg.solve(B[:, 0].contiguous(), rtol=1e-10)
torch.cuda.synchronize()
t0 = time.perf_counter()
singles = [mg.solve(B[:, j].contiguous(), rtol=1e-10) for j in range(len(loads))]
torch.cuda.synchronize()
t_singles = time.perf_counter() - t0

print(f"{mg.operator.shape[0]} P2 DoFs, {len(loads)} load cases")
for j, (load, (u, it, res)) in enumerate(zip(loads, singles)):
    difference = float((U[:, j] - u).abs().max() / u.abs().max())
    print(f"  {load.__name__:12s}: {int(iterations[j])} iterations (solve: {it}), residual {float(residuals[j]):.1e}, "
          f"differs from solve by {difference:.1e}")
    assert float(residuals[j]) <= 1e-10 and difference <= 1e-8
    assert abs(int(iterations[j]) - it) <= 2
print(f"one solve_multi {t_block * 1e3:.1f} ms, {len(loads)} x solve {t_singles * 1e3:.1f} ms")
