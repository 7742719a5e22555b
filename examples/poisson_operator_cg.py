"""The Poisson problem of poisson_large_cg.py solved WITHOUT assembling K: the operator of the
reference's stiffness form is applied matrix-free (layout="operator": every CG iteration forms the
rows of K in registers from the mesh and writes K u; the 48 bytes per element of K never reach
memory), then the same solve on the assembled CSR operator for comparison.

    python examples/poisson_operator_cg.py [n]
"""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_fem import Basis, ElementTri, MeshTri  # noqa: E402  (the MI355X-native package)
from pytorch_fem_solver_amd import meshgen  # noqa: E402

torch.set_default_device("cuda")
torch.set_default_dtype(torch.float64)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
mesh_np = meshgen.unit_square(n, 0.25, 0)
basis = Basis(MeshTri(triangulation=mesh_np), ElementTri(polynomial_order=1, integration_order=3))


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def load(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return 2.0 * math.pi**2 * torch.sin(math.pi * x) * torch.sin(math.pi * y) * b.v


A = basis.integrate_bilinear_form(stiffness, layout="operator")  # launches nothing
f = basis.integrate_linear_form(load)
pts = torch.as_tensor(mesh_np["vertices"])
exact = (torch.sin(math.pi * pts[:, 0]) * torch.sin(math.pi * pts[:, 1])).reshape(-1, 1)
print(f"{mesh_np['triangles'].shape[0]} elements, {A.shape[0]} DoFs, {A}")
for name, op in (("matrix-free", A), ("CSR", basis.integrate_bilinear_form(stiffness, layout="csr"))):
    basis.solve(op, basis.solution_tensor(), f)  # warm-up (the ring plan is built on first use)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u = basis.solve(op, basis.solution_tensor(), f, method="cg")
    torch.cuda.synchronize()
    print(f"CG on the {name:11s} operator: {time.perf_counter() - t0:.2f} s, "
          f"max nodal error {float((u - exact).abs().max()):.2e}")
