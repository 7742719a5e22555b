"""The Poisson problem of poisson_operator_cg.py with QUADRATIC elements, solved without assembling K:
layout="matrix_free" gives an operator that forms the rows of the P2 stiffness matrix in registers
from the mesh's row plan in every CG iteration and writes K u (tfem_p2_apply_rows); the 12 bytes per
entry of K never reach memory.  The strict layout raises NotImplementedError instead of assembling
when a basis has no such launch.  Then the same solve on the assembled CSR operator for comparison.

    python examples/poisson_p2_operator_cg.py [n]
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
mesh_np = meshgen.unit_square(n, 0.25, 0)
basis = Basis(MeshTri(triangulation=mesh_np), ElementTri(polynomial_order=2, integration_order=4))


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def load(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return 2.0 * math.pi**2 * torch.sin(math.pi * x) * torch.sin(math.pi * y) * b.v


A = basis.integrate_bilinear_form(stiffness, layout="matrix_free")  # builds the row plan, assembles nothing
K = basis.integrate_bilinear_form(stiffness, layout="csr")
f = basis.integrate_linear_form(load)
free = basis._basis_parameters["inner_dofs"]
print(f"{mesh_np['triangles'].shape[0]} elements, {A.shape[0]} DoFs, {A}")
assert A.matrix_free

x_free, it_free, res_free = A.solve_cg(f, free=free, rtol=1e-10)
x_csr, it_csr, res_csr = K.solve_cg(f, free=free, rtol=1e-10)
diff = float((x_free - x_csr).abs().max() / x_csr.abs().max())
print(f"CG on the matrix-free operator: {it_free} iterations, residual {res_free:.1e}")
print(f"CG on the CSR operator        : {it_csr} iterations, residual {res_csr:.1e}")
print(f"max difference of the two solutions, relative to the largest entry: {diff:.1e}")
assert res_free <= 1e-10 and abs(it_free - it_csr) <= 25 and diff <= 1e-8

for name, op in (("matrix-free", A), ("CSR", K)):
    basis.solve(op, basis.solution_tensor(), f, method="cg")  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u = basis.solve(op, basis.solution_tensor(), f, method="cg")
    torch.cuda.synchronize()
    # the vertex DoFs come first: the nodal error of the quadratic solution at the mesh's vertices
    pts = torch.as_tensor(mesh_np["vertices"])
    exact = torch.sin(math.pi * pts[:, 0]) * torch.sin(math.pi * pts[:, 1])
    err = float((u.reshape(-1)[: pts.shape[0]] - exact).abs().max())
    print(f"Basis.solve on the {name:11s} operator: {time.perf_counter() - t0:.2f} s, max nodal error {err:.2e}")
    assert err <= 10.0 * (math.pi / n) ** 3, "a quadratic element resolves sin(pi x) sin(pi y) to O(h^3)"
