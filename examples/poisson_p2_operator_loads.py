"""The four load cases of poisson_p2_multiple_loads.py with QUADRATIC elements and WITHOUT K:
layout="matrix_free" gives an operator over the P2 row plan, and ONE Basis.solve call with an (N, 4)
right-hand side runs one block CG on it -- every iteration is one tfem_p2_apply_rows_multi call that
reads the plan's records and the pattern's column indices once, forms every row of K once in
registers and multiplies it with the four values of each column's row.  The 12 bytes per entry of K
never reach memory.  Then the same systems through solve_cg_multi, with the residual of every column.

    python examples/poisson_p2_operator_loads.py [n]
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
MODES = ((1, 1), (2, 1), (1, 3), (2, 2))


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def load(i, j):
    def linear(b):
        x, y = torch.split(b.integration_points, 1, dim=-1)
        return math.pi**2 * (i * i + j * j) * torch.sin(i * math.pi * x) * torch.sin(j * math.pi * y) * b.v

    return linear


A = basis.integrate_bilinear_form(stiffness, layout="matrix_free")  # builds the row plan, assembles nothing
F = torch.cat([basis.integrate_linear_form(load(i, j)) for i, j in MODES], dim=1)  # (N, 4)
free = basis._basis_parameters["inner_dofs"]
# the vertex DoFs come first: the nodal error of the quadratic solutions at the mesh's vertices
pts = torch.as_tensor(mesh_np["vertices"])
exact = torch.stack([torch.sin(i * math.pi * pts[:, 0]) * torch.sin(j * math.pi * pts[:, 1]) for i, j in MODES], dim=1)
print(f"{mesh_np['triangles'].shape[0]} elements, {A.shape[0]} DoFs, {len(MODES)} load cases, {A}")
assert A.matrix_free

basis.solve(A, torch.zeros_like(F), F)  # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
U = basis.solve(A, torch.zeros_like(F), F)  # (N, 4) in, (N, 4) out: one block CG, K never assembled
torch.cuda.synchronize()
t_block = time.perf_counter() - t0

X, its, res = A.solve_cg_multi(F, free=free, rtol=1e-10)
# the residual of every column on the free DoFs, from one application of the operator to the block
R = (F - A @ X)[free]
for c, (i, j) in enumerate(MODES):
    err = float((U[: pts.shape[0], c] - exact[:, c]).abs().max())
    rel = float(R[:, c].norm() / F[free][:, c].norm())
    print(f"mode ({i}, {j}): max nodal error {err:.2e}; solve_cg_multi {int(its[c])} iterations, "
          f"residual {float(res[c]):.1e} (recomputed {rel:.1e})")
    # a quadratic element resolves sin(i pi x) sin(j pi y) to O(h^3), h = max(i, j) / n per half wave
    assert err <= 10.0 * (max(i, j) * math.pi / n) ** 3
    assert float(res[c]) <= 1e-10 and rel <= 1e-9
assert A.matrix_free and A._csr is None, "nothing was assembled behind the operator"
print(f"block solve of {len(MODES)} load cases on the matrix-free operator: {t_block:.2f} s")
