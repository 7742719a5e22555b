"""One mesh, one variable-coefficient operator, several load cases, ONE block solve:

    -div(kappa grad u) + c u = f_j,   kappa(x, y) = 1 + x y,   c(x, y) = exp(-x)

for four sources f_j whose solutions are known (u_j = sin(i pi x) sin(j pi y)):

    f = (kappa pi^2 (i^2 + j^2) + c) s_x s_y - pi (i y c_x s_y + j x s_x c_y)

The operator is matrix-free (layout="operator") and carries the programs of kappa and c; Basis.solve
with an (N, 4) right-hand side runs one block CG whose every iteration is ONE
tfem_p1_apply_rings_coef_multi call: the coefficients are evaluated once per row and triangle for
the four columns.  Then the same systems one by one.

    python examples/poisson_variable_coefficient_loads.py [n]
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 600
mesh_np = meshgen.unit_square(n, 0.25, 0)
basis = Basis(MeshTri(triangulation=mesh_np), ElementTri(polynomial_order=1, integration_order=3))
MODES = ((1, 1), (2, 1), (1, 3), (2, 2))


def a(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return (1.0 + x * y) * (b.v_grad @ b.v_grad.mT) + torch.exp(-x) * (b.v @ b.v.mT)


def load(i, j):
    def linear(b):
        x, y = torch.split(b.integration_points, 1, dim=-1)
        sx, sy = torch.sin(i * math.pi * x), torch.sin(j * math.pi * y)
        cx, cy = torch.cos(i * math.pi * x), torch.cos(j * math.pi * y)
        f = ((1.0 + x * y) * math.pi**2 * (i * i + j * j) + torch.exp(-x)) * sx * sy \
            - math.pi * (i * y * cx * sy + j * x * sx * cy)
        return f * b.v

    return linear


A = basis.integrate_bilinear_form(a, layout="operator")  # launches nothing
# decided on first use (the ring plan is built then); checked BEFORE solving: a CSR fallback would
# solve the same systems, silently
assert A.matrix_free, "the coefficient launches apply to a P1 basis with a ring plan"
F = torch.cat([basis.integrate_linear_form(load(i, j)) for i, j in MODES], dim=1)  # (N, 4)
pts = torch.as_tensor(mesh_np["vertices"])
exact = torch.stack([torch.sin(i * math.pi * pts[:, 0]) * torch.sin(j * math.pi * pts[:, 1]) for i, j in MODES], dim=1)
print(f"{mesh_np['triangles'].shape[0]} elements, {A.shape[0]} DoFs, {len(MODES)} load cases, {A}")

# warm-up, and the iteration counts of the block CG that Basis.solve runs
_, its, res = A.solve_cg_multi(F, free=basis._basis_parameters["inner_dofs"])
print(f"block CG: iterations {its.tolist()}, relative residuals {[f'{float(r):.1e}' for r in res]}")
torch.cuda.synchronize()
t0 = time.perf_counter()
U = basis.solve(A, torch.zeros_like(F), F)  # (N, 4) in, (N, 4) out: one block CG
torch.cuda.synchronize()
t_block = time.perf_counter() - t0
t0 = time.perf_counter()
singles = [basis.solve(A, basis.solution_tensor(), F[:, [c]]) for c in range(len(MODES))]
torch.cuda.synchronize()
t_single = time.perf_counter() - t0
# what the mesh resolves: the (2, 2) and (1, 3) modes carry the largest error, O(h^2)
bound = 4.0 * (math.pi / n) ** 2 * 10
for c, (i, j) in enumerate(MODES):
    err = float((U[:, c] - exact[:, c]).abs().max())
    diff = float((U[:, c] - singles[c].reshape(-1)).abs().max())
    print(f"mode ({i}, {j}): max nodal error {err:.2e} (bound {bound:.2e}), block against single solve {diff:.1e}")
    assert err <= bound and diff <= 1e-8
print(f"block solve {t_block:.2f} s, {len(MODES)} single solves {t_single:.2f} s")
