"""The four load cases of poisson_multiple_loads.py with QUADRATIC elements on the ASSEMBLED operator:
layout="csr" stores K once, and ONE Basis.solve call with an (N, 4) right-hand side runs one block CG
on it -- every iteration is one tfem_csr_spmm launch that reads vals, colind and rowptr once and
multiplies every entry with the four values of its column's row -- then the same systems one by one
(tfem_csr_spmv).

    python examples/poisson_p2_multiple_loads.py [n]
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


K = basis.integrate_bilinear_form(stiffness, layout="csr")
F = torch.cat([basis.integrate_linear_form(load(i, j)) for i, j in MODES], dim=1)  # (N, 4)
# the vertex DoFs come first: the nodal error of the quadratic solutions at the mesh's vertices
pts = torch.as_tensor(mesh_np["vertices"])
exact = torch.stack([torch.sin(i * math.pi * pts[:, 0]) * torch.sin(j * math.pi * pts[:, 1]) for i, j in MODES], dim=1)
print(f"{mesh_np['triangles'].shape[0]} elements, {K.shape[0]} DoFs, {len(MODES)} load cases, {K}")

basis.solve(K, torch.zeros_like(F), F, method="cg")  # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
U = basis.solve(K, torch.zeros_like(F), F, method="cg")  # (N, 4) in, (N, 4) out: one block CG
torch.cuda.synchronize()
t_block = time.perf_counter() - t0
t0 = time.perf_counter()
singles = [basis.solve(K, basis.solution_tensor(), F[:, [c]], method="cg") for c in range(len(MODES))]
torch.cuda.synchronize()
t_single = time.perf_counter() - t0
for c, (i, j) in enumerate(MODES):
    err = float((U[: pts.shape[0], c] - exact[:, c]).abs().max())
    diff = float((U[:, c] - singles[c].reshape(-1)).abs().max())
    print(f"mode ({i}, {j}): max nodal error {err:.2e}, block against single solve {diff:.1e}")
    # a quadratic element resolves sin(i pi x) sin(j pi y) to O(h^3), h = max(i, j) / n per half wave
    assert err <= 10.0 * (max(i, j) * math.pi / n) ** 3 and diff <= 1e-8
print(f"block solve {t_block:.2f} s, {len(MODES)} single solves {t_single:.2f} s")
