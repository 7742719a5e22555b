"""One mesh, one operator whose coefficient exists only as numbers, several load cases, ONE block
solve:

    -div(kappa grad u) = f_j,   kappa one value per element (a material constant per cell: here a
                                checkerboard of 4 x 4 patches with kappa = 1 and kappa = 4)

for four loads f_j = sin(i pi x) sin(j pi y).  ``basis.coefficient(values)`` marks the (E,) values as
data, layout="matrix_free" gives an operator that stores no matrix, and Basis.solve with an (N, 4)
right-hand side runs one block CG whose every iteration is ONE tfem_p1_apply_rings_field_multi call:
the values of a tile's elements are read and reduced once for the four columns.  Then the same systems
one by one.

    python examples/poisson_coefficient_field_loads.py [n]
"""
import math
import os
import sys
import time

import numpy as np
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

# the material: one number per element, from the cell's centroid
centroid = np.asarray(mesh_np["vertices"])[np.asarray(mesh_np["triangles"])].mean(1)
patch = (np.floor(4.0 * centroid[:, 0]) + np.floor(4.0 * centroid[:, 1])) % 2
kappa = basis.coefficient(torch.tensor(np.where(patch == 0, 1.0, 4.0)))  # (E,)


def load(i, j):
    def linear(b):
        x, y = torch.split(b.integration_points, 1, dim=-1)
        return torch.sin(i * math.pi * x) * torch.sin(j * math.pi * y) * b.v

    return linear


# the strict request: raises instead of assembling where the data launches do not take the basis
A = basis.integrate_bilinear_form(lambda b: kappa * (b.v_grad @ b.v_grad.mT), layout="matrix_free")
assert A.matrix_free
F = torch.cat([basis.integrate_linear_form(load(i, j)) for i, j in MODES], dim=1)  # (N, 4)
print(f"{mesh_np['triangles'].shape[0]} elements, {A.shape[0]} DoFs, {len(MODES)} load cases, {A}")

# the launches of the block solve, counted at the library
lib = basis._engine.lib
calls = {"tfem_p1_apply_rings_field_multi": 0, "tfem_p1_apply_rings_field": 0, "tfem_p1_rings_field": 0,
         "tfem_csr_spmv": 0}


def counting(name, inner):
    def call(*args):
        calls[name] += 1
        return inner(*args)

    return call


inner = {name: getattr(lib, name) for name in calls}
for name in calls:
    setattr(lib, name, counting(name, inner[name]))
torch.cuda.synchronize()
t0 = time.perf_counter()
U = basis.solve(A, torch.zeros_like(F), F)  # (N, 4) in, (N, 4) out: one block CG
torch.cuda.synchronize()
t_block = time.perf_counter() - t0
for name in calls:
    setattr(lib, name, inner[name])
assembled = int(A._csr is not None) + calls["tfem_p1_rings_field"] + calls["tfem_csr_spmv"]
print(f"block solve: {calls['tfem_p1_apply_rings_field_multi']} block applications, "
      f"{calls['tfem_p1_apply_rings_field']} single-vector launch (the diagonal), assembled: {assembled}")
assert assembled == 0 and calls["tfem_p1_apply_rings_field_multi"] > 0 and calls["tfem_p1_apply_rings_field"] <= 1

t0 = time.perf_counter()
singles = [basis.solve(A, basis.solution_tensor(), F[:, [c]]) for c in range(len(MODES))]
torch.cuda.synchronize()
t_single = time.perf_counter() - t0
scale = float(U.abs().max())
for c, (i, j) in enumerate(MODES):
    diff = float((U[:, c] - singles[c].reshape(-1)).abs().max())
    print(f"load ({i}, {j}): max |u| {float(U[:, c].abs().max()):.3e}, block against single solve {diff / scale:.1e} "
          f"of the largest entry")
    assert diff <= 1e-9 * scale
assert A._csr is None
print(f"block solve {t_block:.2f} s, {len(MODES)} single solves {t_single:.2f} s")
