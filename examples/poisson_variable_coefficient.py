"""-div(kappa grad u) = f on the unit square with a variable diffusion coefficient
kappa(x, y) = 1 + x y and the manufactured solution u = sin(pi x) sin(pi y):

    f = 2 pi^2 (1 + x y) sin(pi x) sin(pi y) - pi (y cos(pi x) sin(pi y) + x sin(pi x) cos(pi y))

The coefficient is written as an expression of the integration points' columns in front of the
stiffness integrand; the package evaluates it per triangle INSIDE the launches (no (E, Q, 3, 3)
integrand exists).  Solved with the matrix-free operator (layout="operator") and with the assembled
CSR operator, on two mesh sizes: the L2 error of a P1 solution falls by ~4 when h halves.

    python examples/poisson_variable_coefficient.py [n]
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_fem import Basis, ElementTri, MeshTri  # noqa: E402  (the MI355X-native package)
from pytorch_fem_solver_amd import meshgen  # noqa: E402

torch.set_default_device("cuda")
torch.set_default_dtype(torch.float64)


def a(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return (1.0 + x * y) * (b.v_grad @ b.v_grad.mT)


def l(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    sx, sy, cx, cy = torch.sin(math.pi * x), torch.sin(math.pi * y), torch.cos(math.pi * x), torch.cos(math.pi * y)
    f = 2.0 * math.pi**2 * (1.0 + x * y) * sx * sy - math.pi * (y * cx * sy + x * sx * cy)
    return f * b.v


def solve(n):
    mesh_np = meshgen.unit_square(n, 0.0, 0)
    basis = Basis(MeshTri(triangulation=mesh_np), ElementTri(polynomial_order=1, integration_order=3))
    A = basis.integrate_bilinear_form(a, layout="operator")  # launches nothing
    # decided on first use (the ring plan is built then); checked BEFORE solving: a CSR fallback
    # would solve the same system, silently
    assert A.matrix_free, "the coefficient launches apply to a P1 basis with a ring plan"
    K, f = basis.assemble_system(a, l, layout="csr")
    M = basis.integrate_bilinear_form(lambda b: b.v @ b.v.mT, layout="csr")
    pts = torch.as_tensor(mesh_np["vertices"])
    exact = (torch.sin(math.pi * pts[:, 0]) * torch.sin(math.pi * pts[:, 1])).reshape(-1, 1)
    errors = {}
    for name, op in (("matrix-free, variable coefficients", A), ("CSR", K)):
        u = basis.solve(op, basis.solution_tensor(), f, method="cg")
        e = (u - exact).reshape(-1)
        errors[name] = math.sqrt(float(torch.dot(e, M.matvec(e))))
    print(A)
    return mesh_np["triangles"].shape[0], errors


n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
coarse, fine = solve(n), solve(2 * n)
for elements, errors in (coarse, fine):
    for name, err in errors.items():
        print(f"{elements:9d} elements  L2 error {err:.3e}  {name}")
for (name, e0), e1 in zip(coarse[1].items(), fine[1].values()):
    ratio = e0 / e1
    print(f"error ratio h -> h/2: {ratio:.2f}  {name}")
    assert 3.5 < ratio < 4.5, "a P1 solution converges with h^2 in L2"
mf, csr = list(fine[1].values())
assert abs(mf - csr) <= 1e-6 * csr, "both operators solve the same system"
