"""A few launches of every variant of the P1 launch, for `rocprofv3 --pmc SQ_INSTS_VALU ...`:
which variant issues how many vector instructions (tools/count_valu.sh summarises; the
coefficient launches of two programs share a kernel name: the summary gives mean, min and max)."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pytorch_fem_solver_amd as tf  # noqa: E402
from pytorch_fem_solver_amd import meshgen  # noqa: E402
from pytorch_fem_solver_amd.basis import forms  # noqa: E402

torch.set_default_dtype(torch.float64)
torch.set_default_device("cuda")
basis = tf.Basis(tf.MeshTri(meshgen.unit_square(2236, 0.25, 0)), tf.ElementTri(1, 3))
eng = basis._engine


def load(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return 2.0 * math.pi**2 * torch.sin(math.pi * x) * torch.sin(math.pi * y) * b.v


program = forms.trace(load, basis, (), {}).coefficient.program()
one = forms.compile_program(("c", 1.0))
poly = forms.compile_program(("add", ("mul", ("x",), ("y",)), ("c", 1.0)))
pts = eng.geometry()[2]
fq = (torch.sin(pts[..., 0]) * pts[..., 1]).contiguous()
for _ in range(5):
    eng.bilinear(1.0, 0.0)
for _ in range(6):
    eng.assemble_system(1.0, 0.0, fq)
for _ in range(7):
    eng.assemble_system(1.0, 0.0, source=one)
for _ in range(8):
    eng.assemble_system(1.0, 0.0, source=poly)
for _ in range(9):
    eng.assemble_system(1.0, 0.0, source=program)
# the variable-coefficient launches (k_p1_coef_rows: store and apply mode), one program after the other:
# kappa = 1 + x y (10 and 11 launches), kappa = 1 + 0.5 sin(3x) cos(2y) (12 and 13)
trig = forms.compile_program(("add", ("c", 1.0), ("mul", ("mul", ("c", 0.5), ("sin", ("mul", ("c", 3.0), ("x",)))),
                                                  ("cos", ("mul", ("c", 2.0), ("y",))))))
u = torch.rand(eng.n_dofs)
for count, kappa in ((10, poly), (12, trig)):
    for _ in range(count):
        eng.bilinear_coef(1.0, 0.0, kappa, None)
    for _ in range(count + 1):
        eng._apply_rings_coef(1.0, 0.0, kappa, None, u)
torch.cuda.synchronize()
