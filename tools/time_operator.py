"""Developer tool (GPU box): the matrix-free P1 operator (tfem_p1_apply_rings) against the CSR
SpMV on the assembled operator of the same mesh, the K-only assembly launch, and CG per iteration.

    python tools/time_operator.py [n] [--cg-n 1000] [--no-cg] [--cg-loop both] [--reps 200]

S(n) (default 2236: 9,999,392 elements), fp64, stiffness.  Every launch timed with events over
`reps` back-to-back launches after a warm-up (steady state); run under
`rocprofv3 --kernel-trace --stats` for the kernel trace and, in a run of its own, under
`rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU` for the apply launch's vector instructions.
Algorithmic bytes: apply = row record + coordinates + u + y per row (each once), SpMV = values +
column ids per entry, row pointer + x + y per row."""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import pytorch_fem_solver_amd as tf  # noqa: E402
from pytorch_fem_solver_amd import meshgen  # noqa: E402

HBM = 8e12  # bytes/s, MI355X peak


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def main():
    p = argparse.ArgumentParser()
    p.add_argument("n", type=int, nargs="?", default=2236)
    p.add_argument("--cg-n", type=int, default=1000)
    p.add_argument("--no-cg", action="store_true")
    p.add_argument("--cg-loop", choices=("torch", "fused", "both"), default="both",
                   help="the CG loop to time: the torch operations, the tfem_cg_* launches, or one after the other")
    p.add_argument("--reps", type=int, default=200)
    args = p.parse_args()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    print(f"kernel sources {bench.source_sha()}")

    mesh_np = meshgen.unit_square(args.n, 0.25, 0)
    basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
    eng = basis._engine
    op = basis.integrate_bilinear_form(stiffness, layout="operator")
    K = op.to_csr()
    assert op.matrix_free
    n, nnz, n_el = K.shape[0], K.nnz, mesh_np["triangles"].shape[0]
    plan = eng.ring_plan()
    slots = int(plan["layout"][6])
    u = torch.rand(n)
    y = torch.empty(n)
    y_csr = K.matvec(u)
    eng.apply(1.0, 0.0, u, out=y)
    torch.cuda.synchronize()
    err = ((y - y_csr).abs().max() / y_csr.abs().max()).item()
    vals = torch.empty(nnz)
    t_apply = timed(lambda: eng.apply(1.0, 0.0, u, out=y), args.reps)
    t_diag = timed(lambda: eng.operator_diagonal(1.0, 0.0), args.reps)
    t_spmv = timed(lambda: K.matvec(u), args.reps)
    t_kasm = timed(lambda: eng.bilinear(1.0, 0.0, out=vals), args.reps)
    rec = 4 * int(plan["layout"][7])
    b_apply = n * (rec + 16 + 8 + 8)
    b_spmv = nnz * 12 + n * 24
    print(f"S({args.n}): {n_el} elements, {n} rows, nnz {nnz}, {slots}-slot records, chunked {plan['chunked']}; "
          f"apply vs SpMV max rel diff {err:.1e}")
    print(f"apply  k_p1_apply_rows   {t_apply:8.1f} us   algorithmic {b_apply / 1e6:7.1f} MB  "
          f"{b_apply / t_apply / 1e3:6.0f} GB/s  {b_apply / t_apply / 1e-6 / HBM * 100:5.1f} % of 8 TB/s")
    print(f"diag   k_p1_apply_rows   {t_diag:8.1f} us   (u = NULL; includes the allocation of y)")
    print(f"SpMV   tfem_csr_spmv     {t_spmv:8.1f} us   algorithmic {b_spmv / 1e6:7.1f} MB  "
          f"{b_spmv / t_spmv / 1e3:6.0f} GB/s  {b_spmv / t_spmv / 1e-6 / HBM * 100:5.1f} % of 8 TB/s")
    print(f"K-only k_p1_rings        {t_kasm:8.1f} us")
    print(f"apply / SpMV = {t_apply / t_spmv:.2f}")
    del K, vals, op, basis, eng, y_csr

    if args.no_cg:
        return
    mesh_np = meshgen.unit_square(args.cg_n, 0.25, 0)
    basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
    op = basis.integrate_bilinear_form(stiffness, layout="operator")
    K = basis.integrate_bilinear_form(stiffness, layout="csr")
    f = basis.integrate_linear_form(
        lambda b: 2.0 * math.pi**2 * torch.sin(math.pi * b.integration_points[..., [0]])
        * torch.sin(math.pi * b.integration_points[..., [1]]) * b.v)
    free = basis._basis_parameters["inner_dofs"]
    loops = ("torch", "fused") if args.cg_loop == "both" else (args.cg_loop,)
    for loop in loops:
        op.solve_cg(f, free=free, maxiter=50, loop=loop)  # plan, warm-up
        K.solve_cg(f, free=free, maxiter=50, loop=loop)
    for name, A in (("operator", op), ("CSR", K)):
        for loop in loops:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, it, res = A.solve_cg(f, free=free, rtol=1e-10, loop=loop)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"CG {name:8s} {loop:5s} loop S({args.cg_n}) {K.shape[0]} DoFs: {it} iterations, residual {res:.1e}, "
                  f"{dt:.3f} s, {dt / it * 1e6:.1f} us per iteration")


if __name__ == "__main__":
    main()
