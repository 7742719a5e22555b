"""Developer tool (GPU box): the matrix-free P2 operator (tfem_p2_apply_rows, layout="matrix_free")
against tfem_csr_spmv on the assembled K of the same basis, and CG with each.

    python tools/time_p2_operator.py [n] [--delaunay 200000] [--blocks 10] [--per-block 20] [--cg-iters 200] [--cg-loop both]

S(n) (default 707: 999,698 elements, BASELINE config 3) with ElementTri(2, 2), fp64, stiffness; then
the Morton-permuted Delaunay mesh D(200000, 2) (vertices with 8 .. 15 neighbours: long rows).  One
process.  Both applications are warmed up, then they alternate in blocks of `per-block` calls, each
block between two device events: blocks * per-block >= 200 applications of each; minimum and median
of the per-application time over the blocks.  Algorithmic bytes (computed here from nnz, n_dofs and
the plan's byte size):
    SpMV on K    : nnz * (8 + 4) values and column ids + 8 (n + 1) rowptr + 8 n u + 8 n y
    matrix-free  : nnz * 4 column ids + the plan's rows, descriptors and vertex lists (its element
                   codes are not read) + 16 n_verts coordinates + 8 n u + 8 n y
(gathered u, and coordinates gathered by several tiles, are counted once).  CG: `cg-iters`
iterations of conjugate_gradients with each operator (rtol 0, so none stops early), a host clock
around the loop that ends in a device synchronise."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import pytorch_fem_solver_amd as tf  # noqa: E402
from pytorch_fem_solver_amd import meshgen  # noqa: E402
from pytorch_fem_solver_amd.sparse import _into, conjugate_gradients, fused_conjugate_gradients  # noqa: E402

HBM = 8e12  # bytes/s, MI355X peak


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def load(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return torch.sin(3.0 * x) * torch.cos(2.0 * y) * b.v


def blocks_of(variants, n_blocks, per_block, warmup=2):
    """{name: [us per call]}: the variants take turns block by block, one event pair per block."""
    times = {name: [] for name in variants}
    for r in range(warmup + n_blocks):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_block):
                fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b) * 1e3 / per_block)
    return times


def measure(label, mesh_np, args):
    basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(2, 2))
    eng = basis._engine
    op = basis.integrate_bilinear_form(stiffness, layout="matrix_free")
    K = basis.integrate_bilinear_form(stiffness, layout="csr")
    assert op.matrix_free and "P2 rows" in repr(op)
    z = eng.p2_plan()["layout"]
    n, nnz, n_verts = K.shape[0], K.nnz, int(z[2])
    plan_read = int(z[19])  # the packed plan in front of the element codes of the load-vector launch
    b_spmv = nnz * 12 + 8 * (n + 1) + 16 * n
    b_free = nnz * 4 + plan_read + 16 * n_verts + 16 * n
    print(f"{label}: {mesh_np['triangles'].shape[0]} elements, {n} DoFs, nnz {nnz}, {int(z[0])} + {int(z[1])} tiles, "
          f"{int(z[18])} long rows, plan {plan_read / 1e6:.1f} MB read of {int(z[16]) / 1e6:.1f} MB, "
          f"renumbered {eng.renumbered}")
    # engine numbering on both sides: what a CG iteration launches
    Ks = K._stored()
    u = torch.rand(n)
    y = torch.empty(n)
    variants = {"matrix-free apply": lambda: eng._apply_p2_rows(1.0, 0.0, u, out=y), "SpMV on K": lambda: Ks.matvec(u)}
    got, want = variants["matrix-free apply"]().clone(), variants["SpMV on K"]()
    absK = tf.CSRMatrix(Ks.crow_indices, Ks.col_indices, Ks.values.abs(), Ks.shape)
    print(f"  max row-wise difference of the two applications {float(((got - want).abs() / absK.matvec(u)).max()):.1e}")
    times = blocks_of(variants, args.blocks, args.per_block)
    for name, t in times.items():
        lo, med = min(t), statistics.median(t)
        nbytes = b_spmv if "SpMV" in name else b_free
        print(f"  {name:18s} min {lo:7.1f} us  median {med:7.1f} us per application ({len(t)} blocks of {args.per_block});  "
              f"{nbytes / 1e6:6.1f} MB algorithmic, {nbytes / lo / 1e6:5.2f} TB/s = {nbytes / lo / 1e-6 / HBM * 100:4.1f} % of 8 TB/s "
              f"at the minimum")
    # CG: the same loop, the two operators
    f = eng._dofs_in(basis.integrate_linear_form(load).reshape(-1))
    free = basis._basis_parameters["inner_dofs"]
    if eng.renumbered:
        free = eng._inv.to(free.device)[free]
    diag = eng._apply_p2_rows(1.0, 0.0, None)
    loops = ("torch", "fused") if args.cg_loop == "both" else (args.cg_loop,)
    for name, fn, prepare, dg in (
            ("matrix-free apply", lambda v: eng._apply_p2_rows(1.0, 0.0, v),
             lambda v, out: eng._prepared_apply(1.0, 0.0, v, out), diag),
            ("SpMV on K", Ks.matvec, Ks._prepared_spmv, Ks.diagonal())):
        for loop in loops:
            solve, matvec = (conjugate_gradients, fn) if loop == "torch" else (fused_conjugate_gradients, _into(prepare))
            solve(matvec, dg, f, free, None, 0.0, 25)  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, it, res = solve(matvec, dg, f, free, None, 0.0, args.cg_iters)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"  CG with {name:18s} {loop:5s} loop {it} iterations in {dt * 1e3:7.1f} ms: "
                  f"{dt / it * 1e6:6.1f} us per iteration, residual {res:.2e}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("n", type=int, nargs="?", default=707)
    p.add_argument("--delaunay", type=int, default=200000)
    p.add_argument("--blocks", type=int, default=10)
    p.add_argument("--per-block", type=int, default=20)
    p.add_argument("--cg-iters", type=int, default=200)
    p.add_argument("--cg-loop", choices=("torch", "fused", "both"), default="both",
                   help="the CG loop to time: the torch operations, the tfem_cg_* launches, or one after the other")
    args = p.parse_args()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    print(f"kernel sources {bench.source_sha()}")
    measure(f"S({args.n}) P2", meshgen.unit_square(args.n, 0.25, 0), args)
    if args.delaunay > 0:
        native = meshgen.delaunay_square(args.delaunay, 2)
        morton = meshgen.permute_mesh(native, vertex_order=meshgen.morton_order(native["vertices"]))
        measure(f"D({args.delaunay}, 2) Morton, P2", morton, args)


if __name__ == "__main__":
    main()
