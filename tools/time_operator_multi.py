"""Developer tool (GPU box): the matrix-free P1 operator on k vectors at once
(tfem_p1_apply_rings_multi) against k back-to-back single-vector launches (tfem_p1_apply_rings)
and k SpMVs on the assembled operator of the same mesh; block CG against CG per column.

    python tools/time_operator_multi.py [n] [--parent-lib libtfem_hip.so of another build]
                                        [--samples 40] [--cg-n 1000] [--no-cg]

S(n) (default 2236: 9,999,392 elements), fp64, stiffness, order 3.  One process; every variant is
timed with events around ONE call (= k launches for the single-vector and SpMV variants), the
variants take turns round by round, `samples` rounds after a warm-up; min / median / spread
(median - min) per variant.  --parent-lib: the single-vector entry point of ANOTHER build of the
library (the commit before the block launch), loaded beside this one and called on the same plan
and buffers.  TFEM_APPLY_NV caps the columns per pass: "4 as 2 x NV2" is the block launch in two
passes of the next narrower width, the comparison that decides which widths are built.
Algorithmic bytes per row: record + coordinates once (32) + u and y per column (16 k)."""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import pytorch_fem_solver_amd as tf  # noqa: E402
from pytorch_fem_solver_amd import _native, meshgen  # noqa: E402

HBM = 8e12  # bytes/s, MI355X peak


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def rounds(variants, samples, warmup=5):
    """{name: [us per call]}: the variants take turns, one event pair per call."""
    times = {name: [] for name in variants}
    for r in range(warmup + samples):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    return times


def capped(cap, fn):
    def call():
        os.environ["TFEM_APPLY_NV"] = str(cap)
        try:
            fn()
        finally:
            del os.environ["TFEM_APPLY_NV"]
    return call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("n", type=int, nargs="?", default=2236)
    p.add_argument("--parent-lib", default=None)
    p.add_argument("--samples", type=int, default=40)
    p.add_argument("--cg-n", type=int, default=1000)
    p.add_argument("--no-cg", action="store_true")
    args = p.parse_args()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    print(f"kernel sources {bench.source_sha()}")

    mesh_np = meshgen.unit_square(args.n, 0.25, 0)
    basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
    eng = basis._engine
    op = basis.integrate_bilinear_form(stiffness, layout="operator")
    K = op.to_csr()
    assert op.matrix_free and not eng.renumbered
    n, nnz = K.shape[0], K.nnz
    plan = eng.ring_plan()
    z = plan["layout"]
    rec = 4 * int(z[7])
    print(f"S({args.n}): {mesh_np['triangles'].shape[0]} elements, {n} rows, nnz {nnz}, {int(z[6])}-slot records, "
          f"chunked {plan['chunked']}, {int(z[3])} local vertices per tile at most; {args.samples} samples per variant")

    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        res, argt = _native.SIGNATURES["tfem_p1_apply_rings"]
        parent.tfem_p1_apply_rings.restype, parent.tfem_p1_apply_rings.argtypes = res, argt
        assert not hasattr(parent, "tfem_p1_apply_rings_multi"), "--parent-lib must be a build without the block launch"
    d = eng._inputs()

    def parent_apply(u, y):
        st = parent.tfem_p1_apply_rings(
            _native.ptr(d["coords"]), eng.real_bytes, n, eng.quad_order, 1.0, 0.0, _native.ptr(plan["blob"]),
            ctypes.c_void_p(z.ctypes.data), _native.ptr(u), _native.ptr(y), eng._stream())
        assert st == 0

    spread = {}
    for k in (1, 2, 4, 8):
        U = torch.rand(n, k)
        Y = torch.empty(n, k)
        cols = [U[:, j].contiguous() for j in range(k)]
        outs = [torch.empty(n) for _ in range(k)]
        block_in = U if k > 1 else cols[0]
        block_out = Y if k > 1 else outs[0]
        variants = {"block": lambda: eng._apply_rings(1.0, 0.0, block_in, out=block_out)}
        if k >= 4:
            variants[f"block as 2 x NV{k // 2}"] = capped(k // 2, variants["block"])
        variants[f"{k} single"] = lambda: [eng._apply_rings(1.0, 0.0, c, out=o) for c, o in zip(cols, outs)]
        if parent is not None:
            variants[f"{k} single, parent build"] = lambda: [parent_apply(c, o) for c, o in zip(cols, outs)]
        variants[f"{k} SpMV"] = lambda: [K.matvec(c) for c in cols]
        # the block launch computes what the single launches compute
        variants["block"]()
        variants[f"{k} single"]()
        torch.cuda.synchronize()
        got = block_out.reshape(n, k)
        err = max(float((got[:, j] - outs[j]).abs().max() / outs[j].abs().max()) for j in range(k))
        times = rounds(variants, args.samples)
        b_block = n * (rec + 16 + 16 * k)
        b_single = n * (rec + 16 + 16) * k
        b_spmv = (nnz * 12 + n * 24) * k
        print(f"k = {k}: block vs single launches max rel diff {err:.1e}; bytes per row: block {rec + 16 + 16 * k}, "
              f"{k} single {(rec + 32) * k}")
        for name, t in times.items():
            lo, med = min(t), statistics.median(t)
            spread[(k, name)] = (lo, med)
            nbytes = b_spmv if "SpMV" in name else (b_single if "single" in name else b_block)
            print(f"  {name:26s} min {lo:8.1f} us  median {med:8.1f} us  spread {med - lo:6.1f} us   "
                  f"{nbytes / 1e6:7.1f} MB  {nbytes / lo / 1e-6 / HBM * 100:5.1f} % of 8 TB/s at the minimum")
    ref = "4 single, parent build" if parent is not None else "4 single"
    (b_lo, b_med), (s_lo, s_med) = spread[(4, "block")], spread[(4, ref)]
    margin = max(b_med - b_lo, s_med - s_lo)
    print(f"k = 4 condition: block median {b_med:.1f} us against {ref} median {s_med:.1f} us, gain {s_med - b_med:.1f} us, "
          f"larger min-to-median spread {margin:.1f} us: {'MET' if s_med - b_med > margin else 'NOT MET'}")
    del K, op, basis, eng

    if args.no_cg:
        return
    mesh_np = meshgen.unit_square(args.cg_n, 0.25, 0)
    basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
    op = basis.integrate_bilinear_form(stiffness, layout="operator")
    free = basis._basis_parameters["inner_dofs"]

    def source(i, j):
        return lambda b: (math.pi**2 * (i * i + j * j) * torch.sin(i * math.pi * b.integration_points[..., [0]])
                          * torch.sin(j * math.pi * b.integration_points[..., [1]]) * b.v)

    F = torch.cat([basis.integrate_linear_form(source(i, j)) for i, j in ((1, 1), (2, 1), (1, 3), (2, 2))], dim=1)
    op.solve_cg(F[:, 0], free=free, maxiter=50)  # plan, warm-up
    op.solve_cg_multi(F, free=free, maxiter=50)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    X, its, res = op.solve_cg_multi(F, free=free, rtol=1e-10)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    total = int(its.max())
    print(f"block CG S({args.cg_n}) {op.shape[0]} DoFs, 4 columns: iterations {its.tolist()}, residuals "
          f"{[f'{float(r):.1e}' for r in res]}, {dt:.3f} s, {dt / total * 1e6:.1f} us per iteration, "
          f"{dt / int(its.sum()) * 1e6:.1f} us per iteration per column")
    t_single, it_single = 0.0, 0
    for j in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, it, r = op.solve_cg(F[:, j], free=free, rtol=1e-10)
        torch.cuda.synchronize()
        t_single += time.perf_counter() - t0
        it_single += it
        diff = float((X[:, j] - x).abs().max() / x.abs().max())
        print(f"  CG column {j}: {it} iterations, residual {r:.1e}, max rel diff to the block solve {diff:.1e}")
    print(f"CG per column (solve_cg, the single-vector launch: unchanged by the block launch): {t_single:.3f} s for "
          f"{it_single} iterations, {t_single / it_single * 1e6:.1f} us per iteration per column")


if __name__ == "__main__":
    main()
