"""Developer tool (GPU box): the variable-coefficient P1 operator on k vectors at once
(tfem_p1_apply_rings_coef_multi) against k back-to-back single-vector launches
(tfem_p1_apply_rings_coef), and the fused block CG on that operator.

    python tools/time_coef_multi.py [--n 2236] [--delaunay 1000000] [--samples 40]
                                    [--parent-lib libtfem_hip.so of another build]
                                    [--cg-n 1000] [--cg-iters 200] [--no-apply] [--no-cg]
                                    [--tree checkout of another commit, built] [--log FILE]

Meshes: S(n) (default 2236: 9,999,392 elements, 7-slot records, chunked) and a Delaunay mesh of
--delaunay vertices (15-slot records, renumbered inside the engine; 0 skips it); fp64, order 3;
kappa = 1 + x y, kappa = 1 + 0.5 sin(3x) cos(2y), and the latter with c = exp(-x).  One process;
every variant is timed with events around ONE call (= k launches for the single-vector variants),
the variants take turns round by round, `samples` rounds after a warm-up; min / median / spread
(median - min) per variant.  --parent-lib: tfem_p1_apply_rings_coef of ANOTHER build of the library
(the commit before the block launch), loaded beside this one and called on the same plan and buffers:
the single launch did not change.  TFEM_APPLY_NV caps the columns per pass: "block as 2 x NV2" is
the block launch in two passes of the next narrower width, the comparison that decides which
widths are built.

Block CG: Basis-level solve_cg_multi(loop="fused") with 4 columns on S(cg-n) (default 1000: 1e6
DoFs), kappa = 1 + 0.5 sin(3x) cos(2y), c = exp(-x), a fixed number of iterations (rtol = 0); time per
iteration and column.  --tree: the package (and bench.py) of ANOTHER checkout, where the fused loop
takes the coefficient operator column by column; only the CG part runs then (--no-apply is implied)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch


def kappa_xy(x, y):
    return 1.0 + x * y


def kappa_trig(x, y):
    return 1.0 + 0.5 * torch.sin(3 * x) * torch.cos(2 * y)


def c_exp(x, y):
    return torch.exp(-x)


def form(kappa, c):
    def a(b):
        x, y = torch.split(b.integration_points, 1, dim=-1)
        out = kappa(x, y) * (b.v_grad @ b.v_grad.mT)
        return out if c is None else out + c(x, y) * (b.v @ b.v.mT)

    return a


FORMS = (("kappa = 1 + x y", kappa_xy, None), ("kappa = 1 + 0.5 sin(3x) cos(2y)", kappa_trig, None),
         ("kappa = 1 + 0.5 sin(3x) cos(2y), c = exp(-x)", kappa_trig, c_exp))


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
    p.add_argument("--n", type=int, default=2236)
    p.add_argument("--delaunay", type=int, default=1000000)
    p.add_argument("--samples", type=int, default=40)
    p.add_argument("--parent-lib", default=None)
    p.add_argument("--cg-n", type=int, default=1000)
    p.add_argument("--cg-iters", type=int, default=200)
    p.add_argument("--no-apply", action="store_true")
    p.add_argument("--no-cg", action="store_true")
    p.add_argument("--tree", default=None)
    p.add_argument("--log", default=None)
    args = p.parse_args()
    if args.samples < 30:
        p.error("--samples: at least 30 calls per variant")
    tree = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    import bench
    import pytorch_fem_solver_amd as tf
    from pytorch_fem_solver_amd import _native, meshgen

    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"kernel sources {bench.source_sha()}" + (f"  (tree {args.tree})" if args.tree else ""))
    if not (args.no_apply or args.tree):
        apply_part(args, tf, _native, meshgen, say)
    if not args.no_cg:
        cg_part(args, tf, meshgen, say)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def apply_part(args, tf, _native, meshgen, say):
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        res, argt = _native.SIGNATURES["tfem_p1_apply_rings_coef"]
        parent.tfem_p1_apply_rings_coef.restype, parent.tfem_p1_apply_rings_coef.argtypes = res, argt
        assert not hasattr(parent, "tfem_p1_apply_rings_coef_multi"), "--parent-lib must be a build without the block launch"
    meshes = [(f"S({args.n})", lambda: meshgen.unit_square(args.n, 0.25, 0))]
    if args.delaunay > 0:
        meshes.append((f"Delaunay({args.delaunay})", lambda: meshgen.delaunay_square(args.delaunay, 3)))
    verdicts = []
    for mesh_name, make in meshes:
        mesh_np = make()
        basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
        eng = basis._engine
        n = eng.n_dofs
        plan = eng._coef_rings()
        z = plan["layout"]
        d = eng._inputs()
        say(f"{mesh_name}: {mesh_np['triangles'].shape[0]} elements, {n} rows, {int(z[6])}-slot records, chunked "
            f"{plan['chunked']}, renumbered {eng.renumbered}, {int(z[3])} local vertices per tile at most; "
            f"{args.samples} samples per variant")
        for form_name, kappa, c in FORMS:
            op = basis.integrate_bilinear_form(form(kappa, c), layout="operator")
            assert op.matrix_free and op._programs is not None
            kp, cp = op._programs
            alpha, beta = op.alpha, op.beta

            def parent_apply(u, y):
                st = parent.tfem_p1_apply_rings_coef(
                    _native.ptr(d["coords"]), eng.real_bytes, n, eng.quad_order, alpha, beta, eng._program_ref(kp),
                    eng._program_ref(cp), _native.ptr(plan["blob"]), ctypes.c_void_p(z.ctypes.data), _native.ptr(u),
                    _native.ptr(y), eng._stream())
                assert st == 0

            say(f"  {form_name}")
            for k in (2, 4, 8):
                U = torch.rand(n, k)
                Y = torch.empty(n, k)
                cols = [U[:, j].contiguous() for j in range(k)]
                outs = [torch.empty(n) for _ in range(k)]
                variants = {"block": lambda: eng._apply_rings_coef(alpha, beta, kp, cp, U, out=Y)}
                if k >= 4:
                    variants[f"block as 2 x NV{k // 2}"] = capped(k // 2, variants["block"])
                variants[f"{k} single"] = lambda: [eng._apply_rings_coef(alpha, beta, kp, cp, u, out=o)
                                                   for u, o in zip(cols, outs)]
                if parent is not None:
                    variants[f"{k} single, parent build"] = lambda: [parent_apply(u, o) for u, o in zip(cols, outs)]
                # the block launch computes what the single launches compute, bit for bit
                variants["block"]()
                variants[f"{k} single"]()
                torch.cuda.synchronize()
                same = all(torch.equal(Y[:, j], outs[j]) for j in range(k))
                times = rounds(variants, args.samples)
                say(f"    k = {k}: block equals the single launches bit for bit: {same}")
                stat = {}
                for name, t in times.items():
                    lo, med = min(t), statistics.median(t)
                    stat[name] = (lo, med)
                    say(f"      {name:26s} min {lo:8.1f} us  median {med:8.1f} us  spread {med - lo:6.1f} us   "
                        f"{med / k:7.1f} us per column")
                if k == 4:
                    ref = "4 single, parent build" if parent is not None else "4 single"
                    (b_lo, b_med), (s_lo, s_med) = stat["block"], stat[ref]
                    margin = max(b_med - b_lo, s_med - s_lo)
                    met = s_med - b_med > margin
                    verdicts.append(met)
                    say(f"    k = 4 condition: block median {b_med:.1f} us against {ref} median {s_med:.1f} us, gain "
                        f"{s_med - b_med:.1f} us, larger min-to-median spread {margin:.1f} us: {'MET' if met else 'NOT MET'}")
                del U, Y, cols, outs
        del basis, eng, op
        torch.cuda.empty_cache()
    say(f"k = 4 condition on every mesh and form: {'MET' if all(verdicts) else 'NOT MET'}")


def cg_part(args, tf, meshgen, say):
    import math

    mesh_np = meshgen.unit_square(args.cg_n, 0.25, 0)
    basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
    op = basis.integrate_bilinear_form(form(kappa_trig, c_exp), layout="operator")
    assert op.matrix_free and op._programs is not None
    free = basis._basis_parameters["inner_dofs"]

    def source(i, j):
        return lambda b: (math.pi**2 * (i * i + j * j) * torch.sin(i * math.pi * b.integration_points[..., [0]])
                          * torch.sin(j * math.pi * b.integration_points[..., [1]]) * b.v)

    F = torch.cat([basis.integrate_linear_form(source(i, j)) for i, j in ((1, 1), (2, 1), (1, 3), (2, 2))], dim=1)
    op.solve_cg_multi(F, free=free, rtol=0.0, maxiter=20, loop="fused")  # plan, warm-up
    runs = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, its, _ = op.solve_cg_multi(F, free=free, rtol=0.0, maxiter=args.cg_iters, loop="fused")
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / args.cg_iters * 1e6)
        assert its.tolist() == [args.cg_iters] * 4
    lo, med = min(runs), statistics.median(runs)
    say(f"fused block CG, S({args.cg_n}) {op.shape[0]} DoFs, kappa = 1 + 0.5 sin(3x) cos(2y), c = exp(-x), 4 columns, "
        f"{args.cg_iters} iterations, 5 runs: min {lo:.1f} us per iteration, median {med:.1f} us, "
        f"{med / 4:.1f} us per iteration and column")


if __name__ == "__main__":
    main()
