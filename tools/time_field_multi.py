"""Developer tool (GPU box): the P1 operator with coefficient DATA on k vectors at once
(tfem_p1_apply_rings_field_multi) against k back-to-back single-vector launches
(tfem_p1_apply_rings_field), and the fused block CG on that operator.

    python tools/time_field_multi.py [--n 2236] [--delaunay 1000000] [--samples 40]
                                     [--parent-lib libtfem_hip.so of another build]
                                     [--cg-n 1000] [--cg-iters 200] [--no-apply] [--no-cg]
                                     [--tree checkout of another commit, built] [--log FILE]

Meshes: S(n) (default 2236: 9,999,392 elements, 7-slot records, chunked) and a Delaunay mesh of
--delaunay vertices (15-slot records, renumbered inside the engine; 0 skips it); fp64, order 3;
kappa as (E, Q) values, kappa as (E, 1) values, and kappa (E, Q) with c (E, Q).  One process; every
variant is timed with events around ONE call (= k launches for the single-vector variants), the
variants take turns round by round, `samples` rounds after a warm-up; min / median / spread
(median - min) per variant.  --parent-lib: tfem_p1_apply_rings_field of ANOTHER build of the library
(the commit before the block launch), loaded beside this one and called on the same plan and buffers.
TFEM_APPLY_NV caps the columns per pass: "block as 2 x NV2" is the block launch in two passes of the
next narrower width, the comparison that decides which widths are built.  Per mesh and form the LDS
of a pass of every width and the workgroups per CU it leaves room for (160 KB per CU) are printed.

Block CG: Basis-level solve_cg_multi(loop="fused") with 4 columns on S(cg-n) (default 1000: 1e6
DoFs), kappa (E, Q) and c (E, 1) values, a fixed number of iterations (rtol = 0); time per iteration
and column.  --tree: the package (and bench.py) of ANOTHER checkout, where the fused loop takes the
data operator column by column; only the CG part runs then (--no-apply is implied)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

FORMS = (("kappa (E, Q)", "points", None), ("kappa (E, 1)", "element", None),
         ("kappa (E, Q), c (E, Q)", "points", "points"))


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


def values(n_elems, n_quad, kind, seed):
    """Seeded values in [0.5, 1.5]: (E, Q), (E, 1) or None."""
    if kind is None:
        return None
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return 0.5 + torch.rand(n_elems, n_quad if kind == "points" else 1, generator=gen, device="cuda")


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
        res, argt = _native.SIGNATURES["tfem_p1_apply_rings_field"]
        parent.tfem_p1_apply_rings_field.restype, parent.tfem_p1_apply_rings_field.argtypes = res, argt
        assert not hasattr(parent, "tfem_p1_apply_rings_field_multi"), "--parent-lib must be a build without the block launch"
    meshes = [(f"S({args.n})", lambda: meshgen.unit_square(args.n, 0.25, 0))]
    if args.delaunay > 0:
        meshes.append((f"Delaunay({args.delaunay})", lambda: meshgen.delaunay_square(args.delaunay, 3)))
    verdicts = []
    for mesh_name, make in meshes:
        mesh_np = make()
        basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
        eng = basis._engine
        n = eng.n_dofs
        plan = eng.ring_plan()
        z = plan["layout"]
        d = eng._inputs()
        lds_vert, lds_elem = (int(z[3]) + 1) & ~1, max(int(z[17]), 1)
        say(f"{mesh_name}: {mesh_np['triangles'].shape[0]} elements, {n} rows, {int(z[6])}-slot records, chunked "
            f"{plan['chunked']}, renumbered {eng.renumbered}, at most {int(z[3])} local vertices and {int(z[17])} elements "
            f"per tile; {args.samples} samples per variant")
        for form_name, k_kind, c_kind in FORMS:
            fields = (values(eng.n_elems, eng.n_quad, k_kind, 1), values(eng.n_elems, eng.n_quad, c_kind, 2))
            alpha, beta = 1.0, (0.0 if c_kind is None else 1.0)
            es = 7 if beta != 0.0 else 1
            lds = {w: 8 * ((2 + w) * lds_vert + es * lds_elem) for w in (1, 2, 4, 8)}
            say(f"  {form_name}: LDS per pass " + ", ".join(
                f"{'single' if w == 1 else f'NV{w}'} {b} B ({min(8, (160 * 1024) // b)} per CU by LDS)"
                + ("" if b <= 64 * 1024 else " [does not fit]") for w, b in lds.items()))

            def parent_apply(u, y):
                st = parent.tfem_p1_apply_rings_field(
                    _native.ptr(d["coords"]), eng.real_bytes, n, eng.quad_order, alpha, beta, *eng._field_args(fields),
                    _native.ptr(plan["blob"]), ctypes.c_void_p(z.ctypes.data), _native.ptr(u), _native.ptr(y),
                    eng._stream())
                assert st == 0

            for k in (2, 4, 8):
                if eng.field_refusal(beta, "apply", k) is not None:
                    say(f"    k = {k}: {eng.field_refusal(beta, 'apply', k)}")
                    continue
                U = torch.rand(n, k)
                Y = torch.empty(n, k)
                cols = [U[:, j].contiguous() for j in range(k)]
                outs = [torch.empty(n) for _ in range(k)]
                variants = {"block": lambda: eng._apply_rings_field(alpha, beta, fields, U, out=Y)}
                if k >= 4:
                    variants[f"block as 2 x NV{k // 2}"] = capped(k // 2, variants["block"])
                variants[f"{k} single"] = lambda: [eng._apply_rings_field(alpha, beta, fields, u, out=o)
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
                    verdicts.append(met and same)
                    say(f"    k = 4 condition: block median {b_med:.1f} us against {ref} median {s_med:.1f} us, gain "
                        f"{s_med - b_med:.1f} us, larger min-to-median spread {margin:.1f} us: {'MET' if met else 'NOT MET'}")
                del U, Y, cols, outs
            del fields
        del basis, eng
        torch.cuda.empty_cache()
    say(f"k = 4 condition on every mesh and form: {'MET' if verdicts and all(verdicts) else 'NOT MET'}")


def cg_part(args, tf, meshgen, say):
    import math

    mesh_np = meshgen.unit_square(args.cg_n, 0.25, 0)
    basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
    eng = basis._engine
    kq = basis.coefficient(values(eng.n_elems, eng.n_quad, "points", 1))
    cq = basis.coefficient(values(eng.n_elems, eng.n_quad, "element", 2).reshape(-1))
    op = basis.integrate_bilinear_form(lambda b: kq * (b.v_grad @ b.v_grad.mT) + cq * (b.v @ b.v.mT),
                                       layout="matrix_free")
    assert op.matrix_free and op._fields is not None
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
    say(f"fused block CG, S({args.cg_n}) {op.shape[0]} DoFs, kappa (E, Q) and c (E, 1) values, 4 columns, "
        f"{args.cg_iters} iterations, 5 runs: min {lo:.1f} us per iteration, median {med:.1f} us, "
        f"{med / 4:.1f} us per iteration and column")


if __name__ == "__main__":
    main()
