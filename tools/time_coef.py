"""Developer tool (GPU box): the variable-coefficient launches (tfem_p1_rings_coef,
tfem_p1_apply_rings_coef) against the constant-coefficient launches of the same mesh and against
the torch path of the same callable.

    python tools/time_coef.py [--n 2236] [--delaunay 1000000] [--reps 30] [--torch-path] [--log FILE]

Meshes: S(n) (default 2236: 9,999,392 elements) and a Delaunay mesh of --delaunay vertices (~2e6
elements; 0 skips it); fp64, order 3, kappa = 1 + x y (two stack entries, no library call) and
kappa = 1 + 0.5 sin(3x) cos(2y).  Every launch is timed on its own with a pair of events after a
warm-up; min / median of `reps` launches (calls, for the whole-call rows) are reported.  --torch-path times ONLY the torch path
(TFEM_KERNEL=gather is set before the engine is built; on a tree without the coefficient launches
this is what the callable costs).  Counters: run the tool under `rocprofv3 --pmc SQ_INSTS_VALU --`
in a run of its own (no tracing flags beside it)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)  # us
    return min(out), statistics.median(out)


def kappa_xy(x, y):
    return 1.0 + x * y


def kappa_trig(x, y):
    return 1.0 + 0.5 * torch.sin(3 * x) * torch.cos(2 * y)


def form(kappa):
    def a(b):
        x, y = torch.split(b.integration_points, 1, dim=-1)
        return kappa(x, y) * (b.v_grad @ b.v_grad.mT)

    return a


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=2236)
    p.add_argument("--delaunay", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--torch-path", action="store_true")
    p.add_argument("--log", default=None)
    args = p.parse_args()
    if args.torch_path:
        os.environ["TFEM_KERNEL"] = "gather"
    import bench
    import pytorch_fem_solver_amd as tf
    from pytorch_fem_solver_amd import meshgen

    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    lines = [f"kernel sources {bench.source_sha()}  TFEM_KERNEL={os.environ.get('TFEM_KERNEL', 'auto')}"]

    def say(text):
        print(text, flush=True)
        lines.append(text)

    meshes = [(f"S({args.n})", lambda: meshgen.unit_square(args.n, 0.25, 0))]
    if args.delaunay > 0:
        meshes.append((f"Delaunay({args.delaunay})", lambda: meshgen.delaunay_square(args.delaunay, 3)))
    for mesh_name, make in meshes:
        mesh_np = make()
        basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(1, 3))
        eng = basis._engine
        n, n_el = eng.n_dofs, mesh_np["triangles"].shape[0]
        u = torch.rand(n)
        say(f"{mesh_name}: {n_el} elements, {n} rows, renumbered {eng.renumbered}")
        if not args.torch_path:
            y = torch.empty(n)
            vals = torch.empty(int(eng.csr_structure()[1].shape[0]))
            eng_u = eng._dofs_in(u)
            t = timed(lambda: eng.bilinear(1.0, 0.0, out=vals), args.reps)
            say(f"  constant   assembly  k_p1_rings        min {t[0]:9.1f} us  median {t[1]:9.1f} us")
            t = timed(lambda: eng._apply_rings(1.0, 0.0, eng_u, out=y), args.reps)
            say(f"  constant   apply     k_p1_apply_rows   min {t[0]:9.1f} us  median {t[1]:9.1f} us")
        for kname, kappa in (("1 + x y", kappa_xy), ("1 + 0.5 sin(3x) cos(2y)", kappa_trig)):
            a = form(kappa)
            if args.torch_path:
                # the whole call: torch builds the (E, Q, 3, 3) integrand, the generic kernels reduce and scatter
                t = timed(lambda: basis.integrate_bilinear_form(a, layout="csr"), args.reps, warm=2)
                say(f"  kappa = {kname}: torch path integrate_bilinear_form  min {t[0]:9.1f} us  median {t[1]:9.1f} us")
                continue
            op = basis.integrate_bilinear_form(a, layout="operator")
            assert op.matrix_free
            kp, cp = op._programs
            t = timed(lambda: eng.bilinear_coef(1.0, 0.0, kp, cp, out=vals), args.reps)
            say(f"  kappa = {kname}: assembly  k_p1_coef_rows  min {t[0]:9.1f} us  median {t[1]:9.1f} us")
            t = timed(lambda: eng._apply_rings_coef(1.0, 0.0, kp, cp, eng_u, out=y), args.reps)
            say(f"  kappa = {kname}: apply     k_p1_coef_rows  min {t[0]:9.1f} us  median {t[1]:9.1f} us")
            t = timed(lambda: basis.integrate_bilinear_form(a, layout="csr"), args.reps, warm=2)
            say(f"  kappa = {kname}: integrate_bilinear_form (trace + launch + wrap)  min {t[0]:9.1f} us  median {t[1]:9.1f} us")
        del basis, eng
        torch.cuda.empty_cache()
    if args.log:
        with open(args.log, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
