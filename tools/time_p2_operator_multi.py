"""Developer tool (GPU box): the matrix-free P2 operator on k vectors in one call
(tfem_p2_apply_rows_multi) against k back-to-back single-vector launches (tfem_p2_apply_rows) of this
build and of the parent commit's library, against tfem_csr_spmm on the assembled K, and against the
same block forced into two passes of the next narrower width; then fused block CG per iteration and
column at k = 4 against the parent commit's column loop.

    python tools/time_p2_operator_multi.py [n] [--delaunay 200000] [--parent-lib libtfem_hip.so of the
                                           parent commit's build] [--samples 40] [--cg-iters 200]
                                           [--no-cg] [--no-regs] [--log FILE]

S(n) (default 707: 999,698 elements) with ElementTri(2, 2), fp64, stiffness; then the Morton-numbered
Delaunay mesh D(200000, 2) (vertices with 8 .. 15 neighbours: long rows).  One process; every variant
is timed with events around ONE call (= k launches for the single-vector variants), the variants take
turns round by round, `samples` rounds after a warm-up; min / median / spread (median - min) per
variant.  The single-vector variants call the C entry point directly, of this build and, with
--parent-lib, of ANOTHER build of the library (the commit before the block launch), loaded beside
this one and called on the same plan and buffers; the block goes through Engine._apply_p2_rows.  The
CG part then also runs the parent commit's column loop (a contiguous pair of columns, one launch per
column) on that library.  TFEM_P2_APPLY_NV caps the columns per pass: "block as 2 x NVw" is the block launch
in passes of the next narrower width, the comparison that decides which widths are built.  A
difference counts only when it lies outside both spreads.
Algorithmic bytes of one application (gathered u and coordinates counted once):
    block     : nnz * 4 column ids + the plan's rows, descriptors and vertex lists + 16 n_verts + 16 n k
    k single  : k times the block's bytes at k = 1
    SpMM on K : nnz * 12 + 8 (n + 1) + 16 n k
Registers per instance: csrc/tfem_p2apply_multi.hip compiled to assembly here, tools/kernel_regs.py."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import bench  # noqa: E402
import pytorch_fem_solver_amd as tf  # noqa: E402
from pytorch_fem_solver_amd import _native, meshgen  # noqa: E402

HBM = 8e12  # bytes/s, MI355X peak
WIDTHS = (2, 4, 8)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


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
        os.environ["TFEM_P2_APPLY_NV"] = str(cap)
        try:
            fn()
        finally:
            del os.environ["TFEM_P2_APPLY_NV"]
    return call


def registers():
    """The register table of the block kernels, or the reason there is none."""
    import __graft_entry__ as entry

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return [f"  (no register table: {hipcc} not found)"]
    name = "tfem_p2apply_multi.hip"
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + entry.PER_FILE_FLAGS.get(name, [])
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "p2apply_multi.s")
        subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-I" + os.path.join(HERE, "include"), "-o", asm,
                        os.path.join(entry.CSRC, name)], check=True, capture_output=True)
        out = subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_regs.py"), asm, "k_p2_apply"],
                             check=True, capture_output=True, text=True).stdout
    return ["  " + line for line in out.splitlines()]


def cg_time(op, B, free, iters):
    """us per iteration and column: the median of three fused solves after a warm-up, and the spread."""
    op.solve_cg_multi(B, free=free, rtol=0.0, maxiter=20, loop="fused")
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, its, _ = op.solve_cg_multi(B, free=free, rtol=0.0, maxiter=iters, loop="fused")
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / iters / B.shape[1] * 1e6)
        assert its.tolist() == [iters] * B.shape[1]
    return statistics.median(runs), max(runs) - min(runs)


def measure(label, mesh_np, args, parent):
    basis = tf.Basis(tf.MeshTri(mesh_np), tf.ElementTri(2, 2))
    eng = basis._engine
    op = basis.integrate_bilinear_form(stiffness, layout="matrix_free")
    K = basis.integrate_bilinear_form(stiffness, layout="csr")
    assert op.matrix_free and "P2 rows" in repr(op)
    plan = eng.p2_plan()
    z = plan["layout"]
    n, nnz, n_verts = K.shape[0], K.nnz, int(z[2])
    plan_read = int(z[19])  # the packed plan in front of the element codes of the load-vector launch
    fixed = nnz * 4 + plan_read + 16 * n_verts
    say(f"{label}: {mesh_np['triangles'].shape[0]} elements, {n} DoFs, nnz {nnz}, {int(z[0])} + {int(z[1])} tiles, "
        f"{int(z[18])} long rows, plan {plan_read / 1e6:.1f} MB read, renumbered {eng.renumbered}; "
        f"{args.samples} samples per variant")
    Ks = K._stored()  # engine numbering on every side: what a CG iteration launches
    d = eng._inputs()
    colind = eng.csr_structure()[1]

    def raw_apply(lib, u, y):
        st = lib.tfem_p2_apply_rows(
            _native.ptr(d["coords"]), eng.real_bytes, eng.quad_order, 1.0, 0.0, _native.ptr(plan["blob"]),
            ctypes.c_void_p(z.ctypes.data), _native.ptr(colind), int(colind.shape[0]), _native.ptr(u), _native.ptr(y),
            n, eng._stream())
        assert st == 0

    table = {}
    for k in WIDTHS:
        U, Y = torch.rand(n, k), torch.empty(n, k)
        cols = [U[:, j].contiguous() for j in range(k)]
        outs = [torch.empty(n) for _ in range(k)]
        Ysp = torch.empty(n, k)
        spmm = Ks._prepared_spmv(U, Ysp)
        variants = {"block": lambda: eng._apply_p2_rows(1.0, 0.0, U, out=Y)}
        narrower = k // 2 if k <= 4 else 2  # widths built: 2 and 4
        if k >= 4:
            variants[f"block as {k // narrower} x NV{narrower}"] = capped(narrower, variants["block"])
        variants[f"{k} single"] = lambda: [raw_apply(eng.lib, c, o) for c, o in zip(cols, outs)]
        if parent is not None:
            variants[f"{k} single, parent build"] = lambda: [raw_apply(parent, c, o) for c, o in zip(cols, outs)]
        variants["SpMM on K"] = spmm
        # the block launch computes what the single launches compute, bit for bit
        variants["block"]()
        variants[f"{k} single"]()
        torch.cuda.synchronize()
        same = all(torch.equal(Y[:, j], outs[j]) for j in range(k))
        if k >= 4:
            Y.fill_(0)
            variants[f"block as {k // narrower} x NV{narrower}"]()
            torch.cuda.synchronize()
            same = same and all(torch.equal(Y[:, j], outs[j]) for j in range(k))
        times = rounds(variants, args.samples)
        b_block = fixed + 16 * n * k
        b_single = (fixed + 16 * n) * k
        b_spmm = nnz * 12 + 8 * (n + 1) + 16 * n * k
        say(f"  k = {k}: the block equals the {k} single launches bit for bit: {same}")
        for name, t in times.items():
            lo, med = min(t), statistics.median(t)
            table[(k, name)] = (lo, med)
            nbytes = b_spmm if "SpMM" in name else (b_single if "single" in name else b_block)
            say(f"    {name:26s} min {lo:8.1f} us  median {med:8.1f} us  spread {med - lo:6.1f} us   "
                f"{nbytes / 1e6:7.1f} MB  {nbytes / lo / 1e-6 / HBM * 100:5.1f} % of 8 TB/s at the minimum")
        assert same, "the block launch must reproduce the single launches"
        del U, Y, cols, outs, Ysp, spmm, variants
    ref = "4 single, parent build" if parent is not None else "4 single"
    (b_lo, b_med), (s_lo, s_med) = table[(4, "block")], table[(4, ref)]
    margin = max(b_med - b_lo, s_med - s_lo)
    say(f"  k = 4: block median {b_med:.1f} us against {ref} median {s_med:.1f} us, gain {s_med - b_med:.1f} us, larger "
        f"min-to-median spread {margin:.1f} us: the block launch is "
        f"{'FASTER' if s_med - b_med > margin else 'NOT FASTER'} than 4 single launches ({s_med / b_med:.2f} x)")
    (n_lo, n_med) = table[(4, "block as 2 x NV2")]
    margin = max(b_med - b_lo, n_med - n_lo)
    say(f"  width 4 against two passes of width 2: {b_med:.1f} us against {n_med:.1f} us, larger spread {margin:.1f} us: "
        f"width 4 {'STAYS' if n_med - b_med > margin else 'IS NOT FASTER than two passes of 2'}")

    if not args.no_cg:
        free = basis._basis_parameters["inner_dofs"]
        loads = torch.rand(n, 4, generator=torch.Generator(device="cuda").manual_seed(1))
        op.diagonal()
        t_block, s_block = cg_time(op, loads, free, args.cg_iters)
        say(f"  fused block CG, k = 4, {args.cg_iters} iterations, one tfem_p2_apply_rows_multi call per iteration: "
            f"{t_block:7.1f} us per iteration and column (spread {s_block:.1f})")
        # the parent commit's Engine._prepared_apply for a P2 block: a contiguous pair of columns, one launch per column
        original = eng._prepared_apply

        def column_loop(alpha, beta, u, y, programs=None, fields=None):
            if u.dim() != 2 or u.shape[1] < 2:
                return original(alpha, beta, u, y, programs, fields)
            u_col, y_col = torch.empty(n), torch.empty(n)
            one = (lambda: raw_apply(parent, u_col, y_col)) if parent is not None else original(alpha, beta, u_col, y_col)
            assert alpha == 1.0 and beta == 0.0

            def columns():
                for j in range(u.shape[1]):
                    u_col.copy_(u[:, j])
                    one()
                    y[:, j].copy_(y_col)

            return columns

        eng._prepared_apply = column_loop
        try:
            t_loop, s_loop = cg_time(op, loads, free, args.cg_iters)
        finally:
            del eng._prepared_apply
        whose = "the parent build's" if parent is not None else "this build's"
        say(f"  fused block CG, k = 4, the parent commit's column loop on {whose} tfem_p2_apply_rows:      "
            f"{t_loop:7.1f} us per iteration and column (spread {s_loop:.1f})")
        t_csr, s_csr = cg_time(K, loads, free, args.cg_iters)
        say(f"  fused block CG, k = 4, the assembled CSR (tfem_csr_spmm):                                   "
            f"{t_csr:7.1f} us per iteration and column (spread {s_csr:.1f})")
        margin = max(s_block, s_loop)
        say(f"  block CG: {t_loop / t_block:.2f} x over the column loop, "
            f"{'outside' if t_loop - t_block > margin else 'INSIDE'} the larger spread {margin:.1f} us")
    del op, K, Ks, basis, eng
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("n", type=int, nargs="?", default=707)
    p.add_argument("--delaunay", type=int, default=200000)
    p.add_argument("--parent-lib", default=None)
    p.add_argument("--samples", type=int, default=40)
    p.add_argument("--cg-iters", type=int, default=200)
    p.add_argument("--no-cg", action="store_true")
    p.add_argument("--no-regs", action="store_true")
    p.add_argument("--log", default=None)
    args = p.parse_args()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    say(f"kernel sources {bench.source_sha()}, {torch.cuda.get_device_name(0)}")
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        res, argt = _native.SIGNATURES["tfem_p2_apply_rows"]
        parent.tfem_p2_apply_rows.restype, parent.tfem_p2_apply_rows.argtypes = res, argt
        assert not hasattr(parent, "tfem_p2_apply_rows_multi"), "--parent-lib must be a build without the block launch"
        say("parent build: loaded beside this one, without tfem_p2_apply_rows_multi")
    if args.n > 0:
        measure(f"S({args.n}) P2", meshgen.unit_square(args.n, 0.25, 0), args, parent)
    if args.delaunay > 0:
        native = meshgen.delaunay_square(args.delaunay, 2)
        morton = meshgen.permute_mesh(native, vertex_order=meshgen.morton_order(native["vertices"]))
        measure(f"D({args.delaunay}, 2) Morton, P2", morton, args, parent)
    if not args.no_regs:
        say("registers per instance (tools/kernel_regs.py on csrc/tfem_p2apply_multi.hip, gfx950):")
        for line in registers():
            say(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
