"""Developer tool (GPU box): the CSR operator on k vectors at once (tfem_csr_spmm) against k
tfem_csr_spmv launches on contiguous columns, the fused block CG on the CSR, and -- for context --
the same block CG through the P2 matrix-free operator (column by column).

    python tools/time_spmm.py [--p1-n 1000] [--p2-n 707] [--samples 40] [--cg-iters 200] [--runs 3]
                              [--no-launch] [--no-cg] [--no-context]
                              [--tree checkout of another commit, built] [--log FILE]

Matrices: the stiffness CSR of S(p1-n) with ElementTri(1, 3) (default 1000: 1,002,001 rows) and of
S(p2-n) with ElementTri(2, 2) (default 707: 2,002,225 rows); fp64; k = 2, 4, 8.

(a) launches.  One process; the prepared launches of CSRMatrix._prepared_spmv on the stored arrays,
    one tfem_csr_spmm call against k tfem_csr_spmv calls on contiguous columns, each variant between
    two device events around ONE call (= k launches for the column variant), the variants take turns
    round by round, `samples` rounds after a warm-up; min and median per variant.  Algorithmic bytes
    from the shapes (x counted once per launch, as if every gathered row were read once):
        SpMM      : nnz (8 + 4) + 8 (n + 1) + 8 n k (x) + 8 n k (y)
        k x SpMV  : k (nnz (8 + 4) + 8 (n + 1) + 8 n + 8 n)
    and bytes / median time for both.
(b) fused block CG on the CSR: CSRMatrix.solve_cg_multi(loop="fused") on the DoFs inside the
    boundary, random right-hand sides, rtol = 0 and `cg-iters` iterations; a host clock around the
    solve that ends in a device synchronise; the median of three solves after a warm-up, per iteration
    and column.
(c) context: the same block through the P2 matrix-free operator (layout="matrix_free"), whose block
    application goes column by column.

--tree: the package (and bench.py) of ANOTHER built checkout, where the block path of the CSR is the
column loop (no tfem_csr_spmm: part (a) and (c) are skipped there).  Then this process measures
nothing itself: it starts `runs` child processes for this tree and `runs` for the other, taking turns,
one at a time, and reports per case the median and the spread (max - min) over the runs of each
tree.  What must hold at k = 4: (a) the SpMM median below the column variant's by more than the
larger spread, (b) this tree's time below the other tree's by more than the larger spread; the
verdict is printed as MET / NOT MET.  A child that fails ends the session: nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 4, 8)


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def rounds(variants, samples, warmup=5):
    """{name: [us per call]}: the variants take turns, one event pair per call."""
    import torch

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


def launch_part(label, K, args, say, out):
    import torch

    S = K._stored()
    n, nnz = S.shape[0], S.nnz
    for k in WIDTHS:
        X, Y = torch.rand(n, k), torch.empty(n, k)
        cols = [X[:, j].contiguous() for j in range(k)]
        outs = [torch.empty(n) for _ in range(k)]
        block = S._prepared_spmv(X, Y)
        singles = [S._prepared_spmv(c, o) for c, o in zip(cols, outs)]
        variants = {"spmm": block, "spmv": lambda: [one() for one in singles]}
        variants["spmm"]()
        variants["spmv"]()
        torch.cuda.synchronize()
        same = all(torch.equal(Y[:, j], outs[j]) for j in range(k))
        times = rounds(variants, args.samples)
        nbytes = {"spmm": nnz * 12 + 8 * (n + 1) + 16 * n * k, "spmv": k * (nnz * 12 + 8 * (n + 1) + 16 * n)}
        say(f"  (a) {label}, k = {k}: SpMM equals the {k} SpMV launches bit for bit: {same}")
        for name, what in (("spmm", "1 tfem_csr_spmm"), ("spmv", f"{k} tfem_csr_spmv")):
            lo, med = min(times[name]), statistics.median(times[name])
            say(f"      {what:16s} min {lo:8.1f} us  median {med:8.1f} us of {len(times[name])} calls   "
                f"{nbytes[name] / 1e6:7.1f} MB algorithmic, {nbytes[name] / med / 1e6:5.2f} TB/s at the median")
            out[f"a|{label}|k={k}|{name}"] = med
        assert same, "the block launch must reproduce the single launches"
        del X, Y, cols, outs, block, singles


def cg_time(op, B, free, iters):
    """us per iteration and column: the median of three solves after a warm-up."""
    import torch

    op.solve_cg_multi(B, free=free, rtol=0.0, maxiter=20, loop="fused")
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, its, _ = op.solve_cg_multi(B, free=free, rtol=0.0, maxiter=iters, loop="fused")
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / iters / B.shape[1] * 1e6)
        assert its.tolist() == [iters] * B.shape[1]
    return statistics.median(runs)


def measure(args, tree, say):
    """One pass over every part this tree can run; {case: figure in us}."""
    sys.path.insert(0, tree)
    import torch

    import bench
    import pytorch_fem_solver_amd as tf
    from pytorch_fem_solver_amd import _native, meshgen

    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    has_spmm = hasattr(_native.load(), "tfem_csr_spmm")
    say(f"kernel sources {bench.source_sha()}, tfem_csr_spmm {'present' if has_spmm else 'absent: the column loop'}")
    out = {}
    for label, n, element in ((f"S({args.p1_n}) P1", args.p1_n, (1, 3)), (f"S({args.p2_n}) P2", args.p2_n, (2, 2))):
        basis = tf.Basis(tf.MeshTri(meshgen.unit_square(n, 0.25, 0)), tf.ElementTri(*element))
        K = basis.integrate_bilinear_form(stiffness, layout="csr")
        free = basis._basis_parameters["inner_dofs"]
        say(f"{label}: {K.shape[0]} rows, {K.nnz} entries, renumbered {K.perm is not None}")
        if has_spmm and not args.no_launch:
            launch_part(label, K, args, say, out)
        gen = torch.Generator(device="cuda").manual_seed(1)
        loads = torch.rand(K.shape[0], max(WIDTHS), generator=gen)
        if not args.no_cg:
            for k in WIDTHS:
                t = cg_time(K, loads[:, :k].contiguous(), free, args.cg_iters)
                say(f"  (b) {label}, k = {k}: fused block CG on the CSR, {args.cg_iters} iterations: "
                    f"{t * k:8.1f} us per iteration, {t:7.1f} us per iteration and column")
                out[f"b|{label}|k={k}"] = t
        if has_spmm and not args.no_context and element[0] == 2:
            op = basis.integrate_bilinear_form(stiffness, layout="matrix_free")
            assert op.matrix_free
            for k in WIDTHS:
                t = cg_time(op, loads[:, :k].contiguous(), free, args.cg_iters)
                say(f"  (c) {label}, k = {k}: the same block CG through the P2 matrix-free operator (column by column): "
                    f"{t * k:8.1f} us per iteration, {t:7.1f} us per iteration and column")
                out[f"c|{label}|k={k}"] = t
            del op
        del basis, K, loads
        torch.cuda.empty_cache()
    return out


def compare(args, say):
    """Child processes for this tree and args.tree, taking turns; medians, spreads and the verdicts."""
    other = os.path.abspath(args.tree)
    passed = [a for a in sys.argv[1:]]
    results = {"this": [], "other": []}
    for run in range(args.runs):
        for which, tree in (("this", HERE), ("other", other)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", tree] + passed
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            say(f"--- run {run + 1} of {args.runs}, {'this tree' if which == 'this' else 'the --tree checkout'}")
            record = None
            for line in done.stdout.splitlines():
                if line.startswith("RESULT "):
                    record = json.loads(line[7:])
                else:
                    say(line)
            if done.returncode != 0 or record is None:
                say(f"the child ended with status {done.returncode}: nothing more is started\n{done.stderr[-3000:]}")
                return False
            results[which].append(record)
    say("--- over the runs: median and spread (max - min) in us")

    def stat(records, key):
        values = [r[key] for r in records]
        return statistics.median(values), max(values) - min(values)

    verdicts = []
    for key in sorted(results["this"][0]):
        part, label, k = key.split("|")[:3]
        if part == "a":
            if not key.endswith("|spmm"):
                continue
            (fast, s_fast), (slow, s_slow) = stat(results["this"], key), stat(results["this"], key[:-4] + "spmv")
            names = ("1 tfem_csr_spmm", f"{k[2:]} tfem_csr_spmv")
        elif part == "b":
            (fast, s_fast), (slow, s_slow) = stat(results["this"], key), stat(results["other"], key)
            names = ("this tree", "the --tree checkout")
        else:
            med, spread = stat(results["this"], key)
            say(f"  (c) {label}, {k}: {med:8.1f} us per iteration and column, spread {spread:.1f} (context only)")
            continue
        margin = max(s_fast, s_slow)
        met = slow - fast > margin
        unit = "per call" if part == "a" else "per iteration and column"
        say(f"  ({part}) {label}, {k}: {names[0]} {fast:8.1f} us (spread {s_fast:.1f}) against {names[1]} {slow:8.1f} us "
            f"(spread {s_slow:.1f}) {unit}: {slow / fast:.2f} x" + (f", k = 4 condition {'MET' if met else 'NOT MET'}" if k == "k=4" else ""))
        if k == "k=4":
            verdicts.append(met)
    say(f"k = 4 conditions, (a) and (b) on both matrices: {'MET' if verdicts and all(verdicts) else 'NOT MET'}")
    return True


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--p1-n", type=int, default=1000)
    p.add_argument("--p2-n", type=int, default=707)
    p.add_argument("--samples", type=int, default=40)
    p.add_argument("--cg-iters", type=int, default=200)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--child-timeout", type=int, default=600, help="seconds a child process may take")
    p.add_argument("--no-launch", action="store_true")
    p.add_argument("--no-cg", action="store_true")
    p.add_argument("--no-context", action="store_true")
    p.add_argument("--tree", default=None)
    p.add_argument("--log", default=None)
    p.add_argument("--child", default=None, help=argparse.SUPPRESS)  # the tree a child process measures
    args = p.parse_args()
    if args.samples < 30:
        p.error("--samples: at least 30 calls per variant")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    ok = True
    if args.child:
        print("RESULT " + json.dumps(measure(args, args.child, say)), flush=True)
    elif args.tree:
        ok = compare(args, say)
    else:
        measure(args, HERE, say)
    if args.log and not args.child:
        with open(args.log, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
