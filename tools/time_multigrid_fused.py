"""Times the outer loop of the multigrid-preconditioned CG, one GPU, one process: ``solve`` and
``solve_multi`` of GeometricMultigrid (--kind p1: unit_square(n, 0.25, 0) refined `levels` times; the
defaults, 31 and 5, give 986,049 vertices) or of P2Multigrid (--kind p2: refined 4 times with the P2
level on top, 986,049 P2 DoFs) with the loop of torch operations (``loop="torch"``) and the fused
loop (``loop="fused"``, csrc/tfem_pcg.hip) in its two forms of the host read, "drain" and "overlap"
(multigrid._PCG_READ).  Right-hand sides: the load vector of 2 pi^2 sin(pi x) sin(pi y), scaled
differently per column.

    python tools/time_multigrid_fused.py [--kind p1|p2] [--n 31] [--levels L] [--solves 20]
                                         [--rtol 1e-10] [--widths 1 2 4 8] [--label TEXT] [--log FILE]

Width 1 is ``solve`` on one vector, every other width ``solve_multi``.  For every width the three
variants take turns, `solves` solves each after two warm-up solves each; per variant the iterations,
the median and the range of the ms per solve, the ms per iteration, and that minus the separately
timed cycle of the width (the launches of ``_cycle`` alone, back to back): the outer loop's own
cost per iteration.  Wall time around a synchronised device.  One process is one run: run it three
times and compare the medians with the spread between the runs.  What is printed is also appended
to --log (default profiles/mg_fused.log)."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pytorch_fem_solver_amd import GeometricMultigrid, P2Multigrid, _native, meshgen, multigrid  # noqa: E402
from time_multigrid import load, stiffness, timed  # noqa: E402
from time_multigrid_multi import SCALES  # noqa: E402

VARIANTS = (("torch", "torch", None), ("fused, drain", "fused", "drain"), ("fused, overlap", "fused", "overlap"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("p1", "p2"), default="p1")
    ap.add_argument("--n", type=int, default=31)
    ap.add_argument("--levels", type=int, default=None)
    ap.add_argument("--solves", type=int, default=20)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--label", default="")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "mg_fused.log"))
    args = ap.parse_args()
    torch.set_default_device("cuda")
    torch.set_default_dtype(torch.float64)
    lines = []
    shipped_read = multigrid._PCG_READ  # None: by the width

    def say(text):
        print(text, flush=True)
        lines.append(text)

    mesh = meshgen.unit_square(args.n, 0.25, 0)
    if args.kind == "p1":
        build = lambda: GeometricMultigrid(mesh, 5 if args.levels is None else args.levels, stiffness,  # noqa: E731
                                           quadrature_order=2)
    else:
        build = lambda: P2Multigrid(mesh, 4 if args.levels is None else args.levels, stiffness,  # noqa: E731
                                    quadrature_order=3)
    t_setup, mg = timed(build)
    say(f"== {args.label or 'run'}: {mg!r}, {torch.cuda.get_device_name()}, rtol {args.rtol:g}, "
        f"{args.solves} solves per variant")
    say(f"set-up: {t_setup:.2f} s")
    f = mg.basis.integrate_linear_form(load).reshape(-1, 1)
    top = len(mg.levels) - 1

    for k in args.widths:
        scales = torch.tensor([SCALES[j % len(SCALES)] * (1 + j // len(SCALES)) for j in range(k)])
        B = (f * scales).contiguous()
        b = B[:, 0].contiguous()

        def solve(loop, read):
            multigrid._PCG_READ = read or multigrid._PCG_READ
            if k == 1:
                x, it, res = mg.solve(b, rtol=args.rtol, loop=loop)
                return x, [it], res
            X, its, res = mg.solve_multi(B, rtol=args.rtol, loop=loop)
            return X, its.tolist(), float(res.max())

        results = {}
        for name, loop, read in VARIANTS:  # warm-up: buffers of the width, prepared launches, pinned memory
            solve(loop, read)
            results[name] = solve(loop, read)
        times = {name: [] for name, _, _ in VARIANTS}
        for _ in range(args.solves):
            for name, loop, read in VARIANTS:
                seconds, _ = timed(lambda: solve(loop, read))
                times[name].append(seconds)
        # the cycle of the width alone, as the fused loop issues it: no copy in, no clone out
        buffers = mg._buffers if k == 1 else mg._block_buffers(k)
        applies, stream = mg._level_applies(), _native.current_stream(mg.device)
        cycle = lambda: mg._cycle(top, buffers, None if k == 1 else k, applies, stream)  # noqa: E731
        cycle()
        t_cycle, _ = timed(cycle, 50)
        what = "solve" if k == 1 else f"solve_multi, k = {k}"
        say(f"{what}: one cycle alone {t_cycle * 1e3:.3f} ms")
        x_ref = results["torch"][0]
        for name, _, _ in VARIANTS:
            x, its, res = results[name]
            med = statistics.median(times[name])
            per_it = med / max(its)
            say(f"  {name:15s}: iterations {its}, largest residual {res:.1e}, {med * 1e3:7.2f} ms per solve "
                f"({min(times[name]) * 1e3:.2f} - {max(times[name]) * 1e3:.2f}), {per_it * 1e3:.3f} ms per iteration, "
                f"outer loop {(per_it - t_cycle) * 1e3:.3f} ms per iteration, against the torch loop's solution "
                f"{float((x - x_ref).abs().max() / x_ref.abs().max()):.1e}")
        t = statistics.median(times["torch"])
        shipped = shipped_read or ("overlap" if k <= multigrid._PCG_OVERLAP_WIDTHS else "drain")
        say(f"  {what}: torch / drain {t / statistics.median(times['fused, drain']):.2f}, torch / overlap "
            f"{t / statistics.median(times['fused, overlap']):.2f}; loop=\"fused\" reads \"{shipped}\" at this width")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
