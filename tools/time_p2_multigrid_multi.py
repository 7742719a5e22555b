"""Times P2Multigrid.solve_multi on k right-hand sides against k calls of P2Multigrid.solve, one GPU,
one process: the P2 Poisson problem of tools/time_p2_multigrid.py (unit_square(n, 0.25, 0) refined
`levels` times with the P2 level on top; the defaults, 31 and 4, give 986,049 P2 DoFs), right-hand
sides the load vector of 2 pi^2 sin(pi x) sin(pi y) scaled differently per column.

    python tools/time_p2_multigrid_multi.py [--n 31] [--levels 4] [--runs 3] [--rtol 1e-10]
                                            [--widths 2 4 8] [--log FILE]

For every width k the two take turns, `runs` runs each after one warm-up each; medians and ranges are
printed.  Then the time of one block V-cycle at every k against one single cycle, and how each divides
into the P2 level's operator launches, its tfem_mg_* launches (the sweeps and the two P2 transfers)
and the P1 cycle below -- each class of launches timed on its own, back to back, in the numbers one
cycle issues them (as tools/time_p2_multigrid.py does for the single cycle).  Wall time around a
synchronised device.  What is printed is also written to --log (default
profiles/p2_multigrid_multi.log, appended)."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pytorch_fem_solver_amd import P2Multigrid, meshgen  # noqa: E402
from time_multigrid import cycle_parts, load, stiffness, timed  # noqa: E402
from time_multigrid_multi import SCALES, spread  # noqa: E402


def parts_text(parts):
    return (f"P2 operator launches {parts[0] * 1e3:.3f} ms, tfem_mg launches of the P2 level {parts[1] * 1e3:.3f} ms, "
            f"the P1 cycle {parts[2] * 1e3:.3f} ms (sum {sum(parts) * 1e3:.3f} ms: "
            f"{', '.join(f'{100 * p / sum(parts):.0f} %' for p in parts)})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=31)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--widths", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "p2_multigrid_multi.log"))
    args = ap.parse_args()
    torch.set_default_device("cuda")
    torch.set_default_dtype(torch.float64)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    t_setup, mg = timed(lambda: P2Multigrid(meshgen.unit_square(args.n, 0.25, 0), args.levels, stiffness,
                                            quadrature_order=3))
    say(repr(mg))
    say(f"set-up: {t_setup:.2f} s")
    f = mg.basis.integrate_linear_form(load).reshape(-1, 1)
    n = f.shape[0]
    top = len(mg.levels) - 1

    for k in args.widths:
        scales = torch.tensor([SCALES[j % len(SCALES)] * (1 + j // len(SCALES)) for j in range(k)])
        B = (f * scales).contiguous()
        columns = [B[:, j].contiguous() for j in range(k)]

        def block():
            return mg.solve_multi(B, rtol=args.rtol)

        def singles():
            return [mg.solve(b, rtol=args.rtol) for b in columns]

        block(), singles()  # warm-up: buffers of the width, prepared launches
        times = {"solve_multi": [], "k x solve": []}
        for run in range(args.runs):
            seconds, (X, its, res) = timed(block)
            times["solve_multi"].append(seconds)
            say(f"k = {k} run {run + 1} solve_multi: iterations {its.tolist()}, largest residual {float(res.max()):.1e}, "
                f"{seconds * 1e3:9.2f} ms")
            seconds, results = timed(singles)
            times["k x solve"].append(seconds)
            say(f"k = {k} run {run + 1} {k} x solve   : iterations {[r[1] for r in results]}, largest residual "
                f"{max(r[2] for r in results):.1e}, {seconds * 1e3:9.2f} ms")
        X_single = torch.stack([r[0] for r in results], dim=1)
        say(f"k = {k}: the two solutions differ by {float((X - X_single).abs().max() / X_single.abs().max()):.1e} "
            f"(relative, max norm)")
        med = {name: statistics.median(v) for name, v in times.items()}
        say(f"k = {k} median of {args.runs}: solve_multi {spread(times['solve_multi'])}, {k} x solve "
            f"{spread(times['k x solve'])}, ratio {med['k x solve'] / med['solve_multi']:.2f}, per column "
            f"{med['solve_multi'] / k * 1e3:.2f} ms against {med['k x solve'] / k * 1e3:.2f} ms")

    reps = 20
    r = torch.randn(n)
    mg._vcycle_into(r)
    t_single, _ = timed(lambda: mg._vcycle_into(r), reps)
    say(f"one single V({mg.nu},{mg.nu}) cycle: {t_single * 1e3:.3f} ms; alone: {parts_text(cycle_parts(mg, reps, bottom=top))}")
    for k in args.widths:
        R = torch.randn(n, k)
        mg._vcycle_multi_into(R)
        t_block, _ = timed(lambda: mg._vcycle_multi_into(R), reps)
        say(f"one block cycle, k = {k}: {t_block * 1e3:.3f} ms = {t_block / t_single:.2f} single cycles "
            f"({t_block / k * 1e3:.3f} ms per column); alone: {parts_text(cycle_parts(mg, reps, k, bottom=top))}")
        x, ax, _ = mg._block_buffers(k)[top]
        t_top, _ = timed(lambda: mg._level_applies()[-1](x, ax), reps)
        say(f"  one block P2 apply, k = {k}: {t_top * 1e6:.1f} us")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
