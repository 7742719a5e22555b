"""Times GeometricMultigrid.solve_multi on k right-hand sides against k calls of
GeometricMultigrid.solve, one GPU, one process: the Poisson problem of tools/time_multigrid.py
(unit_square(n, 0.25, 0) refined `levels` times; the defaults, 31 and 5, give 986,049 vertices),
right-hand sides the load vector of 2 pi^2 sin(pi x) sin(pi y) scaled differently per column.

    python tools/time_multigrid_multi.py [--n 31] [--levels 5] [--runs 3] [--rtol 1e-10] [--widths 2 4 8]

For every width k the two take turns, `runs` runs each after one warm-up each; medians and ranges are
printed.  Then the time of one block V-cycle at every k against one single cycle, and how each divides
into the operator launches, the tfem_mg_* launches and the coarse product -- each class of launches
timed on its own, back to back, in the numbers and sizes one cycle issues them (as
tools/time_multigrid.py does for the single cycle).  Wall time around a synchronised device."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_fem_solver_amd import GeometricMultigrid, meshgen  # noqa: E402
from time_multigrid import cycle_parts, load, stiffness, timed  # noqa: E402

SCALES = (1.0, -2.0, 0.5, 3.0, -0.25, 1.5, -4.0, 0.75)


def spread(values):
    return f"{statistics.median(values) * 1e3:.2f} ms ({min(values) * 1e3:.2f} - {max(values) * 1e3:.2f})"


def parts_text(parts):
    return (f"operator launches {parts[0] * 1e3:.3f} ms, tfem_mg launches {parts[1] * 1e3:.3f} ms, coarse product "
            f"{parts[2] * 1e3:.3f} ms (sum {sum(parts) * 1e3:.3f} ms: "
            f"{', '.join(f'{100 * p / sum(parts):.0f} %' for p in parts)})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=31)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--widths", type=int, nargs="+", default=[2, 4, 8])
    args = ap.parse_args()
    torch.set_default_device("cuda")
    torch.set_default_dtype(torch.float64)

    t_setup, mg = timed(lambda: GeometricMultigrid(meshgen.unit_square(args.n, 0.25, 0), args.levels, stiffness,
                                                   quadrature_order=2))
    print(mg)
    print(f"set-up: {t_setup:.2f} s")
    f = mg.basis.integrate_linear_form(load).reshape(-1, 1)
    n = f.shape[0]

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
            print(f"k = {k} run {run + 1} solve_multi: iterations {its.tolist()}, largest residual {float(res.max()):.1e}, "
                  f"{seconds * 1e3:9.2f} ms")
            seconds, results = timed(singles)
            times["k x solve"].append(seconds)
            print(f"k = {k} run {run + 1} {k} x solve   : iterations {[r[1] for r in results]}, largest residual "
                  f"{max(r[2] for r in results):.1e}, {seconds * 1e3:9.2f} ms")
        X_single = torch.stack([r[0] for r in results], dim=1)
        print(f"k = {k}: the two solutions differ by {float((X - X_single).abs().max() / X_single.abs().max()):.1e} "
              f"(relative, max norm)")
        med = {name: statistics.median(v) for name, v in times.items()}
        print(f"k = {k} median of {args.runs}: solve_multi {spread(times['solve_multi'])}, {k} x solve "
              f"{spread(times['k x solve'])}, ratio {med['k x solve'] / med['solve_multi']:.2f}, per column "
              f"{med['solve_multi'] / k * 1e3:.2f} ms against {med['k x solve'] / k * 1e3:.2f} ms")

    reps = 20
    r = torch.randn(n)
    mg._vcycle_into(r)
    t_single, _ = timed(lambda: mg._vcycle_into(r), reps)
    print(f"one single V({mg.nu},{mg.nu}) cycle: {t_single * 1e3:.3f} ms; alone: {parts_text(cycle_parts(mg, reps))}")
    for k in args.widths:
        R = torch.randn(n, k)
        mg._vcycle_multi_into(R)
        t_block, _ = timed(lambda: mg._vcycle_multi_into(R), reps)
        print(f"one block cycle, k = {k}: {t_block * 1e3:.3f} ms = {t_block / t_single:.2f} single cycles "
              f"({t_block / k * 1e3:.3f} ms per column); alone: {parts_text(cycle_parts(mg, reps, k))}")
        top = len(mg.levels) - 1
        x, ax, _ = mg._block_buffers(k)[top]
        t_top, _ = timed(lambda: mg._level_applies()[-1](x, ax), reps)
        print(f"  one block apply on the finest level, k = {k}: {t_top * 1e6:.1f} us")


if __name__ == "__main__":
    main()
