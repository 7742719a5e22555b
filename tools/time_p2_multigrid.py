"""Times P2Multigrid.solve against the Jacobi-preconditioned fused CG (FormOperator.solve_cg) on the
same P2 system, one GPU, one process: the Poisson problem of examples/poisson_p2_multigrid.py on
unit_square(n, 0.25, 0) refined `levels` times with the P2 level on top (the defaults, 31 and 4, give
986,049 P2 DoFs).

    python tools/time_p2_multigrid.py [--n 31] [--levels 4] [--runs 3] [--rtol 1e-10] [--log FILE]

The two solvers take turns, `runs` runs each after one warm-up each, and the medians are printed;
then the time of one V-cycle and how it divides into the P2 level's operator launches, its
tfem_mg_* launches (the sweeps and the two P2 transfers) and the P1 cycle below -- each class timed
on its own, back to back, in the numbers one cycle issues them (2 nu applies and 2 nu sweeps, one
restriction, one prolongation, one P1 cycle).  Wall time around a synchronised device.  What is
printed is also written to --log (default profiles/p2_multigrid.log, appended)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=31)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "p2_multigrid.log"))
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
    say(f"set-up (refinement on the host, {len(mg.levels)} bases, plans, diagonals, coarse factor): {t_setup:.2f} s")
    for level in mg.levels:
        say(f"  {level}")
    f = mg.basis.integrate_linear_form(load)
    free = mg.basis._basis_parameters["inner_dofs"]

    def multigrid():
        return mg.solve(f, rtol=args.rtol)

    def jacobi():
        return mg.operator.solve_cg(f, free=free, rtol=args.rtol)

    multigrid(), jacobi()  # warm-up: plans, prepared launches
    times = {"multigrid": [], "jacobi": []}
    for run in range(args.runs):
        for name, fn in (("multigrid", multigrid), ("jacobi", jacobi)):
            seconds, (x, it, res) = timed(fn)
            times[name].append(seconds)
            say(f"run {run + 1} {name:9s}: {it:5d} iterations, residual {res:.1e}, {seconds * 1e3:9.2f} ms")
    x_mg, x_j = multigrid()[0], jacobi()[0]
    say(f"the two solutions differ by {float((x_mg - x_j).abs().max() / x_j.abs().max()):.1e} (relative, max norm)")
    med = {k: statistics.median(v) for k, v in times.items()}
    say(f"median of {args.runs}: multigrid {med['multigrid'] * 1e3:.2f} ms, Jacobi CG {med['jacobi'] * 1e3:.2f} ms, "
        f"ratio {med['jacobi'] / med['multigrid']:.2f}")

    top = mg.levels[-1]
    r = torch.randn(top.n)
    reps = 20
    mg._vcycle_into(r)
    t_cycle, _ = timed(lambda: mg._vcycle_into(r), reps)
    parts = cycle_parts(mg, reps, bottom=len(mg.levels) - 1)  # the P2 level alone, the P1 cycle below it
    say(f"one V({mg.nu},{mg.nu}) cycle: {t_cycle * 1e3:.3f} ms; alone: P2 operator launches {parts[0] * 1e3:.3f} ms, "
        f"tfem_mg launches of the P2 level {parts[1] * 1e3:.3f} ms, the P1 cycle {parts[2] * 1e3:.3f} ms "
        f"(sum {sum(parts) * 1e3:.3f} ms: {', '.join(f'{100 * p / sum(parts):.0f} %' for p in parts)})")
    t_top, _ = timed(lambda: mg._level_applies()[-1](top.x, top.ax), reps)
    say(f"one P2 apply: {t_top * 1e6:.1f} us")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
