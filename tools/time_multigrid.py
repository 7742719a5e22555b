"""Times GeometricMultigrid.solve against the Jacobi-preconditioned fused CG (FormOperator.solve_cg)
on the same system, one GPU, one process: the Poisson problem of examples/poisson_multigrid.py on
unit_square(n, 0.25, 0) refined `levels` times (the defaults, 31 and 5, give 986,049 vertices).

    python tools/time_multigrid.py [--n 31] [--levels 5] [--runs 3] [--rtol 1e-10]

The two solvers take turns, `runs` runs each after one warm-up each, and the medians are printed;
then the time of one V-cycle and how it divides into the operator launches, the tfem_mg_* launches
and the coarse solve -- each class of launches timed on its own, back to back, in the numbers and
sizes one cycle issues them (2 nu applies and 2 nu sweeps per level, one restriction and one
prolongation per level, one coarse solve).  Wall time around a synchronised device."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_fem_solver_amd import GeometricMultigrid, _native, meshgen  # noqa: E402


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


def load(b):
    x, y = torch.split(b.integration_points, 1, dim=-1)
    return 2.0 * math.pi**2 * torch.sin(math.pi * x) * torch.sin(math.pi * y) * b.v


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def cycle_parts(mg, reps, k=None, bottom=1):
    """Seconds per cycle of (operator launches, tfem_mg launches, what lies below), each class alone:
    the launches of the levels from ``bottom`` up on the single-vector buffers (k None) or the block
    buffers of the width k, and the cycle of the level under ``bottom`` (the coarse solve for 1)."""
    buffers = mg._buffers if k is None else mg._block_buffers(k)
    applies = mg._level_applies()
    stream = _native.current_stream(mg.device)
    tops = range(bottom, len(mg.levels))

    def operators():
        for l in tops:
            x, ax, _ = buffers[l]
            for _ in range(2 * mg.nu):
                applies[l](x, ax)

    def transfers():
        for l in tops:
            level = mg.levels[l]
            level.smooth(buffers[l], k, True, stream)
            for _ in range(2 * mg.nu - 1):
                level.smooth(buffers[l], k, False, stream)
            level.restrict_residual(buffers[l], buffers[l - 1], k, stream)
            level.prolong_add(buffers[l], buffers[l - 1], k, stream)

    def below():
        mg._cycle(bottom - 1, buffers, k, applies, stream)

    return tuple(timed(fn, reps)[0] for fn in (operators, transfers, below))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=31)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-10)
    args = ap.parse_args()
    torch.set_default_device("cuda")
    torch.set_default_dtype(torch.float64)

    t_setup, mg = timed(lambda: GeometricMultigrid(meshgen.unit_square(args.n, 0.25, 0), args.levels, stiffness,
                                                   quadrature_order=2))
    print(mg)
    print(f"set-up (refinement on the host, {len(mg.levels)} bases, diagonals, coarse factor): {t_setup:.2f} s")
    for level in mg.levels:
        print(f"  {level}")
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
            print(f"run {run + 1} {name:9s}: {it:5d} iterations, residual {res:.1e}, {seconds * 1e3:9.2f} ms")
    x_mg, x_j = multigrid()[0], jacobi()[0]
    print(f"the two solutions differ by {float((x_mg - x_j).abs().max() / x_j.abs().max()):.1e} (relative, max norm)")
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"median of {args.runs}: multigrid {med['multigrid'] * 1e3:.2f} ms, Jacobi CG {med['jacobi'] * 1e3:.2f} ms, "
          f"ratio {med['jacobi'] / med['multigrid']:.2f}")

    r = torch.randn(mg.operator.shape[0])
    reps = 20
    t_cycle, _ = timed(lambda: mg._vcycle_into(r), reps)
    parts = cycle_parts(mg, reps)
    print(f"one V({mg.nu},{mg.nu}) cycle: {t_cycle * 1e3:.3f} ms; alone: operator launches {parts[0] * 1e3:.3f} ms, "
          f"tfem_mg launches {parts[1] * 1e3:.3f} ms, coarse solve {parts[2] * 1e3:.3f} ms "
          f"(sum {sum(parts) * 1e3:.3f} ms: {', '.join(f'{100 * p / sum(parts):.0f} %' for p in parts)})")
    top = mg.levels[-1]
    t_top, _ = timed(lambda: mg._level_applies()[-1](top.x, top.ax), reps)
    print(f"one apply on the finest level: {t_top * 1e6:.1f} us")


if __name__ == "__main__":
    main()
