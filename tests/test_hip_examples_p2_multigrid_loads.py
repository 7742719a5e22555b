"""examples/poisson_p2_multigrid_loads.py runs as a script on the GPU (-m gpu) at its smallest
setting -- a 4 x 4 coarse mesh refined once, 289 P2 DoFs, four load cases -- and its own checks pass:
every column of P2Multigrid.solve_multi converges and agrees with P2Multigrid.solve on that column."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_p2_multigrid_loads_example_runs_and_agrees_with_solve():
    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_p2_multigrid_loads.py"), "4", "1"],
                          capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    print(done.stdout)
    assert re.search(r"^289 P2 DoFs, 4 load cases$", done.stdout, re.M), done.stdout
    rows = re.findall(r"^\s+mode \((\d), (\d)\)\s*: (\d+) iterations \(solve: (\d+)\), residual ([0-9.e+-]+), "
                      r"differs from solve by ([0-9.e+-]+)$", done.stdout, re.M)
    assert [(int(r[0]), int(r[1])) for r in rows] == [(1, 1), (2, 1), (1, 3), (3, 2)], done.stdout
    for row in rows:
        assert abs(int(row[2]) - int(row[3])) <= 2 and int(row[2]) <= 20
        assert float(row[4]) <= 1e-10 and float(row[5]) <= 1e-8
    assert re.search(r"^one solve_multi [0-9.]+ ms, 4 x solve [0-9.]+ ms$", done.stdout, re.M), done.stdout
