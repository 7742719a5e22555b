"""examples/poisson_p2_multigrid.py runs as a script on the GPU (-m gpu), as the examples of
test_hip_examples.py do, and the error it prints against the exact solution falls with the mesh
size as P2 elements promise: by about 8 per refinement (h^3) or more; at least 6 is asserted."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_p2_multigrid_example_runs_and_converges_with_h():
    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_p2_multigrid.py"), "8", "3"],
                          capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    rows = re.findall(r"^level (\d+): (\d+) DoFs, (\d+) iterations, .* max nodal error ([0-9.e+-]+),", done.stdout, re.M)
    assert [int(r[0]) for r in rows] == [1, 2, 3], done.stdout
    assert [int(r[1]) for r in rows] == [33 * 33, 65 * 65, 129 * 129]
    errors = [float(r[3]) for r in rows]
    print(done.stdout)
    for coarse, fine in zip(errors, errors[1:]):
        assert coarse >= 6.0 * fine, errors
    assert all(int(r[2]) <= 20 for r in rows)
