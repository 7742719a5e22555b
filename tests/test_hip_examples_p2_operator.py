"""examples/poisson_p2_operator_cg.py runs as a script on the GPU (-m gpu), as the examples of
test_hip_examples.py do: exit code 0; its own assertions are the checks."""

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_p2_operator_example_runs():
    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_p2_operator_cg.py"), "60"],
                          capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "matrix-free, P2 rows" in done.stdout, "the example prints the operator it solved with"
