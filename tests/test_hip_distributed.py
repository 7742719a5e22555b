"""BASELINE config 4 on the GPU with more than one rank (-m gpu): N processes of
tests/sharded/check_sharded_assembly.py under torch.distributed.run share the test box's one card and
exchange over gloo -- shards, ring plans with the interface tiles first, the two-stream step of
bench.py, pack / all-reduce / unpack -- and every rank compares what it holds with the operator of
the whole mesh (fp64, 1e-12).  Over RCCL (one rank per GPU) the same script runs with
--backend nccl; that needs more than one GPU and is the driver's scaling run."""

import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "tests", "sharded", "check_sharded_assembly.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, out_dir, *extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), SCRIPT, "--out-dir", str(out_dir), *extra]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    ranks = []
    for r in range(world):
        with open(os.path.join(out_dir, f"rank{r}.json")) as fh:
            ranks.append(json.load(fh))
    return ranks


@pytest.mark.parametrize("world,layout", [(2, "strips"), (3, "strips"), (2, "partition"), (4, "partition")])
def test_sharded_assembly_with_interface_tiles_first(world, layout, tmp_path):
    ranks = _run(world, tmp_path, "--layout", layout)
    for r in ranks:
        assert r["err_values"] <= 1e-12 and r["err_vector"] <= 1e-12, r
        assert r["err_values_oracle"] <= 1e-12 and r["err_vector_oracle"] <= 1e-12, r
        assert 0 < r["priority_tiles"] < r["tiles"], r
        assert r["interface_entries"] > 0
    assert len({r["interface_entries"] for r in ranks}) == 1  # one global interface numbering


@pytest.mark.parametrize("world,layout,stepper", [(2, "partition", "sharded"), (3, "partition", "sharded-first"),
                                                  (2, "strips", "sharded")])
def test_sharded_steps_of_the_bench(world, layout, stepper, tmp_path):
    """parallel.ShardedSteps (the steps bench.py --gpus N times): rotating pairs, the exchange of a
    step beside the next step's launch; every pair ends with the operator of the whole mesh."""
    ranks = _run(world, tmp_path, "--layout", layout, "--stepper", stepper)
    for r in ranks:
        assert r["err_values"] <= 1e-12 and r["err_vector"] <= 1e-12 and r["mode"] == "eager", r
        assert r["err_values_oracle"] <= 1e-12 and r["err_vector_oracle"] <= 1e-12, r


@pytest.mark.parametrize("stepper", ["graph", "graph-first"])
def test_steps_recorded_into_hip_graphs_over_rccl_one_rank(stepper, tmp_path):
    """The HIP-graph form of the steps needs RCCL (gloo cannot be captured) and the test box has one
    GPU: ONE rank over RCCL, the exchange carrying an arbitrary set of entries through pack ->
    all-reduce -> unpack inside the captured graph; replays and eager steps mixed; against the
    operator of the whole mesh."""
    ranks = _run(1, tmp_path, "--layout", "partition", "--backend", "nccl", "--stepper", stepper)
    assert ranks[0]["mode"] == "graph" and ranks[0]["err_values"] <= 1e-12 and ranks[0]["err_vector"] <= 1e-12, ranks
    assert ranks[0]["err_values_oracle"] <= 1e-12 and ranks[0]["err_vector_oracle"] <= 1e-12, ranks


def test_bench_default_scaling_is_config_4_and_one_rank_over_rccl_takes_graphs(tmp_path):
    """bench.py's N > 1 defaults: --scaling strong (BASELINE config 4).  And the whole N > 1 machinery
    with ONE rank over RCCL (torch.distributed.run, world size 1 is treated as N = 1 by bench.py, so
    the check of the graph mode over RCCL is tests/sharded/check_sharded_assembly.py above)."""
    sys.path.insert(0, REPO)
    import bench

    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "8"]
        args = bench.parse()
    finally:
        sys.argv = old
    assert args.scaling == "strong" and args.step_mode == "auto" and not args.interface_first


def test_bench_plain_run_on_one_gpu_dumps_the_last_step(tmp_path):
    """bench.py --gpus 1 without --full: the headline line alone (no CPU baseline, no other
    configurations, no stiffness-only timings), exactly --steps timed steps, and --dump-outputs
    holds what the last step computed -- K (seeded sample) and f against the numpy oracle."""
    import numpy as np

    sys.path.insert(0, REPO)
    from conftest import scaled_error
    from oracle import assembly_oracle as orc
    from pytorch_fem_solver_amd import meshgen

    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
           "--grid", "64", "--dump-outputs", str(out_dir)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    lines = [line for line in done.stdout.splitlines() if line.startswith('{"metric"')]
    assert len(lines) == 1, done.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 5 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["dtype"] == "f64" and out["higher_is_better"] is True and out["unit"] == "Melements/s"
    for key in ("cpu_baseline", "other_configs", "api_ms_per_step"):
        assert key not in out, key
    assert "stiffness_only" not in out["roofline"]

    mesh = meshgen.unit_square(64, 0.25, 0)
    verts, tris = mesh["vertices"], mesh["triangles"]
    nv = verts.shape[0]
    rowptr, colind, slots = orc.csr_pattern(tris, nv)
    k_local, _ = orc.p1_assemble(verts, tris, 3, "stiffness")
    f_local, _ = orc.p1_assemble(verts, tris, 3, "load")
    want_vals = orc.assemble_csr_values(k_local, slots, colind.shape[0])
    want_f = orc.assemble_linear(f_local, tris, nv)
    got = {name: np.load(out_dir / f"{name}.npy") for name in ("K_values", "K_rows", "K_cols", "f")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["K_values"].size == colind.shape[0]  # below the sample size: every entry, in CSR order
    assert np.array_equal(got["K_rows"], np.repeat(np.arange(nv), np.diff(rowptr)))
    assert np.array_equal(got["K_cols"], colind)
    assert scaled_error(got["K_values"], want_vals) <= 1e-12
    assert scaled_error(got["f"].reshape(want_f.shape), want_f) <= 1e-12


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_runs_with_two_ranks(scaling, tmp_path):
    """The driver's multi-GPU command line (bench.py under torch.distributed.run), two ranks on the
    one card over gloo, small mesh: one JSON line from rank 0 with the contract's keys."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--steps", "20", "--warmup", "5", "--grid", "256", "--backend", "gloo", "--scaling", scaling]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    lines = [line for line in done.stdout.splitlines() if line.startswith('{"metric"')]
    assert len(lines) == 1, done.stdout[-2000:]
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in out, key
    assert out["n_gpus"] == 2 and out["steps"] == 20 and out["warmup"] == 5 and out["scaling"] == scaling
    assert out["value"] > 0 and out["config"]["interface_tiles_first"] is None  # one launch per step by default
    assert out["config"]["world_size"] == 2 and out["config"]["backend"] == "gloo" and len(out["config"]["devices"]) == 2
    assert out["config"]["step_mode"] == "eager" and out["config"]["host_us_per_step"] > 0
    n_elems = 2 * 256 * 256
    assert out["config"]["elements_per_gpu"] == (n_elems if scaling == "weak" else n_elems // 2)
