"""bench.py contract tests: JSON shape, weak-scaling distributed path
(gloo, world_size 2 — the driver launches the same way on GPU nodes)."""

import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def last_json_line(text):
    for line in reversed(text.strip().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{text}")


def check_contract(out, n_gpus):
    assert out["metric"] == "solver_wall_clock_ms"
    assert out["unit"] == "ms"
    assert out["n_gpus"] == n_gpus
    assert out["higher_is_better"] is False
    assert out["scaling"] == "weak"
    assert out["data"] == "synthetic"
    assert out["value"] > 0
    assert out["ms_per_step"] == out["value"]
    assert 0.0 <= out["slo_attainment_pct"] <= 100.0
    assert out["config"]["variants"] == n_gpus * 8


class TestBench:
    def test_single_process(self):
        proc = subprocess.run(
            [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
             "--variants-per-gpu", "8", "--full", "--no-observed-slo"],
            cwd=ROOT,
            capture_output=True,
            text=True,
            timeout=300,
        )
        assert proc.returncode == 0, proc.stderr
        out = last_json_line(proc.stdout)
        check_contract(out, n_gpus=1)
        # the headline is the capacity-constrained greedy solve; the
        # easier unlimited argmin rides along as a secondary series
        assert out["unlimited_ms_per_step"] > 0
        assert "greedy-limited" in out["config"]["solver_mode"]

    def test_plain_run_is_lean_and_dumps_outputs(self, tmp_path):
        """A plain run reports only the headline, and --dump-outputs
        writes the last timed step's arrays, identical from run to run."""
        import numpy as np

        dumps = []
        for name in ("a", "b"):
            proc = subprocess.run(
                [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
                 "--variants-per-gpu", "8", "--dump-outputs", str(tmp_path / name)],
                cwd=ROOT,
                capture_output=True,
                text=True,
                timeout=300,
            )
            assert proc.returncode == 0, proc.stderr
            out = last_json_line(proc.stdout)
            check_contract(out, n_gpus=1)
            assert out["steps"] == 2
            assert out["dtype"] == "fp64"
            assert "unlimited_ms_per_step" not in out
            assert "observed_slo_attainment_pct" not in out
            files = sorted(p.name for p in (tmp_path / name).iterdir())
            assert files == ["sizing.npy", "solution.npy"]
            dumps.append({f: np.load(tmp_path / name / f) for f in files})

        solution, sizing = dumps[0]["solution.npy"], dumps[0]["sizing.npy"]
        assert solution.dtype == np.float64 and solution.shape == (8, 6)
        assert sizing.dtype == np.float64 and sizing.shape == (8, 3, 7)
        assert np.isfinite(solution).all() and np.isfinite(sizing).all()
        # every allocated variant's row repeats its sizing entry
        allocated = solution[:, 0] >= 0
        assert allocated.any()
        for i in np.flatnonzero(allocated):
            acc = int(solution[i, 0])
            assert solution[i, 1] >= 1
            assert sizing[i, acc, 1] == solution[i, 2]  # batch size
        for f in dumps[0]:
            np.testing.assert_array_equal(dumps[0][f], dumps[1][f])

    def test_two_rank_gloo(self):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1")
        proc = subprocess.run(
            [
                sys.executable, "-m", "torch.distributed.run",
                "--nnodes=1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", "29517",
                "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
                "--variants-per-gpu", "8", "--backend", "gloo",
            ],
            cwd=ROOT,
            capture_output=True,
            text=True,
            timeout=600,
            env=env,
        )
        assert proc.returncode == 0, proc.stderr
        check_contract(last_json_line(proc.stdout), n_gpus=2)
