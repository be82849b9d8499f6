"""bench.py's N>1 launch path on CPU: started plainly (no RANK in the environment) with
--gpus N it must spawn its own ranks, rendezvous on 127.0.0.1 and let rank 0 print ONE JSON
line — the form the round driver uses.  `--rehearse-launch` keeps GPU and evaluation out of it
(it is a launch-path test, not a measurement)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


@pytest.mark.parametrize("n", [2, 3])
def test_plain_launch_spawns_its_ranks(n):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--rehearse-launch"],
                       env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out == {"rehearsal": True, "n_gpus": n, "max_rank_seen": n - 1}


@pytest.mark.parametrize("branch,path", [("own", "own"), ("children_failed", "rccl"), ("connect_failed", "rccl"), ("warmup_timeout", "rccl"),
                                         ("rccl_failed", "none")])
def test_comm_path_selection_branches(branch, path):
    """What the N > 1 timed step contains (bench.choose_comm_path), every branch forced with simulated outcomes under gloo:
    the library's mailboxes, the torch.distributed fallback when the child check / the wiring / a warm-up wait failed (one
    rank's time-out is everybody's), and 'none' only when the fallback failed too."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rehearse-launch", "--rehearse-comm", branch],
                       env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["comm"]["path"] == path and out["comm"]["world_size"] == 2
    assert (out["comm"]["why"] == "") == (path == "own")


def test_failed_rank_fails_the_launch():
    """Without a GPU a real run cannot start: every rank dies, and the parent must report it (non-zero
    exit, no JSON line) instead of hanging at a barrier."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_dump_outputs_writes_a_fixed_sample_within_the_budget(tmp_path):
    """`--dump-outputs`: a buffer over its share of the budget is written as the same sample on every run, every file
    together under 64 MB; a small buffer is written whole."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(5_000_000, dtype=torch.float64)
    small = 0.5 * torch.arange(1000, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"jac_coord": big, "hess_coord": small})
    a, b = np.load(tmp_path / "a" / "jac_coord.npy"), np.load(tmp_path / "b" / "jac_coord.npy")
    assert a.dtype == np.float64 and np.array_equal(a, b) and 0 < a.size < big.numel()
    assert np.all(np.diff(a) > 0) and a[-1] < big.numel()      # distinct entries of the buffer, in buffer order
    assert np.array_equal(np.load(tmp_path / "a" / "hess_coord.npy"), small.numpy())
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64_000_000


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_what_they_computed(tmp_path, built):
    """A plain one-GPU run: exactly `--steps` timed steps, the headline line without the `--full` entries, and
    `--dump-outputs` holding the jac / hess values of the last step — checked against the CPU oracle at the bench's own
    seeded point."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from infiniteexamodels.jl_amd import transcribe, workloads
    from pyoracle import OracleModel
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--supports", "20000", "--steps", "7",
                        "--warmup", "2", "--dump-outputs", str(tmp_path)], env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["steps"] == 7 and j["warmup"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["higher_is_better"] is True and j["dtype"] == "f64" and j["metric"] and j["unit"]
    assert not set(j) & {"roofline", "pair_ms", "fused_pair", "escape34_variant", "cpu_baseline"}
    om = OracleModel(transcribe.exa_core(workloads.quadrotor(20000)).to_blob())
    x, y = bench.eval_point(om.nvar, om.ncon, om.x0, om.nvar // 22)
    for name, want in (("jac_coord", om.jac_coord(x)), ("hess_coord", om.hess_coord(x, y, 1.0))):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == want.shape, name
        scale = np.maximum(np.abs(want), 1e-10 * max(1.0, np.abs(want).max()))
        assert float((np.abs(got - want) / scale).max()) <= 1e-10, name
