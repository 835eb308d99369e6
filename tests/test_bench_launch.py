"""bench.py --gpus N outside a launcher starts N ranks itself (one process per
GPU, torch.distributed.run as a child process) instead of silently running
one rank.  SFM_BENCH_LAUNCH_CHECK makes every rank report
its rendezvous and exit before any GPU work, so this runs on CPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["SFM_BENCH_LAUNCH_CHECK"] = "1"
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def test_self_launch_spawns_n_ranks():
    rows = _run(["--gpus", "2", "--steps", "1"])
    assert sorted(r["rank"] for r in rows) == [0, 1]
    assert all(r["world"] == 2 and r["gpus"] == 2 for r in rows)
    assert sorted(r["local_rank"] for r in rows) == [0, 1]


def test_single_gpu_runs_in_process():
    rows = _run(["--gpus", "1"])
    assert rows == [{"rank": 0, "world": 1, "local_rank": 0, "gpus": 1}]


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)   # module level: argument helpers and the ABI binding only (no GPU work)
    return m


def test_loop_replica_line():
    """C5 at N > 1 is N independent sequences: the
    aggregate is named as such, over the slowest replica, with every
    replica's own rate beside it."""
    b = _bench_module()
    r = {"metric": "C5 incremental loop images/sec, fixed write-back", "value": 30.0, "seconds": 10.0,
         "unit": "images/s", "ba_calls": 299}
    out = b.loop_replica_line(r, [10.0, 12.0, 11.0, 10.5], 300)
    assert out["replicas"] == 4 and out["seconds"] == 12.0
    assert abs(out["value"] - 4 * 300 / 12.0) < 1e-9
    assert out["per_replica_images_per_sec"] == [30.0, 25.0, 300 / 11.0, 300 / 10.5]
    assert out["slowest_replica_images_per_sec"] == 25.0
    assert "aggregate of 4 independent replicas" in out["metric"] and out["scaling"].startswith("weak")
    assert out["ba_calls"] == 299 and r["value"] == 30.0   # the rank's own line is not modified


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times the C4 steps and nothing else: every --full section
    of the line is empty, --steps is the number of timed steps, and
    --dump-outputs leaves the adjusted parameters of the last step as float64
    arrays that a second run with the same arguments reproduces."""
    import numpy as np

    def run(out):
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                            "--warmup", "1", "--n-cam", "40", "--n-pt", "4000", "--dump-outputs", str(out)],
                           env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
        assert len(lines) == 1, r.stdout
        return lines[0], {n: np.load(out / f"{n}.npy") for n in ("extr", "intr", "X", "summary")}

    line, a = run(tmp_path / "a")
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "LM-iters/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    # value = LM iterations of the timed steps / their wall time
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 * 2 - 2 * line["lm_iterations_per_solve"]) < 1e-6
    for k in ("roofline", "cpu_baseline", "match", "ba_snavely", "ba_pcie_inclusive", "loop",
              "loop_fixed_writeback", "filter", "ba_dense_s", "ba_radial3", "ba_radial3_percam"):
        assert line[k] is None, k
    assert a["extr"].shape == (6 * 40,) and a["X"].shape == (3 * 4000,) and a["summary"].shape == (8,)
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
    assert a["summary"][0] == line["lm_iterations_per_solve"] and a["summary"][7] == line["rmse_final"]
    assert line["rmse_final"] < line["rmse_initial"]
    _, b = run(tmp_path / "b")
    assert np.array_equal(a["summary"][:4], b["summary"][:4])
    for n in ("extr", "intr", "X"):   # same seeded scene, same solve: equal to rounding of the reductions
        assert np.allclose(a[n], b[n], rtol=1e-9, atol=1e-9), n


@pytest.mark.gpu
def test_loop_replicas_two_ranks_one_gpu():
    """bench.py's N > 1 loop branch end to end on one GPU: two ranks (the
    RCCL communicator cannot span one device twice, so the BA exchange falls
    back to the gloo hook, which the line names), each running its own short
    sequence; rank 0 prints one line whose loop entry is the replica
    aggregate."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["SFM_BENCH_SAME_DEVICE"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--full", "--steps", "1", "--warmup", "0", "--n-cam", "40", "--n-pt", "4000",
           "--loop-images", "12", "--allow-host-allreduce", "--no-match", "--no-snavely", "--no-radial3",
           "--no-filter", "--no-dense", "--no-pmc", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["n_gpus"] == 2 and "gloo" in line["config"]["transport"]
    lp = line["loop_fixed_writeback"]
    assert lp["replicas"] == 2 and len(lp["per_replica_images_per_sec"]) == 2
    assert abs(lp["value"] - 2 * 12 / lp["seconds"]) < 1e-6
    assert lp["kept_images"] >= 10 and lp["ba_calls"] == 11
