"""bench.py's launcher and sharding logic without a GPU: `--gpus 2` must start two ranks itself (gloo, a CPU stand-in for the
solver: RYDIFF_BENCH_STANDIN=1), deal the c4 parameter sets over them, gather the results and print ONE JSON line that says
n_gpus == 2.  The numbers of a stand-in run mean nothing; the plumbing is what is tested."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _run(*argv, env_extra=None):
    env = dict(os.environ, RYDIFF_BENCH_STANDIN="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=300)


def test_gpus_flag_spawns_the_ranks_and_reports_them():
    r = _run("--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "10", "--chunk", "3", "--time-steps", "8")
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["ranks"] == 2
    assert out["config"]["workload"].startswith("c4")          # the multi-rank default workload
    assert out["scaling"] == "strong"
    assert out["config"]["trajectories_total"] == 10 and out["config"]["trajectories_this_rank"] == 5
    assert out["config"]["gathered_parameter_sets"] == 10       # all_gather of the per-set gradients reached every rank
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0
    assert "standin" in out["data"]


def test_single_rank_default_is_the_headline_workload():
    r = _run("--steps", "1", "--warmup", "0", "--time-steps", "8")
    assert r.returncode == 0, r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and out["config"]["workload"].startswith("c3") and out["scaling"] == "weak"


def _line(r):
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_repeat_run_to_run_and_with_full(tmp_path):
    """--dump-outputs: the last timed step's outputs as float64 .npy files (at most 64 MiB in all); the inputs are seeded, so
    the same arguments — with or without --full, which only adds secondary figures — write the same arrays."""
    import numpy as np

    runs = {"a": (), "b": (), "full": ("--full",)}
    for name, extra in runs.items():
        out = _line(_run("--steps", "2", "--warmup", "1", "--time-steps", "8", "--dump-outputs", str(tmp_path / name), *extra))
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["dtype"] == "c128" and out["higher_is_better"] is True
    names = sorted(p.name for p in (tmp_path / "a").glob("*.npy"))
    assert names == ["expect_sum_z.npy", "grad_delta.npy", "grad_omega.npy"]
    assert np.load(tmp_path / "a" / "expect_sum_z.npy").shape == (1, 9)
    assert np.load(tmp_path / "a" / "grad_omega.npy").shape == (1, 4)
    for name in runs:
        assert sum(p.stat().st_size for p in (tmp_path / name).glob("*.npy")) <= 64 << 20
        for f in names:
            a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / name / f)
            assert a.dtype == np.float64 and np.array_equal(a, b)


def test_dump_outputs_gather_every_parameter_set_over_the_ranks(tmp_path):
    import numpy as np

    out = _line(_run("--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "10", "--chunk", "3", "--time-steps", "8",
                     "--dump-outputs", str(tmp_path)))
    assert out["n_gpus"] == 2
    ex = np.load(tmp_path / "expect_sum_z.npy")
    assert ex.shape == (10, 9) and len(np.unique(ex[:, 0])) == 10  # one row per parameter set, rank 1's sets included
    assert np.load(tmp_path / "grad_delta.npy").shape == (10, 4)


def test_rank_count_must_match_the_flag():
    r = _run("--gpus", "4", env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "must match" in (r.stderr + r.stdout)


def _load_bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_state_sharded_leg_failure_only_costs_its_field(tmp_path, monkeypatch):
    """The secondary c5 leg of the --full line runs in a child process group.  Here the child ends with an
    error on any machine (no GPU, or RYDIFF_LIB names a library that does not exist): the function must hand back an `error`
    field (rc and stderr tail) and nothing else."""
    import argparse

    bench = _load_bench()
    monkeypatch.setenv("RYDIFF_LIB", str(tmp_path / "missing" / "librydiff.so"))
    env_backup = os.environ.pop("RYDIFF_BENCH_STANDIN", None)
    try:
        out = bench.c5_leg_in_child_group(argparse.Namespace(variant=0), 1)
    finally:
        if env_backup is not None:
            os.environ["RYDIFF_BENCH_STANDIN"] = env_backup
    assert set(out) == {"error"} and "rc" in out["error"]


def test_state_sharded_leg_is_killed_as_a_group_on_timeout(tmp_path, monkeypatch):
    """A leg that hangs (here: a stand-in 'interpreter' that starts a grandchild and sleeps) is killed with its whole process
    group after the time limit; the caller gets an `error` field and carries on — no os._exit from a GPU-initialised rank."""
    import argparse
    import time

    bench = _load_bench()
    pidfile = tmp_path / "grandchild.pid"
    fake = tmp_path / "hang.sh"
    fake.write_text(f"#!/bin/bash\nsleep 300 &\necho $! > {pidfile}\nsleep 300\n")
    fake.chmod(0o755)
    monkeypatch.setattr(bench.sys, "executable", str(fake))
    monkeypatch.setattr(bench, "C5_LEG_TIMEOUT_S", 2.0)
    t0 = time.time()
    out = bench.c5_leg_in_child_group(argparse.Namespace(variant=0), 2)
    assert set(out) == {"error"} and "killed" in out["error"]
    assert time.time() - t0 < 30
    grandchild = int(pidfile.read_text())
    time.sleep(0.5)
    alive = Path(f"/proc/{grandchild}").exists() and "Z" not in Path(f"/proc/{grandchild}/stat").read_text().split()[2]
    assert not alive
