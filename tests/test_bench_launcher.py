"""bench.py's rank launcher: `python3 bench.py --gpus N` starts N ranks itself
(one torch.distributed.run child, before any GPU call in the parent) unless it
already is a rank (WORLD_SIZE set)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_launcher_decision():
    assert bench.launcher_command(["--gpus", "1"], 1, {}) is None
    assert bench.launcher_command(["--gpus", "8"], 8, {"WORLD_SIZE": "8"}) is None
    cmd = bench.launcher_command(["--gpus", "8", "--steps", "3"], 8, {"RNVP_BENCH_PORT": "29777"})
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29777"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"]
    assert os.path.samefile(cmd[-5], os.path.join(ROOT, "bench.py"))
    # a free port is picked when none is given
    cmd = bench.launcher_command(["--gpus", "2"], 2, {})
    assert int(cmd[cmd.index("--master-port") + 1]) > 0


def test_launcher_spawns_ranks_on_cpu():
    """the real launcher path, stopped in each rank before the GPU"""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1]
    assert all(d["world_size"] == 2 and d["master"] == "127.0.0.1" for d in lines)


def test_rank_refuses_mismatched_world():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--launch-check"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


@pytest.mark.gpu
def test_two_rank_line_is_complete():
    """`bench.py --gpus 2 --full` (ranks sharing the GPU over gloo, a small
    custom model): rank 0's single JSON line carries the whole-job value, the
    roofline, the data-parallel diagnostics AND the CPU baseline -- what a
    full multi-GPU run records."""
    env = dict(os.environ, RNVP_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
                        "--size", "32", "--res-blocks", "1", "--base-dim", "8", "--batch", "4", "--full",
                        "--no-secondary", "--cpu-steps", "1", "--cpu-batch", "2"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["global_batch"] == 8
    assert d["roofline"]["bound"] in ("hbm", "mfma") and d["roofline"]["peak"] > 0
    assert d["dp"]["world_size_rccl"] == 2 and len(d["dp"]["rank_ms_per_step"]) == 2
    cb = d["cpu_baseline"]
    assert cb and cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port"


def test_full_option_gates_the_instrumented_step(monkeypatch, capsys):
    """--full is off by default, and --pmc-markers (markers around the
    instrumented eager step, which only --full runs) is refused without it"""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--pmc-markers", "m.json", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.pmc_markers == "m.json" and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--pmc-markers", "m.json"])
    with pytest.raises(SystemExit):
        bench.parse()
    assert "--full" in capsys.readouterr().err


def _plain_dump_run(out, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--size", "32", "--res-blocks", "1", "--base-dim", "8", "--batch", "4",
                        "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    import numpy as np
    return lines[0], {p.name[:-4]: np.load(str(p), allow_pickle=False) for p in sorted(out.iterdir())}


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """`bench.py --gpus 1 --steps 1 --warmup 1 --dump-outputs DIR` (a small
    custom model): the line holds the headline figure and ms_per_step of the
    timed step and none of the --full measurements; DIR holds the last
    step's arrays as finite float32 / float64 .npy files, 64 MB at the most."""
    import numpy as np
    d, arrays = _plain_dump_run(tmp_path / "dump", 1)
    assert d["steps"] == 1 and d["warmup"] == 1 and d["unit"] == "images/sec" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 / 4 - 1) < 1e-2
    assert d["roofline"] is None and d["kernel_families"] is None and d["cpu_baseline"] is None
    assert "secondary" not in d and "dp" not in d
    assert sorted(arrays) == ["arena_index", "bn_buffers", "exp_avg", "exp_avg_sq", "grad", "log_prob",
                              "mean_log_likelihood", "param", "x_logit"]
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), name
    assert arrays["log_prob"].shape == (4,) and arrays["x_logit"].shape == (4, 3, 32, 32)
    # the 3.06 M-element arenas are written at bench.DUMP_ARENA_SAMPLE fixed, sorted indices
    idx = arrays["arena_index"]
    assert idx.shape == (bench.DUMP_ARENA_SAMPLE,) and (np.diff(idx) >= 0).all() and 0 <= idx[0] and idx[-1] < 3.1e6
    assert all(arrays[k].shape == idx.shape for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
    # an Adam update happened: moments are non-zero, and the bits/dim of the
    # line (one timed step) is the one its mean_log_likelihood gives (train.py:203-204)
    assert np.abs(arrays["exp_avg"]).max() > 0 and arrays["exp_avg_sq"].min() >= 0
    D = 3 * 32 * 32
    bpd = (-float(arrays["mean_log_likelihood"][0]) + np.log(256.0) * D) / (D * np.log(2.0))
    assert abs(bpd - d["bits_per_dim"]) < 1e-3


@pytest.mark.gpu
def test_dumped_outputs_repeat_from_run_to_run(tmp_path):
    """Two runs with the same arguments dump the same last-step outputs.  The
    last timed step starts from the run's initial state (timed_with_rewind),
    so only the summation order of one step's floating-point atomics (fp32
    eps 6e-8, fp64 for the batch statistics) separates the runs: inputs and
    sample indices bitwise equal, every output within 1e-5 relative L2 -- two
    orders above that rounding, three below what a state carried over the
    earlier, chaotically amplified steps gives (1e-2 and more)."""
    import numpy as np
    _, a = _plain_dump_run(tmp_path / "a", 3)
    _, b = _plain_dump_run(tmp_path / "b", 3)
    assert sorted(a) == sorted(b)
    for k in ("x_logit", "arena_index"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("log_prob", "mean_log_likelihood", "param", "grad", "exp_avg", "exp_avg_sq", "bn_buffers"):
        x, y = a[k].astype(np.float64), b[k].astype(np.float64)
        rel = float(np.linalg.norm(x - y) / np.linalg.norm(x))
        print("%s: relative L2 between two runs %.3g" % (k, rel))
        assert rel < 1e-5, (k, rel)
