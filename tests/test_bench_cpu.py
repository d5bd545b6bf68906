"""bench.py launcher logic (CPU, nothing launched): `python bench.py --gpus N` started as a
plain process re-runs itself as N torchrun ranks in a child process (never exec), one rank
per GPU, with the driver's flags passed through (reference launch: main.py:133-154)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_launch_command_shape():
    import bench
    a = type("A", (), {"gpus": 8})()
    cmd = bench.launch_command(a, ["--gpus", "8", "--steps", "5", "--warmup", "2"], 29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert "--master-addr=127.0.0.1" in cmd and "--master-port=29511" in cmd
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "5", "--warmup", "2"]


def test_gpus_n_spawns_child_torchrun(monkeypatch):
    import bench
    calls = []

    def fake_call(cmd, env=None):
        calls.append((cmd, env))
        return 3

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 3  # the child's exit status is the bench's
    (cmd, env), = calls
    assert "--nproc-per-node=2" in cmd and cmd[-4:] == ["--gpus", "2", "--steps", "3"]
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch, capsys):
    """--full is off by default; the options that only mean something with the profiling
    steps are refused without it instead of being silently ignored; --steps >= 1."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 4, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--ops-out", "ops.txt", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.ops_out == "ops.txt" and a.dump_outputs == "d"
    for argv in (["--ops-out", "ops.txt"], ["--steps", "0"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        with pytest.raises(SystemExit) as e:
            bench.parse()
        assert e.value.code == 2
    capsys.readouterr()


def test_dump_outputs_writes_one_float32_array_per_loss(tmp_path):
    import numpy as np
    import torch
    import bench
    ld = {"loss_all": torch.tensor(1.5, dtype=torch.float64), "coarse_l1_loss": torch.tensor([0.25]).bfloat16()}
    out = tmp_path / "sub" / "dump"
    bench.dump_outputs(str(out), ld)
    assert sorted(p.name for p in out.iterdir()) == ["coarse_l1_loss.npy", "loss_all.npy"]
    for k, v in (("loss_all", 1.5), ("coarse_l1_loss", 0.25)):
        x = np.load(out / f"{k}.npy")
        assert x.dtype == np.float32 and x.shape == (1,) and float(x[0]) == v


def test_report_line_plain_vs_full(capsys):
    """A plain run's line carries the throughput figures and none of the --full legs."""
    import json
    import bench
    a = type("A", (), dict(batch=8, steps=4, warmup=1, workload="c2", precision="bf16", height=256, width=512,
                           graph=0, full=False))()
    bench.report(a, 0.2, 0.2, 3.0, None, {}, None, 0, 1)
    d = json.loads(capsys.readouterr().out)
    assert d["ms_per_step"] == 50.0 and d["value"] == 160.0 and d["steps"] == 4 and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["dtype"] == "bf16" and d["metric"].startswith("train frames/s")
    assert not {"roofline", "step_breakdown_ms", "cpu_baseline", "warp", "clip_prep"} & set(d)


def test_bench_refuses_timing_switches():
    """A DVIE_*_DBG variable (timing-only kernel ablations, wrong results) makes bench.py exit
    non-zero before anything runs."""
    import bench
    with pytest.raises(SystemExit) as e:
        bench.refuse_timing_switches({"DVIE_HALO_DBG": "8"})
    assert e.value.code == 2
    bench.refuse_timing_switches({"DVIE_HALO_DBG": "", "DVIE_1X1_DBG": "0", "DVIE_PRECISION": "bf16"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"], capture_output=True,
                       text=True, env=dict(os.environ, DVIE_1X1_DBG="2"), timeout=120)
    assert r.returncode == 2 and "DVIE_1X1_DBG" in r.stderr
