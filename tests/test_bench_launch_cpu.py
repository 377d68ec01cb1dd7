"""bench.py --gpus N: the launcher logic that must run before anything touches the GPU (VERDICT r1 #1,
ADVICE r1): a plain `python bench.py --gpus N` starts N ranks as a child torchrun; a WORLD_SIZE that
disagrees with --gpus is refused instead of silently benchmarking a different rank count."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2
    assert "WORLD_SIZE=3" in p.stderr and p.stdout.strip() == ""


def test_self_launch_builds_a_child_torchrun(monkeypatch):
    bench = _load_bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("CORSAIR_DIST_BACKEND", raising=False)
    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--workload", "table"])
    with pytest.raises(SystemExit) as e:
        bench.maybe_self_launch(types.SimpleNamespace(gpus=4))
    assert e.value.code == 7                      # the child's return code is ours
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--workload", "table"]
    # no GPU in the build container: fewer devices than ranks -> the ranks share devices over gloo
    assert seen["env"]["CORSAIR_DIST_BACKEND"] == "gloo"


def test_single_gpu_and_torchrun_ranks_do_not_relaunch(monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr(bench.subprocess, "call", lambda *a, **k: pytest.fail("must not launch"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.maybe_self_launch(types.SimpleNamespace(gpus=1))
    monkeypatch.setenv("WORLD_SIZE", "8")
    bench.maybe_self_launch(types.SimpleNamespace(gpus=8))


def test_table_label_histogram():
    bench = _load_bench()
    lab = bench.sym_labels("table", 830)
    vals, cnt = np.unique(lab, return_counts=True)
    assert dict(zip(vals.tolist(), cnt.tolist())) == {1: 233, 2: 422, 3: 7, 4: 128, 12: 40}
    chair = bench.sym_labels("chair", 652)
    assert (chair == 1).sum() == 650 and (chair == 4).sum() == 2
    assert len(bench.sym_labels("table", 64)) == 64


def test_batches_in_flight_pass_is_skipped_when_a_step_holds_a_collective():
    """The crash fixed in 86a7de4 (`--workload stress --gpus 2`): the extra three-batches-in-flight pass drives the steps
    from three host threads; with an all-gather inside the step the ranks' collectives mis-pair.  The decision is one
    function: never with a collective in the step on several ranks, never for strong-scaling steps."""
    bench = _load_bench()
    plain = types.SimpleNamespace()
    coll = types.SimpleNamespace(collective_in_step=True)
    strong = types.SimpleNamespace(collective_in_step=True, scaling="strong")
    assert bench.overlap_probe_allowed(1, 8, False, 1, plain)
    assert bench.overlap_probe_allowed(1, 8, False, 8, plain)          # chair / table: no collective in the step
    assert bench.overlap_probe_allowed(1, 8, False, 1, coll)           # one rank: nothing to mis-pair
    assert not bench.overlap_probe_allowed(1, 8, False, 2, coll)       # stress on 2 ranks
    assert not bench.overlap_probe_allowed(1, 8, False, 1, strong) and not bench.overlap_probe_allowed(1, 8, False, 4, strong)
    assert not bench.overlap_probe_allowed(3, 8, False, 1, plain) and not bench.overlap_probe_allowed(1, 1, False, 1, plain)
    assert not bench.overlap_probe_allowed(1, 8, True, 1, plain)
    assert bench.StressWorkload.collective_in_step and bench.StrongEvalWorkload.collective_in_step
    assert not getattr(bench.RegistrationWorkload, "collective_in_step", False)


def test_gpus8_launcher_end_to_end_on_cpu_ranks():
    """BASELINE.json configs[3] is `--gpus 8`; the first hardware run of it is the driver's.  Everything around the
    kernels runs here with EIGHT CPU ranks (`--workload dry`: no kernels, no GPU): the parent starts a child torchrun on a
    free port of 127.0.0.1, the ranks form the gloo control plane, the sharding collectives of the setup run (11 items on 8
    ranks: voxel counts all-gathered, balanced shards, the embedded-catalog all-gather), the timed region and the
    three-batches-in-flight pass are bracketed by barriers, the time is the max over ranks, and rank 0 alone prints
    exactly ONE JSON line on stdout -- gloo's connection notices and the other seven ranks print nothing there."""
    import json

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--workload", "dry", "--steps", "4",
                        "--warmup", "1", "--full"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["steps"] == 4 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["dist"]["backend"] == "gloo" and len(out["dist"]["rank_elapsed_s"]) == 8
    assert out["config"]["parallelism"] == "dp8" and out["config"]["catalog"] == 11
    assert out["batches_in_flight"]["identical_results"] is True and out["config"]["value_pass"] == "3 batches in flight"
    assert "DRY RUN" in out["metric"] and "not a measurement" in out["config"]["workload"]
    # the launcher chose gloo because the ranks share devices (none without a GPU, the one device of a one-GPU box)
    n_dev = _load_bench().visible_device_count()
    assert n_dev < 8 and "8 ranks on %d visible device(s): ranks share devices, backend gloo" % n_dev in p.stderr


def test_plain_run_times_only_the_headline_pass_and_dumps_its_outputs(tmp_path):
    """Without --full ONE pass runs (the batches-in-flight one, as its log shows: one timed region, no comparison with a
    sequential pass, no probe), the line carries the headline alone (no sequential pass, legs or baselines), and
    --dump-outputs writes the last timed step's arrays as float32 / float64 .npy."""
    import re

    import json

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "dry", "--steps", "5",
                        "--warmup", "2", "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 5 and out["warmup"] == 2 and out["value_pass"] == "3 batches in flight"
    log = p.stderr.splitlines()
    assert len([l for l in log if re.match(r"\[bench\] timed region: 5 steps in [0-9.]+s, 3 batches in flight$", l)]) == 1, log
    assert len([l for l in log if "timed region" in l]) == 1, log
    assert not [l for l in log if "identical results" in l or "stand-alone" in l], log
    for k in ("sequential", "batches_in_flight", "roofline", "kernel_ms", "workloads", "cpu_baseline"):
        assert k not in out, k
    assert out["outputs_dumped"] == ["step_value"]
    v = np.load(tmp_path / "out" / "step_value.npy")
    assert v.dtype == np.float64 and float(v) == float(np.sin(2 + 5 - 1))     # step W + K - 1 of rank 0


def test_plain_warmup_covers_every_worker_and_one_embed_group():
    """The untimed steps in front of a plain run's batches-in-flight pass: W, but at least one per worker and one whole
    embed group (never more than W + K)."""
    bench = _load_bench()
    assert bench.in_flight_warmup_steps(2, 8, 3, 4) == 4       # the defaults: one forward of 4 batches, every worker a step
    assert bench.in_flight_warmup_steps(2, 8, 3, 1) == 3
    assert bench.in_flight_warmup_steps(6, 8, 3, 4) == 6
    assert bench.in_flight_warmup_steps(0, 2, 3, 4) == 2


def test_headline_pass_is_fixed_a_priori_not_by_speed():
    """`value` is the three-batches-in-flight pass whenever that pass ran with identical results -- whichever
    pass came out faster -- and the sequential pass otherwise; legs follow the same rule."""
    import inspect

    bench = _load_bench()
    src = inspect.getsource(bench.main) + inspect.getsource(bench.extra_workload_leg)
    assert "overlap[0] < elapsed" not in src and "piped_elapsed < elapsed" not in src
    leg = {"value": 10.0, "ms_per_step": 1.0, "steps": 8, "value_pass": "three batches in flight",
           "sequential": {"value": 12.0}, "batches_in_flight": {"identical_results": True},
           "roofline": {"kernel": "k", "frac": 0.25, "peak": 1.0, "unit": "TFLOP/s"}, "config": {"workload": "configs[2]: x"}}
    # depth of the batches-in-flight pass: the fullest rounds in 3..6, the larger depth on ties
    assert [bench.auto_in_flight(k) for k in (20, 8, 10, 12, 7, 2, 1)] == [5, 4, 5, 6, 4, 3, 3]
    s = bench.leg_summary(leg)
    assert s["value"] == 10.0 and s["sequential_value"] == 12.0 and s["workload"] == "configs[2]" and s["roofline_frac"] == 0.25
