"""bench.py --dump-outputs on every workload, at small sizes: the files are the arrays the last timed step returned, with
the names, shapes and dtypes a caller of that path receives (float32 kept, ids / counts / flags as float64), and a plain
run (the batches-in-flight pass alone) writes the same arrays as a --full run (sequential pass first, then the same
steps in flight)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir)]
                       + list(args), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    files = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    assert sorted(files) == line["outputs_dumped"]
    return line, files


def _check_registration(d, C):
    assert d["query_desc"].dtype == np.float32 and d["query_desc"].shape == (32, 256)
    assert np.allclose(np.linalg.norm(d["query_desc"], axis=1), 1.0, atol=1e-4)
    top = d["top1_cad"]
    assert top.dtype == np.float64 and top.shape == (32,) and np.all((top >= 0) & (top < C) & (top == np.round(top)))
    for k in ("T_best", "T_ransac"):
        assert d[k].dtype == np.float32 and d[k].shape == (32, 4, 4)
        assert np.array_equal(d[k][:, 3], np.tile(np.float32([0, 0, 0, 1]), (32, 1))), k
    for k in ("cd_best", "cd_ransac"):
        assert d[k].dtype == np.float64 and d[k].shape == (32,) and np.all(np.isfinite(d[k]) & (d[k] >= 0)), k
    assert np.all(d["cd_best"] <= d["cd_ransac"])            # the best hypothesis is the Chamfer minimum, vanilla included
    assert d["sym_success"].dtype == np.float64 and set(np.unique(d["sym_success"])) <= {0.0, 1.0}
    it = d["ransac_iters"]
    assert it.dtype == np.float64 and it.ndim == 1 and len(it) >= 32          # one count per RANSAC problem of the step
    assert np.all((it >= 0) & (it <= 100000) & (it == np.round(it)))


def test_dump_outputs_chair_plain_equals_full(gpu, tmp_path):
    line, plain = _bench(tmp_path / "plain", "--catalog", "24", "--steps", "3", "--warmup", "1")
    assert line["value_pass"] == "3 batches in flight" and "sequential" not in line
    _check_registration(plain, 24)
    line, full = _bench(tmp_path / "full", "--catalog", "24", "--steps", "3", "--warmup", "1", "--full",
                        "--no-extra-workloads", "--no-cpu-baseline")
    assert line["batches_in_flight"]["identical_results"] is True
    assert sorted(plain) == sorted(full)
    for k in plain:
        assert np.array_equal(plain[k], full[k]), k


def test_dump_outputs_table(gpu, tmp_path):
    _, d = _bench(tmp_path / "t", "--workload", "table", "--catalog", "24", "--steps", "2", "--warmup", "1")
    _check_registration(d, 24)


def test_dump_outputs_stress(gpu, tmp_path):
    _, d = _bench(tmp_path / "s", "--workload", "stress", "--catalog", "4096", "--steps", "2", "--warmup", "1")
    ids = d["topk_ids"]
    assert sorted(d) == ["desc_last_batch", "topk_ids"]
    assert ids.dtype == np.float64 and ids.shape == (10240, 10) and np.all((ids >= 0) & (ids < 4096))
    assert all(len(set(r)) == 10 for r in ids[:256])
    desc = d["desc_last_batch"]
    assert desc.dtype == np.float32 and desc.shape == (64, 256)
    assert np.allclose(np.linalg.norm(desc, axis=1), 1.0, atol=1e-4)


def test_dump_outputs_strong(gpu, tmp_path):
    from corsair_amd import cache

    _, d = _bench(tmp_path / "g", "--scaling", "strong", "--catalog", "24", "--queries", "40", "--steps", "2",
                  "--warmup", "1")
    assert sorted(d) == sorted(cache.NAMES)
    for k in ("Ts_est_ransac", "Ts_est_best"):
        assert d[k].dtype == np.float32 and d[k].shape == (40, 4, 4), k
    assert d["sym_ransac_success"].dtype == np.float64 and set(np.unique(d["sym_ransac_success"])) <= {0.0, 1.0}
    for k in cache.NAMES:
        assert len(d[k]) == 40 and np.all(np.isfinite(d[k])), k
