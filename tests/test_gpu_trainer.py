"""The epoch trainer on a small synthetic split (16 objects x 3 000 points: four shapes, four samples of
each; batches of 4: four steps per epoch; validation on 16 objects of four other shapes): a run is reproducible to the bit, a resumed run equals one that never stopped, training improves the validation
figures, and the command line trains, resumes and writes checkpoints the inference pipeline loads."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from corsair_amd import synth, train as T, training as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

N_OBJ, N_POINTS = 16, 3000


def _split(first, n=N_OBJ):
    """n objects in families of four: disjoint 3 000-point samples of the synthetic shapes first, first + 1, ...
    (synth.make_cloud, as tools/triplet_batch.py uses it).  Distance matrix: 0.1 inside a family, 0.3 - 0.4 between
    families, so filter_data keeps every object, positives are other samples of the anchor's shape (or the anchor
    itself) and negatives are other shapes."""
    clouds, fam = [], []
    for s in range(n // 4):
        pc = synth.make_cloud(first + s, 15000)
        clouds += [pc[k * N_POINTS:(k + 1) * N_POINTS] for k in range(4)]
        fam += [s] * 4
    fam = np.array(fam)
    a = np.random.default_rng(5).uniform(0.3, 0.4, (n, n))
    d = (a + a.T) / 2
    d[fam[:, None] == fam[None, :]] = 0.1
    np.fill_diagonal(d, 0.0)
    return clouds, d


def _cfg(**kw):
    base = dict(batch_size=4, sample=256, lr=0.05, lr_step=1, lr_gamma=0.9, pos_ratio=0.3, neg_ratio=0.5, seed=31)
    base.update(kw)
    return T.TrainConfig(**base)


def _trainer(gpu, cfg, val=False):
    clouds, d = _split(0)
    src = TR.TripletSource(clouds, d, cfg.voxel_size, cfg.pos_ratio, cfg.neg_ratio, device=gpu)
    vsrc = None
    if val:
        vc, vd = _split(N_OBJ // 4, 16)           # held-out shapes
        vsrc = TR.TripletSource(vc, vd, cfg.voxel_size, cfg.pos_ratio, cfg.neg_ratio, device=gpu)
    model, head = T.build_model(cfg, gpu)
    return T.Trainer(model, head, src, cfg, vsrc)


def _state(tr):
    """Everything a run leaves behind: weights and BatchNorm statistics, momentum buffers, scheduler."""
    out = {"m." + k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    out.update({"h." + k: v.detach().clone() for k, v in tr.head.state_dict().items()})
    for i, p in enumerate(tr.opt.param_groups[0]["params"]):
        buf = tr.opt.state.get(p, {}).get("momentum_buffer")
        if buf is not None:
            out["mom.%d" % i] = buf.detach().clone()
    return out, tr.sched.state_dict(), tr.opt.param_groups[0]["lr"]


def _same(a, b):
    return a[1] == b[1] and a[2] == b[2] and a[0].keys() == b[0].keys() and all(torch.equal(a[0][k], b[0][k]) for k in a[0])


def _figures(recs):
    return [{k: v for k, v in r.items() if k not in T.TIMING_FIELDS} for r in recs]


@pytest.fixture(scope="module")
def two_epochs(gpu, tmp_path_factory):
    tr = _trainer(gpu, _cfg(), val=True)
    recs = tr.fit(0, 2, str(tmp_path_factory.mktemp("run_a")))
    return _state(tr), recs


def test_run_is_reproducible(gpu, two_epochs, tmp_path):
    state_a, recs_a = two_epochs
    tr = _trainer(gpu, _cfg(), val=True)
    recs_b = tr.fit(0, 2, str(tmp_path / "b"))
    assert _same(state_a, _state(tr))
    assert _figures(recs_a) == _figures(recs_b)
    assert all(np.isfinite(r["loss"]) and r["steps"] == 4 for r in recs_a)
    assert any(k.startswith("mom.") for k in state_a[0]) and any("running_mean" in k for k in state_a[0])
    other = _trainer(gpu, _cfg(seed=32), val=True)
    other.fit(0, 1, str(tmp_path / "c"))
    assert not torch.equal(_state(other)[0]["m.conv1.kernel"], state_a[0]["m.conv1.kernel"])


def test_resume_equals_uninterrupted(gpu, two_epochs, tmp_path):
    state_a, recs_a = two_epochs
    out = str(tmp_path / "r")
    first = _trainer(gpu, _cfg(), val=True)
    recs0 = first.fit(0, 1, out)
    del first
    tr = _trainer(gpu, _cfg(), val=True)               # everything anew
    start = tr.resume(os.path.join(out, "last.pth"))
    assert start == 1
    recs1 = tr.fit(start, 1, out)
    assert _same(state_a, _state(tr))                  # weights, BatchNorm statistics, momentum, scheduler
    assert _figures(recs_a) == _figures(recs0 + recs1)
    assert sorted(os.listdir(out)) == ["epoch_000.pth", "epoch_001.pth", "last.pth", "log.jsonl"]
    lines = [json.loads(ln) for ln in open(os.path.join(out, "log.jsonl"))]
    assert [ln["epoch"] for ln in lines] == [0, 1]


def test_it_learns(gpu, tmp_path):
    """Strict comparisons against the run's own starting point.  Measured with these settings (10 epochs, lr 0.05 x 0.9
    per epoch): validation loss 1.799 -> 1.367, mean PiN + NiN distance - mean PiP distance -0.006 -> 0.159, triplet
    accuracy 0.625 -> 0.875 (0.75 or more from the fifth epoch on); lr 0.1 x 0.8 and 0.02 x 0.9 improve all three as
    well."""
    tr = _trainer(gpu, _cfg(), val=True)
    before = tr.validate()
    tr.fit(0, 10, str(tmp_path / "l"))
    after = tr.validate()
    print("validation before:", before, "after:", after)
    assert after["val_loss"] < before["val_loss"]
    assert (after["val_neg_dist"] - after["val_pos_dist"]) > (before["val_neg_dist"] - before["val_pos_dist"])
    assert after["val_triplet_acc"] >= before["val_triplet_acc"]
    assert tr.validate() == after                       # fixed poses: validating changes nothing


def test_cli_trains_resumes_and_loads_into_pipeline(gpu, tmp_path):
    import torch.nn.functional as F

    from corsair_amd import backend as B, harness
    from corsair_amd.utils import ckpts

    # four shapes x four disjoint samples of each: the computed Chamfer matrix has three neighbours per object
    cdir = tmp_path / "clouds"
    cdir.mkdir()
    for s in range(4):
        pc = synth.make_cloud(s, 15000)
        for k in range(4):
            np.save(cdir / ("obj_%d_%d.npy" % (s, k)), pc[k * N_POINTS:(k + 1) * N_POINTS])
    out = str(tmp_path / "out")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "corsair_amd.train", "--clouds-dir", str(cdir), "--out", out, "--epochs", "1",
            "--batch-size", "4", "--sample", "256", "--lr", "0.01", "--pos-ratio", "0.3", "--n-points", str(N_POINTS)]
    lines = []
    for extra in ([], ["--resume", os.path.join(out, "last.pth")]):
        r = subprocess.run(base + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(recs) == 1                           # one JSON line per epoch
        lines += recs
    assert [r["epoch"] for r in lines] == [0, 1] and all(np.isfinite(r["loss"]) for r in lines)
    d = np.load(os.path.join(out, "dist_mat.npy"))
    assert d.shape == (16, 16) and np.allclose(d, d.T)
    assert os.path.exists(os.path.join(out, "epoch_001.pth"))

    sd, emb = ckpts.load_state_dicts(os.path.join(out, "last.pth"))
    pipe = harness.Pipeline(sd, emb, device=gpu)
    clouds = [synth.make_cloud(c, 15000)[:4000] for c in (0, 4)]
    xyz = torch.from_numpy(np.concatenate(clouds, 0).astype(np.float32)).to(gpu)
    offsets = [0, len(clouds[0]), len(clouds[0]) + len(clouds[1])]
    got = pipe.embed_batch(xyz, offsets)
    model, head = T.build_model(T.TrainConfig(), gpu, (sd, emb))
    ME = T._shim()
    model.eval()
    head.eval()
    with torch.no_grad():
        _, grid, _ = B.voxelize(xyz, offsets, pipe.cfg.voxel_size)
        o, feat = model(ME.SparseTensor(torch.ones((grid.shape[0], 1), device=gpu), grid))
        g = F.normalize(head(feat), dim=1)
    assert torch.equal(got.F, o.F)
    assert torch.allclose(got.desc, g, atol=2e-6)
