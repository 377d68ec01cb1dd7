"""The Python surfaces of the ICP with an isotropic scale on the GPU: backend.icp_batch(with_scaling=...),
registration.sym_pose_batch(icp_with_scaling=...), the harness' per-query arrays and aggregate, and shapenet_eval's
max_log_scale / scale outputs."""
import numpy as np
import pytest
import torch

from tests import icp_ref
from tests import icp_scale_ref as ref
from tests import test_gpu_icp as pt
from tests import test_gpu_icp_scale as gs
from tests.test_gpu_icp_plane_surfaces import _Profile, _workload

pytestmark = pytest.mark.gpu
_same = pt._same


@pytest.mark.parametrize("plane", (False, True))
def test_backend_icp_batch_with_scaling(gpu, plane):
    from corsair_amd import backend as B

    src, tgt, nrm, T0 = gs._problem(3)              # 257 sources (too small by 1.08) against 511 targets
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu)
    args = (to(src), [0, len(src)], to(tgt), [0, len(tgt)], [0], [0], to(T0).reshape(1, 4, 4), gs.MAX_DIST, 10)
    kw = dict(tgt_normals=to(nrm) if plane else None)
    want = ref.icp(src, tgt, nrm if plane else None, T0, gs.MAX_DIST, 10)
    with _Profile() as prof:
        r = B.icp_batch(*args, with_scaling=True, return_corr=True, **kw)
    assert prof.n["icp"] == 1
    assert _same(r.T.cpu().numpy().reshape(16), want["T"]) and _same(r.T32.cpu().numpy().reshape(16), want["T32"])
    assert _same(r.scale.cpu().numpy()[0], np.float64(want["scale"])) and int(r.iters[0]) == want["iters"] > 1
    assert np.array_equal(r.corr.cpu().numpy(), want["corr"]) and r.corr_off == [0, len(src)]
    assert r.scale.dtype == torch.float64 and r.wfitness is None and want["scale"] > 1.01
    q = B.icp_batch(*args, with_scaling=True, **kw)                 # without return_corr: the same numbers, no list
    assert q.corr is None and q.corr_off is None
    for name in ("T", "T32", "fitness", "rmse", "iters", "ncorr", "scale"):
        assert _same(getattr(q, name).cpu().numpy(), getattr(r, name).cpu().numpy()), name
    # the interval is passed through; positional users of IcpResult see what they saw
    narrow = B.icp_batch(*args, with_scaling=True, scale_bounds=(0.99, 1.01), **kw)
    assert 0.99 <= float(narrow.scale[0]) <= 1.01 and int(narrow.iters[0]) < want["iters"]
    off = B.icp_batch(*args, **kw)
    assert off.scale is None and len(off) == 10 and off[8] is None and B.IcpResult._fields[:9] == (
        "T", "T32", "fitness", "rmse", "iters", "ncorr", "corr", "corr_off", "wfitness")


def _small_queries(dev, shrink=1.05):
    """tests/test_gpu_icp.py's pair batch with every query 5 % smaller than its CAD (about the origin of its own frame)."""
    F0, x0, off0, F1, x1, off1, Ts = pt._pair_batch(dev)
    return F0, (x0.double() / shrink).float(), off0, F1, x1, off1, Ts


def test_sym_pose_batch_with_scaling(gpu):
    from corsair_amd import backend as B, registration as R

    F0, x0, off0, F1, x1, off1, _ = _small_queries(gpu)
    kw = dict(k_nn=5, max_corr=0.2, seed=0, max_iter=2000, force_gate=True)
    icp = dict(icp_max_iter=30, icp_max_dist=0.06)
    with _Profile() as prof:
        rigid = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], **icp, **kw)
    assert prof.n["icp"] == 1 and rigid.icp_scale is None
    # without scaling: the fields and bits of a call that never heard of the option -- cs_icp_batch's restatement
    explicit = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_with_scaling=False, icp_scale_bounds=(0.9, 1.1),
                                **icp, **kw)
    assert vars(explicit).keys() == vars(rigid).keys()
    for name, v in vars(rigid).items():
        w = getattr(explicit, name)
        if torch.is_tensor(v):
            assert _same(v.cpu().numpy(), w.cpu().numpy()), name
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, w), name
        else:
            assert v == w, name
    want = icp_ref.icp_batch(x0.cpu().numpy(), off0, x1.cpu().numpy(), off1, [0, 1], [0, 1], rigid.T_best.cpu().numpy(),
                             0.06, 30)
    for p in range(2):
        assert _same(rigid.T_icp[p].cpu().numpy().reshape(16), want[p]["T32"]) and int(rigid.icp_iters[p]) == want[p]["iters"]
    for est in ("point", "plane"):
        with _Profile() as prof:
            on = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_with_scaling=True, icp_estimation=est,
                                  icp_normal_k=8, **icp, **kw)
        assert prof.n["icp"] == 1
        for name in ("T_best", "cd_best", "T_ransac", "cd_ransac", "iters", "T_all", "cd_all", "inliers"):
            assert _same(getattr(on, name).cpu().numpy(), getattr(rigid, name).cpu().numpy()), name
        sc = on.icp_scale.cpu().numpy()
        cd_on, cd_off = on.cd_icp.cpu().numpy(), rigid.cd_icp.cpu().numpy()
        print(est, "icp_scale", sc, "cd_icp", cd_on, "rigid cd_icp", cd_off, "updates", on.icp_iters.cpu().numpy())
        assert sc.dtype == np.float64 and np.all(np.abs(sc - 1.05) <= 0.25 * 0.05)
        assert np.all(cd_on < cd_off)
        # T_icp is the similarity: its determinant carries the scale, and cd_icp is cs_chamfer_1dir under it
        det = np.linalg.det(on.T_icp.cpu().numpy().astype(np.float64)[:, :3, :3])
        assert np.all(np.abs(np.cbrt(det) - sc) < 1e-5)
        assert _same(cd_on, B.chamfer_1dir(x0, off0, x1, off1, [0, 1], [0, 1], on.T_icp).cpu().numpy())
    bounded = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_with_scaling=True, icp_scale_bounds=(0.98, 1.02),
                               **icp, **kw)
    assert np.all(np.abs(bounded.icp_scale.cpu().numpy() - 1.0) <= 0.02)
    with pytest.raises(ValueError, match="out of scope"):
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_with_scaling=True, icp_estimation="plane",
                         icp_kernel="huber", icp_kernel_scale=0.03, **icp, **kw)


def test_harness_per_query_key_sets_and_aggregate(gpu):
    from corsair_amd import cache as C, harness as H

    F0, x0, off0, F1, x1, off1, Ts = _small_queries(gpu)
    desc = torch.zeros((2, 0), dtype=torch.float32, device=gpu)
    qs, cat = H.EmbeddedSet(F0, x0, off0, desc), H.EmbeddedSet(F1, x1, off1, desc)
    args = (np.arange(2), cat, np.arange(2), np.asarray([1, 2]), np.stack(Ts), np.stack([np.eye(4)] * 2))
    rigid_cfg = H.Config(ransac_max_iter=2000, icp_max_iter=30)
    rigid = H.register_queries(pt._Pipe(gpu, rigid_cfg), qs, *args)
    assert set(rigid) == set(C.NAMES) | set(C.ICP_NAMES)            # an unscaled run: the key set it always had
    cfg = H.Config(ransac_max_iter=2000, icp_max_iter=30, icp_with_scaling=True)
    cfg.check_icp()
    got = H.register_queries(pt._Pipe(gpu, cfg), qs, *args)
    assert set(got) == set(C.NAMES) | set(C.ICP_NAMES) | set(C.ICP_SCALE_NAMES)
    for k in C.NAMES:
        assert _same(got[k], rigid[k]), k
    for k in C.ICP_NAMES:
        assert got[k].dtype == C.ICP_DTYPES[k] and len(got[k]) == 2, k
    assert got["icp_scale"].dtype == np.float64 and got["icp_scale"].shape == (2,)
    # the rotation loss is taken on the rotation: finite, and not inflated by the 5 % in the 3x3 block
    assert np.all(np.isfinite(got["r_losses_icp"])) and np.all(got["r_losses_icp"] <= rigid["r_losses_icp"] + 1e-3)
    empty = H.register_queries(pt._Pipe(gpu, cfg), qs, np.arange(0), *args[1:])
    assert set(empty) == set(got) and empty["icp_scale"].dtype == np.float64 and len(empty["icp_scale"]) == 0
    ev = H.finish_eval({}, got, False)
    dev = np.abs(got["icp_scale"] - 1.0)
    assert ev.icp["scale_dev_mean"] == float(dev.mean()) and ev.icp["scale_dev_max"] == float(dev.max())
    assert "icp scale" in ev.report
    plain = H.finish_eval({}, rigid, False)
    assert "scale_dev_mean" not in plain.icp and "icp scale" not in plain.report
    with pytest.raises(ValueError, match="robust"):
        H.Config(icp_max_iter=5, icp_estimation="plane", icp_kernel="tukey", icp_with_scaling=True).check_icp()
    with pytest.raises(ValueError, match="icp_max_iter"):
        H.Config(icp_with_scaling=True).check_icp()


def _in_draw_range(s, m=0.1):
    return float(np.exp(-m)) <= s <= float(np.exp(m))


def test_shapenet_eval_scale_outputs(gpu, tmp_path):
    import csv

    from corsair_amd import harness, shapenet_eval as S, synth

    _, (sd, emb) = _workload()
    pipe = harness.Pipeline(sd, emb, device=gpu)
    clouds = [synth.make_cloud(50 + i, 4000) for i in range(2)]
    # small poses: the network of this test is untrained, its features survive a few degrees
    base = dict(n_poses_per_model=2, ransac_max_iter=2000, max_translation=0.2, max_roll_deg=10.0, max_pitch_deg=10.0,
                max_yaw_deg=10.0, icp_max_iter=30, icp_estimation="plane")
    never = S.evaluate(pipe, clouds, S.Config(**base), pairs_per_batch=2)
    zero = S.evaluate(pipe, clouds, S.Config(max_log_scale=0.0, **base), pairs_per_batch=2)
    assert len(never) == len(zero) == 4
    for a, b in zip(never, zero):                                   # max_log_scale = 0: the same keys and the same values
        assert set(a) == set(b) and "scale_gt" not in a
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    # ... and the default path draws nothing new: its poses are the pose draws of a fresh generator and nothing in between
    # (every other output of the default is pinned by the unchanged tests/test_gpu_cli.py, test_gpu_next_rows.py and
    # test_gpu_icp_plane_surfaces.py).  With a positive max_log_scale one more number is drawn after every pose.
    cfg0 = S.Config(**base)
    rng = np.random.default_rng(cfg0.random_seed)
    for r in never:
        assert np.array_equal(r["pose_gt"], S.generate_random_pose(cfg0, rng))
    rng = np.random.default_rng(cfg0.random_seed)
    drawn = []
    for _ in range(4):
        pose = S.generate_random_pose(cfg0, rng)
        drawn.append((pose, float(np.exp(rng.uniform(-0.1, 0.1)))))
    on = S.evaluate(pipe, clouds, S.Config(max_log_scale=0.1, icp_with_scaling=True, **base), pairs_per_batch=2)
    scale_keys = {"scale_gt", "scale_icp", "scale_err_icp"}
    for a, b in zip(never, on):
        assert set(b) - scale_keys == set(a) and scale_keys <= set(b)
    err = [r["scale_err_icp"] for r in on]
    print("scale_gt", [r["scale_gt"] for r in on], "scale_icp", [r["scale_icp"] for r in on], "scale error", err,
          "rre_icp", [r["rre_icp"] for r in on])
    assert all(_in_draw_range(r["scale_gt"]) for r in on)
    for r, (pose, s_gt) in zip(on, drawn):
        assert np.array_equal(r["pose_gt"], pose) and r["scale_gt"] == s_gt
    off_scaled = S.evaluate(pipe, clouds, S.Config(max_log_scale=0.1, **base), pairs_per_batch=2)
    assert all(set(r) == set(never[0]) for r in off_scaled)        # scaling off: no scale key, whatever the poses were
    assert all(r["scale_err_icp"] == abs(r["scale_icp"] / r["scale_gt"] - 1.0) for r in on)
    assert all(e <= 0.05 for e in err)
    t = S.threshold_table(on)
    assert {"scale<=0.05", "scale<=0.1", "scale<=0.2"} <= set(t["icp"]) and "scale<=0.05" not in t["sym"]
    assert "scale error" in S.summary(on) and "scale error" not in S.summary(never)
    S.write_results(on, ["a", "b"], str(tmp_path / "on.csv"), str(tmp_path / "on.npz"))
    rows = list(csv.reader(open(tmp_path / "on.csv")))
    assert tuple(rows[0]) == S.CSV_COLUMNS + S.ICP_CSV_COLUMNS + S.SCALE_CSV_COLUMNS and len(rows) == 5
    z = np.load(tmp_path / "on.npz")
    assert z["scale_icp"].shape == (4,) and set(scale_keys) <= set(z.files)
    S.write_results(never, ["a", "b"], str(tmp_path / "off.csv"), str(tmp_path / "off.npz"))
    assert tuple(next(csv.reader(open(tmp_path / "off.csv")))) == S.CSV_COLUMNS + S.ICP_CSV_COLUMNS
    assert not set(scale_keys) & set(np.load(tmp_path / "off.npz").files)
    with pytest.raises(ValueError, match="icp_max_iter"):
        S.evaluate(pipe, clouds, S.Config(icp_with_scaling=True), pairs_per_batch=2)
