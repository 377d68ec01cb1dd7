"""The Python surfaces of the Generalized-ICP refinement on the GPU: backend.icp_batch(estimation="gicp"),
registration.sym_pose_batch(icp_estimation="gicp") with and without the caller's normals, the harness evaluation,
shapenet_eval's optional ICP outputs, and the lattice fixture of DESIGN 19 through the library."""
import numpy as np
import pytest
import torch

from tests import gicp_ref as ref
from tests import test_gpu_icp as pt
from tests.test_gpu_icp_plane_surfaces import _Profile, _workload

pytestmark = pytest.mark.gpu
_same = pt._same


def test_sym_pose_batch_gicp(gpu):
    from corsair_amd import backend as B, registration as R

    F0, x0, off0, F1, x1, off1, _ = pt._pair_batch(gpu)
    kw = dict(k_nn=5, max_corr=0.2, seed=0, max_iter=2000, force_gate=True)
    icp = dict(icp_max_iter=5, icp_max_dist=0.06)
    with _Profile() as prof:
        plain = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], **kw)
    assert prof.n == {"icp": 0, "normals": 0} and plain.T_icp is None and plain.icp_mrmse is None
    with _Profile() as prof:
        got = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_estimation="gicp", icp_normal_k=8, **icp, **kw)
    assert prof.n == {"icp": 1, "normals": 2}                            # the CAD voxels' and the query voxels' normals
    for name in ("T_best", "cd_best", "T_ransac", "cd_ransac", "T_all", "cd_all", "inliers", "iters"):   # every pre-ICP field
        assert _same(getattr(plain, name).cpu().numpy(), getattr(got, name).cpu().numpy()), name
    assert np.array_equal(plain.ok, got.ok) and np.array_equal(plain.best, got.best) and got.icp_wfitness is None
    n0, n1 = B.estimate_normals(x0, off0, 8), B.estimate_normals(x1, off1, 8)
    want = ref.icp_batch(x0.cpu().numpy(), n0.cpu().numpy(), off0, x1.cpu().numpy(), n1.cpu().numpy(), off1, [0, 1], [0, 1],
                         got.T_best.cpu().numpy(), 0.06, 5)
    for p in range(2):
        assert _same(got.T_icp[p].cpu().numpy().reshape(16), want[p]["T32"])
        assert _same(got.icp_fitness[p].cpu().numpy(), np.float64(want[p]["fitness"]))
        assert _same(got.icp_rmse[p].cpu().numpy(), np.float64(want[p]["rmse"]))
        assert _same(got.icp_mrmse[p].cpu().numpy(), np.float64(want[p]["mrmse"]))
        assert int(got.icp_iters[p]) == want[p]["iters"]
    assert _same(got.cd_icp.cpu().numpy(), B.chamfer_1dir(x0, off0, x1, off1, [0, 1], [0, 1], got.T_icp).cpu().numpy())
    # normals the caller supplies are used as they are: no estimation launch, the same result
    with _Profile() as prof:
        given = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_estimation="gicp", normals0=n0, normals1=n1, **icp, **kw)
    assert prof.n == {"icp": 1, "normals": 0}
    for name in ("T_icp", "cd_icp", "icp_fitness", "icp_rmse", "icp_mrmse", "icp_iters"):
        assert _same(getattr(given, name).cpu().numpy(), getattr(got, name).cpu().numpy()), name
    with _Profile() as prof:
        half = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_estimation="gicp", icp_normal_k=8, normals1=n1, **icp, **kw)
    assert prof.n == {"icp": 1, "normals": 1} and _same(half.T_icp.cpu().numpy(), got.T_icp.cpu().numpy())
    # backend.icp_batch(estimation="gicp") equals the raw call's outputs above, and another epsilon is another result
    r = B.icp_batch(x0, off0, x1, off1, [0, 1], [0, 1], got.T_best, 0.06, 5, tgt_normals=n1, estimation="gicp", src_normals=n0)
    assert _same(r.T32.cpu().numpy(), got.T_icp.cpu().numpy()) and _same(r.mrmse.cpu().numpy(), got.icp_mrmse.cpu().numpy())
    other = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_estimation="gicp", normals0=n0, normals1=n1,
                             gicp_epsilon=0.5, **icp, **kw)
    assert not _same(other.T_icp.cpu().numpy(), got.T_icp.cpu().numpy())
    plane = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_estimation="plane", normals1=n1, **icp, **kw)
    assert plane.icp_mrmse is None and not _same(plane.T_icp.cpu().numpy(), got.T_icp.cpu().numpy())
    with pytest.raises(ValueError, match="normals0"):
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_estimation="plane", normals0=n0, **icp, **kw)


def test_harness_evaluation_with_gicp_refinement(gpu):
    from corsair_amd import cache as C, harness

    (catalog, queries, best_match, table, base_T, lib_T, syms), (sd, emb) = _workload()
    args = (best_match, table, base_T, lib_T, syms, "chair", True)
    kw = dict(force_gate=True, batch_size=4)                       # 10 queries: three registration batches
    plain_pipe = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(ransac_max_iter=2000))
    cat, qs = plain_pipe.embed_clouds(catalog), plain_pipe.embed_clouds(queries)
    plain = harness.run_eval(plain_pipe, cat, qs, *args, **kw)
    cfg = harness.Config(ransac_max_iter=2000, icp_max_iter=5, icp_estimation="gicp", icp_normal_k=8)
    pipe = harness.Pipeline(sd, emb, device=gpu, config=cfg)
    with _Profile() as prof:
        res = harness.run_eval(pipe, cat, qs, *args, **kw)
    # the catalog's normals once per evaluation, the queries' once per batch; one ICP call per batch, profile family "icp"
    assert prof.n == {"icp": 3, "normals": 4}
    assert res.icp is not None and "icp refinement" in res.report
    assert set(res.per_query) == set(C.NAMES) | set(C.ICP_NAMES)
    for k in C.NAMES:                                              # the nine arrays do not see the refinement
        assert _same(np.asarray(res.per_query[k]), np.asarray(plain.per_query[k])), k
    plane_cfg = harness.Config(ransac_max_iter=2000, icp_max_iter=5, icp_estimation="plane", icp_normal_k=8)
    plane = harness.run_eval(harness.Pipeline(sd, emb, device=gpu, config=plane_cfg), cat, qs, *args, **kw)
    assert any(not _same(np.asarray(res.per_query[k]), np.asarray(plane.per_query[k])) for k in C.ICP_NAMES)


def test_shapenet_eval_gicp_outputs(gpu):
    from corsair_amd import harness, shapenet_eval as S, synth

    _, (sd, emb) = _workload()
    pipe = harness.Pipeline(sd, emb, device=gpu)
    clouds = [synth.make_cloud(50 + i, 4000) for i in range(3)]
    base = dict(n_poses_per_model=1, ransac_max_iter=2000, max_translation=0.5)
    off = S.evaluate(pipe, clouds, S.Config(**base), pairs_per_batch=2)
    icp_keys = {"T_est_icp", "rte_icp", "rre_icp", "chamfer_dist_icp", "icp_iters"}
    with _Profile() as prof:
        on = S.evaluate(pipe, clouds, S.Config(icp_max_iter=10, icp_estimation="gicp", gicp_epsilon=0.01, **base), pairs_per_batch=2)
    assert prof.n == {"icp": 2, "normals": 4}                      # two batches, both clouds' normals in each
    for a, b in zip(off, on):
        assert icp_keys <= set(b) and set(b) - icp_keys == set(a)
        for k in a:                                                # every output of today is what it was
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert b["T_est_icp"].shape == (4, 4) and 0 <= b["icp_iters"] <= 10 and np.isfinite(b["rre_icp"])
    assert set(S.threshold_table(on)) == {"ransac", "sym", "icp"} and S.summary(on).count("icp:") == 3


def test_lattice_fixture_returns_the_restatements_bits(gpu):
    """DESIGN 19's fixture through the library: the three estimations return the bits of their restatements and therefore
    their ordering -- GICP nearer the true pose than point and plane, in fewer updates."""
    from corsair_amd import backend as B

    f, want = ref.lattice_fixture(), ref.lattice_runs()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu)
    src, tgt, sn, tn = to(f["src"]), to(f["tgt"]), to(f["snrm"]), to(f["tnrm"])
    eye = torch.eye(4, device=gpu)[None]
    args = (src, [0, len(f["src"])], tgt, [0, len(f["tgt"])], [0], [0], eye, 0.06, 30)
    runs = {"point": B.icp_batch(*args), "plane": B.icp_batch(*args, tgt_normals=tn),
            "gicp": B.icp_batch(*args, tgt_normals=tn, estimation="gicp", src_normals=sn, gicp_epsilon=1e-3)}
    err = {}
    for k, r in runs.items():
        assert _same(r.T.cpu().numpy().reshape(16), want[k]["T"]), k
        assert _same(r.T32.cpu().numpy().reshape(16), want[k]["T32"]), k
        assert int(r.iters[0]) == want[k]["iters"] and int(r.ncorr[0]) == want[k]["ncorr"], k
        assert _same(r.fitness.cpu().numpy()[0], np.float64(want[k]["fitness"])), k
        assert _same(r.rmse.cpu().numpy()[0], np.float64(want[k]["rmse"])), k
        err[k] = ref.pose_errors(r.T.cpu().numpy(), f["G"])
    assert _same(runs["gicp"].mrmse.cpu().numpy()[0], np.float64(want["gicp"]["mrmse"]))
    for other in ("point", "plane"):
        assert err["gicp"][0] < err[other][0] and err["gicp"][1] < err[other][1], (other, err)
    assert 0 < int(runs["gicp"].iters[0]) < min(int(runs["point"].iters[0]), int(runs["plane"].iters[0]))
