"""The Python surfaces of the point-to-plane refinement on the GPU: backend.icp_batch(tgt_normals=...),
registration.sym_pose_batch(icp_estimation=...), the harness evaluation with its cache and its profile counters, and
shapenet_eval's optional ICP outputs."""
import functools

import numpy as np
import pytest
import torch

from tests import icp_plane_ref as ref
from tests import test_gpu_icp as pt

pytestmark = pytest.mark.gpu
_same = pt._same


def _launches(family):
    from corsair_amd import _lib

    return _lib.prof_get(family)[1]


class _Profile:
    """cs_prof_* around a block: launches per family afterwards."""
    def __enter__(self):
        from corsair_amd import _lib

        _lib.prof_enable(True)
        _lib.prof_reset()
        return self

    def __exit__(self, *exc):
        from corsair_amd import _lib

        torch.cuda.synchronize()
        self.n = {f: _launches(f) for f in ("icp", "normals")}
        _lib.prof_enable(False)


def test_sym_pose_batch_estimations(gpu):
    from corsair_amd import backend as B, registration as R

    F0, x0, off0, F1, x1, off1, _ = pt._pair_batch(gpu)
    kw = dict(k_nn=5, max_corr=0.2, seed=0, max_iter=2000, force_gate=True)
    fields = ("T_best", "cd_best", "T_ransac", "cd_ransac", "T_icp", "cd_icp", "icp_fitness", "icp_rmse", "icp_iters")
    with _Profile() as prof:
        off = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], **kw)
    assert prof.n == {"icp": 0, "normals": 0} and off.T_icp is None          # ICP off: nothing new is launched
    with _Profile() as prof:
        plain = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_max_iter=5, icp_max_dist=0.06, **kw)
    assert prof.n == {"icp": 1, "normals": 0}
    point = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_max_iter=5, icp_max_dist=0.06, icp_estimation="point",
                             icp_normal_k=8, **kw)
    for name in fields:                                                      # "point" = a call without the argument
        assert _same(getattr(plain, name).cpu().numpy(), getattr(point, name).cpu().numpy()), name
    with _Profile() as prof:
        plane = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_max_iter=5, icp_max_dist=0.06,
                                 icp_estimation="plane", icp_normal_k=8, **kw)
    assert prof.n == {"icp": 1, "normals": 1}
    for name in fields[:4]:
        assert _same(getattr(plain, name).cpu().numpy(), getattr(plane, name).cpu().numpy()), name
    nrm = B.estimate_normals(x1, off1, 8)
    want = ref.icp_batch(x0.cpu().numpy(), off0, x1.cpu().numpy(), nrm.cpu().numpy(), off1, [0, 1], [0, 1],
                         plane.T_best.cpu().numpy(), 0.06, 5)
    for p in range(2):
        assert _same(plane.T_icp[p].cpu().numpy().reshape(16), want[p]["T32"])
        assert _same(plane.icp_fitness[p].cpu().numpy(), np.float64(want[p]["fitness"]))
        assert _same(plane.icp_rmse[p].cpu().numpy(), np.float64(want[p]["rmse"]))
        assert int(plane.icp_iters[p]) == want[p]["iters"]
    assert not _same(plane.T_icp.cpu().numpy(), plain.T_icp.cpu().numpy())
    assert _same(plane.cd_icp.cpu().numpy(), B.chamfer_1dir(x0, off0, x1, off1, [0, 1], [0, 1], plane.T_icp).cpu().numpy())
    # normals the caller supplies are used as they are: no estimation launch, the same result
    with _Profile() as prof:
        given = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_max_iter=5, icp_max_dist=0.06,
                                 icp_estimation="plane", normals1=nrm, **kw)
    assert prof.n == {"icp": 1, "normals": 0} and _same(given.T_icp.cpu().numpy(), plane.T_icp.cpu().numpy())
    # backend.icp_batch(tgt_normals=...) directly
    r = B.icp_batch(x0, off0, x1, off1, [0, 1], [0, 1], plane.T_best, 0.06, 5, tgt_normals=nrm)
    assert _same(r.T32.cpu().numpy(), plane.T_icp.cpu().numpy())
    with pytest.raises(ValueError, match="icp_estimation"):
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_max_iter=5, icp_max_dist=0.06, icp_estimation="line", **kw)


@functools.lru_cache(maxsize=None)
def _workload():
    from corsair_amd import harness, synth

    data = harness.SyntheticScan2CAD(n_catalog=12, n_query=10, n_points=3000).build()
    catalog, queries, best_match, base_T, lib_T, syms = data.eval_inputs()
    return (catalog, queries, best_match, data.table(), base_T, lib_T, syms), synth.make_state_dicts(31)


def test_harness_evaluation_with_plane_refinement(gpu, tmp_path):
    from corsair_amd import cache as C, harness

    (catalog, queries, best_match, table, base_T, lib_T, syms), (sd, emb) = _workload()
    args = (best_match, table, base_T, lib_T, syms, "chair", True)
    kw = dict(force_gate=True, batch_size=4)                       # 10 queries: three registration batches
    plain_pipe = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(ransac_max_iter=2000))
    cat, qs = plain_pipe.embed_clouds(catalog), plain_pipe.embed_clouds(queries)
    with _Profile() as prof:
        plain = harness.run_eval(plain_pipe, cat, qs, *args, **kw)
    assert prof.n == {"icp": 0, "normals": 0} and plain.icp is None and cat.normal is None
    cfg = harness.Config(ransac_max_iter=2000, icp_max_iter=5, icp_estimation="plane", icp_normal_k=8)
    pipe = harness.Pipeline(sd, emb, device=gpu, config=cfg)
    with _Profile() as prof:
        res = harness.run_eval(pipe, cat, qs, *args, cache_dir=str(tmp_path), **kw)
    # the catalog's normals once per evaluation, not once per batch; one ICP call per batch
    assert prof.n == {"icp": 3, "normals": 1}
    assert not res.from_cache and res.icp is not None and "icp refinement" in res.report
    assert set(res.per_query) == set(C.NAMES) | set(C.ICP_NAMES)
    for k in C.NAMES:                                              # the nine arrays do not see the refinement
        assert _same(np.asarray(res.per_query[k]), np.asarray(plain.per_query[k])), k
    # the cache round-trips (its format does not record the estimation)
    with _Profile() as prof:
        again = harness.run_eval(pipe, cat, qs, *args, cache_dir=str(tmp_path), **kw)
    assert again.from_cache and prof.n == {"icp": 0, "normals": 0}
    for k in C.NAMES + C.ICP_NAMES:
        assert _same(np.asarray(again.per_query[k]), np.asarray(res.per_query[k])), k
    assert again.icp == res.icp
    # the point estimation on the same queries launches no normals
    pcfg = harness.Config(ransac_max_iter=2000, icp_max_iter=5)
    with _Profile() as prof:
        point = harness.run_eval(harness.Pipeline(sd, emb, device=gpu, config=pcfg), cat, qs, *args, **kw)
    assert prof.n == {"icp": 3, "normals": 0} and point.icp is not None
    # gather carries the normals along
    with_n = pipe.with_normals(cat)
    sub = with_n.gather([3, 3, 0])
    o = with_n.offsets
    assert _same(sub.normal.cpu().numpy(), torch.cat([with_n.normal[o[3]:o[4]]] * 2 + [with_n.normal[o[0]:o[1]]]).cpu().numpy())
    assert pipe.with_normals(with_n) is with_n and plain_pipe.with_normals(cat) is cat


def test_shapenet_eval_icp_outputs(gpu, tmp_path):
    import csv

    from corsair_amd import harness, shapenet_eval as S, synth

    _, (sd, emb) = _workload()
    pipe = harness.Pipeline(sd, emb, device=gpu)
    clouds = [synth.make_cloud(50 + i, 4000) for i in range(3)]
    base = dict(n_poses_per_model=1, ransac_max_iter=2000, max_translation=0.5)
    off = S.evaluate(pipe, clouds, S.Config(**base), pairs_per_batch=2)
    icp_keys = {"T_est_icp", "rte_icp", "rre_icp", "chamfer_dist_icp", "icp_iters"}
    assert len(off) == 3 and not icp_keys & set(off[0])
    assert set(S.threshold_table(off)) == {"ransac", "sym"} and "icp" not in S.summary(off)
    S.write_results(off, ["a", "b", "c"], str(tmp_path / "off.csv"), str(tmp_path / "off.npz"))
    assert tuple(next(csv.reader(open(tmp_path / "off.csv")))) == S.CSV_COLUMNS
    assert set(np.load(tmp_path / "off.npz").files) == {"poses_gt", "poses_pred_sym", "poses_pred_ransac"}
    for est in ("point", "plane"):
        on = S.evaluate(pipe, clouds, S.Config(icp_max_iter=10, icp_estimation=est, **base), pairs_per_batch=2)
        for a, b in zip(off, on):
            assert icp_keys <= set(b) and set(b) - icp_keys == set(a)
            for k in a:                                            # every output of today is what it was
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
            assert b["T_est_icp"].shape == (4, 4) and 0 <= b["icp_iters"] <= 10 and np.isfinite(b["rre_icp"])
        assert set(S.threshold_table(on)) == {"ransac", "sym", "icp"} and S.summary(on).count("icp:") == 3
        S.write_results(on, ["a", "b", "c"], str(tmp_path / "on.csv"), str(tmp_path / "on.npz"))
        rows = list(csv.reader(open(tmp_path / "on.csv")))
        assert tuple(rows[0]) == S.CSV_COLUMNS + S.ICP_CSV_COLUMNS and len(rows) == 4 and len(rows[1]) == len(rows[0])
        assert np.load(tmp_path / "on.npz")["poses_pred_icp"].shape == (3, 4, 4)
