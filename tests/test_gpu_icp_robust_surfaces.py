"""The Python surfaces of the robust point-to-plane refinement on the GPU: backend.icp_batch(kernel=...) and
IcpResult.wfitness, registration.sym_pose_batch(icp_kernel=...) and icp_wfitness, harness.Config.check_icp and the two
command lines."""
import numpy as np
import pytest
import torch

from tests import icp_robust_ref as ref
from tests import test_gpu_icp as pt
from tests.test_gpu_icp_plane_surfaces import _Profile

pytestmark = pytest.mark.gpu
_same = pt._same


def test_icp_batch_keywords_and_wfitness(gpu):
    from corsair_amd import backend as B

    _, x0, off0, _, x1, off1, Ts = pt._pair_batch(gpu)
    nrm = B.estimate_normals(x1, off1, 8)
    T0 = torch.from_numpy(np.stack([pt._perturbed(T, 2.0, 0.01, np.random.default_rng(3)) for T in Ts])).to(gpu)
    args = (x0, off0, x1, off1, [0, 1], [0, 1], T0, 0.06, 5)
    plain = B.icp_batch(*args, tgt_normals=nrm)
    l2 = B.icp_batch(*args, tgt_normals=nrm, kernel="l2", kernel_scale=0.01)
    assert plain.wfitness is None and l2.wfitness is None           # the default launches nothing new
    for a, b in zip(plain[:6], l2[:6]):
        assert _same(a.cpu().numpy(), b.cpu().numpy())
    point = B.icp_batch(*args)
    assert point.wfitness is None and B.icp_batch(*args, kernel="l2").wfitness is None
    for kernel in ("huber", "cauchy", "tukey"):
        r = B.icp_batch(*args, tgt_normals=nrm, kernel=kernel, kernel_scale=0.01)
        want = ref.icp_batch(x0.cpu().numpy(), off0, x1.cpu().numpy(), nrm.cpu().numpy(), off1, [0, 1], [0, 1],
                             T0.cpu().numpy(), 0.06, 5, kernel=kernel, kernel_scale=0.01)
        assert r.wfitness.dtype == torch.float64 and tuple(r.wfitness.shape) == (2,)
        for p in range(2):
            assert _same(r.T[p].cpu().numpy().reshape(16), want[p]["T"])
            assert _same(r.wfitness[p].cpu().numpy(), np.float64(want[p]["wfitness"]))
            assert _same(r.fitness[p].cpu().numpy(), np.float64(want[p]["fitness"]))
            assert int(r.iters[p]) == want[p]["iters"]
            assert 0.0 < float(r.wfitness[p]) <= float(r.fitness[p])     # (Huber's weights are all 1 once |r| <= k)
    for kw in (dict(kernel="tukey", kernel_scale=0.01), dict(kernel="huber")):
        with pytest.raises(ValueError, match="tgt_normals"):      # robust kernels exist for the plane estimation only
            B.icp_batch(*args, **kw)
    with pytest.raises(ValueError, match="kernel"):
        B.icp_batch(*args, tgt_normals=nrm, kernel="gm", kernel_scale=0.01)


def test_sym_pose_batch_kernel(gpu):
    from corsair_amd import backend as B, registration as R

    F0, x0, off0, F1, x1, off1, _ = pt._pair_batch(gpu)
    kw = dict(k_nn=5, max_corr=0.2, seed=0, max_iter=2000, force_gate=True, icp_max_iter=5, icp_max_dist=0.06,
              icp_estimation="plane", icp_normal_k=8)
    fields = ("T_best", "cd_best", "T_ransac", "cd_ransac", "T_icp", "cd_icp", "icp_fitness", "icp_rmse", "icp_iters")
    plain = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], **kw)
    with _Profile() as prof:
        l2 = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_kernel="l2", icp_kernel_scale=0.5, **kw)
    assert prof.n == {"icp": 1, "normals": 1}
    assert plain.icp_wfitness is None and l2.icp_wfitness is None
    for name in fields:                                             # the defaults return what they returned before
        assert _same(getattr(plain, name).cpu().numpy(), getattr(l2, name).cpu().numpy()), name
    with _Profile() as prof:
        tukey = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_kernel="tukey", icp_kernel_scale=0.01, **kw)
    assert prof.n == {"icp": 1, "normals": 1}
    for name in fields[:4]:
        assert _same(getattr(plain, name).cpu().numpy(), getattr(tukey, name).cpu().numpy()), name
    nrm = B.estimate_normals(x1, off1, 8)
    want = ref.icp_batch(x0.cpu().numpy(), off0, x1.cpu().numpy(), nrm.cpu().numpy(), off1, [0, 1], [0, 1],
                         tukey.T_best.cpu().numpy(), 0.06, 5, kernel="tukey", kernel_scale=0.01)
    for p in range(2):
        assert _same(tukey.T_icp[p].cpu().numpy().reshape(16), want[p]["T32"])
        assert _same(tukey.icp_wfitness[p].cpu().numpy(), np.float64(want[p]["wfitness"]))
        assert _same(tukey.icp_fitness[p].cpu().numpy(), np.float64(want[p]["fitness"]))
        assert int(tukey.icp_iters[p]) == want[p]["iters"]
    assert _same(tukey.cd_icp.cpu().numpy(), B.chamfer_1dir(x0, off0, x1, off1, [0, 1], [0, 1], tukey.T_icp).cpu().numpy())
    off = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], k_nn=5, max_corr=0.2, seed=0, max_iter=2000, force_gate=True)
    assert off.T_icp is None and off.icp_wfitness is None
    with pytest.raises(ValueError, match="icp_kernel"):
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_kernel="gm", icp_kernel_scale=0.01, **kw)
    with pytest.raises(ValueError, match="plane"):
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_kernel="huber", icp_kernel_scale=0.01,
                         **dict(kw, icp_estimation="point"))
    with pytest.raises(ValueError, match="icp_kernel_scale"):
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_kernel="huber", **kw)


def test_harness_pipeline_passes_the_kernel(gpu):
    from corsair_amd import harness
    from tests.test_gpu_icp_plane_surfaces import _workload

    (catalog, queries, best_match, table, base_T, lib_T, syms), (sd, emb) = _workload()
    args = (best_match, table, base_T, lib_T, syms, "chair", True)
    kw = dict(force_gate=True, batch_size=4)
    base = dict(ransac_max_iter=2000, icp_max_iter=5, icp_estimation="plane", icp_normal_k=8)
    pipe = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(**base))
    cat, qs = pipe.embed_clouds(catalog), pipe.embed_clouds(queries)
    plain = harness.run_eval(pipe, cat, qs, *args, **kw)
    with _Profile() as prof:
        robust = harness.run_eval(harness.Pipeline(sd, emb, device=gpu, config=harness.Config(icp_kernel="cauchy", **base)),
                                  cat, qs, *args, **kw)
    assert prof.n == {"icp": 3, "normals": 1}
    from corsair_amd import cache as C

    for k in C.NAMES:                                               # the nine arrays do not see the refinement
        assert _same(np.asarray(robust.per_query[k]), np.asarray(plain.per_query[k])), k
    assert set(robust.per_query) == set(C.NAMES) | set(C.ICP_NAMES)  # the cache keeps its format
    assert not _same(np.asarray(robust.per_query["Ts_est_icp"]), np.asarray(plain.per_query["Ts_est_icp"]))


def test_config_and_command_lines(gpu):
    from corsair_amd import harness, shapenet_eval as S

    harness.Config(icp_estimation="plane", icp_kernel="huber", icp_kernel_scale=0.02).check_icp()
    assert harness.Config(icp_kernel="tukey", icp_estimation="plane").icp_scale() == harness.Config().voxel_size
    with pytest.raises(ValueError, match="icp_kernel"):
        harness.Config(icp_estimation="plane", icp_kernel="l1").check_icp()
    with pytest.raises(ValueError, match="plane"):
        harness.Config(icp_kernel="tukey").check_icp()
    base = ["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"]
    a = harness.build_parser().parse_args(base + ["--icp-estimation", "plane", "--icp-kernel", "tukey",
                                                  "--icp-kernel-scale", "0.02"])
    assert (a.icp_kernel, a.icp_kernel_scale) == ("tukey", 0.02)
    a = S.build_parser().parse_args(["--ckpt", "c", "--icp-kernel", "huber", "--icp-kernel-scale", "0.03"])
    assert (a.icp_kernel, a.icp_kernel_scale) == ("huber", 0.03)
    assert S.Config(icp_kernel="huber", icp_kernel_scale=0.03).icp_scale() == 0.03
