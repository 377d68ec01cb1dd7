"""The Python surfaces of Fast Global Registration on the GPU: registration.sym_pose_batch(registration="fgr") against the
hand composition of its stages, its composition with the ICP refinement, the untouched default, and the two command lines."""
import csv
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_icp as pt
from tests.test_gpu_cli import _norm, _raw_real_clouds, ckpt_file  # noqa: F401  (ckpt_file: the module's fixture)

pytestmark = pytest.mark.gpu
_same = pt._same
KW = dict(k_nn=5, max_corr=0.2, seed=0, max_iter=2000, force_gate=True)
SYMS = [1, 2]                      # the second pair has K = 4 parts and the mirrored configurations


class _Profile:
    """cs_prof_* around a block: launches per family afterwards."""
    FAMILIES = ("fgr", "ransac_hyp", "ransac_eval", "icp")

    def __enter__(self):
        from corsair_amd import _lib

        _lib.prof_enable(True)
        _lib.prof_reset()
        return self

    def __exit__(self, *exc):
        from corsair_amd import _lib

        torch.cuda.synchronize()
        self.n = {f: _lib.prof_get(f)[1] for f in self.FAMILIES}
        _lib.prof_enable(False)


def _hand_lists(F0, x0, off0, F1, x1, off1, syms, k=5, n_anchor=100):
    """Stages 1 - 3 of sym_pose_batch by hand: the vanilla correspondence lists of every pair, then the lists of every
    part configuration.  Returns (src, tgt, offsets, prob_pair)."""
    from corsair_amd import backend as B, registration as R
    from corsair_amd._lib import to_host

    dev = F0.device
    P = len(off0) - 1
    n0 = [off0[p + 1] - off0[p] for p in range(P)]
    n1 = [off1[p + 1] - off1[p] for p in range(P)]
    nn = B.knn_feat(F0, off0, F1, off1, k)
    desc_v = np.asarray([[off0[p], off0[p], off1[p], n0[p], off0[p]] for p in range(P)], dtype=np.int64).reshape(P, 5)
    v_src, v_tgt = B.corr_assemble(x0, x1, None, nn, desc_v, off0[-1], max(n0))
    src, tgt, lens, pair = [v_src], [v_tgt], [n0[p] * k for p in range(P)], list(range(P))
    Ks = [4 if int(syms[p]) >= 2 else 2 for p in range(P)]
    anc0 = [R.draw_anchors(n0[p], n_anchor, 2 * p) for p in range(P)]
    anc1 = [R.draw_anchors(n1[p], n_anchor, 2 * p + 1) for p in range(P)]
    assert all(a is not None for a in anc0 + anc1)
    a_all = torch.from_numpy(np.concatenate([np.stack(anc0), np.stack(anc1)])).to(dev)
    off_all = list(off0) + [off0[-1] + o for o in off1[1:]]
    c, cnt, mcd, mer = to_host(*B.symcut_fit(torch.cat([F0, F1]), torch.cat([x0, x1]), off_all, a_all, Ks + Ks, 50, 10, 300))
    cand = list(range(P))
    g0, ok0 = R.gate_and_order_batch(c[:P], cnt[:P], mcd[:P], mer[:P], n0, Ks, cand, R.GATE_ANY)
    g1, ok1 = R.gate_and_order_batch(c[P:], cnt[P:], mcd[P:], mer[P:], n1, Ks, cand, R.GATE_ANY)
    ok = ok0 & ok1
    sel0, sel1 = np.zeros((P, 4, 3)), np.zeros((P, 4, 3))
    sel0[ok], sel1[ok] = g0[ok], g1[ok]
    good = [p for p in range(P) if ok[p]]
    assert good
    lab0 = B.symcut_labels(x0, off0, Ks, torch.from_numpy(sel0).to(dev))
    lab1 = B.symcut_labels(x1, off1, Ks, torch.from_numpy(sel1).to(dev))
    seg, perms = [], []
    for p in good:
        for cfg in R.part_configs(Ks[p], int(syms[p])):
            seg.append(p)
            perms.append(cfg + [-3] * (8 - len(cfg)))
    cl = np.asarray([n0[p] for p in seg], dtype=np.int64)
    row_start = np.concatenate([[0], np.cumsum(cl)])
    order = B.partition_by_label(lab0, torch.tensor(off0, dtype=torch.int64, device=dev), P)
    nn_cfg = B.knn_feat(F0[order], off0, F1, off1, k, qseg=seg, tseg=seg, qlabel=lab0[order].contiguous(), tlabel=lab1,
                        perm=torch.tensor(perms, dtype=torch.int32, device=dev))
    bad = to_host(B.cfg_bad(nn_cfg, torch.from_numpy(row_start).to(dev), len(seg)))[0] > 0
    keep = [j for j in range(len(seg)) if not bad[j]]
    assert keep
    out_first = np.concatenate([[0], np.cumsum(cl[keep])])
    desc = np.asarray([[off0[seg[j]], row_start[j], off1[seg[j]], cl[j], out_first[i]] for i, j in enumerate(keep)],
                      dtype=np.int64)
    s_src, s_tgt = B.corr_assemble(x0, x1, order, nn_cfg, desc, int(out_first[-1]), int(cl[keep].max()))
    src.append(s_src)
    tgt.append(s_tgt)
    for j in keep:
        lens.append(n0[seg[j]] * k)
        pair.append(seg[j])
    return torch.cat(src), torch.cat(tgt), np.concatenate([[0], np.cumsum(lens)]).tolist(), pair


def test_sym_pose_batch_fgr_equals_the_hand_composition(gpu):
    from corsair_amd import backend as B, registration as R

    F0, x0, off0, F1, x1, off1, _ = pt._pair_batch(gpu)
    with _Profile() as prof:
        res = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, SYMS, registration="fgr", **KW)
    assert prof.n["fgr"] == 1 and prof.n["ransac_hyp"] == 0 and prof.n["ransac_eval"] == 0
    src, tgt, offs, pair = _hand_lists(F0, x0, off0, F1, x1, off1, SYMS)
    assert res.n_problems == len(pair) > 2 and res.prob_pair == pair and any(c is not None for c in res.prob_cfg)
    r = B.fgr_batch(src, tgt, offs, KW["max_corr"], seed=KW["seed"])
    assert _same(res.T_all.cpu().numpy(), r.T.cpu().numpy())
    assert _same(res.inliers.cpu().numpy(), r.inliers.cpu().numpy()) and _same(res.iters.cpu().numpy(), r.iters.cpu().numpy())
    cd = B.chamfer_1dir(x0, off0, x1, off1, pair, pair, r.T).cpu().numpy()
    assert _same(res.cd_all.cpu().numpy(), cd)
    best = np.arange(2)
    for j in range(2, len(pair)):                       # the first strict minimum, vanilla first
        if cd[best[pair[j]]] > cd[j]:
            best[pair[j]] = j
    assert np.array_equal(res.best, best)
    assert _same(res.T_best.cpu().numpy(), r.T.cpu().numpy()[best]) and _same(res.cd_best.cpu().numpy(), cd[best])
    assert _same(res.T_ransac.cpu().numpy(), r.T.cpu().numpy()[:2])
    print("fgr: updates", r.iters.cpu().numpy(), "tuples", r.n_tuple.cpu().numpy(), "chamfer", cd)
    # the options reach the call
    other = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, SYMS, registration="fgr", fgr_mu_floor=0.1, fgr_iterations=7,
                             fgr_tuple_test=False, **KW)
    r2 = B.fgr_batch(src, tgt, offs, KW["max_corr"], mu_floor=0.1, iteration_number=7, tuple_test=False, seed=KW["seed"])
    assert _same(other.T_all.cpu().numpy(), r2.T.cpu().numpy()) and int(other.iters.max()) <= 7
    assert np.all(r2.n_tuple.cpu().numpy() == -1)
    with pytest.raises(ValueError, match="registration"):
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, SYMS, registration="teaser", **KW)
    with pytest.raises(TypeError):                       # keyword-only
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, SYMS, 5, 0.2, 0, None, 100, 2000, 0.999, True, True, None, 0, None,
                         "point", 16, None, None, False, None, "l2", None, "fgr")


def test_fgr_composes_with_the_icp_refinement(gpu):
    from corsair_amd import backend as B, registration as R

    F0, x0, off0, F1, x1, off1, _ = pt._pair_batch(gpu)
    plain = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, SYMS, registration="fgr", **KW)
    with _Profile() as prof:
        on = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, SYMS, registration="fgr", icp_max_iter=5, icp_max_dist=0.06, **KW)
    assert prof.n["fgr"] == 1 and prof.n["icp"] == 1 and plain.T_icp is None
    for name in ("T_best", "cd_best", "T_all", "cd_all", "inliers", "iters"):
        assert _same(getattr(on, name).cpu().numpy(), getattr(plain, name).cpu().numpy()), name
    want = B.icp_batch(x0, off0, x1, off1, [0, 1], [0, 1], on.T_best, 0.06, 5)
    assert _same(on.T_icp.cpu().numpy(), want.T32.cpu().numpy()) and _same(on.icp_iters.cpu().numpy(), want.iters.cpu().numpy())
    assert _same(on.cd_icp.cpu().numpy(), B.chamfer_1dir(x0, off0, x1, off1, [0, 1], [0, 1], on.T_icp).cpu().numpy())


def test_default_estimator_is_untouched(gpu):
    from corsair_amd import registration as R

    F0, x0, off0, F1, x1, off1, _ = pt._pair_batch(gpu)
    with _Profile() as prof:
        never = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, SYMS, **KW)
    assert prof.n["fgr"] == 0 and prof.n["ransac_hyp"] > 0
    with _Profile() as prof:
        named = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, SYMS, registration="ransac", fgr_mu_floor=0.5,
                                 fgr_iterations=3, fgr_tuple_test=False, **KW)
    assert prof.n["fgr"] == 0
    assert vars(never).keys() == vars(named).keys()
    for name, v in vars(never).items():
        w = getattr(named, name)
        if torch.is_tensor(v):
            assert _same(v.cpu().numpy(), w.cpu().numpy()), name
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, w), name
        else:
            assert v == w, name


def test_harness_cli_accepts_fgr(gpu, ckpt_file, tmp_path):  # noqa: F811
    from corsair_amd import cache, harness

    path, _, _ = ckpt_file
    clouds = [_norm(c) for c in _raw_real_clouds()[:2]]
    cat_dir, q_dir = tmp_path / "cads", tmp_path / "scans"
    cat_dir.mkdir()
    q_dir.mkdir()
    for i, c in enumerate(clouds):
        np.save(cat_dir / f"cad_{i:03d}.npy", c)
        np.save(q_dir / f"scan_{i:03d}.npy", c[::-1].copy())
    argv = ["--ckpt", path, "--catalog-dir", str(cat_dir), "--query-dir", str(q_dir), "--category", "chair",
            "--cache-dir", str(tmp_path / "cache"), "--n-points", "4000", "--registration", "fgr", "--fgr-mu-floor", "0.05"]
    with _Profile() as prof:
        res = harness.main(argv)
    assert prof.n["fgr"] >= 1 and prof.n["ransac_hyp"] == 0
    assert sorted(p.name for p in (tmp_path / "cache").iterdir()) == sorted(f"{n}_chair_top1.npy" for n in cache.NAMES)
    assert all(len(res.per_query[k]) == 2 for k in cache.NAMES)
    cfg = harness.Config(registration="fgr", fgr_mu_floor=0.05)
    cfg.check_icp()
    with pytest.raises(ValueError, match="registration"):
        harness.Config(registration="teaser").check_icp()
    with pytest.raises(ValueError, match="fgr_mu_floor"):
        harness.Config(registration="fgr", fgr_mu_floor=0.0).check_icp()
    with pytest.raises(SystemExit):
        harness.build_parser().parse_args(argv[:-4] + ["--registration", "teaser"])


def test_shapenet_eval_cli_accepts_fgr(gpu, ckpt_file, tmp_path):  # noqa: F811
    from corsair_amd import shapenet_eval as S

    path, _, _ = ckpt_file
    d = tmp_path / "03001627" / "test"
    d.mkdir(parents=True)
    for i, c in enumerate(_raw_real_clouds()[:2]):
        np.save(d / f"m{i}.npy", c[:4000])
    with _Profile() as prof:
        results, csv_file, npz_file = S.main(["--shapenet-root", str(tmp_path), "--category", "chair", "--n-models", "0",
                                              "--n-poses-per-model", "1", "--ckpt", path, "--random-seed", "4",
                                              "--registration", "fgr", "--fgr-mu-floor", "0.05",
                                              "--out-dir", str(tmp_path / "out")])
    assert prof.n["fgr"] >= 1 and prof.n["ransac_hyp"] == 0
    assert os.path.basename(csv_file) == "results-shapenet-seed4-chair-2-1.csv"
    rows = list(csv.reader(open(csv_file)))
    assert tuple(rows[0]) == S.CSV_COLUMNS and len(rows) == 3
    z = np.load(npz_file)
    assert z["poses_gt"].shape == (2, 4, 4) and z["poses_pred_sym"].shape == (2, 4, 4) and len(results) == 2
    assert np.all(np.isfinite(z["poses_pred_sym"]))
