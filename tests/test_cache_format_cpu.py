"""Result-cache format (evaluation.py:390-441): files written by corsair_amd.cache have the names,
shapes and dtypes of the reference's shipped caches, and round-trip."""
import os

import numpy as np

# the reference's shipped data/cache_pose_best for (chair, top1), the nine files unchanged (tests/golden/make_fixtures.py)
REF_CACHE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cache_pose_best")


def test_round_trip(tmp_path):
    from corsair_amd import cache

    rng = np.random.default_rng(0)
    Q = 7
    res = {"Ts_est_ransac": rng.standard_normal((Q, 4, 4)).astype(np.float32),
           "Ts_est_best": rng.standard_normal((Q, 4, 4)).astype(np.float32),
           "t_losses_ransac": rng.random(Q).astype(np.float32), "t_losses_sym": rng.random(Q).astype(np.float32),
           "r_losses_ransac": rng.random(Q), "r_losses_sym": rng.random(Q),
           "sym_ransac_success": rng.random(Q) > 0.5,
           "chamfer_dist_ransac": rng.random(Q), "chamfer_dist_sym": rng.random(Q)}
    assert cache.load_results(str(tmp_path), "chair", True) is None
    cache.save_results(str(tmp_path), "chair", True, res)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{n}_chair_top1.npy" for n in cache.NAMES)
    back = cache.load_results(str(tmp_path), "chair", True)
    for k in cache.NAMES:
        assert np.array_equal(back[k], res[k]), k
    assert np.load(tmp_path / "Ts_est_best_chair_top1.npy").shape == (Q, 16)
    assert cache.load_results(str(tmp_path), "chair", False) is None


def test_reads_the_reference_shipped_cache():
    from corsair_amd import cache
    from corsair_amd.harness import aggregate

    r = cache.load_results(REF_CACHE, "chair", True)
    assert r is not None and r["Ts_est_best"].shape == (993, 4, 4) and r["sym_ransac_success"].dtype == bool
    a = aggregate(r["r_losses_sym"], r["t_losses_sym"])
    assert abs(a["rre_mean_deg"] - 38.74) < 0.01 and abs(100 * a["rre_15"] - 59.82) < 0.01  # README.md:176
