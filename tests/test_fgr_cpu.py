"""The restatement of cs_fgr_batch (tests/fgr_ref.py) on the CPU: what the estimator is for (a pose from a list that is
four fifths outliers, where a least-squares fit fails), its schedule, its order-independence, its identity answers, the
golden file, and the places the feature is declared in."""
import functools
import math
import os

import numpy as np
import pytest

from tests import fgr_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fgr_case.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _restated(p):
    g = _golden()
    a, b = int(g["off"][p]), int(g["off"][p + 1])
    return ref.fgr(g["src"][a:b], g["tgt"][a:b], float(g["max_corr"]), tuple_test_on=bool(g["tuple_test"][p]),
                   seed=int(g["seed"]))


def test_least_squares_fails_on_the_outlier_case():
    g = _golden()
    n = int(g["off"][1])
    assert n == 600
    deg, _ = ref.pose_error(ref.horn_fit(g["src"][:n], g["tgt"][:n]), g["R"][0], g["t"][0])
    print("Horn on all pairs: %.2f degrees" % deg)
    assert deg > 5.0


def test_tuple_test_and_line_process_recover_the_pose():
    g = _golden()
    for p in (0, 1):                        # 80 % and 90 % outliers
        r = _restated(p)
        deg, dt = ref.pose_error(r["T"], g["R"][p], g["t"][p])
        print("problem %d: %.3f degrees, %.4f, %d tuples, %d updates" % (p, deg, dt, r["n_tuple"], r["iters"]))
        assert deg < 1.0 and dt < 0.01
        assert 10 <= r["n_tuple"] <= 1000 and r["iters"] == 64


def test_mu_schedule_reaches_the_floor():
    # mu is divided after the updates of iterations 0, 4, 8, ...: eleven divisions by iteration 40, and 1.4^-11 < 0.025
    assert 1.4 ** -10 > 0.025 > 1.4 ** -11
    g = _golden()
    a, b = int(g["off"][2]), int(g["off"][3])
    mus = [ref.fgr(g["src"][a:b], g["tgt"][a:b], 0.05, tuple_test_on=False, iteration_number=n)["mu"] for n in (40, 41, 64)]
    want = 1.0
    for _ in range(11):
        want = want / 1.4
    assert mus[0] > 0.025 and mus[1] == want and mus[2] == want and want < 0.025


def test_pair_order_does_not_matter_without_the_tuple_test():
    g = _golden()
    a, b = int(g["off"][2]), int(g["off"][3])
    src, tgt = g["src"][a:b], g["tgt"][a:b]
    base = ref.fgr(src, tgt, 0.05, tuple_test_on=False)
    perm = np.random.default_rng(3).permutation(len(src))
    other = ref.fgr(src[perm], tgt[perm], 0.05, tuple_test_on=False)
    assert base["iters"] == 64
    for k in ("T", "T32"):
        assert _same(base[k], other[k])
    assert all(base[k] == other[k] for k in ("inliers", "rmse", "iters", "n_tuple"))


def test_trial_chunking_does_not_matter():
    g = _golden()
    src, tgt = g["src"][:600], g["tgt"][:600]
    for max_tuple in (50, 1000):
        a = ref.fgr(src, tgt, 0.05, max_tuple=max_tuple, iteration_number=4, chunk=4096)
        b = ref.fgr(src, tgt, 0.05, max_tuple=max_tuple, iteration_number=4, chunk=7)
        assert a["n_tuple"] == b["n_tuple"] and _same(a["T"], b["T"])


def test_identity_answers():
    src, tgt, _, _ = ref.outlier_case(30, 0.0, 5)
    eye = np.asarray(ref.IDENTITY)

    def identity(r):
        return np.array_equal(r["T"], eye) and r["iters"] == 0

    assert not identity(ref.fgr(src, tgt, 0.05, tuple_test_on=False))
    assert identity(ref.fgr(src[:9], tgt[:9], 0.05, tuple_test_on=False))              # fewer than ten working pairs
    few = ref.fgr(src, tgt, 0.05, max_tuple=3)                                          # three tuples = nine pairs
    assert few["n_tuple"] == 3 and identity(few)
    one = np.tile(src[:1], (30, 1))
    r = ref.fgr(one, one, 0.05, tuple_test_on=False)                                    # g = 0
    assert identity(r) and r["inliers"] == 30 and r["rmse"] == 0.0
    bad = src.copy()
    bad[4, 0] = np.nan
    for tuple_test in (False, True):
        r = ref.fgr(bad, tgt, 0.05, tuple_test_on=tuple_test)                           # a NaN coordinate
        assert identity(r) and r["n_tuple"] == (0 if tuple_test else -1)
    assert identity(ref.fgr(src[:0], tgt[:0], 0.05)) and ref.fgr(src[:0], tgt[:0], 0.05)["inliers"] == 0


def test_golden_file_is_reproduced():
    g = _golden()
    for p in range(len(g["off"]) - 1):
        r = _restated(p)
        assert _same(r["T"], g["T"][p]) and _same(r["T32"], g["T32"][p]), p
        assert _same(np.float64(r["rmse"]), g["rmse"][p]), p
        assert (r["inliers"], r["iters"], r["n_tuple"]) == (g["inliers"][p], g["iters"][p], g["n_tuple"][p]), p
    assert g["iters"][3] == 0 and np.array_equal(g["T"][3], np.asarray(ref.IDENTITY))


def test_generator_matches_the_scalar_definition():
    def scalar(seed, itr, j):
        m = (1 << 64) - 1
        x = (seed + 0x9E3779B97F4A7C15 * (itr * 64 + j + 1)) & m
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        return x ^ (x >> 31)

    for seed in (0, 1, (1 << 64) - 1):
        for itr in (0, 1, 59999, (1 << 38) - 1):
            for j in range(3):
                assert int(ref.rng_u64(seed, np.asarray([itr], np.uint64), j)[0]) == scalar(seed, itr, j)
                assert int(ref.rng_index(seed, np.asarray([itr], np.uint64), j, 600)[0]) == ((scalar(seed, itr, j) >> 32) * 600) >> 32


def test_declared_everywhere():
    from corsair_amd import _lib

    assert "cs_fgr_batch" in _lib.header_symbols()
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    assert "fgr.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert '"fgr"' in open(os.path.join(csrc, "runtime.hip")).read()
    head = open(_lib.HEADER_PATH).read()
    for word in ("cs_fgr_batch", '"fgr"', "[O3D-knowledge]", "tuple_scale", "mu_floor"):
        assert word in head, word
    import inspect

    from corsair_amd import backend, registration

    assert list(inspect.signature(backend.fgr_batch).parameters) == [
        "src", "tgt", "offsets", "max_corr", "mu_floor", "division_factor", "iteration_number", "tuple_test", "tuple_scale",
        "max_tuple", "seed"]
    assert backend.FgrResult._fields == ("T", "T64", "inliers", "rmse", "iters", "n_tuple")
    # keyword-only behind the existing parameters: the defaults, and a value in the next positional slot is refused
    assert registration.sym_pose_batch.__kwdefaults__ == {"registration": "ransac", "fgr_mu_floor": 0.025,
                                                          "fgr_iterations": 64, "fgr_tuple_test": True}
    z = np.zeros((0, 16), np.float32)
    n_pos = len(inspect.signature(registration.sym_pose_batch).parameters)
    with pytest.raises(TypeError):
        registration.sym_pose_batch(*([z, z, [0], z, z, [0], []] + [None] * (n_pos - 7) + ["fgr"]))
    with pytest.raises(ValueError, match="registration"):
        registration.sym_pose_batch(z, z, [0], z, z, [0], [], registration="teaser")
    assert math.isclose(inspect.signature(backend.fgr_batch).parameters["mu_floor"].default, 0.025)
