"""Generates tests/golden/fgr_case.npz, the fixture of tests/test_fgr_cpu.py: a few small correspondence problems with the
outputs tests/fgr_ref.py (the restatement of cs_fgr_batch) gives for them.

  src, tgt, off       the pairs of all problems (f32 [M,3]) and their offsets
  R, t                the true pose of every problem
  max_corr, seed      the call's arguments; every other argument is the default
  tuple_test          per problem: 1 = run with the tuple test, 0 = without
  T, T32, inliers, rmse, iters, n_tuple      the restatement's outputs

Problem 0 is the case the estimator was introduced on: 600 pairs in a 1.0 x 1.6 x 0.8 box, random pose, 0.005 noise, 80 %
of the targets replaced by uniform draws in the posed box (a least-squares fit on all pairs is more than 5 degrees off).
Problem 1: the same at 90 % outliers; problem 2: 120 pairs, a tenth outliers, no tuple test; problem 3: 9 pairs, no
tuple test (the fewer-than-ten rule counts working pairs, and the tuple test would repeat these nine).
Run from the repository root:  python tests/golden/make_fgr_fixture.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import fgr_ref as ref  # noqa: E402

MAX_CORR = 0.05
SEED = 0
# (pairs, outlier share, generator seed, tuple test)
CASES = ((600, 0.8, 0, 1), (600, 0.9, 1, 1), (120, 0.1, 2, 0), (9, 0.0, 3, 0))


def main():
    src, tgt, Rs, ts, out = [], [], [], [], []
    for n, share, seed, tuple_test in CASES:
        s, q, R, t = ref.outlier_case(n, share, seed)
        src.append(s)
        tgt.append(q)
        Rs.append(R)
        ts.append(t)
        out.append(ref.fgr(s, q, MAX_CORR, tuple_test_on=bool(tuple_test), seed=SEED))
    deg, _ = ref.pose_error(ref.horn_fit(src[0], tgt[0]), Rs[0], ts[0])
    assert deg > 5.0, deg
    off = np.concatenate([[0], np.cumsum([c[0] for c in CASES])]).astype(np.int64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fgr_case.npz")
    np.savez_compressed(path, src=np.concatenate(src), tgt=np.concatenate(tgt), off=off, R=np.stack(Rs), t=np.stack(ts),
                        max_corr=np.float64(MAX_CORR), seed=np.int64(SEED),
                        tuple_test=np.asarray([c[3] for c in CASES], np.int32),
                        T=np.stack([o["T"] for o in out]), T32=np.stack([o["T32"] for o in out]),
                        inliers=np.asarray([o["inliers"] for o in out], np.int32),
                        rmse=np.asarray([o["rmse"] for o in out], np.float64),
                        iters=np.asarray([o["iters"] for o in out], np.int32),
                        n_tuple=np.asarray([o["n_tuple"] for o in out], np.int32))
    print(path, "horn %.2f deg" % deg, [(o["n_tuple"], o["iters"], o["inliers"]) for o in out])


if __name__ == "__main__":
    main()
