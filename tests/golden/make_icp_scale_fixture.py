"""Generates tests/golden/icp_scale_boxes.npz, the fixture of tests/test_icp_scale_cpu.py: a chair-like set of boxes (seat,
back, four legs) sampled on its surface and thinned to one sample per voxel.

  tgt, nrm        the target cloud and the outward face normal of every row (f32)
  src_full        a second, independent sampling of the same surfaces (f32, the target's frame, true size)
  src_half        the rows of src_full on one side of a plane through the centroid: a half-space view
  voxel           the thinning voxel; the tests use max_dist = 2 voxels

The tests shrink or grow a source by a true scale, move it by a pose and start 5 degrees / 0.02 off: all of that is derived
from the seed in the test, so this file only fixes the geometry.  Run:  python tests/golden/make_icp_scale_fixture.py"""
import os

import numpy as np

SEED = 1
VOXEL = 0.04
N_SAMPLES = 10000
# (centre, half-extent) of every box
BOXES = [((0.0, 0.0, 0.0), (0.25, 0.25, 0.03)),          # seat
         ((0.0, -0.22, 0.33), (0.25, 0.03, 0.30)),        # back
         ((0.21, 0.21, -0.23), (0.03, 0.03, 0.20)), ((-0.21, 0.21, -0.23), (0.03, 0.03, 0.20)),
         ((0.21, -0.21, -0.23), (0.03, 0.03, 0.20)), ((-0.21, -0.21, -0.23), (0.03, 0.03, 0.20))]


def sample(rng, n):
    faces = []
    for c, h in BOXES:
        for ax in range(3):
            u, v = [a for a in range(3) if a != ax]
            for sg in (-1.0, 1.0):
                faces.append((c, h, ax, u, v, sg, 4.0 * h[u] * h[v]))
    area = np.array([f[-1] for f in faces])
    pick = rng.choice(len(faces), n, p=area / area.sum())
    pts, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for i, k in enumerate(pick):
        c, h, ax, u, v, sg, _ = faces[k]
        pts[i, ax] = c[ax] + sg * h[ax]
        pts[i, u] = c[u] + rng.uniform(-h[u], h[u])
        pts[i, v] = c[v] + rng.uniform(-h[v], h[v])
        nrm[i, ax] = sg
    return pts, nrm


def thin(pts, nrm, voxel):
    """The first sample of every voxel, in sample order."""
    _, first = np.unique(np.floor(pts / voxel).astype(np.int64), axis=0, return_index=True)
    first.sort()
    return pts[first], nrm[first]


def main():
    rng = np.random.default_rng(SEED)
    tgt, nrm = thin(*sample(rng, N_SAMPLES), VOXEL)
    src, _ = thin(*sample(rng, N_SAMPLES), VOXEL)
    view = np.array([0.6, 0.64, 0.48])
    half = src[(src - src.mean(0)) @ view > 0.0]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "icp_scale_boxes.npz")
    np.savez_compressed(out, tgt=tgt.astype(np.float32), nrm=nrm.astype(np.float32), src_full=src.astype(np.float32),
                        src_half=half.astype(np.float32), voxel=np.float64(VOXEL))
    print(out, "tgt", len(tgt), "src_full", len(src), "src_half", len(half))


if __name__ == "__main__":
    main()
