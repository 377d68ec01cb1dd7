"""Fixtures of the partial-view tests: the geometry tests/test_view_cpu.py judges the restatement on (sphere
lattices, two planes), the defined cases of the header, and the batch tests/test_gpu_view.py compares bit for bit."""
import math

import numpy as np

from corsair_amd import views as V

# ---- a camera at the origin that looks along +z ------------------------------------------------------------------------------
EYE = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 3), dtype=np.float32)


# ---- the sphere ----------------------------------------------------------------------------------------------------------
SPHERE = ((1000, 64, 0.16), (2000, 96, 0.12), (4000, 128, 0.08))     # rows, image side, point_size = depth_tol
SPHERE_DIRECTIONS = ((0.0, 0.0, 1.0), (1.0, 1.0, 1.0), (-0.3, 0.9, -0.2))
SPHERE_DISTANCE, SPHERE_FOV = 3.0, 50.0
# The splat that must leak, in row spacings sqrt(4 pi / n).  A square covers the pixels floor(u - h) .. floor(u + h): at most
# its side plus one pixel across.  A pixel is 0.27 - 0.29 spacings at the sphere's near side in the three configurations, so a
# square of half a spacing covers at most 0.79 spacings, while neighbouring rows of the lattice are about one spacing apart:
# the near squares cannot close the image, and a far row whose centre pixel falls into a gap is visible.
LEAK_SPACINGS = 0.5


def spacing(n):
    return math.sqrt(4.0 * math.pi / n)


def fibonacci_sphere(n):
    """n rows on the unit sphere, f64: the golden-angle lattice."""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def sphere_camera(direction):
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    return d, V.look_at(SPHERE_DISTANCE * d, np.zeros(3))


def incidence(points, d):
    """The cosine between the outward normal of a row of the unit sphere and the direction to an eye at 3 d:
    (3c - 1) / sqrt(10 - 6c) with c the cosine between the row and d."""
    c = points @ d
    return (3.0 * c - 1.0) / np.sqrt(10.0 - 6.0 * c)


# ---- two planes ----------------------------------------------------------------------------------------------------------
def two_planes():
    """A 21 x 21 patch at pitch 0.03, 0.3 in front of a 41 x 41 one; the camera 3 away from the back one on the axis.
    Returns (xyz f32, camera, number of front rows)."""
    a = (np.arange(21) - 10) * 0.03
    b = (np.arange(41) - 20) * 0.03
    fx, fy = np.meshgrid(a, a, indexing="ij")
    bx, by = np.meshgrid(b, b, indexing="ij")
    front = np.stack([fx.ravel(), fy.ravel(), np.full(fx.size, 0.3)], 1)
    back = np.stack([bx.ravel(), by.ravel(), np.zeros(bx.size)], 1)
    return _f32(np.concatenate([front, back])), V.look_at([0.0, 0.0, 3.0], [0.0, 0.0, 0.0]), len(front)


# ---- the defined cases of the header ------------------------------------------------------------------------------------------
def defined_cases():
    """name -> (xyz f32 [m,3], camera [12], width, height, focal, point_size, depth_tol)."""
    nan, inf = float("nan"), float("inf")
    c = {}
    c["empty"] = (_f32([]), EYE, 8, 8, 8.0, 0.05, 0.05)
    c["one_row"] = (_f32([[0.05, 0.05, 2]]), EYE, 8, 8, 8.0, 0.05, 0.05)
    c["behind"] = (_f32([[0, 0, -1], [0.1, 0.1, 2], [0, 0, -1e-30]]), EYE, 8, 8, 8.0, 0.05, 0.05)
    c["z_zero"] = (_f32([[0.1, 0.1, 0], [0, 0, 0], [0, 0, 1]]), EYE, 8, 8, 8.0, 0.05, 0.05)
    c["nonfinite"] = (_f32([[nan, 0, 1], [0, inf, 1], [0, 0, inf], [-inf, 0, 2], [0, nan, nan], [0.1, 0, 1]]), EYE, 8, 8, 8.0,
                      0.05, 0.05)
    c["large"] = (_f32([[1e5, 0, 1e6], [1e29, 2e29, 1e30], [1e30, 1e30, 1], [-1e6, 1e6, 1e6], [3e38, 3e38, 3e38]]), EYE, 8,
                  8, 8.0, 0.05, 0.05)
    # u = -0.4: out of frame, but its square of 1.2 pixels reaches column 0, where the second row (u = 0.4, Z = 2) lies
    c["reach_in"] = (_f32([[-0.55, 0, 1], [-0.9, 0, 2]]), EYE, 8, 8, 8.0, 0.3, 0.3)
    c["reach_in_control"] = (_f32([[-0.9, 0, 2]]), EYE, 8, 8, 8.0, 0.3, 0.3)
    c["on_the_lens"] = (_f32([[0, 0, 1e-6], [0.5, 0.5, 4]]), EYE, 64, 64, 32.0, 0.05, 0.05)
    # one row at each border of a 16 x 16 image (focal 16, Z = 1: u = 16 x + 8), squares of 2.4 pixels
    c["borders"] = (_f32([[-0.49, 0, 1], [0.49, 0, 1], [0, -0.49, 1], [0, 0.49, 1], [-0.49, -0.49, 1], [0.49, 0.49, 1]]), EYE,
                    16, 16, 16.0, 0.3, 0.05)
    c["image_1x1"] = (_f32([[0, 0, 1], [0.2, -0.3, 3], [0.6, 0, 1], [0, 0, 1.02]]), EYE, 1, 1, 1.0, 0.1, 0.05)
    c["image_7x5"] = (_f32([[0, 0, 1], [0.3, 0.2, 1], [-0.4, -0.3, 1.5], [0.1, -0.05, 2], [0, 0.36, 1], [0.3, 0.2, 1.01]]), EYE,
                      7, 5, 7.0, 0.2, 0.05)
    # five rows on one ray (0.01, 0.02, 1) x Z and a tolerance below every gap: the nearest alone survives
    ray = np.array([0.01, 0.02, 1.0])
    c["tight_tol"] = (_f32([ray * z for z in (2.0, 1.5, 1.0, 1.25, 3.0)]), EYE, 8, 8, 8.0, 0.05, 1e-3)
    c["equal_z"] = (_f32([[0.01, 0, 2], [0.02, 0, 2]]), EYE, 8, 8, 8.0, 0.05, 1e-9)
    return c


# ---- the batch of the device tests ---------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, 257, 1500)
OFF = np.concatenate([[0], np.cumsum(SIZES)]).tolist()
IMAGES = ((1, 1), (7, 5), (64, 64), (256, 256))      # (width, height)
FOV, POINT_SIZE, DEPTH_TOL = 40.0, 0.05, 0.05


def batch(seed):
    """{"xyz": f32 [sum SIZES, 3], "cams": f64 [8,12]}: noisy shells of radius 0.5, each under a camera of its own at 1.2 - 2
    from the centre; the camera of the 257-row segment stands INSIDE its shell, so rows lie behind it, out of frame and
    close enough for the 16-pixel cap.  Two draws have the same shapes and different values."""
    rng = np.random.default_rng(seed)
    xyz, cams = [], []
    for s, n in enumerate(SIZES):
        p = rng.standard_normal((n, 3))
        p = 0.5 * p / np.linalg.norm(p, axis=1, keepdims=True) + rng.normal(0, 0.004, (n, 3))
        xyz.append(p)
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        if n == 257:
            cams.append(V.look_at(0.45 * d, -0.5 * d + 0.1 * rng.standard_normal(3)))
        else:
            cams.append(V.look_at(rng.uniform(1.2, 2.0) * d, 0.05 * rng.standard_normal(3)))
    return {"xyz": _f32(np.concatenate(xyz)), "cams": np.stack(cams)}


def focal(width):
    return V.focal_from_fov(width, FOV)
