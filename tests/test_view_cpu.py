"""Partial views without a GPU: tests/view_ref.py (the bit-exact restatement of cs_render_views that the GPU
tests compare with) against geometry that does not share its code -- the incidence angle on a sphere, the shadow of one plane
on another --, the defined cases of the header, the permutation property, the camera helpers, the options of shapenet_eval,
the sources and the ABI's refusals."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from tests import view_cases as VC
from tests import view_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_fast_fma_is_the_exact_one():
    from tests import icp_ref

    rng = np.random.default_rng(5)
    for _ in range(3000):
        a, b, c = rng.standard_normal(3) * 10.0 ** rng.integers(-30, 30, 3)
        assert ref.fma(a, b, c) == icp_ref.fma(a, b, c)
    for a, b, c in ((1e200, 1e200, 1.0), (-1e200, 1e200, 1.0), (3.0, -2.0, 6.0), (5e-324, 0.5, 0.0), (1e-200, 1e-200, 5e-324),
                    (float("inf"), 0.0, 1.0), (1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, -1.0)):
        got, want = ref.fma(a, b, c), icp_ref.fma(a, b, c) if abs(a) < 1e100 else None
        if want is not None:
            assert got == want or (math.isnan(got) and math.isnan(want)), (a, b, c)
    assert ref.fma(1e200, 1e200, 1.0) == float("inf") and ref.fma(-1e200, 1e200, 1.0) == -float("inf")
    assert math.copysign(1.0, ref.fma(3.0, -2.0, 6.0)) == 1.0


# ---- the sphere --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,side,size", VC.SPHERE)
def test_sphere_against_the_incidence_angle(rows, side, size):
    """Every row seen at an incidence cosine of 0.6 or more is visible, every row of the far side hidden; the band between
    (22.9 % of a sphere's area) is not compared.  The hidden rows with a positive cosine are the grazing-surface property of
    the header: a neighbour's camera-facing square covers their centre pixel from more than depth_tol in front.  Measured
    with this restatement on the nine configurations: nothing hidden above 0.449, nothing visible below 0.172.  A square of
    half a row spacing must leak (tests/view_cases.py: why); measured 89 - 408 far rows visible.  (At 1.07 spacings this
    lattice leaked 0 rows, at 0.9 spacings 0 - 10.)"""
    from corsair_amd import views as V

    pts = VC.fibonacci_sphere(rows)
    x = pts.astype(np.float32)
    f = V.focal_from_fov(side, VC.SPHERE_FOV)
    for direction in VC.SPHERE_DIRECTIONS:
        d, cam = VC.sphere_camera(direction)
        io = VC.incidence(pts, d)
        vis, _, st = ref.render_one(x, cam, side, side, f, size, size)
        vis = vis.astype(bool)
        band = float(((io > 0.0) & (io < 0.6)).mean())
        hidden = io[~vis & (io > 0.0)]
        print("%d rows, %s: %d visible; band %.3f; hidden up to %.3f, visible down to %.3f"
              % (rows, direction, st[2], band, hidden.max() if len(hidden) else 0.0, io[vis].min()))
        assert st[0] == st[1] == rows                         # the whole sphere is in front and in frame
        assert vis[io >= 0.6].all()
        assert not vis[io <= 0.0].any()
        assert band <= 0.25
        small, _, _ = ref.render_one(x, cam, side, side, f, VC.LEAK_SPACINGS * VC.spacing(rows), size)
        leaked = int((small.astype(bool) & (io <= 0.0)).sum())
        print("   a square of %.1f spacings lets %d far rows through" % (VC.LEAK_SPACINGS, leaked))
        assert leaked > 0


def test_two_planes():
    from corsair_amd import views as V

    xyz, cam, n_front = VC.two_planes()
    vis, _, st = ref.render_one(xyz, cam, 128, 128, V.focal_from_fov(128, 30.0), 0.045, 0.045)
    vis = vis.astype(bool)
    back = xyz[n_front:]
    r = np.abs(back[:, :2]).max(1)                             # the shadow of a square patch is a square: of half side 1 / 3
    assert st[0] == st[1] == len(xyz) == 441 + 1681
    assert vis[:n_front].all()
    assert not vis[n_front:][r <= 0.25].any()
    assert vis[n_front:][r > 0.40].all()


# ---- the defined cases of the header ------------------------------------------------------------------------------------------
def test_defined_cases():
    cases = VC.defined_cases()
    out = {k: ref.render_one(*v) for k, v in cases.items()}
    inf = float("inf")
    vis, z, st = out["empty"]
    assert len(vis) == 0 and st == [0, 0, 0, 0] and (z == inf).all()
    vis, z, st = out["one_row"]
    assert vis.tolist() == [1] and st == [1, 1, 1, 1] and z[4, 4] == 2.0 and np.isfinite(z).sum() == 1
    vis, z, st = out["behind"]
    assert vis.tolist() == [0, 1, 0] and st[:3] == [1, 1, 1]
    vis, z, st = out["z_zero"]                                   # Z = 0 is not in front: the threshold is strict
    assert vis.tolist() == [0, 0, 1] and st == [1, 1, 1, 4]       # u = v = 4.0 exactly: floor(4 - h) is the pixel before
    vis, z, st = out["nonfinite"]
    assert vis.tolist() == [0, 0, 0, 0, 0, 1] and st[:3] == [1, 1, 1]
    vis, z, st = out["large"]                                    # 10^6 and 10^30 project like any row; 3e38 overflows nothing
    assert vis.tolist() == [1, 1, 0, 0, 0] and st[:3] == [5, 2, 2] and z[5, 4] == float(np.float32(1e30))
    vis, z, st = out["reach_in"]                                 # in front, out of frame, and it still hides the row behind
    assert vis.tolist() == [0, 0] and st[:3] == [2, 1, 0] and z[4, 0] == 1.0
    assert out["reach_in_control"][0].tolist() == [1]
    vis, z, st = out["on_the_lens"]                              # the cap: 33 x 33 pixels, not the whole image
    assert st[3] == 33 * 33 and vis.tolist() == [1, 0] and (z[16:49, 16:49] < 1e-5).all() and z[15, 32] == inf
    vis, z, st = out["borders"]                                  # squares of 2.4 pixels, clipped at every border
    assert vis.all() and st[:3] == [6, 6, 6]                     # a centre on a pixel boundary (8.0) covers 6 pixels, not 5
    assert np.isfinite(z[8, :]).tolist() == [True] * 3 + [False] * 10 + [True] * 3
    assert np.isfinite(z[:, 8]).tolist() == [True] * 3 + [False] * 10 + [True] * 3
    assert np.isfinite(z[0, :3]).all() and np.isfinite(z[15, 13:]).all() and st[3] == 4 * 18 + 2 * 9
    vis, z, st = out["image_1x1"]                                # one pixel: the nearest rows within the tolerance
    assert z.shape == (1, 1) and z[0, 0] == 1.0 and vis.tolist() == [1, 0, 0, 1] and st == [4, 3, 2, 1]
    vis, z, st = out["image_7x5"]
    assert z.shape == (5, 7) and vis.tolist() == [1, 1, 1, 0, 0, 1] and st == [6, 5, 4, 19]
    vis, z, st = out["tight_tol"]
    assert vis.tolist() == [0, 0, 1, 0, 0] and st[:3] == [5, 5, 1]
    vis, z, st = out["equal_z"]
    assert vis.tolist() == [1, 1] and st[:3] == [2, 2, 2] and z[4, 4] == 2.0


def test_a_permuted_segment_gives_the_permuted_mask():
    d = VC.batch(3)
    a, b = VC.OFF[-2], VC.OFF[-1]
    x, cam = d["xyz"][a:b], d["cams"][-1]
    args = (64, 64, VC.focal(64), VC.POINT_SIZE, VC.DEPTH_TOL)
    vis, z, st = ref.render_one(x, cam, *args)
    perm = np.random.default_rng(0).permutation(len(x))
    pvis, pz, pst = ref.render_one(x[perm], cam, *args)
    assert 0 < st[2] < st[1] and np.array_equal(pvis, vis[perm]) and pz.tobytes() == z.tobytes() and pst == st
    # the batch call: segment by segment, rows outside the table untouched
    visible, depth, stat = ref.render(d["xyz"], VC.OFF, d["cams"], *args)
    assert np.array_equal(visible[a:b], vis) and stat[-1].tolist() == st and depth.dtype == np.float32
    assert stat[0].tolist() == [0, 0, 0, 0] and np.isinf(depth[0]).all()
    inside = stat[VC.SIZES.index(257)]                           # the camera inside its shell: rows behind it and out of frame
    assert inside[0] < 257 and inside[1] < inside[0]


# ---- the camera helpers --------------------------------------------------------------------------------------------------
def test_camera_helpers():
    from corsair_amd import views as V

    rng = np.random.default_rng(1)
    dirs = list(rng.standard_normal((20, 3))) + [np.array(v, float) for v in ((0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, -1),
                                                                               (1, 1, 1), (1, -1, 0))]
    for d in dirs:
        eye = rng.standard_normal(3)
        cam = V.look_at(eye, eye + 2.5 * d).reshape(3, 4)
        Rm, t = cam[:, :3], cam[:, 3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Rm) - 1.0) <= 1e-15
        assert np.abs(Rm @ eye + t).max() <= 1e-14               # the eye is the camera's origin
        p = Rm @ (eye + 2.5 * d) + t
        assert abs(p[0]) <= 1e-14 and abs(p[1]) <= 1e-14 and abs(p[2] - 2.5 * np.linalg.norm(d)) <= 1e-13   # the centre lies on +z
    cam = V.look_at([0, 0, -2], [0, 0, 0], up=[0, 1, 0]).reshape(3, 4)
    assert np.abs(cam[2, :3] - [0, 0, 1]).max() == 0 and cam[2, 3] == 2.0
    for bad in ((np.zeros(3), np.zeros(3), None), ([0, 0, 0], [0, 0, 1], [0, 0, 2])):
        with pytest.raises(ValueError):
            V.look_at(*bad)
    assert abs(V.focal_from_fov(256, 90.0) - 128.0) < 1e-12 and abs(V.focal_from_fov(64, 50.0) - 32.0 / math.tan(math.radians(25))) < 1e-12
    for fov in (0.0, 180.0, -5.0, float("nan")):
        with pytest.raises(ValueError):
            V.focal_from_fov(64, fov)
    lo, hi = np.array([[-1.0, -2.0, -2.0], [0, 0, 0]]), np.array([[1.0, 2.0, 2.0], [2, 2, 2]])
    cams = V.view_cameras(lo, hi, [[0, 0, 5.0], [1, 1, 1]], 3.0).reshape(2, 3, 4)
    eye0 = -cams[0][:, :3].T @ cams[0][:, 3]
    assert np.abs(eye0 - [0, 0, 9.0]).max() < 1e-12              # half diagonal 3, distance 3
    mid1 = cams[1][:, :3] @ np.ones(3) + cams[1][:, 3]
    assert abs(mid1[0]) < 1e-12 and abs(mid1[1]) < 1e-12 and abs(mid1[2] - 3.0 * math.sqrt(3.0)) < 1e-12
    with pytest.raises(ValueError):
        V.view_cameras(lo, lo, [[0, 0, 1], [0, 0, 1]], 3.0)
    assert list(inspect.signature(V.render_views).parameters) == ["xyz", "offsets", "cams", "width", "height", "focal",
                                                                  "point_size", "depth_tol", "return_depth"]
    assert V.ViewResult._fields == ("visible", "stat", "depth") and V.FAMILY == "view"
    assert V.torch is __import__("torch") and not hasattr(__import__("corsair_amd.backend").backend, "render_views")
    with pytest.raises(Exception, match="device tensor"):
        V.render_views(__import__("torch").zeros((4, 3)), [0, 4], None, 8, 8, 8.0, 0.1, 0.1)


# ---- shapenet_eval ---------------------------------------------------------------------------------------------------------
def test_config_and_parser():
    from corsair_amd import shapenet_eval as SE

    c = SE.Config()
    assert (c.partial_view, c.view_fov_deg, c.view_size, c.view_distance, c.view_point_size, c.view_depth_tol) == \
        (False, 40, 256, 3.0, 1.5, 1.5)
    c.check_partial_view()
    SE.Config(partial_view=True, view_fov_deg=179.0, view_size=1, view_distance=1.01, view_point_size=0.1,
              view_depth_tol=9.0).check_partial_view()
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(partial_view=1), "partial_view"), (dict(view_fov_deg=0.0), "view_fov_deg"),
                     (dict(view_fov_deg=180.0), "view_fov_deg"), (dict(view_fov_deg=nan), "view_fov_deg"),
                     (dict(view_size=0), "view_size"), (dict(view_size=4097), "view_size"), (dict(view_size=64.0), "view_size"),
                     (dict(view_distance=1.0), "view_distance"), (dict(view_distance=inf), "view_distance"),
                     (dict(view_point_size=0.0), "view_point_size"), (dict(view_point_size=nan), "view_point_size"),
                     (dict(view_depth_tol=-1.0), "view_depth_tol"), (dict(view_depth_tol="a"), "view_depth_tol")):
        with pytest.raises(ValueError, match=word):
            SE.Config(**kw).check_partial_view()
    a = SE.build_parser().parse_args([])
    assert (a.partial_view, a.view_fov, a.view_size, a.view_distance, a.view_point_size, a.view_depth_tol) == \
        (False, 40.0, 256, 3.0, 1.5, 1.5)
    a = SE.build_parser().parse_args(["--partial-view", "--view-fov", "60", "--view-size", "128", "--view-distance", "2.5",
                                      "--view-point-size", "2", "--view-depth-tol", "1"])
    assert (a.partial_view, a.view_fov, a.view_size, a.view_distance, a.view_point_size, a.view_depth_tol) == \
        (True, 60.0, 128, 2.5, 2.0, 1.0)
    help_text = " ".join(SE.build_parser().format_help().split())
    assert help_text.count("untuned, no real scan measured") >= 9
    with pytest.raises(ValueError, match="view_size"):           # evaluate checks the fields before it touches a device
        SE.evaluate(None, [], SE.Config(partial_view=True, view_size=0))
    assert SE.VIEW_CSV_COLUMNS == ("visible_share",) and SE.VIEW_MIN_ROWS == 10


def test_the_pose_list_does_not_see_the_option():
    from corsair_amd import shapenet_eval as SE

    rng = np.random.default_rng(2)
    clouds = [rng.standard_normal((50, 3)).astype(np.float32), rng.standard_normal((70, 3))]
    label = lambda pc, thr: 1
    lists = []
    for on in (False, True):
        cfg = SE.Config(partial_view=on, n_poses_per_model=3)
        jobs = SE.build_jobs(clouds, cfg, np.random.default_rng(cfg.random_seed), label)
        lists.append(b"".join(j[4].tobytes() + j[3].tobytes() for j in jobs))
        assert [(j[0], j[1]) for j in jobs] == [(m, p) for m in range(2) for p in range(3)]
    assert lists[0] == lists[1]
    # the directions come from (seed, job index) alone: the same for a job wherever its batch begins, different per job and seed
    d = [SE.view_direction(31, j) for j in range(4)]
    assert all(abs(np.linalg.norm(v) - 1.0) < 1e-15 for v in d) and np.array_equal(d[2], SE.view_direction(31, 2))
    assert not np.array_equal(d[0], d[1]) and not np.array_equal(d[0], SE.view_direction(32, 0))
    state = np.random.default_rng(31).bit_generator.state
    g = np.random.default_rng(31)
    SE.view_direction(31, 0)
    assert g.bit_generator.state == state
    src = inspect.getsource(SE.partial_views)
    assert "rng" not in src and src.count("select_rows") >= 1 and ".cpu()" not in src and "synchronize" not in src


# ---- sources and documents -------------------------------------------------------------------------------------------------
def test_source_layout_and_documents():
    header = open(os.path.join(ROOT, "include", "corsair_hip.h")).read()
    assert "int cs_render_views(" in header and '"view"' in header
    at = header.index("cs_render_views:")
    block = " ".join(header[at:header.index("int cs_render_views(")].split())
    for words in ("fma(R_c2, z, fma(R_c1, y, fma(R_c0, x, t_c)))", "min(((0.5 * focal) * point_size) / Z, 16.0)", "33 x 33",
                  "IN FRONT", "IN FRAME", "u64 atomicMin", "Z - zbuf[s,cv,cu] < depth_tol", "SET of its rows", "Grazing",
                  "CS_VIEW_CHUNK_BYTES", "hidden_point_removal", "[-1, width]"):
        assert words in block, words
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    text = open(os.path.join(csrc, "view.hip")).read()
    for word in ("hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "hipStreamSynchronize", "hipDeviceSynchronize",
                 "atomicCAS", "hipMalloc(", "atomicAdd(float", "atomicAdd(double"):
        assert word not in text, word
    assert "atomicMin(" in text and "atomicAdd(" in text and "PoolBuf<" in text and 'ProfScope prof("view"' in text
    assert '#include "view_plan.h"' in text
    plan = open(os.path.join(csrc, "view_plan.h")).read()
    assert "#include <hip" not in plan and "__global__" not in plan and "common.h" not in plan   # plain C++: the sanitizer program builds it
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "view.hip" in make and "view.o: nn_common.h view_plan.h" in make
    assert '"view"' in open(os.path.join(csrc, "runtime.hip")).read()
    backend = open(os.path.join(ROOT, "corsair_amd", "backend.py")).read()
    assert "render_views" not in backend
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for words in ("cs_render_views", "--partial-view", "untuned, no real scan measured"):
        assert words in readme, words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 26." in design and "cs_render_views" in design and "not measured" in design.lower() and "Katz" in design
    for name, word in (("INTEGRATION.md", "CS_VIEW_CHUNK_BYTES"), ("tools/README.md", "view_bench.py"),
                       ("tools/README.md", "partial_view_eval.py"), ("tools/README.md", "view_plan_check.cpp")):
        assert word in open(os.path.join(ROOT, name)).read(), name


def test_library_exports_and_refusals_without_a_device():
    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    sigs = _lib._declare(lib)
    assert "cs_render_views" in sigs and "cs_render_views" in set(_lib.header_symbols())
    INVALID, UNSUPPORTED = -1, -5
    off0 = (ctypes.c_int64 * 2)(0, 0)
    one = (ctypes.c_int64 * 2)(0, 4)
    bad = (ctypes.c_int64 * 2)(5, 2)
    neg = (ctypes.c_int64 * 2)(-1, 2)
    huge = (ctypes.c_int64 * 2)(0, 1 << 31)
    nan, inf = float("nan"), float("inf")
    f = lib.cs_render_views
    # argument checks come before any device work: a call without segments needs no GPU
    ok = lambda **kw: f(None, kw.get("off", off0), kw.get("n", 0), kw.get("cam"), kw.get("w", 8), kw.get("h", 8),
                        kw.get("focal", 8.0), kw.get("ps", 0.1), kw.get("tol", 0.1), None, None, kw.get("stat"), None)
    assert ok() == 0 and ok(w=1, h=1) == 0 and ok(w=4096, h=4096) == 0
    for v in (0.0, -1.0, nan, inf, -inf):
        assert ok(focal=v) == INVALID and b"focal" in lib.cs_last_error()
        assert ok(ps=v) == INVALID and b"point_size" in lib.cs_last_error()
        assert ok(tol=v) == INVALID and b"depth_tol" in lib.cs_last_error()
    for v in (0, -1, 4097):
        assert ok(w=v) == UNSUPPORTED and b"width" in lib.cs_last_error()
        assert ok(h=v) == UNSUPPORTED and b"height" in lib.cs_last_error()
    assert f(None, None, 0, None, 8, 8, 8.0, 0.1, 0.1, None, None, None, None) == INVALID and b"NULL offset" in lib.cs_last_error()
    assert ok(n=-1) == INVALID and ok(off=bad, n=1) == INVALID and ok(off=neg, n=1) == INVALID
    assert ok(off=huge, n=1) == UNSUPPORTED and b"2^31" in lib.cs_last_error()
    assert ok(n=1) == INVALID and b"d_cam or d_stat" in lib.cs_last_error()            # an empty segment still needs both
    buf = (ctypes.c_double * 16)()
    assert ok(n=1, cam=buf) == INVALID and ok(n=1, stat=buf) == INVALID
    assert ok(off=one, n=1, cam=buf, stat=buf) == INVALID and b"d_xyz or d_visible" in lib.cs_last_error()
