"""Shared input builders for the parity tests (seeded, small enough for the CPU oracle)."""
import numpy as np

from corsair_amd import synth
from oracle import sparse


def make_batch(cloud_ids, n_points=10000, voxel=0.03, pose_ids=None):
    """Quantised + collated batch like CustomizeCADLib.collate_pair_fn (utils/Info/CADLib.py:148-178):
    returns coords int32 [N,4], feats f32 [N,1], origins f32 [N,3], offsets list."""
    grids, origins = [], []
    for j, cid in enumerate(cloud_ids):
        pc = synth.make_cloud(cid, 15000)[:n_points]
        if pose_ids is not None and pose_ids[j] is not None:
            pc = synth.apply_pose(pc, synth.random_pose(pose_ids[j], max_trans=0.0))
        xyz, grid, _ = sparse.quantize_cloud(pc, voxel)
        grids.append(grid)
        origins.append(xyz)
    coords = sparse.sparse_collate(grids)
    feats = np.ones((coords.shape[0], 1), np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in grids])]).tolist()
    return coords, feats, np.concatenate(origins, 0).astype(np.float32), offsets


LEGS = {4: np.array([[0.3, 0, 0.3], [-0.3, 0, 0.3], [-0.3, 0, -0.3], [0.3, 0, -0.3]]),
        2: np.array([[0.3, 0, 0.1], [-0.3, 0, -0.1]])}


def legged_object(seed, n_legs, n_per_leg=400):
    """A 2- or 4-legged object (legs parallel to y, 4 legs = 4-fold symmetric about y) whose 16-d
    'features' encode only the height of a point: the 50 feature-NN of an anchor are one slice of every
    leg, so symmetric_cut4's k-means finds the legs and its gate opens (utils/symmetry.py:232-243), while
    the vanilla 5-NN correspondences of find_kcorr land on a random leg (1/n_legs of them consistent with
    any one pose).  Returns (xyz f32 [n,3], feat f32 [n,16])."""
    rng = np.random.default_rng(seed)
    pts, feat = [], []
    for leg in LEGS[n_legs]:
        h = rng.uniform(-0.5, 0.5, n_per_leg)
        pts.append(leg + np.stack([rng.normal(0, 0.01, n_per_leg), h, rng.normal(0, 0.01, n_per_leg)], 1))
        f = np.zeros((n_per_leg, 16))
        f[:, 0] = h
        f[:, 1] = rng.normal(0, 1e-3, n_per_leg)
        feat.append(f)
    xyz = np.concatenate(pts).astype(np.float32)
    F = np.concatenate(feat).astype(np.float32)
    perm = rng.permutation(len(xyz))
    return xyz[perm], F[perm]


def rot_y_pose(deg, trans=(0.05, -0.02, 0.03)):
    t = np.deg2rad(deg)
    c, s = np.cos(t), np.sin(t)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = trans
    return T


# ---- the ICP units' source text ------------------------------------------------------------------
ICP_UNITS = ("icp.h", "icp_sums.h", "icp_assoc.hip", "icp_step.hip", "icp.hip")
ICP_KERNELS = ["k_icp_exact", "k_icp_f16", "k_icp_frame", "k_icp_init", "k_icp_step"]


def icp_unit_texts():
    """{file name: text} of the five files the batched ICP is made of (corsair_amd/csrc)."""
    import os

    from corsair_amd import _lib

    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    return {n: open(os.path.join(csrc, n)).read() for n in ICP_UNITS}


def assert_five_icp_kernels():
    """No estimation adds a kernel: over the ICP units together the kernel DEFINITIONS (not mentions in comments) are the five
    of ICP_KERNELS, each once, the host unit has none, and the estimation is still a template argument of the sums and the
    step."""
    import re

    units = icp_unit_texts()
    text = "\n".join(units.values())
    kernels = re.findall(r"^__global__ [^\n]*?void (k_\w+)\(", text, flags=re.M)
    assert sorted(kernels) == ICP_KERNELS
    assert text.count("__global__") == 5
    assert "__global__" not in units["icp.hip"]
    assert "icp_block_sums<EST>" in text and "k_icp_step<EST>" in text


# ---- the k-NN units' source text -------------------------------------------------------------------------------
KNN_UNITS = ("knn.h", "knn_exact.hip", "knn_f16.hip", "knn.hip")
KNN_KERNELS = ["k_count_flags", "k_knf_pack_queries", "k_knf_pack_targets", "k_knn_f16", "k_knn_feat", "k_knn_rescore_f16",
               "k_label_starts", "k_seg_keys"]


def assert_eight_knn_kernels():
    """cs_knn_feat has two paths and no third: over the k-NN units together the kernel DEFINITIONS (not mentions in comments)
    are the eight of KNN_KERNELS, each once, the shared header has none, and the radix sort's library is included by one unit."""
    import os
    import re

    from corsair_amd import _lib

    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    units = {n: open(os.path.join(csrc, n)).read() for n in KNN_UNITS}
    text = "\n".join(units.values())
    kernels = re.findall(r"^__global__ [^\n]*?void (k_\w+)\(", text, flags=re.M)
    assert sorted(kernels) == KNN_KERNELS
    assert text.count("__global__") == len(KNN_KERNELS)
    assert "__global__" not in units["knn.h"]
    assert [n for n in KNN_UNITS if re.search(r"^\s*#\s*include\s*<hipcub", units[n], flags=re.M)] == ["knn_f16.hip"]
    assert "hipcub" not in "".join(units[n] for n in KNN_UNITS if n != "knn_f16.hip")


# ---- the 3-d f16 ranking scan's source text ----------------------------------------------------------------------
CHAMFER_KERNELS = ["k_chamfer", "k_chamfer2", "k_chamfer_f16", "k_chamfer_finish", "k_chamfer_mfma", "k_chamfer_pack",
                   "k_chamfer_pack16"]


def assert_one_chf_rank_scan():
    """k_chamfer_f16 and k_icp_f16 share ONE scan: the f16 MFMA over the CHF_PITCH image stands in chf_rank.h and in neither
    kernel's file, the CHF_* constants are defined in one file, and chamfer.hip defines its seven kernels, each once."""
    import glob
    import os
    import re

    from corsair_amd import _lib

    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    text = {os.path.basename(p): open(p).read() for ext in ("*.h", "*.hip") for p in glob.glob(os.path.join(csrc, ext))}
    mfma = "__builtin_amdgcn_mfma_f32_32x32x16_f16"
    assert mfma in text["chf_rank.h"] and "CHF_PITCH" in text["chf_rank.h"]
    assert mfma not in text["chamfer.hip"] and mfma not in text["icp_assoc.hip"]
    define = r"constexpr[^;\n]*?\b(CHF_\w+)\s*=|#\s*define\s+(CHF_\w+)"
    defined = {n: sorted(a or b for a, b in re.findall(define, t)) for n, t in text.items()}
    assert {n: d for n, d in defined.items() if d} == {"chf_rank.h": ["CHF_NG", "CHF_PITCH", "CHF_ROWS", "CHF_SCALE"]}
    kernels = re.findall(r"^__global__ [^\n]*?void (k_\w+)\(", text["chamfer.hip"], flags=re.M)
    assert sorted(kernels) == CHAMFER_KERNELS
    assert text["chamfer.hip"].count("__global__") == len(CHAMFER_KERNELS)
    assert "__global__" not in text["chf_rank.h"]


# ---- operator-level contract tests: column views of wider buffers ------------------------------------------
# A quiet NaN whose payload no arithmetic produces: a buffer filled with it shows both a stray WRITE (the bits
# change) and a stray READ (a NaN reaches the result).
SENTINEL_BITS = 0x7FC5A5A5


def sentinel_buffer(n, ld, device):
    """f32 [n, ld] device buffer, every element SENTINEL_BITS."""
    import torch

    return torch.full((n, ld), SENTINEL_BITS, dtype=torch.int32, device=device).view(torch.float32)


def column_view(values, device, col0=0, ld=None):
    """values (f32 ndarray [n, c]) as columns col0 .. col0 + c of a sentinel-filled [n, ld] device buffer: returns
    (wide buffer, the view).  ld None: a plain contiguous tensor (wide is the tensor itself)."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(device)
    if ld is None:
        return t, t
    n, c = values.shape
    assert col0 + c <= ld
    wide = sentinel_buffer(n, ld, device)
    wide[:, col0:col0 + c] = t
    view = wide[:, col0:col0 + c]
    assert n <= 1 or view.stride(0) == ld
    return wide, view


def outside_view_untouched(wide, col0, c):
    """Every element of the sentinel-filled buffer outside columns col0 .. col0 + c still holds SENTINEL_BITS."""
    import torch

    bits = wide.view(torch.int32).cpu().numpy()
    mask = np.ones(bits.shape, bool)
    mask[:, col0:col0 + c] = False
    return bool((bits[mask] == SENTINEL_BITS).all())


EPILOGUES = [(mode, res, relu) for mode in ("scale+shift", "shift", "none") for res in (False, True)
             for relu in (False, True)]   # the twelve combinations of include/corsair_hip.h


def epilogue_args(rng, n, c, combo):
    """(scale, shift, residual, relu) ndarrays / None for one of EPILOGUES; values of mixed sign so that ReLU bites."""
    mode, res, relu = combo
    scale = rng.uniform(-1.5, 1.5, c).astype(np.float32) if mode == "scale+shift" else None
    shift = rng.standard_normal(c).astype(np.float32) if mode != "none" else None
    residual = rng.standard_normal((n, c)).astype(np.float32) if res else None
    return scale, shift, residual, relu
