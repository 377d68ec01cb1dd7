"""Thin torch-tensor front ends of the C ABI (include/corsair_hip.h).

Everything here launches hand-written HIP kernels through libcorsair_hip.so; torch only owns the
device buffers and the stream.  No CPU fallback: inputs must be CUDA(HIP) tensors.
"""
from __future__ import annotations

import ctypes
from ctypes import c_void_p
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, i32_array, i64_array, ptr, stream_ptr

KERNEL_VOLUME = 27


def _dev(t, dtype, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.CorsairHipError(f"{what} must be a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, got {t.dtype}")
    return t


def _rows(t, what):
    """(tensor, leading dimension) of a 2-D tensor whose rows are contiguous."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{what} must be 2-D with unit inner stride")
    return t, t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


class CoordMap:
    """Owns one cs_coordmap handle (coordinates of one tensor stride + hash index)."""

    def __init__(self, handle, device):
        self._h = c_void_p(handle)
        self.device = device
        lib = _lib.load()
        self.n = int(lib.cs_coordmap_size(self._h))
        self.tensor_stride = int(lib.cs_coordmap_tensor_stride(self._h))
        self._coords = None

    @classmethod
    def create(cls, coords, tensor_stride=1):
        _lib.require_gpu()
        coords = _dev(coords, torch.int32, "coordinates").contiguous()
        if coords.dim() != 2 or coords.shape[1] != 4:
            raise ValueError("coordinates must be int32 [N, 4] (batch, x, y, z)")
        out = c_void_p()
        check(_lib.load().cs_coordmap_create(ptr(coords), coords.shape[0], tensor_stride,
                                             stream_ptr(), ctypes.byref(out)))
        return cls(out.value, coords.device)

    @classmethod
    def pyramid(cls, coords, n_levels=4, n_batch=0, tensor_stride=1):
        """The maps of tensor strides ts, 2 ts, 4 ts, ... in ONE library call (cs_coordmap_pyramid): the same maps as
        create() followed by chained stride(2) calls, with one host wait instead of one per level.  n_batch > 0 announces
        sparse_collate's order (rows grouped by sample, batch indices < n_batch)."""
        _lib.require_gpu()
        coords = _dev(coords, torch.int32, "coordinates").contiguous()
        if coords.dim() != 2 or coords.shape[1] != 4:
            raise ValueError("coordinates must be int32 [N, 4] (batch, x, y, z)")
        outs = (c_void_p * n_levels)()
        check(_lib.load().cs_coordmap_pyramid(ptr(coords), coords.shape[0], tensor_stride, n_levels, int(n_batch or 0),
                                              stream_ptr(), outs))
        return [cls(h, coords.device) for h in outs]

    def stride(self, s=2):
        out = c_void_p()
        check(_lib.load().cs_coordmap_stride(self._h, s, stream_ptr(), ctypes.byref(out)))
        return CoordMap(out.value, self.device)

    @property
    def coords(self):
        """int32 [n,4] device tensor (a copy owned by torch)."""
        if self._coords is None:
            t = torch.empty((self.n, 4), dtype=torch.int32, device=self.device)
            if self.n:
                src = _lib.load().cs_coordmap_coords(self._h)
                _hip_memcpy_d2d(t.data_ptr(), src, self.n * 16)
            self._coords = t
        return self._coords

    def __del__(self):
        try:
            if self._h:
                _lib.load().cs_coordmap_free(self._h)
                self._h = None
        except Exception:
            pass


def _hip_memcpy_d2d(dst, src, nbytes):
    # tiny helper through torch: wrap the library-owned memory without taking ownership
    import ctypes as C

    hip = _hip_runtime()
    rc = hip.hipMemcpyAsync(c_void_p(dst), c_void_p(src), C.c_size_t(nbytes), 3,
                            c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _lib.CorsairHipError(f"hipMemcpyAsync failed with {rc}")


_hip = None


def _hip_runtime():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
    return _hip


class KernelMap:
    """Owns one cs_kernelmap handle (int32 [n_out,27] neighbour table on the device)."""

    def __init__(self, handle, in_map, out_map, transposed, kernel_size=3):
        self._h = c_void_p(handle)
        self.kvol = int(kernel_size) ** 3
        lib = _lib.load()
        self.n_out = int(lib.cs_kernelmap_rows(self._h))
        self.n_in = in_map.n
        self._num_pairs = None
        self.transposed = transposed
        # stride 1 (in map == out map): the data gradient runs on this same map with mirrored offsets (conv_dgrad)
        self.stride1 = not transposed and in_map.tensor_stride == out_map.tensor_stride
        self.device = in_map.device

    @property
    def num_pairs(self):
        """Resolved on first use: building a map does not wait for its pair count."""
        if self._num_pairs is None:
            self._num_pairs = int(_lib.load().cs_kernelmap_num_pairs(self._h))
        return self._num_pairs

    @classmethod
    def build(cls, in_map, out_map, kernel_size=3, transposed=False):
        out = c_void_p()
        check(_lib.load().cs_kernelmap_build(in_map._h, out_map._h, kernel_size,
                                             1 if transposed else 0, stream_ptr(),
                                             ctypes.byref(out)))
        return cls(out.value, in_map, out_map, transposed, kernel_size)

    @classmethod
    def build_many(cls, specs):
        """The kernel maps of one batch in one library call (cs_kernelmap_build_many: independent chains on up to three
        streams).  specs: (in_map, out_map[, kernel_size[, transposed]]) tuples; returns the maps in that order."""
        full = [(sp[0], sp[1], sp[2] if len(sp) > 2 else 3, bool(sp[3]) if len(sp) > 3 else False) for sp in specs]
        n = len(full)
        if n == 0:
            return []
        VP, CI = c_void_p * n, ctypes.c_int * n
        ins = VP(*[sp[0]._h.value for sp in full])
        outs = VP(*[sp[1]._h.value for sp in full])
        ks = CI(*[int(sp[2]) for sp in full])
        tr = CI(*[1 if sp[3] else 0 for sp in full])
        kms = VP()
        check(_lib.load().cs_kernelmap_build_many(n, ins, outs, ks, tr, stream_ptr(), kms))
        return [cls(kms[i], full[i][0], full[i][1], full[i][3], full[i][2]) for i in range(n)]

    def export(self):
        """Canonical (k, in_row, out_row) int32 triples sorted by (k, out_row)."""
        n = max(self.num_pairs, 1)
        k = torch.empty(n, dtype=torch.int32, device=self.device)
        i = torch.empty(n, dtype=torch.int32, device=self.device)
        o = torch.empty(n, dtype=torch.int32, device=self.device)
        got = check(_lib.load().cs_kernelmap_export(self._h, ptr(k), ptr(i), ptr(o), n, stream_ptr()))
        return k[:got], i[:got], o[:got]

    def table(self):
        t = torch.empty((self.n_out, KERNEL_VOLUME), dtype=torch.int32, device=self.device)
        if self.n_out:
            _hip_memcpy_d2d(t.data_ptr(), _lib.load().cs_kernelmap_table(self._h), self.n_out * 27 * 4)
        return t

    def __del__(self):
        try:
            if self._h:
                _lib.load().cs_kernelmap_free(self._h)
                self._h = None
        except Exception:
            pass


def conv_fwd(kmap, x, weight, scale=None, shift=None, residual=None, relu=False, out=None,
             n_out=None):
    """Sparse convolution forward with fused epilogue (cs_conv_fwd).  x/out/residual may be column
    slices of wider row-major buffers."""
    x, ld_in = _rows(_dev(x, torch.float32, "input features"), "input features")
    weight = _dev(weight, torch.float32, "kernel").contiguous()
    if weight.dim() == 2:
        cin, cout = weight.shape
    else:
        cin, cout = weight.shape[1], weight.shape[2]
    if x.shape[1] != cin:
        raise ValueError(f"input has {x.shape[1]} channels, kernel expects {cin}")
    n_in = x.shape[0]
    if kmap is None:
        n_out = n_in
    else:
        n_out = kmap.n_out
    if out is None:
        out = torch.empty((n_out, cout), dtype=torch.float32, device=x.device)
    out, ld_out = _rows(out, "output")
    if out.shape[0] != n_out or out.shape[1] != cout:
        raise ValueError("output buffer has the wrong shape")
    ld_res = 0
    if residual is not None:
        residual, ld_res = _rows(_dev(residual, torch.float32, "residual"), "residual")
    check(_lib.load().cs_conv_fwd(kmap._h if kmap is not None else None, n_in, n_out, ptr(x), ld_in,
                                  cin, ptr(weight), cout, ptr(scale), ptr(shift), ptr(residual),
                                  ld_res, 1 if relu else 0, ptr(out), ld_out, stream_ptr()))
    return out


def conv_wgrad(kmap, x, g):
    """Weight gradient of conv_fwd(kmap, x, W) for the output gradient g (cs_conv_wgrad): [27, cin, cout], or
    [cin, cout] for kernel size 1 (kmap None, or a strided / transposed map of kernel size 1).  x and g may be
    column slices of wider row-major buffers."""
    x, ld_in = _rows(_dev(x, torch.float32, "input features"), "input features")
    g, ld_g = _rows(_dev(g, torch.float32, "output gradient"), "output gradient")
    n_in, cin = x.shape
    n_out, cout = g.shape
    if kmap is not None and (kmap.n_in, kmap.n_out) != (n_in, n_out):
        raise ValueError(f"kernel map is for {kmap.n_in} -> {kmap.n_out} rows, tensors have {n_in} -> {n_out}")
    kvol = 1 if kmap is None else kmap.kvol
    dw = torch.empty((cin, cout) if kvol == 1 else (kvol, cin, cout), dtype=torch.float32, device=x.device)
    check(_lib.load().cs_conv_wgrad(kmap._h if kmap is not None else None, n_in, n_out, ptr(x), ld_in, cin, ptr(g),
                                    ld_g, cout, ptr(dw), stream_ptr()))
    return dw


def dgrad_weight(kmap, weight):
    """W' of the data gradient: conv_fwd(reverse map, gY, W') = dL/dx of conv_fwd(kmap, x, W).  With
    k = (dx+1) + 3(dy+1) + 9(dz+1) mirroring an offset maps k to 26 - k:
      stride 1 (the map is its own reverse, T[T[o][k]][26-k] = o):   W'[k] = W[26-k]^T
      strided / transposed (reverse = the other map, same k):        W'[k] = W[k]^T
      kernel size 1 (kmap None, or a strided / transposed map):      W' = W^T"""
    if kmap is None or kmap.kvol == 1:
        return weight.reshape(weight.shape[-2:]).t().contiguous()
    if kmap.stride1:
        return weight.flip(0).transpose(1, 2).contiguous()
    return weight.transpose(1, 2).contiguous()


def conv_dgrad(kmap, rev_kmap, g, weight):
    """Input gradient of conv_fwd(kmap, x, weight) for the output gradient g: cs_conv_fwd on the reverse map
    (no kernel of its own).  rev_kmap: for a stride-1 map the map itself (None is accepted), for a strided map
    (fine -> coarse) the transposed map coarse -> fine, for a transposed map the strided map fine -> coarse;
    ignored for kmap None (1x1)."""
    wt = dgrad_weight(kmap, weight)
    if kmap is None:
        return conv_fwd(None, g, wt)
    if kmap.stride1:
        rev_kmap = kmap if rev_kmap is None else rev_kmap
    if rev_kmap is None or (rev_kmap.n_in, rev_kmap.n_out, rev_kmap.kvol) != (kmap.n_out, kmap.n_in, kmap.kvol):
        raise ValueError("conv_dgrad: the reverse map must take the forward's output rows to its input rows")
    return conv_fwd(rev_kmap, g, wt)


def affine_act(x, scale=None, shift=None, residual=None, relu=False, out=None):
    x, ld_in = _rows(_dev(x, torch.float32, "input"), "input")
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    out, ld_out = _rows(out, "output")
    ld_res = 0
    if residual is not None:
        residual, ld_res = _rows(residual, "residual")
    check(_lib.load().cs_affine_act(x.shape[0], x.shape[1], ptr(x), ld_in, ptr(scale), ptr(shift),
                                    ptr(residual), ld_res, 1 if relu else 0, ptr(out), ld_out,
                                    stream_ptr()))
    return out


def row_l2_normalize(x, eps=0.0, out=None):
    if out is None and torch.is_grad_enabled() and x.requires_grad:   # training: same kernel, with a backward
        from .autograd import RowL2NormalizeFunction

        return RowL2NormalizeFunction.apply(x, float(eps))
    x, ld_in = _rows(_dev(x, torch.float32, "input"), "input")
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    out, ld_out = _rows(out, "output")
    check(_lib.load().cs_row_l2_normalize(x.shape[0], x.shape[1], ptr(x), ld_in, float(eps), ptr(out),
                                          ld_out, stream_ptr()))
    return out


def segmented_max(x, coords, n_batch):
    """Per-sample column max; `coords` is the int32 [n,4] coordinate tensor (batch in column 0)."""
    if torch.is_grad_enabled() and x.requires_grad:   # training: same kernel, gradient to the first maximal row
        from .autograd import SegmentedMaxFunction

        return SegmentedMaxFunction.apply(x, coords, int(n_batch))
    x, ld_in = _rows(_dev(x, torch.float32, "input"), "input")
    coords = _dev(coords, torch.int32, "coords")
    out = torch.empty((n_batch, x.shape[1]), dtype=torch.float32, device=x.device)
    check(_lib.load().cs_segmented_max(x.shape[0], x.shape[1], ptr(x), ld_in, ptr(coords),
                                       coords.stride(0), n_batch, ptr(out), stream_ptr()))
    return out


def instance_norm(x, seg, weight=None, bias=None, eps=1e-8, out=None):
    """cs_instance_norm: x f32 [n,c] rows grouped by sample, seg int32 [n_batch+1] device row offsets.  x and out
    may be column slices of wider row-major buffers."""
    x, ld_in = _rows(_dev(x, torch.float32, "input"), "input")
    seg = _dev(seg, torch.int32, "segment offsets").contiguous()
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    out, ld_out = _rows(_dev(out, torch.float32, "output"), "output")
    if out.shape != x.shape:
        raise ValueError("instance_norm: output buffer has the wrong shape")
    w = _dev(weight, torch.float32, "weight").contiguous().reshape(-1) if weight is not None else None
    b = _dev(bias, torch.float32, "bias").contiguous().reshape(-1) if bias is not None else None
    for t, name in ((w, "weight"), (b, "bias")):
        if t is not None and t.numel() != x.shape[1]:
            raise ValueError("instance_norm: %s must have %d entries" % (name, x.shape[1]))
    check(_lib.load().cs_instance_norm(x.shape[0], x.shape[1], ptr(x), ld_in, ptr(seg), seg.numel() - 1,
                                       ptr(w) if w is not None else None, ptr(b) if b is not None else None,
                                       float(eps), ptr(out), ld_out, stream_ptr()))
    return out


def voxelize(xyz, offsets, voxel_size):
    """cs_voxelize / cs_voxelize_f64: xyz f32 or f64 [n,3] device, offsets host list.  The grid index is
    floor(x / voxel) in the cloud's own type, like the reference's NumPy expression: f32 for the catalog
    clouds (utils/Info/CADLib.py:106-121), f64 for posed queries (datasets/CategoryDataset.py:179-197,
    evaluation-shapenet.py:97-119).  Returns (keep_idx int64 [m], grid int32 [m,4], out_offsets list)."""
    f64 = torch.is_tensor(xyz) and xyz.dtype == torch.float64
    xyz = _dev(xyz, torch.float64 if f64 else torch.float32, "xyz").contiguous()
    n = xyz.shape[0]
    nseg = len(offsets) - 1
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=xyz.device)
    grid = torch.empty((max(n, 1), 4), dtype=torch.int32, device=xyz.device)
    h_off = i64_array(offsets)
    h_out = (ctypes.c_int64 * (nseg + 1))()
    fn = _lib.load().cs_voxelize_f64 if f64 else _lib.load().cs_voxelize
    check(fn(ptr(xyz), h_off, nseg, float(voxel_size), ptr(keep), ptr(grid), h_out, stream_ptr()))
    out_off = [int(v) for v in h_out]
    m = out_off[-1]
    return keep[:m], grid[:m], out_off


class TopkCatalog:
    """A fixed retrieval library (cs_topk_catalog): what the matrix-core top-k derives from the catalog rows is made once
    and reused by every l2_topk against it.  Holds a reference to the descriptor tensor."""

    def __init__(self, x):
        self.x = _dev(x, torch.float32, "catalog").contiguous()
        out = c_void_p()
        check(_lib.load().cs_topk_catalog_create(ptr(self.x), self.x.shape[0], self.x.shape[1], stream_ptr(),
                                                 ctypes.byref(out)))
        self._h = out
        self.shape = self.x.shape

    def __del__(self):
        try:
            if self._h:
                _lib.load().cs_topk_catalog_free(self._h)
                self._h = None
        except Exception:
            pass


def l2_topk(q, x, k, return_distance=False, squared=False):
    """x: catalog tensor or TopkCatalog.  squared=True (with return_distance): the squared distances the ranking was
    made on (shard merges)."""
    q = _dev(q, torch.float32, "queries").contiguous()
    idx = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
    dist = torch.empty((q.shape[0], k), dtype=torch.float64, device=q.device) if return_distance else None
    if isinstance(x, TopkCatalog):
        if x.shape[1] != q.shape[1]:
            raise ValueError("query and catalog dimensions differ")
        check(_lib.load().cs_l2_topk_catalog(ptr(q), q.shape[0], x._h, k, ptr(idx), ptr(dist), 1 if squared else 0,
                                             stream_ptr()))
        return (idx, dist) if return_distance else idx
    x = _dev(x, torch.float32, "catalog").contiguous()
    fn = _lib.load().cs_l2_topk_sq if squared else _lib.load().cs_l2_topk
    check(fn(ptr(q), q.shape[0], ptr(x), x.shape[0], q.shape[1], k, ptr(idx), ptr(dist), stream_ptr()))
    return (idx, dist) if return_distance else idx


def knn_feat(qf, qoff, tf, toff, k, qseg=None, tseg=None, qlabel=None, tlabel=None, perm=None,
             return_distance=False):
    """Batched feature k-NN.  qoff/toff: host offset lists of the segment tables; qseg/tseg: per
    problem segment ids (default: problem p uses segment p of both).  perm: int32 [n_prob,8] device
    tensor when labels are used.  Output rows are problem-major."""
    qf = _dev(qf, torch.float32, "query features").contiguous()
    tf = _dev(tf, torch.float32, "target features").contiguous()
    if qseg is None:
        qseg = list(range(len(qoff) - 1))
        tseg = list(range(len(toff) - 1))
    n_prob = len(qseg)
    total = sum(int(qoff[s + 1]) - int(qoff[s]) for s in qseg)
    idx = torch.empty((total, k), dtype=torch.int32, device=qf.device)
    dist = torch.empty((total, k), dtype=torch.float64, device=qf.device) if return_distance else None
    check(_lib.load().cs_knn_feat(ptr(qf), i64_array(qoff), ptr(tf), i64_array(toff), i32_array(qseg),
                                  i32_array(tseg), n_prob, qf.shape[1], k, ptr(qlabel), ptr(tlabel),
                                  ptr(perm), ptr(idx), ptr(dist), stream_ptr()))
    return (idx, dist) if return_distance else idx


def hardest_negatives(qf, qxyz, qoff, tf, txyz, toff, anchors, radius, qseg=None, tseg=None, return_distance=False):
    """cs_hardest_negatives: for every anchor (int32 [A] device, GLOBAL rows of qf) the feature-nearest row of its
    problem's target segment that is not within `radius` of the anchor's canonical point (radius <= 0: no exclusion).
    qf / tf f32 [n, C] device (unit inner stride, any leading dimension), qxyz / txyz f32 [n, 3] row-aligned with them,
    qoff / toff host offset lists, qseg / tseg per problem segment ids (default: problem p uses segment p of both).
    Returns int32 [A] rows LOCAL to the target segment (-1: no admissible row) and, with return_distance, the f64
    feature distances (+inf for -1).  No host wait."""
    qf, ld_q = _rows(_dev(qf, torch.float32, "query features"), "query features")
    tf, ld_t = _rows(_dev(tf, torch.float32, "target features"), "target features")
    qxyz = _dev(qxyz, torch.float32, "query points").contiguous()
    txyz = _dev(txyz, torch.float32, "target points").contiguous()
    anchors = _dev(anchors, torch.int32, "anchors").contiguous()
    if qf.shape[1] != tf.shape[1]:
        raise ValueError("hardest_negatives: query and target widths differ")
    if qxyz.shape != (qf.shape[0], 3) or txyz.shape != (tf.shape[0], 3):
        raise ValueError("hardest_negatives: points must be [n, 3], one row per feature row")
    if anchors.dim() != 1:
        raise ValueError("hardest_negatives: anchors must be 1-D")
    if qseg is None:
        qseg = list(range(len(qoff) - 1))
        tseg = list(range(len(toff) - 1))
    if len(qseg) != len(tseg):
        raise ValueError("hardest_negatives: qseg and tseg differ in length")
    if qseg and (int(qoff[max(qseg) + 1]) > qf.shape[0] or int(toff[max(tseg) + 1]) > tf.shape[0]):
        raise ValueError("hardest_negatives: the offset tables exceed the feature matrices")
    n = anchors.shape[0]
    idx = torch.empty(n, dtype=torch.int32, device=qf.device)
    dist = torch.empty(n, dtype=torch.float64, device=qf.device) if return_distance else None
    check(_lib.load().cs_hardest_negatives(ptr(qf), ld_q, ptr(qxyz), i64_array(qoff), ptr(tf), ld_t, ptr(txyz),
                                           i64_array(toff), i32_array(qseg), i32_array(tseg), len(qseg),
                                           int(qf.shape[1]), ptr(anchors), n, float(radius), ptr(idx), ptr(dist),
                                           stream_ptr()))
    return (idx, dist) if return_distance else idx


def hardest_stats(reset=False):
    """cs_hardest_stats: (anchors answered, of those recomputed exhaustively); counts only under CS_HARDNEG_STATS=1."""
    out = (ctypes.c_uint64 * 2)()
    _lib.load().cs_hardest_stats(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


def chamfer_1dir(src, soff, tgt, toff, src_seg, tgt_seg, T):
    """Batched one-directional Chamfer; T f32 [n_prob,4,4] device.  Returns f64 [n_prob]."""
    src = _dev(src, torch.float32, "source").contiguous()
    tgt = _dev(tgt, torch.float32, "target").contiguous()
    T = _dev(T, torch.float32, "transforms").contiguous()
    n_prob = len(src_seg)
    out = torch.empty(n_prob, dtype=torch.float64, device=src.device)
    check(_lib.load().cs_chamfer_1dir(ptr(src), i64_array(soff), ptr(tgt), i64_array(toff),
                                      i32_array(src_seg), i32_array(tgt_seg), n_prob, ptr(T), ptr(out),
                                      stream_ptr()))
    return out


def chamfer_2dir(src, soff, tgt, toff, src_seg, tgt_seg, T):
    """Batched two-directional Chamfer under one pose per problem (cs_chamfer_2dir; profile family "chamfer2"):
    T f32 [n_prob,4,4] device.  Returns f64 [n_prob,2]: [:, 0] forward (posed source -> target, what chamfer_1dir
    returns), [:, 1] backward (target -> posed source, in the target's frame)."""
    src = _dev(src, torch.float32, "source").contiguous()
    tgt = _dev(tgt, torch.float32, "target").contiguous()
    T = _dev(T, torch.float32, "transforms").contiguous()
    n_prob = len(src_seg)
    if len(tgt_seg) != n_prob or T.numel() != 16 * n_prob:
        raise ValueError("chamfer_2dir: %d source segments, %d target segments, %d transform entries"
                         % (n_prob, len(tgt_seg), T.numel()))
    if src.dim() != 2 or src.shape[1] != 3 or tgt.dim() != 2 or tgt.shape[1] != 3:
        raise ValueError("chamfer_2dir: clouds must be [n,3]")
    for name, off, seg, rows in (("source", soff, src_seg, src.shape[0]), ("target", toff, tgt_seg, tgt.shape[0])):
        if n_prob and not (0 <= min(seg) and max(seg) + 1 < len(off)):
            raise ValueError("chamfer_2dir: a %s segment id is outside its offset table" % name)
        if n_prob and not (0 <= int(min(off)) and int(max(off)) <= rows):
            raise ValueError("chamfer_2dir: the %s offset table exceeds the cloud (%d rows)" % (name, rows))
    out = torch.empty((n_prob, 2), dtype=torch.float64, device=src.device)
    if n_prob == 0:
        return out
    check(_lib.load().cs_chamfer_2dir(ptr(src), i64_array(soff), ptr(tgt), i64_array(toff),
                                      i32_array(src_seg), i32_array(tgt_seg), n_prob, ptr(T), ptr(out),
                                      stream_ptr()))
    return out


def hausdorff_1dir(src, soff, tgt, toff, src_seg, tgt_seg, T):
    """Batched directed Hausdorff distance (max over source points of the nearest-target distance)."""
    src = _dev(src, torch.float32, "source").contiguous()
    tgt = _dev(tgt, torch.float32, "target").contiguous()
    T = _dev(T, torch.float32, "transforms").contiguous()
    n_prob = len(src_seg)
    out = torch.empty(n_prob, dtype=torch.float64, device=src.device)
    check(_lib.load().cs_hausdorff_1dir(ptr(src), i64_array(soff), ptr(tgt), i64_array(toff),
                                        i32_array(src_seg), i32_array(tgt_seg), n_prob, ptr(T), ptr(out),
                                        stream_ptr()))
    return out


def _packed_points(xyz, offsets, who):
    xyz = _dev(xyz, torch.float32, "points").contiguous()
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("%s: points must be [n, 3]" % who)
    if len(offsets) < 1 or int(offsets[-1]) > xyz.shape[0]:
        raise ValueError("%s: the offset table exceeds the point array" % who)
    return xyz


def orient_normals(xyz, offsets, normals, view=None, away=True):
    """cs_orient_normals, IN PLACE on `normals` (f32 [n,3] device, contiguous): every normal is flipped to point away from
    (away=True) or towards the view point of its segment -- view f64 [n_seg,3] (host or device), or None for the segment's
    centroid (an exact fixed-point sum: a permuted segment gives the same bits).  The semantics are the header comment of
    cs_orient_normals.  Returns `normals`.  No host wait."""
    xyz = _packed_points(xyz, offsets, "orient_normals")
    if normals.dtype != torch.float32 or normals.shape != xyz.shape or not normals.is_contiguous() or \
            normals.device != xyz.device:
        raise ValueError("orient_normals: normals must be a contiguous f32 tensor of the points' shape and device")
    if view is not None:
        view = torch.as_tensor(view, dtype=torch.float64).to(xyz.device).contiguous()
        if tuple(view.shape) != (len(offsets) - 1, 3):
            raise ValueError("orient_normals: view must be [n_seg, 3]")
    check(_lib.load().cs_orient_normals(ptr(xyz), i64_array(offsets), len(offsets) - 1, ptr(view), 1 if away else 0,
                                        ptr(normals), stream_ptr()))
    return normals


def fpfh(xyz, offsets, normals, radius, max_nn=100):
    """cs_fpfh: Fast Point Feature Histograms, f32 [n,33] device, of packed clouds (host offset list) with ORIENTED normals
    (orient_normals), from the at most max_nn - 1 nearest other rows strictly inside `radius`; 4 <= max_nn <= 128.  The
    semantics are the header comment of cs_fpfh.  No host wait."""
    xyz = _packed_points(xyz, offsets, "fpfh")
    normals = _dev(normals, torch.float32, "normals").contiguous()
    if normals.shape != xyz.shape:
        raise ValueError("fpfh: normals must have the shape of the points")
    out = torch.zeros((xyz.shape[0], 33), dtype=torch.float32, device=xyz.device)
    check(_lib.load().cs_fpfh(ptr(xyz), ptr(normals), i64_array(offsets), len(offsets) - 1, float(radius), int(max_nn),
                              ptr(out), stream_ptr()))
    return out


def fpfh_stats(reset=False):
    """cs_fpfh_stats: (neighbours found, rows whose on-chip list was ranked in parts); counts only under CS_FPFH_STATS=1."""
    out = (ctypes.c_uint64 * 2)()
    _lib.load().cs_fpfh_stats(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


class IcpResult(NamedTuple):
    T: torch.Tensor          # f64 [n_prob,4,4]
    T32: torch.Tensor        # f32 [n_prob,4,4], T cast once
    fitness: torch.Tensor    # f64 [n_prob]
    rmse: torch.Tensor       # f64 [n_prob]
    iters: torch.Tensor      # int32 [n_prob] updates applied
    ncorr: torch.Tensor      # int32 [n_prob]
    corr: Optional[torch.Tensor]   # int32, problem-major (problem p at corr_off[p]): local target row or -1
    corr_off: Optional[list]
    wfitness: Optional[torch.Tensor] = None   # f64 [n_prob] weighted inlier share (a robust kernel was asked for)
    scale: Optional[torch.Tensor] = None      # f64 [n_prob] the factor the call added to T0 (with_scaling was asked for)
    # f64 [n_prob] Mahalanobis rmse of the last evaluation, filled by estimation = "gicp" (GicpResult below).  An attribute, NOT
    # a field of the tuple: the tuple keeps the ten fields above, whose layout callers and tests rely on
    mrmse = None


class GicpResult(IcpResult):
    """The IcpResult of estimation = "gicp": the same ten-field tuple with the attribute `mrmse` set."""
    def __new__(cls, *fields, mrmse=None):
        self = super().__new__(cls, *fields)
        self.mrmse = mrmse
        return self


ICP_KERNELS = {"l2": 0, "huber": 1, "cauchy": 2, "tukey": 3}    # CS_ICP_KERNEL_*


def estimate_normals(xyz, offsets, k=16, radius=None):
    """cs_estimate_normals: one normal per row (f32 [n,3] device) from the k nearest rows of the row's own segment
    (host offset list); 3 <= k <= 32.  The semantics are the header comment of cs_estimate_normals.  With a `radius`:
    cs_estimate_normals_hybrid, the at most k nearest rows strictly inside the radius (k is Open3D's max_nn).  No host
    wait."""
    xyz = _dev(xyz, torch.float32, "points").contiguous()
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("estimate_normals: points must be [n, 3]")
    if len(offsets) < 1 or int(offsets[-1]) > xyz.shape[0]:
        raise ValueError("estimate_normals: the offset table exceeds the point array")
    out = torch.empty_like(xyz)
    if radius is None:
        check(_lib.load().cs_estimate_normals(ptr(xyz), i64_array(offsets), len(offsets) - 1, int(k), ptr(out), stream_ptr()))
    else:
        check(_lib.load().cs_estimate_normals_hybrid(ptr(xyz), i64_array(offsets), len(offsets) - 1, float(radius), int(k),
                                                     ptr(out), stream_ptr()))
    return out


def normals_stats(reset=False):
    """cs_normals_stats: (rows answered by a cell-grid path, of those recomputed by the exhaustive scan); counts only
    under CS_NORMALS_STATS=1."""
    out = (ctypes.c_uint64 * 2)()
    _lib.load().cs_normals_stats(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


def knn_mean_dist(xyz, offsets, k=20):
    """cs_knn_mean_dist: f64 [n] device, the mean distance of every row of packed clouds (host offset list) to the k
    nearest rows of its own segment, itself included (Open3D's average); 2 <= k <= 32.  NaN for a row with a non-finite
    coordinate.  The semantics are the header comment of cs_knn_mean_dist.  No host wait."""
    xyz = _packed_points(xyz, offsets, "knn_mean_dist")
    out = torch.empty(xyz.shape[0], dtype=torch.float64, device=xyz.device)
    check(_lib.load().cs_knn_mean_dist(ptr(xyz), i64_array(offsets), len(offsets) - 1, int(k), ptr(out), stream_ptr()))
    return out


def outlier_statistical(xyz, offsets, k=20, std_ratio=2.0):
    """Open3D's remove_statistical_outlier(k, std_ratio) per segment: cs_knn_mean_dist, then cs_outlier_statistical.
    Returns (keep bool [n], stat f64 [n_seg,4] = (n_valid, mu, sigma, tau) per segment), both on the device; a row is
    kept when 0 < mean < tau = mu + std_ratio * sigma.  The statistic is an exact integer sum: a permuted segment gives
    the permuted mask and the same `stat` bits.  No host wait."""
    mean = knn_mean_dist(xyz, offsets, k)
    n_seg = len(offsets) - 1
    keep = torch.zeros(mean.shape[0], dtype=torch.uint8, device=mean.device)
    stat = torch.zeros((n_seg, 4), dtype=torch.float64, device=mean.device)
    check(_lib.load().cs_outlier_statistical(ptr(mean), i64_array(offsets), n_seg, float(std_ratio), ptr(keep), ptr(stat),
                                             stream_ptr()))
    return keep.bool(), stat


def outlier_radius(xyz, offsets, radius, nb_points):
    """Open3D's remove_radius_outlier(nb_points, radius) per segment, cs_outlier_radius: (keep bool [n], count int32 [n])
    on the device; count = the rows of the segment strictly inside `radius`, the row itself included, and a row is kept
    when count > nb_points.  No host wait."""
    xyz = _packed_points(xyz, offsets, "outlier_radius")
    count = torch.zeros(xyz.shape[0], dtype=torch.int32, device=xyz.device)
    keep = torch.zeros(xyz.shape[0], dtype=torch.uint8, device=xyz.device)
    check(_lib.load().cs_outlier_radius(ptr(xyz), i64_array(offsets), len(offsets) - 1, float(radius), int(nb_points),
                                        ptr(count), ptr(keep), stream_ptr()))
    return keep.bool(), count


def outlier_stats(reset=False):
    """cs_outlier_stats: (rows answered by a cell-grid path, of those recomputed by the exhaustive scan); counts only
    under CS_OUTLIER_STATS=1."""
    out = (ctypes.c_uint64 * 2)()
    _lib.load().cs_outlier_stats(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


def dbscan(xyz, offsets, eps, min_points):
    """Open3D's cluster_dbscan(eps, min_points) per segment, cs_dbscan: (label int32 [n], count int32 [n]) on the device.
    count = the rows of the segment strictly inside `eps`, the row itself included (outlier_radius' count); a row with
    count >= min_points is a core row, the clusters are the connected components of the core rows, numbered 0, 1, ... by
    their smallest row; a non-core row takes the label of its nearest core row inside eps (ties: the smaller row), every
    other row -1.  The labels are a function of the segment alone.  The semantics are the header comment of cs_dbscan.
    No host wait."""
    xyz = _packed_points(xyz, offsets, "dbscan")
    label = torch.full((xyz.shape[0],), -1, dtype=torch.int32, device=xyz.device)
    count = torch.zeros(xyz.shape[0], dtype=torch.int32, device=xyz.device)
    check(_lib.load().cs_dbscan(ptr(xyz), i64_array(offsets), len(offsets) - 1, float(eps), int(min_points), ptr(label),
                                ptr(count), stream_ptr()))
    return label, count


def cluster_largest(label, offsets):
    """cs_cluster_largest on the labels of `dbscan`: (keep bool [n], stat int32 [n_seg,3] = (clusters, id of the largest,
    its size) per segment), both on the device; a row is kept when its label is the largest cluster's (core and border
    rows count, ties go to the smaller id), and a segment without a cluster gives (0, -1, 0) and keeps nothing.  Integer
    atomics only: the same values on any launch shape.  No host wait."""
    label = _dev(label, torch.int32, "label").contiguous()
    if label.dim() != 1 or len(offsets) < 1 or int(offsets[-1]) > label.shape[0]:
        raise ValueError("cluster_largest: label must be [n] and cover the offset table")
    n_seg = len(offsets) - 1
    keep = torch.zeros(label.shape[0], dtype=torch.uint8, device=label.device)
    stat = torch.zeros((n_seg, 3), dtype=torch.int32, device=label.device)
    check(_lib.load().cs_cluster_largest(ptr(label), i64_array(offsets), n_seg, ptr(keep), ptr(stat), stream_ptr()))
    return keep.bool(), stat


def dbscan_stats(reset=False):
    """cs_dbscan_stats: (rows answered by the cell-grid path, border rows); counts only under CS_DBSCAN_STATS=1."""
    out = (ctypes.c_uint64 * 2)()
    _lib.load().cs_dbscan_stats(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


def segment_plane(xyz, offsets, dist, iters=1024, seed=0):
    """Open3D's segment_plane(dist, 3, iters) per segment, cs_segment_plane: (inlier bool [n], plane f64 [n_seg,4] =
    (n_x, n_y, n_z, d) with n . p + d = 0, stat int32 [n_seg,8] = (found, best t, stage-1 count, refit, final count, n_pos,
    n_neg, rows_finite) per segment), all on the device.  `iters` three-row hypotheses are counted, the best is refitted
    over its inliers by an order-free integer covariance, and the mask is that of the refitted plane; the normal points to
    the side most of the other rows are on and n_neg counts the rows beyond it.  A segment without a plane gives a zero
    plane, stat (0, -1, 0, 0, 0, 0, 0, rows_finite) and no inlier.  The semantics are the header comment of
    cs_segment_plane.  No host wait."""
    xyz = _packed_points(xyz, offsets, "segment_plane")
    n_seg = len(offsets) - 1
    inlier = torch.zeros(xyz.shape[0], dtype=torch.uint8, device=xyz.device)
    plane = torch.zeros((n_seg, 4), dtype=torch.float64, device=xyz.device)
    stat = torch.zeros((n_seg, 8), dtype=torch.int32, device=xyz.device)
    check(_lib.load().cs_segment_plane(ptr(xyz), i64_array(offsets), n_seg, float(dist), int(iters), int(seed), ptr(plane),
                                       ptr(stat), ptr(inlier), stream_ptr()))
    return inlier.bool(), plane, stat


def select_rows(keep, offsets):
    """The rows a mask keeps, as (idx int64 [m] device, ascending; new host offsets): plain torch, and the only place where
    the filters wait for the device (the kept rows per segment come to the host, as voxelize's offsets do)."""
    keep = keep.bool()
    if keep.dim() != 1 or len(offsets) < 1 or int(offsets[-1]) > keep.shape[0]:
        raise ValueError("select_rows: keep must be [n] and cover the offset table")
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=keep.device), torch.cumsum(keep.to(torch.int64), 0)])
    at = torch.as_tensor([int(o) for o in offsets], dtype=torch.int64, device=keep.device)
    cnt = (csum[at] - csum[at[0]]).cpu().tolist()
    lo, hi = int(offsets[0]), int(offsets[-1])
    idx = torch.nonzero(keep[lo:hi], as_tuple=False)[:, 0] + lo
    return idx, [int(c) for c in cnt]


def icp_batch(src, soff, tgt, toff, src_seg, tgt_seg, T0, max_dist, max_iter=30, relative_fitness=1e-6,
              relative_rmse=1e-6, return_corr=False, tgt_normals=None, kernel="l2", kernel_scale=None, with_scaling=False,
              scale_bounds=(0.5, 2.0), *, estimation=None, src_normals=None, gicp_epsilon=1e-3):
    """cs_icp_batch: point-to-point ICP of problem p = source segment src_seg[p] of `src` against target segment
    tgt_seg[p] of `tgt` (f32 [n,3] device, host offset lists), started at T0[p] (f32 [n_prob,4,4] device).  The semantics
    are the header comment of cs_icp_batch.  tgt_normals (f32, the shape of `tgt`; estimate_normals): point-to-plane
    estimation instead, cs_icp_plane_batch.  kernel = "huber" / "cauchy" / "tukey" with kernel_scale > 0: the robust
    point-to-plane estimation, cs_icp_plane_robust_batch, which also fills IcpResult.wfitness; it needs tgt_normals (robust
    kernels exist for the plane estimation only, as in Open3D).  with_scaling: cs_icp_scale_batch, either estimation with
    an isotropic scale of the source as one more unknown (Open3D's with_scaling = true for the point estimation); T is then
    a similarity and IcpResult.scale the factor the call added to T0.  A problem whose accumulated scale would leave
    scale_bounds = (min, max), min <= 1 <= max, stops before that update; the default (0.5, 2.0) is untuned.  Robust
    kernels with a scale are out of scope and refused.  estimation = "gicp" (keyword-only, with src_normals and
    gicp_epsilon): plane-to-plane Generalized ICP, cs_icp_gicp_batch, on tgt_normals AND src_normals (f32, the shape of
    `src`, in the source's own frame), both required; gicp_epsilon in [2^-10, 1] is the covariance floor along the normal
    (Open3D's default 1e-3, untuned here) and IcpResult.mrmse the Mahalanobis rmse.  A robust kernel or with_scaling with
    GICP is out of scope and refused.  estimation = None keeps the rule above (tgt_normals decide).  Returns an IcpResult;
    no host wait."""
    if estimation not in (None, "gicp"):
        raise ValueError("icp_batch: estimation must be None or 'gicp', got %r" % (estimation,))
    gicp = estimation == "gicp"
    if gicp:
        if kernel != "l2" or with_scaling:
            raise ValueError("icp_batch: estimation 'gicp' with a robust kernel or with_scaling is out of scope")
        if tgt_normals is None or src_normals is None:
            raise ValueError("icp_batch: estimation 'gicp' needs tgt_normals and src_normals")
        eps = float(gicp_epsilon)
        if not (np.isfinite(eps) and 2.0 ** -10 <= eps <= 1.0):
            raise ValueError("icp_batch: gicp_epsilon must lie in [2^-10, 1], got %r" % (gicp_epsilon,))
    elif src_normals is not None:
        raise ValueError("icp_batch: src_normals are used by estimation = 'gicp' only")
    if with_scaling:
        if kernel != "l2":
            raise ValueError("icp_batch: with_scaling with a robust kernel (%r) is out of scope: robust kernels exist for "
                             "the rigid plane estimation only" % (kernel,))
        try:
            smin, smax = float(scale_bounds[0]), float(scale_bounds[1])
        except (TypeError, ValueError, IndexError):
            raise ValueError("icp_batch: scale_bounds must be a pair (min, max), got %r" % (scale_bounds,))
        if not (np.isfinite(smin) and np.isfinite(smax) and 0.0 < smin <= 1.0 <= smax):
            raise ValueError("icp_batch: scale_bounds must be finite with 0 < min <= 1 <= max, got %r" % (scale_bounds,))
    if kernel not in ICP_KERNELS:
        raise ValueError("icp_batch: kernel must be one of %s, got %r" % (sorted(ICP_KERNELS), kernel))
    if kernel != "l2" and tgt_normals is None:
        raise ValueError("icp_batch: kernel %r needs tgt_normals (robust kernels exist for the plane estimation only)"
                         % (kernel,))
    if kernel != "l2" and kernel_scale is None:
        raise ValueError("icp_batch: kernel %r needs a kernel_scale" % (kernel,))
    src = _dev(src, torch.float32, "source").contiguous()
    tgt = _dev(tgt, torch.float32, "target").contiguous()
    T0 = _dev(T0, torch.float32, "initial transforms").contiguous()
    n_prob = len(src_seg)
    if len(tgt_seg) != n_prob:
        raise ValueError("icp_batch: src_seg and tgt_seg differ in length")
    if T0.numel() != 16 * n_prob:
        raise ValueError("icp_batch: one 4x4 initial transform per problem")
    if src.dim() != 2 or src.shape[1] != 3 or tgt.dim() != 2 or tgt.shape[1] != 3:
        raise ValueError("icp_batch: points must be [n, 3]")
    sane = all(0 <= int(s) < len(soff) - 1 for s in src_seg) and all(0 <= int(t) < len(toff) - 1 for t in tgt_seg)
    if n_prob and sane and (int(soff[max(src_seg) + 1]) > src.shape[0] or int(toff[max(tgt_seg) + 1]) > tgt.shape[0]):
        raise ValueError("icp_batch: the offset tables exceed the point arrays")
    if n_prob and not sane and min(min(src_seg), min(tgt_seg)) >= 0:
        raise ValueError("icp_batch: a segment id exceeds its offset table")
    dev = src.device
    T = torch.empty((n_prob, 4, 4), dtype=torch.float64, device=dev)
    T32 = torch.empty((n_prob, 4, 4), dtype=torch.float32, device=dev)
    fitness = torch.empty(n_prob, dtype=torch.float64, device=dev)
    rmse = torch.empty(n_prob, dtype=torch.float64, device=dev)
    iters = torch.empty(n_prob, dtype=torch.int32, device=dev)
    ncorr = torch.empty(n_prob, dtype=torch.int32, device=dev)
    corr = corr_off = None
    if return_corr:
        lens = [int(soff[s + 1]) - int(soff[s]) for s in src_seg] if sane else []
        corr_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
        corr = torch.full((max(corr_off[-1], 1),), -1, dtype=torch.int32, device=dev)
    head = (i64_array(toff), i32_array(src_seg), i32_array(tgt_seg), n_prob, ptr(T0), float(max_dist), int(max_iter),
            float(relative_fitness), float(relative_rmse))
    tail = head + (ptr(T), ptr(T32), ptr(fitness), ptr(rmse), ptr(iters), ptr(ncorr), ptr(corr), stream_ptr())
    wfitness = scale = None
    nrm = None
    if tgt_normals is not None:
        nrm = _dev(tgt_normals, torch.float32, "target normals").contiguous()
        if nrm.shape != tgt.shape:
            raise ValueError("icp_batch: tgt_normals must have the shape of the target points")
    mrmse = None
    if gicp:
        snrm = _dev(src_normals, torch.float32, "source normals").contiguous()
        if snrm.shape != src.shape:
            raise ValueError("icp_batch: src_normals must have the shape of the source points")
        mrmse = torch.empty(n_prob, dtype=torch.float64, device=dev)
        check(_lib.load().cs_icp_gicp_batch(
            ptr(src), ptr(snrm), i64_array(soff), ptr(tgt), ptr(nrm), *head, eps, ptr(T), ptr(T32), ptr(fitness), ptr(rmse),
            ptr(mrmse), ptr(iters), ptr(ncorr), ptr(corr), stream_ptr()))
    elif with_scaling:
        scale = torch.empty(n_prob, dtype=torch.float64, device=dev)
        check(_lib.load().cs_icp_scale_batch(
            ptr(src), i64_array(soff), ptr(tgt), ptr(nrm), *head, smin, smax, ptr(T), ptr(T32), ptr(fitness), ptr(rmse),
            ptr(scale), ptr(iters), ptr(ncorr), ptr(corr), stream_ptr()))
    elif nrm is None:
        check(_lib.load().cs_icp_batch(ptr(src), i64_array(soff), ptr(tgt), *tail))
    else:
        if kernel == "l2":
            check(_lib.load().cs_icp_plane_batch(ptr(src), i64_array(soff), ptr(tgt), ptr(nrm), *tail))
        else:
            wfitness = torch.empty(n_prob, dtype=torch.float64, device=dev)
            check(_lib.load().cs_icp_plane_robust_batch(
                ptr(src), i64_array(soff), ptr(tgt), ptr(nrm), *head, ICP_KERNELS[kernel], float(kernel_scale), ptr(T),
                ptr(T32), ptr(fitness), ptr(rmse), ptr(wfitness), ptr(iters), ptr(ncorr), ptr(corr), stream_ptr()))
    if corr is not None:
        corr = corr[:corr_off[-1]]
    if gicp:
        return GicpResult(T, T32, fitness, rmse, iters, ncorr, corr, corr_off, wfitness, scale, mrmse=mrmse)
    return IcpResult(T, T32, fitness, rmse, iters, ncorr, corr, corr_off, wfitness, scale)


def icp_stats(reset=False):
    """cs_icp_stats: (256-source workgroups answered by the f16 association, of those recomputed exhaustively), summed
    over the rounds; counts only under CS_ICP_STATS=1."""
    out = (ctypes.c_uint64 * 2)()
    _lib.load().cs_icp_stats(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


def ransac_batch(src, tgt, offsets, max_corr, ransac_n=10, max_iter=100000, confidence=0.999, seed=0):
    """Batched correspondence RANSAC.  Returns (T f32 [n,4,4], inliers int32, rmse f64, iters int32)."""
    src = _dev(src, torch.float32, "source correspondences").contiguous()
    tgt = _dev(tgt, torch.float32, "target correspondences").contiguous()
    n_prob = len(offsets) - 1
    dev = src.device
    T = torch.empty((n_prob, 4, 4), dtype=torch.float32, device=dev)
    inl = torch.empty(n_prob, dtype=torch.int32, device=dev)
    rmse = torch.empty(n_prob, dtype=torch.float64, device=dev)
    iters = torch.empty(n_prob, dtype=torch.int32, device=dev)
    check(_lib.load().cs_ransac_batch(ptr(src), ptr(tgt), i64_array(offsets), n_prob, float(max_corr),
                                      ransac_n, max_iter, float(confidence), int(seed), ptr(T),
                                      ptr(inl), ptr(rmse), ptr(iters), stream_ptr()))
    return T, inl, rmse, iters


class FgrResult(NamedTuple):
    T: torch.Tensor          # f32 [n_prob,4,4], T64 cast once
    T64: torch.Tensor        # f64 [n_prob,4,4]
    inliers: torch.Tensor    # int32 [n_prob] pairs of the problem within max_corr of their target under T64
    rmse: torch.Tensor       # f64 [n_prob] of those inliers
    iters: torch.Tensor      # int32 [n_prob] updates applied
    n_tuple: torch.Tensor    # int32 [n_prob] tuples kept by the tuple test, -1 with the test off


def fgr_batch(src, tgt, offsets, max_corr, mu_floor=0.025, division_factor=1.4, iteration_number=64, tuple_test=True,
              tuple_scale=0.95, max_tuple=1000, seed=0):
    """cs_fgr_batch: Fast Global Registration of the correspondence lists of ransac_batch's layout (f32 [M,3] device pairs,
    host offset list).  The semantics are the header comment of cs_fgr_batch; max_corr only serves the reported inliers and
    rmse.  mu_floor (Open3D's maximum_correspondence_distance, in units of the normalised frame) is untuned.  Returns an
    FgrResult; no host wait."""
    src = _dev(src, torch.float32, "source correspondences").contiguous()
    tgt = _dev(tgt, torch.float32, "target correspondences").contiguous()
    if src.shape != tgt.shape or src.dim() != 2 or src.shape[1] != 3:
        raise ValueError("fgr_batch: correspondences must be two [M, 3] arrays of one shape")
    if len(offsets) < 1 or int(offsets[-1]) > src.shape[0]:
        raise ValueError("fgr_batch: the offset table exceeds the correspondence arrays")
    n_prob = len(offsets) - 1
    dev = src.device
    T = torch.empty((n_prob, 4, 4), dtype=torch.float32, device=dev)
    T64 = torch.empty((n_prob, 4, 4), dtype=torch.float64, device=dev)
    inl = torch.empty(n_prob, dtype=torch.int32, device=dev)
    rmse = torch.empty(n_prob, dtype=torch.float64, device=dev)
    iters = torch.empty(n_prob, dtype=torch.int32, device=dev)
    n_tuple = torch.empty(n_prob, dtype=torch.int32, device=dev)
    check(_lib.load().cs_fgr_batch(ptr(src), ptr(tgt), i64_array(offsets), n_prob, float(max_corr), float(mu_floor),
                                   float(division_factor), int(iteration_number), 1 if tuple_test else 0,
                                   float(tuple_scale), int(max_tuple), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(T), ptr(T64),
                                   ptr(inl), ptr(rmse), ptr(iters), ptr(n_tuple), stream_ptr()))
    return FgrResult(T, T64, inl, rmse, iters, n_tuple)


def partition_by_label(label, d_off, n_cloud):
    """Rows of every cloud stably partitioned by part label (split_corr's part order).  d_off: int64 device
    tensor [n_cloud + 1].  Returns int64 [N] global row indices."""
    label = _dev(label, torch.int32, "labels").contiguous()
    order = torch.empty(label.shape[0], dtype=torch.int64, device=label.device)
    check(_lib.load().cs_partition_by_label(ptr(label), ptr(d_off), n_cloud, ptr(order), stream_ptr()))
    return order


def cfg_bad(nn, d_first, n_cfg):
    """int32 [n_cfg]: 1 where rows [first[j], first[j+1]) of the neighbour lists hold a negative entry."""
    nn = _dev(nn, torch.int32, "neighbour lists").contiguous()
    bad = torch.empty(n_cfg, dtype=torch.int32, device=nn.device)
    check(_lib.load().cs_cfg_bad(ptr(nn), nn.shape[1], ptr(d_first), n_cfg, ptr(bad), stream_ptr()))
    return bad


def rows_nonfinite(x, d_first, n_seg):
    """int32 [n_seg]: 1 where rows [first[j], first[j+1]) of x (f32 [n, dim]) hold a NaN or infinite element."""
    x = _dev(x, torch.float32, "rows").contiguous()
    bad = torch.empty(n_seg, dtype=torch.int32, device=x.device)
    check(_lib.load().cs_rows_nonfinite(ptr(x), x.shape[1], ptr(d_first), n_seg, ptr(bad), stream_ptr()))
    return bad


def corr_assemble(xyz0, xyz1, rows, nn, desc, total, max_len):
    """Correspondence lists of the configurations desc (host int64 [n_cfg, 5] = q_first, n_first, t_first, len,
    out_first): returns (src f32 [total * k, 3], tgt f32 [total * k, 3])."""
    xyz0 = _dev(xyz0, torch.float32, "query xyz").contiguous()
    xyz1 = _dev(xyz1, torch.float32, "CAD xyz").contiguous()
    nn = _dev(nn, torch.int32, "neighbour lists").contiguous()
    k = nn.shape[1]
    dev = xyz0.device
    src = torch.empty((total * k, 3), dtype=torch.float32, device=dev)
    tgt = torch.empty((total * k, 3), dtype=torch.float32, device=dev)
    d_desc = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.int64)).to(dev, non_blocking=True)
    check(_lib.load().cs_corr_assemble(ptr(xyz0), ptr(xyz1), ptr(rows) if rows is not None else None, ptr(nn), k,
                                       ptr(d_desc), len(desc), int(max_len), ptr(src), ptr(tgt), stream_ptr()))
    return src, tgt


def symcut_fit(feat, xyz, offsets, anchors, Ks, n_nn=50, n_init=10, max_iter=300):
    """anchors int32 [n_cloud, n_anchor] device; Ks host list.  Returns centers f64 [c,a,4,3],
    counts int32 [c,a,4], min centre distance f64 [c,a], max error f64 [c,a]."""
    feat = _dev(feat, torch.float32, "features").contiguous()
    xyz = _dev(xyz, torch.float32, "xyz").contiguous()
    anchors = _dev(anchors, torch.int32, "anchors").contiguous()
    nc, na = anchors.shape
    dev = feat.device
    centers = torch.empty((nc, na, 4, 3), dtype=torch.float64, device=dev)
    counts = torch.empty((nc, na, 4), dtype=torch.int32, device=dev)
    mcd = torch.empty((nc, na), dtype=torch.float64, device=dev)
    mer = torch.empty((nc, na), dtype=torch.float64, device=dev)
    check(_lib.load().cs_symcut_fit(ptr(feat), feat.shape[1], ptr(xyz), i64_array(offsets), nc,
                                    ptr(anchors), na, i32_array(Ks), n_nn, n_init, max_iter,
                                    ptr(centers), ptr(counts), ptr(mcd), ptr(mer), stream_ptr()))
    return centers, counts, mcd, mer


def symcut_labels(xyz, offsets, Ks, sel_centers):
    xyz = _dev(xyz, torch.float32, "xyz").contiguous()
    sel_centers = _dev(sel_centers, torch.float64, "centres").contiguous()
    labels = torch.empty(xyz.shape[0], dtype=torch.int32, device=xyz.device)
    check(_lib.load().cs_symcut_labels(ptr(xyz), i64_array(offsets), len(Ks), i32_array(Ks),
                                       ptr(sel_centers), ptr(labels), stream_ptr()))
    return labels


# ---- training batches -------------------------------------------------------------------------------
class RadiusPlan:
    """Owns one cs_radius_plan: the search of radius_pairs_begin, waiting for its fill.  Keeps the point tensors alive
    (the fill reads them again)."""

    def __init__(self, handle, keep):
        self._h = c_void_p(handle)
        self._keep = keep

    def fill(self, row_ptr, total):
        """Target indices int32 [total] of the CSR whose row offsets radius_pairs_begin wrote into row_ptr."""
        idx = torch.empty(max(int(total), 1), dtype=torch.int32, device=row_ptr.device)
        check(_lib.load().cs_radius_pairs_fill(self._h, ptr(row_ptr), ptr(idx), stream_ptr()))
        return idx[:int(total)]

    def __del__(self):
        try:
            if self._h:
                _lib.load().cs_radius_plan_free(self._h)
                self._h = None
        except Exception:
            pass


def radius_pairs_begin(src, soff, tgt, toff, src_seg=None, tgt_seg=None, radius=0.03, k=None):
    """Enqueues cs_radius_pairs: returns (row_ptr int64 [rows+1] device, RadiusPlan).  No host wait: the caller reads
    row_ptr[-1] (with whatever else it needs) and calls plan.fill(row_ptr, total)."""
    src = _dev(src, torch.float64, "source points").contiguous()
    tgt = _dev(tgt, torch.float64, "target points").contiguous()
    if src_seg is None:
        src_seg = list(range(len(soff) - 1))
        tgt_seg = list(range(len(toff) - 1))
    if len(src_seg) != len(tgt_seg):
        raise ValueError("radius_pairs: src_seg and tgt_seg differ in length")
    if k is not None and int(k) < 1:
        raise ValueError("radius_pairs: k must be None or >= 1")
    rows = sum(int(soff[s + 1]) - int(soff[s]) for s in src_seg)
    row_ptr = torch.empty(rows + 1, dtype=torch.int64, device=src.device)
    plan = c_void_p()
    check(_lib.load().cs_radius_pairs(ptr(src), i64_array(soff), ptr(tgt), i64_array(toff), i32_array(src_seg),
                                      i32_array(tgt_seg), len(src_seg), float(radius), int(k or 0), ptr(row_ptr),
                                      stream_ptr(), ctypes.byref(plan)))
    return row_ptr, RadiusPlan(plan.value, (src, tgt))


def radius_pairs(src, soff, tgt, toff, src_seg=None, tgt_seg=None, radius=0.03, k=None):
    """Batched fixed-radius pairs (cs_radius_pairs): f64 [n,3] device points, host offset lists, per-problem segment
    ids (default: problem p uses segment p of both).  Returns the CSR (row_ptr int64 [rows+1], tgt_idx int32 [total])
    over the source rows of all problems, targets local to their segment, each row in ascending (d2, index), at most
    k per row.  One host wait (the total)."""
    row_ptr, plan = radius_pairs_begin(src, soff, tgt, toff, src_seg, tgt_seg, radius, k)
    total = int(_lib.to_host(row_ptr[-1:])[0][0])
    return row_ptr, plan.fill(row_ptr, total)


def sample_pairs(xyz, offsets, base_seg, pos_seg, neg_seg, slots, row_base, row_ptr, tgt_idx, lists, seed, round_,
                 radius, sample, out=None):
    """cs_sample_pairs: PiP (lists & 1) and / or PiN + NiN (lists & 2) of every problem into fixed-capacity buffers.
    xyz f32 [n,3] device (kept canonical points), offsets / *_seg / slots / row_base host lists.  `out` = (pip, pin,
    nin, counts) from an earlier call to complete (the other lists); returns that tuple: int32 [P * sample, 2] each,
    counts int32 [P, 4] = {n_pos, PiP, PiN, NiN}."""
    xyz = _dev(xyz, torch.float32, "points").contiguous()
    n_prob = len(base_seg)
    dev = xyz.device
    if out is None:
        out = tuple(torch.zeros((n_prob * sample, 2), dtype=torch.int32, device=dev) for _ in range(3)) + (
            torch.zeros((n_prob, 4), dtype=torch.int32, device=dev),)
    pip, pin, nin, counts = out
    if tgt_idx is not None and tgt_idx.numel() == 0:   # no pair at all: never read, but must not be NULL
        tgt_idx = torch.zeros(1, dtype=torch.int32, device=dev)
    check(_lib.load().cs_sample_pairs(ptr(xyz), i64_array(offsets), i32_array(base_seg), i32_array(pos_seg),
                                      i32_array(neg_seg), i32_array(slots), n_prob, i64_array(row_base), ptr(row_ptr),
                                      ptr(tgt_idx), int(lists), int(seed) & 0xFFFFFFFFFFFFFFFF, int(round_),
                                      float(radius), int(sample), ptr(pip), ptr(pin), ptr(nin), ptr(counts),
                                      stream_ptr()))
    return out


def transform_f64(xyz, offsets, seg, T):
    """cs_transform_f64: segments seg of xyz (f32 [n,3] device, host offsets) concatenated, each mapped by its f64
    4x4 T[p] (device [P,4,4]) as ((r0 x + r1 y) + r2 z) + t in f64.  Returns f64 [sum, 3]."""
    xyz = _dev(xyz, torch.float32, "points").contiguous()
    T = _dev(T, torch.float64, "transforms").contiguous()
    if T.shape[0] != len(seg):
        raise ValueError("transform_f64: one transform per segment")
    total = sum(int(offsets[s + 1]) - int(offsets[s]) for s in seg)
    out = torch.empty((max(total, 1), 3), dtype=torch.float64, device=xyz.device)
    check(_lib.load().cs_transform_f64(ptr(xyz), i64_array(offsets), i32_array(seg), len(seg), ptr(T), ptr(out),
                                       stream_ptr()))
    return out[:total]


# ---- metric-learning loss ---------------------------------------------------------------------------
PAIR_PULL, PAIR_PUSH = 0, 1


def _pair_loss_args(mats, terms):
    """The host side of cs_pair_loss_*: mats = list of f32 [n, C] device tensors (unit inner stride, any leading
    dimension), terms = list of (a, b, pairs int32 [P, 2], kind, margin, weight) with a, b indices into mats."""
    if not mats:
        raise ValueError("pair_loss: no feature matrix")
    C = int(mats[0].shape[1])
    lds = []
    for m in mats:
        _dev(m, torch.float32, "features")
        _, ld = _rows(m, "features")
        if int(m.shape[1]) != C:
            raise ValueError("pair_loss: the feature matrices differ in width")
        lds.append(ld)
    pairs = []
    for t in terms:
        p = _dev(t[2], torch.int32, "pairs")
        if p.dim() != 2 or p.shape[1] != 2:
            raise ValueError("pair_loss: pairs must be [P, 2]")
        pairs.append(p.contiguous())
    vp = (c_void_p * len(mats))(*[m.data_ptr() for m in mats])
    pp = (c_void_p * max(len(terms), 1))(*[p.data_ptr() if p.numel() else None for p in pairs])
    head = (len(mats), vp, i64_array([m.shape[0] for m in mats]), i32_array(lds), C, len(terms),
            i32_array([t[0] for t in terms]), i32_array([t[1] for t in terms]), i32_array([t[3] for t in terms]),
            (ctypes.c_float * max(len(terms), 1))(*[float(t[4]) for t in terms]),
            (ctypes.c_double * max(len(terms), 1))(*[float(t[5]) for t in terms]), pp,
            i64_array([p.shape[0] for p in pairs]))
    return head, pairs, C


def pair_loss_fwd(mats, terms, out=None):
    """cs_pair_loss_fwd: returns (term losses f64 [T], total f32 [1]) on the device, no host wait.  `out` = the two
    tensors to write into."""
    head, keep, _ = _pair_loss_args(mats, terms)
    dev = mats[0].device
    if out is None:
        out = (torch.empty(max(len(terms), 1), dtype=torch.float64, device=dev),
               torch.empty(1, dtype=torch.float32, device=dev))
    check(_lib.load().cs_pair_loss_fwd(*head, ptr(out[0]), ptr(out[1]), stream_ptr()))
    return out[0][:len(terms)], out[1]


def pair_loss_bwd(mats, terms, grad_up, out=None):
    """cs_pair_loss_bwd: the gradient of every matrix of mats (f32 [n, C], all terms summed into one), scaled by the
    device scalar grad_up (f32, one element).  Returns the list; `out` = tensors to write into."""
    head, keep, C = _pair_loss_args(mats, terms)
    g = _dev(grad_up, torch.float32, "upstream gradient").reshape(-1)
    if g.numel() != 1:
        raise ValueError("pair_loss_bwd: the upstream gradient is one scalar")
    if out is None:
        out = [torch.empty((m.shape[0], C), dtype=torch.float32, device=m.device) for m in mats]
    lds = [_rows(_dev(o, torch.float32, "gradient"), "gradient")[1] for o in out]
    gp = (c_void_p * len(out))(*[o.data_ptr() for o in out])
    check(_lib.load().cs_pair_loss_bwd(*head, ptr(g), gp, i32_array(lds), stream_ptr()))
    return out
