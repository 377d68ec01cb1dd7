/*
 * corsair_hip.h -- C ABI of libcorsair_hip.so, the MI355X (gfx950) native hot path of
 * CORSAIR inference: sparse-voxel ResUNet operators, descriptor top-k, feature k-NN,
 * one-directional Chamfer, batched correspondence RANSAC and the symmetry part-cut.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own:
 * its hot path sits behind the MinkowskiEngine Python operator API and three Python function
 * seams (utils/retrieval.py, utils/eval_pose.py, utils/preprocess.py).  Every entry point below
 * names the reference interface it replaces (file:line relative to the reference tree).
 *
 * Conventions
 *   - plain C, no torch types; every pointer prefixed d_ is a DEVICE pointer owned by the caller
 *     (e.g. tensor.data_ptr()); h_ is a host pointer.  The library owns only the opaque map
 *     handles and an internal scratch pool.
 *   - every call takes the hipStream_t to launch on as a void* (0 = default stream).  Work is
 *     enqueued in stream order: device outputs (d_*) are valid once the stream reaches that point
 *     (synchronise it before reading them on the host); host outputs (h_*, return values, sizes of
 *     maps) are valid on return.  Scratch memory is cached per host thread and handed out again in
 *     stream order, so a thread should keep to one stream (switching streams drains the old one);
 *     different threads may drive different streams concurrently.
 *   - return value 0 = success, negative = error; cs_last_error() returns the (thread-local)
 *     message.  The Python host raises RuntimeError(cs_last_error()), mirroring ME's
 *     RuntimeError on coordinate-key mismatch.
 *   - rows of feature matrices are addressed with an explicit leading dimension (ld, in
 *     elements) so a consumer can write straight into a slice of a wider buffer (this is how
 *     ME.cat -- model/resunet.py:239,246,253 -- is made free).
 */
#ifndef CORSAIR_HIP_H
#define CORSAIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CS_OK 0
#define CS_ERR_INVALID (-1)
#define CS_ERR_HIP (-2)
#define CS_ERR_RANGE (-3)
#define CS_ERR_DUPLICATE (-4)
#define CS_ERR_UNSUPPORTED (-5)
#define CS_ERR_INTERNAL (-6) /* a self-check of the library failed (e.g. CS_RANSAC_CHECK) */

typedef struct cs_coordmap cs_coordmap;   /* coordinates of one tensor stride + hash index (csrc/coordmap.hip) */
typedef struct cs_kernelmap cs_kernelmap; /* output-stationary neighbour table of one conv (csrc/kernelmap.hip) */

const char* cs_last_error(void);
int cs_version(void);
/* number of visible HIP devices (does not initialise a context) */
int cs_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Coordinate maps.  Replaces ME.SparseTensor(feat, coords) coordinate-manager creation
 * (evaluation.py:215-218,246-249) and the strided coordinate generation inside
 * ME.MinkowskiConvolution(stride=2) (model/resunet.py:64-72,80-87,95-103).
 * d_coords: int32 [n,4] rows (batch, x, y, z), unique, |x|,|y|,|z| < 32768, 0 <= batch < 65535.
 * A row outside that range makes cs_coordmap_create / cs_coordmap_pyramid return CS_ERR_RANGE and no map
 * (batch index 65535 is refused: with it a valid coordinate would pack to the hash tables' empty marker).
 * Row order of the created map == input order (evaluation.py:227-229 relies on it).
 * cs_coordmap_stride: output coords = unique rows of floor(c / (s*ts)) * (s*ts), ordered by
 * FIRST OCCURRENCE in input-row order; new tensor stride s*ts.  The floor cells obey the same range: a
 * row whose cell falls on -32768 (x = -32767 at cell 2; x < -32764 at cell 4; x < -32760 at cell 8)
 * makes cs_coordmap_stride return CS_ERR_RANGE and no map; cs_coordmap_pyramid refuses such a batch as a
 * whole (no level is returned) exactly when the chained calls for its n_levels would.
 * ---------------------------------------------------------------------------------------- */
int cs_coordmap_create(const int32_t* d_coords, int64_t n, int tensor_stride, void* stream,
                       cs_coordmap** out);
int cs_coordmap_stride(const cs_coordmap* in, int stride, void* stream, cs_coordmap** out);
/* All coordinate levels a network will ask for, at once (ME's coordinate manager makes the strided maps one by one as
 * model/resunet.py:64-103 reaches each stride-2 convolution): out[0] = cs_coordmap_create(d_coords, n, tensor_stride),
 * out[l] = cs_coordmap_stride(out[l-1], 2) for l < n_levels <= 4 -- identical coordinates, row order and tables, built from
 * the stride-1 rows in one pass with one host wait.  n_batch > 0 announces rows grouped by sample with batch indices
 * < n_batch (sparse_collate's order, utils/Info/CADLib.py:148-178): the per-sample segments the LDS kernel-map path uses are
 * then made in the same pass (n_batch <= 0: on first use, as for cs_coordmap_create). */
int cs_coordmap_pyramid(const int32_t* d_coords, int64_t n, int tensor_stride, int n_levels, int n_batch, void* stream,
                        cs_coordmap** out);
int64_t cs_coordmap_size(const cs_coordmap* m);
int cs_coordmap_tensor_stride(const cs_coordmap* m);
const int32_t* cs_coordmap_coords(const cs_coordmap* m); /* device int32 [n,4] */
void cs_coordmap_free(cs_coordmap* m);

/* ------------------------------------------------------------------------------------------
 * Kernel maps.  Replaces the kernel-map generation + caching of ME's coordinate manager for
 * kernel_size=3 (27 offsets, k = (dx+1) + 3(dy+1) + 9(dz+1)), dilation 1.
 *   transposed == 0: out row o gathers in rows at  o + delta_k * ts_in   (ts_out in {ts_in, 2 ts_in})
 *   transposed == 1: out row o (fine map) gathers in rows (coarse map) at  o - delta_k * ts_out,
 *                    i.e. the strided map with in/out swapped and the same k
 *                    (ME.MinkowskiConvolutionTranspose, model/resunet.py:110-118,131-139,152-160).
 * The table is int32 [n_out, 27], entry = in row or -1.
 * cs_kernelmap_export writes the canonical (k, in_row, out_row) triples sorted by (k, out_row)
 * for bit-exact parity tests; returns the number of pairs (or negative error).
 * ---------------------------------------------------------------------------------------- */
int cs_kernelmap_build(const cs_coordmap* in, const cs_coordmap* out, int kernel_size,
                       int transposed, void* stream, cs_kernelmap** km);
/* cs_kernelmap_build only enqueues work on `stream`; the pair count reaches the host behind it and
 * cs_kernelmap_num_pairs waits for that copy the first time it is asked (then it is cached). */
/* The n maps of one batch (MinkowskiEngine builds them lazily, one per convolution, through the coordinate manager:
 * model/resunet.py:163-237 is what asks for them): the same maps as n calls of cs_kernelmap_build, built as independent
 * chains on several streams that fork from and join `stream` inside the call (CS_KMAP_STREAMS=1..5, default 4).
 * On failure no map is returned (km[i] = NULL for all i). */
int cs_kernelmap_build_many(int n, const cs_coordmap* const* in, const cs_coordmap* const* out, const int* kernel_size,
                            const int* transposed, void* stream, cs_kernelmap** km);
int64_t cs_kernelmap_num_pairs(const cs_kernelmap* km);
int64_t cs_kernelmap_rows(const cs_kernelmap* km);
const int32_t* cs_kernelmap_table(const cs_kernelmap* km);
int64_t cs_kernelmap_export(const cs_kernelmap* km, int32_t* d_k, int32_t* d_in, int32_t* d_out,
                            int64_t capacity, void* stream);
void cs_kernelmap_free(cs_kernelmap* km);

/* ------------------------------------------------------------------------------------------
 * Sparse convolution forward with fused epilogue.  Replaces ME.MinkowskiConvolution /
 * ME.MinkowskiConvolutionTranspose forward (model/resunet.py:49-193, model/residual_block.py:41-53,
 * model/fc.py:63-71) and, fused, ME.MinkowskiBatchNorm in eval mode (model/common.py:22),
 * MEF.relu (model/resunet.py:212-255) and SparseTensor.__iadd__ (model/residual_block.py:70).
 *   out[o, :] = epilogue( sum_{k ascending} sum_{ci ascending} in[nbr[o][k], ci] * W[k, ci, :] )
 * accumulated as ONE f32 fma chain in exactly that order (f32-input MFMA is such a chain), then
 *   v = scale ? fma(v, scale[c], shift[c]) : (shift ? v + shift[c] : v);
 *   v = residual ? v + residual[o, c] : v;   v = relu ? max(v, 0) : v.
 * km == NULL means kernel_size 1 (identity map, n_out == n_in, W is [cin, cout]).
 * ---------------------------------------------------------------------------------------- */
int cs_conv_fwd(const cs_kernelmap* km, int64_t n_in, int64_t n_out, const float* d_in, int ld_in,
                int cin, const float* d_w, int cout, const float* d_scale, const float* d_shift,
                const float* d_residual, int ld_res, int relu, float* d_out, int ld_out,
                void* stream);

/* Weight gradient of that convolution (training through the MinkowskiEngine shim):
 *   d_dw[k, ci, co] = sum_{o : T[o][k] >= 0} in[T[o][k], ci] * gout[o, co]
 * for any map as built (stride 1, strided, transposed); km == NULL means kernel_size 1 (d_dw = in^T gout,
 * [cin, cout]).  d_dw is [kvol, cin, cout] like the forward's W; offsets without a pair get exact zeros.  Rows are
 * summed in fixed chunks of the map's tiling order (f32 MFMA inside a chunk, chunks added in ascending order, no
 * atomics): the result is bit-identical run to run.  ld_in / ld_gout allow column slices of wider buffers.
 * The data gradient is cs_conv_fwd on the reverse map (corsair_amd/backend.py conv_dgrad). */
int cs_conv_wgrad(const cs_kernelmap* km, int64_t n_in, int64_t n_out, const float* d_in, int ld_in, int cin,
                  const float* d_gout, int ld_gout, int cout, float* d_dw, void* stream);

/* Eval-mode batch-norm / bias / residual / ReLU as a stand-alone op (for the unfused, op-by-op
 * MinkowskiEngine-compatible path): same epilogue formula as cs_conv_fwd applied to d_in. */
int cs_affine_act(int64_t n, int c, const float* d_in, int ld_in, const float* d_scale,
                  const float* d_shift, const float* d_residual, int ld_res, int relu,
                  float* d_out, int ld_out, void* stream);

/* Row L2 normalisation out = in / max(||in||_2, eps) (eps = 0 reproduces model/resunet.py:260-262;
 * eps = 1e-12 reproduces nn.functional.normalize at evaluation.py:231,264). */
int cs_row_l2_normalize(int64_t n, int c, const float* d_in, int ld_in, float eps, float* d_out,
                        int ld_out, void* stream);

/* Per-sample column-wise max over rows (model/fc.py:23-29,124-125: split_batch + feat.max(0)).
 * d_batch: int32 batch index of every row, read with stride batch_ld (pass the coords pointer
 * and 4).  d_out: [n_batch, c]; rows of absent samples are -inf. */
int cs_segmented_max(int64_t n, int c, const float* d_in, int ld_in, const int32_t* d_batch,
                     int batch_ld, int n_batch, float* d_out, void* stream);

/* Instance normalisation over the rows of every sample (ME.MinkowskiInstanceNorm, used by the IN
 * variants of the network through model/common.py:23-24; MinkowskiEngine semantics: biased variance,
 * eps 1e-8 added to the variance, affine weight / bias [c]):
 *   out[r, ch] = (in[r, ch] - mean[b, ch]) / sqrt(var[b, ch] + eps) * weight[ch] + bias[ch].
 * d_seg: int32 [n_batch + 1] DEVICE row offsets of the samples (rows grouped by sample, ascending);
 * d_weight / d_bias may be NULL.  Summation order is fixed (see rowops.hip) so that the CPU oracle
 * reproduces the result bit for bit.  Returns without waiting for the stream. */
int cs_instance_norm(int64_t n, int c, const float* d_in, int ld_in, const int32_t* d_seg, int n_batch,
                     const float* d_weight, const float* d_bias, float eps, float* d_out, int ld_out,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Voxel quantisation.  Replaces ME.utils.sparse_quantize(floor(xyz/voxel), return_index=True,
 * return_maps_only=True) (utils/Info/CADLib.py:106-121, datasets/CategoryDataset.py:179-197):
 * for every cloud segment keep the first point of each voxel; kept indices ascending.
 * Grid index = floor(x / voxel) in the cloud's own type (NumPy: `f32 array / python float` divides in f32 —
 * the catalog side, CADLib.py:106-121).  d_xyz f32 [n,3]; h_offsets int64 [n_seg+1] (host); d_keep_idx int64 [n] (capacity n, indices
 * into the concatenated cloud); d_grid int32 [n,4] (batch, x, y, z) of kept rows;
 * h_out_offsets int64 [n_seg+1] (host) receives the kept segment boundaries.
 * Non-finite and far coordinates: a coordinate that is NaN or infinite, or whose grid index is outside
 * [-32767, 32767], makes the call return CS_ERR_RANGE (cs_last_error names cs_voxelize); the outputs are
 * unspecified then, nothing faults, and the next call on the thread is unaffected.  (cs_voxelize_f64 alike.)
 * ---------------------------------------------------------------------------------------- */
int cs_voxelize(const float* d_xyz, const int64_t* h_offsets, int n_seg, double voxel_size,
                int64_t* d_keep_idx, int32_t* d_grid, int64_t* h_out_offsets, void* stream);
/* The same for f64 clouds, floor(x / voxel) in f64: what the QUERY side of the reference quantises —
 * datasets/CategoryDataset.py:179-197 floors the f64 output of apply_transform (datasets/ScannetDataset.py:
 * 278-282, utils/preprocess.py:39-48), evaluation-shapenet.py:97-119 floors `pc @ R.T + t` (f64) and casts
 * the KEPT points to f32 afterwards (:103-105).  Narrowing such a cloud to f32 first moves a point across a
 * voxel boundary on about 2 % of posed clouds; this entry does not narrow.  d_xyz f64 [n,3]; the rest as
 * cs_voxelize.  The caller casts the kept origins to f32 after the selection, as the reference does. */
int cs_voxelize_f64(const double* d_xyz, const int64_t* h_offsets, int n_seg, double voxel_size,
                    int64_t* d_keep_idx, int32_t* d_grid, int64_t* h_out_offsets, void* stream);

/* ------------------------------------------------------------------------------------------
 * Descriptor retrieval.  Replaces scipy cdist + full argsort at utils/retrieval.py:139-177:
 * for every query the k catalog rows with the smallest Euclidean distance, ascending, ties
 * broken by smaller catalog index.  Distances are evaluated in f64 exactly as
 * sum_c (double(q_c) - double(x_c))^2 (c ascending, fma chain); d_dist receives sqrt of it.
 * d_q f32 [nq,d], d_x f32 [nx,d]; d_idx int64 [nq,k]; d_dist f64 [nq,k] (may be NULL).
 * Non-finite rows (cs_l2_topk, cs_l2_topk_sq, cs_l2_topk_catalog, on every path): a catalog row whose canonical
 * squared distance to the query is NaN or +inf is never a neighbour -- the lists are those of the same call with
 * such rows taken out of the catalog, indices mapped back.  When fewer than k rows remain the list ends in
 * (-1, +inf) entries (cs_l2_topk_sq reports +inf too); a query row with a non-finite element gets k of them.
 * These are the only cases in which -1 appears in d_idx.  A non-finite row changes nothing outside itself: every
 * other query's list is what it is without the row, bit for bit.  Finite rows of any magnitude are ordinary rows.
 * ---------------------------------------------------------------------------------------- */
int cs_l2_topk(const float* d_q, int64_t nq, const float* d_x, int64_t nx, int d, int k,
               int64_t* d_idx, double* d_dist, void* stream);
/* Same, but d_dist2 receives the SQUARED distances the ranking was made on: what a multi-GPU run merges the
 * per-shard lists with (catalog sharded over ranks, corsair_amd/sharding.py sharded_topk; the reference is
 * single-device).  Merging by (squared distance, global index) reproduces the single-device list bit for bit. */
int cs_l2_topk_sq(const float* d_q, int64_t nq, const float* d_x, int64_t nx, int d, int k, int64_t* d_idx,
                  double* d_dist2, void* stream);
/* Diagnostics of the large-size path (nq * nx >= 2^24, d = 64 / 128 / 256, k <= 10: shortlist on the
 * f16 matrix cores, exact re-score, verification): {queries that took it, queries recomputed by the
 * f64 path because the verification failed (ties at the k-th neighbour)}. */
void cs_l2_topk_stats(uint64_t out[2], int reset);
/* A retrieval run ranks every scan against ONE fixed library (evaluation.py:264-283: `lib_desc` is embedded once,
 * utils/retrieval.py:139-177 ranks against it): the handle keeps what the matrix-core path derives from the catalog
 * (f16 image, f64 norms) across calls; results are those of cs_l2_topk / cs_l2_topk_sq (squared != 0) on the same
 * arrays.  The caller keeps d_x alive and unchanged for the life of the handle. */
typedef struct cs_topk_catalog cs_topk_catalog;
int cs_topk_catalog_create(const float* d_x, int64_t nx, int d, void* stream, cs_topk_catalog** out);
int cs_l2_topk_catalog(const float* d_q, int64_t nq, const cs_topk_catalog* catalog, int k, int64_t* d_idx,
                       double* d_dist, int squared, void* stream);
void cs_topk_catalog_free(cs_topk_catalog* catalog);

/* ------------------------------------------------------------------------------------------
 * Batched feature k-NN.  Replaces find_knn_cpu / KDTree(feat1).query(feat0, k)
 * (utils/find_nn.py:43-49) as used by find_kcorr (utils/eval_pose.py:48-79) and split_corr
 * (utils/symmetry.py:145-179).  The feature matrices are segmented by host offset tables
 * (h_qoff / h_toff); problem p searches, for every row of query segment h_qseg[p], the k nearest
 * rows of target segment h_tseg[p] (f64 squared distance, c ascending fma chain, ties -> smaller
 * index).  Optional part labels (one per feature row) restrict the search (split_corr): target
 * row j is a candidate of query row i iff d_tlabel[j] == d_perm[p*8 + d_qlabel[i]].
 * Output rows are problem-major (all rows of problem 0, then problem 1, ...):
 * d_idx int32 [sum_p nq_p, k] = target row index LOCAL to the target segment, -1 if fewer than k
 * candidates; d_dist f64 same shape, optional (Euclidean distance).
 * dim is 3, 16, 32 or 33 (cs_fpfh's descriptors; the exhaustive kernel, like 3 and 32); 1 <= k <= 8.
 * Non-finite rows (both paths, labelled or not): a candidate whose canonical f64 squared distance is NaN or
 * +inf is never a neighbour -- the results equal those of the same call with the non-finite target rows removed,
 * indices mapped back; the (-1, +inf) padding applies when fewer than k candidates at finite distance remain, and a
 * query row with a non-finite element gets k times (-1, +inf).  A non-finite row changes nothing outside itself:
 * every other query row, segment and problem has the result it has without it, bit for bit.
 * ---------------------------------------------------------------------------------------- */
int cs_knn_feat(const float* d_qf, const int64_t* h_qoff, const float* d_tf,
                const int64_t* h_toff, const int32_t* h_qseg, const int32_t* h_tseg, int n_prob,
                int dim, int k, const int32_t* d_qlabel, const int32_t* d_tlabel,
                const int32_t* d_perm, int32_t* d_idx, double* d_dist, void* stream);

/* Diagnostics of cs_knn_feat's default path for 16-d features (f16 matrix-core shortlist, canonical f64
 * re-evaluation, verification, exhaustive recomputation of what could not be verified): out =
 * {queries answered, of those recomputed exhaustively}, counted only while the environment variable
 * CS_KNN_STATS=1.  CS_KNN_MFMA=0 selects the exhaustive all-VALU kernel (any other value: the default path); both
 * return the same indices and distances. */
void cs_knn_shortlist_stats(uint64_t out[2], int reset);

/* ------------------------------------------------------------------------------------------
 * One-directional Chamfer.  Replaces apply_transform + chamfer_kdtree_1direction
 * (utils/preprocess.py:39-48,67-70): problem p transforms the source segment with the f32
 * 4x4 row-major matrix d_T[p] (f64 arithmetic), finds for every source point the Euclidean
 * distance to the nearest target point, writes the mean to d_out[p] (f64).
 * Source / target segments are selected per problem by index into the offset tables.
 * Non-finite rows (cs_chamfer_1dir and cs_hausdorff_1dir, all three paths): a target row at NaN or +inf distance
 * is never the nearest; a source row with no target at finite distance (a non-finite source row, a non-finite
 * entry of d_T[p], no finite target row) contributes +inf, so d_out[p] = +inf.  NaN stays
 * the result of an empty SOURCE segment alone.  Problems without a non-finite value are unaffected, bit for bit.
 * ---------------------------------------------------------------------------------------- */
/* Diagnostics of the f16 matrix-core ranking inside cs_chamfer_1dir / cs_hausdorff_1dir (default path): {256-source tiles
 * answered, of those recomputed by the f64 matrix-pipe kernel because a source was within the approximation's error budget
 * of a tie}, counted only while CS_CHAMFER_STATS=1.  CS_CHAMFER_F16=0: the f64 kernel for everything; CS_CHAMFER_MFMA=0: the
 * exhaustive all-VALU chain.  All three return the same canonical distances. */
void cs_chamfer_f16_stats(uint64_t out[2], int reset);
int cs_chamfer_1dir(const float* d_src, const int64_t* h_soff, const float* d_tgt,
                    const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg,
                    int n_prob, const float* d_T, double* d_out, void* stream);

/* Directed Hausdorff distance: same arguments, d_out[p] = MAX over source points of the distance to
 * the nearest target point.  Replaces one direction of chamfer_max in the geometric symmetry test
 * of evaluation-shapenet.py:122-155 (get_symmetry_label), SURVEY 8f rank 2. */
int cs_hausdorff_1dir(const float* d_src, const int64_t* h_soff, const float* d_tgt,
                      const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg,
                      int n_prob, const float* d_T, double* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Two-directional Chamfer of posed clouds: the score of a candidate verification (the two one-directional sums the
 * reference's evaluate_retrieval adds, evaluation-scan2cad.py:356-357), both directions from ONE pose and one call.
 * Arguments and problem selection are those of cs_chamfer_1dir; d_out is f64 [n_prob][2].
 * Problem p, source rows s_i (i < ns), target rows t_j (j < nt), M = d_T[p] (f32, row-major 4x4), everything in f64:
 *   p_i,c   = fma(M_c0, s_i,x, fma(M_c1, s_i,y, fma(M_c2, s_i,z, M_c3)))            -- the chain of cs_chamfer_1dir
 *   d2_ij   = fma(dz, dz, fma(dy, dy, dx * dx)),   (dx, dy, dz) = p_i - t_j
 *   d_out[2p]     = (sum over i of sqrt(min_j d2_ij)) / ns     forward: what cs_chamfer_1dir returns
 *   d_out[2p + 1] = (sum over j of sqrt(min_i d2_ij)) / nt     backward, measured in the frame of the TARGET (the
 *                   source is posed, the target is not: no pose is inverted anywhere)
 * Non-finite rows, both directions, by cs_chamfer_1dir's rules: a pair at NaN or +inf distance is never the nearest
 * (every minimum starts at +inf and is an fmin, in which a NaN operand loses); a row or column without a partner at finite distance
 * contributes +inf, so that direction is +inf.  An empty source segment: forward NaN (and backward +inf unless the target
 * is empty too); an empty target segment: backward NaN, forward +inf as in cs_chamfer_1dir.
 * Reproducibility: every minimum is an exact canonical d2 (order-free); a direction's sum is added per tile of 256
 * consecutive rows by a fixed pairwise tree (row i of the tile at leaf i, strides 128, 64, ... 1), the tiles then left to
 * right.  Two calls return identical bits and a problem's two values do not depend on the other problems of the call.
 * Problems may share source segments, target segments or both: a column minimum belongs to its problem.
 * One path: exhaustive, f64 on the vector unit (each direction searches with its own rows in registers).  Scratch: one
 * f64 per 256-row tile plus the work list, from the calling thread's pool.  Segments hold fewer than 2^31 rows.
 * Profile family "chamfer2".
 * ---------------------------------------------------------------------------------------- */
int cs_chamfer_2dir(const float* d_src, const int64_t* h_soff, const float* d_tgt, const int64_t* h_toff,
                    const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, const float* d_T,
                    double* d_out /* [n_prob][2] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batched correspondence RANSAC.  Replaces registration_based_on_corr ->
 * o3d.pipelines.registration.registration_ransac_based_on_correspondence(src, tgt, corr,
 * max_corr, ransac_n=10) (utils/eval_pose.py:82-100).  Problem p owns correspondences
 * [h_off[p], h_off[p+1]) of d_src/d_tgt (f32 [M,3], pair i = (src_i, tgt_i)).
 * Semantics = Open3D's loop run on one thread, with a counter-based RNG:
 *   for itr in [0, max_iter): stop if itr >= est_k; sample ransac_n pairs (with replacement,
 *   idx = rng(seed, itr, j) mod-free multiply-shift); T = rigid least-squares fit (no scale);
 *   inliers = #{ |T src_i - tgt_i|^2 < max_corr^2 }, err = sum of inlier squared distances -- T, the
 *   transform of the points and the comparison in f64, as Open3D evaluates them (the reference
 *   converts the points to float64, utils/eval_pose.py:83-86; max_corr is the Python float);
 *   better = more inliers, or equal inliers and smaller err; on improvement
 *   est_k = min(est_k, ceil(log(1-confidence) / log(1 - (inliers/M)^ransac_n))).
 * d_T f32 [n_prob,16] row-major 4x4 = the best f64 transform cast once at the end, where the reference
 * casts it (utils/symmetry.py:274) (identity if no hypothesis had an inlier);
 * d_inliers int32 [n_prob]; d_rmse f64 [n_prob]; d_iters int32 [n_prob] = iterations consumed.
 * Non-finite pairs: a pair with a NaN or infinite coordinate is never an inlier (its squared distance is not
 * below max_corr^2); it still counts in M and can be sampled.  A hypothesis whose fit is not finite has no inliers
 * and is never the best.  A problem with no finite pair returns the identity, 0 inliers and rmse 0; an EMPTY problem
 * (no pair at all, anywhere in the batch) returns these and 0 iterations, written by the kernels.  With the
 * prefilter on or off the results are the same, and a problem without a non-finite value has the result it has
 * in a batch without the others, bit for bit.
 * ---------------------------------------------------------------------------------------- */
int cs_ransac_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, int n_prob,
                    double max_corr, int ransac_n, int max_iter, double confidence, uint64_t seed,
                    float* d_T, int32_t* d_inliers, double* d_rmse, int32_t* d_iters,
                    void* stream);
/* Diagnostics of the inlier-count prefilter inside cs_ransac_batch (an f16 matrix-core pass that
 * computes an UPPER bound of every hypothesis' inlier count; only hypotheses whose bound reaches
 * the current best are evaluated exactly, so results do not change).  out = {bound violations,
 * hypotheses checked, sum of (bound - exact)} accumulated by runs with the environment variable
 * CS_RANSAC_CHECK=1 (which recomputes every hypothesis exactly and fails with CS_ERR_INTERNAL on a
 * violation), then {survivors, hypotheses generated} of every run.  CS_RANSAC_PREFILTER=0 turns the
 * prefilter off. */
void cs_ransac_prefilter_stats(uint64_t out[5], int reset);

/* ------------------------------------------------------------------------------------------
 * Symmetry part cut.  Replaces symmetric_cut4 (utils/symmetry.py:182-259) for a batch of
 * clouds: for every (cloud, anchor) the 50 feature-nearest voxels, the fit of
 * sklearn's KMeans(n_clusters=K, random_state=0, n_init=n_init) on their xyz (utils/symmetry.py:216:
 * greedy k-means++ on the constant uniform draws of numpy's RandomState(0) -- the reference hard-codes
 * random_state=0, so the entry point takes no seed --, Lloyd with sklearn's stopping rules, first-best
 * restart; n_init <= 10: that many restarts' draws are tabulated, more is CS_ERR_UNSUPPORTED), the
 * statistics the acceptance gate needs, and finally the labels of every voxel under the accepted model.
 *   cs_symcut_fit: d_feat f32 [N,dim], d_xyz f32 [N,3], h_off int64 [n_cloud+1],
 *     d_anchor int32 [n_cloud, n_anchor] (row index local to the cloud), h_K int32 [n_cloud] in {2,4};
 *     outputs per (cloud, anchor): d_centers f64 [.,4,3], d_counts int32 [.,4] (labels of the WHOLE
 *     cloud), d_min_center_dist f64, d_max_error f64 (max over clusters of mean distance of the
 *     50-NN members to their centre).
 *   cs_symcut_labels: labels of every voxel for the chosen centres (d_sel_centers f64 [n_cloud,4,3]),
 *     argmin distance, ties -> smaller centre index (equidistant voxels and duplicated centres included).
 *     Rows >= K of a cloud's centres are ignored: they may hold anything, NaN included.  An empty cloud
 *     writes no label.
 * Contract (tests/test_gpu_symcut.py, bit for bit against oracle/corsair_oracle.c):
 *   - accepted: dim 16 or 32, n_nn 4..64, n_init 1..10, max_iter >= 1, n_anchor >= 1, K 2 or 4 per cloud;
 *     anything else returns CS_ERR_UNSUPPORTED / CS_ERR_INVALID, writes nothing and leaves the library usable.
 *     Fewer than n_nn rows: the whole cloud is the selection.  Selection ties go to the smaller row.
 *   - every element of the four outputs is written for every (cloud, anchor).  A cloud with fewer rows than K
 *     (0 rows included) gets centres 0, counts 0, min centre distance 0.0 and max error +inf: a model the
 *     reference's gate (dist.min() > 0.15 > max(error)) always refuses.  The anchors of a cloud of 0 rows are
 *     not read; those of every other cloud must be rows of it.
 *   - a cloud of K rows or more whose selected voxels take fewer than K distinct positions gets finite centres
 *     of which two coincide: min centre distance is exactly 0.0 (refused by the gate as well), the counts
 *     still sum to the cloud's size; when every selected voxel is at ONE position all voxels count for centre 0
 *     and max error is +inf (the other clusters have no member).  Rows K..3 of the centres and counts are 0.
 *   - the result of a (cloud, anchor) depends on that cloud, that anchor and the parameters alone: not on the
 *     other clouds or anchors of the call, their number or their order.
 * ---------------------------------------------------------------------------------------- */
int cs_symcut_fit(const float* d_feat, int dim, const float* d_xyz, const int64_t* h_off,
                  int n_cloud, const int32_t* d_anchor, int n_anchor, const int32_t* h_K,
                  int n_nn, int n_init, int max_iter, double* d_centers,
                  int32_t* d_counts, double* d_min_center_dist, double* d_max_error,
                  void* stream);
int cs_symcut_labels(const float* d_xyz, const int64_t* h_off, int n_cloud, const int32_t* h_K,
                     const double* d_sel_centers, int32_t* d_labels, void* stream);

/* ------------------------------------------------------------------------------------------
 * Correspondence assembly of sym_pose.  Replaces the index plumbing between find_kcorr / split_corr and
 * registration_based_on_corr (utils/eval_pose.py:48-87, utils/symmetry.py:145-179, 303-356): the reference
 * builds, per part configuration, `xyzA_corrs` / `xyzB_corrs` by boolean-mask gathers and np.concatenate.
 *   cs_partition_by_label: d_label int32 [N] (part label per voxel, clamped to 0..7), d_off int64 [n_cloud+1]
 *     (DEVICE) -> d_order int64 [N]: rows of every cloud stably partitioned by label (parts in order, original
 *     order inside a part).
 *   cs_cfg_bad: d_nn int32 [.., k], d_first int64 [n_cfg+1] (DEVICE, row ranges) -> d_bad int32 [n_cfg]: 1 when a
 *     range holds a negative neighbour (a CAD part with fewer than k voxels; the reference dies there, this
 *     build drops the configuration, DESIGN "Deliberate differences").  Over the vanilla list with one range per
 *     pair (CAD clouds of k voxels or more) it is the test "a query descriptor row of the pair is not finite".
 *   cs_rows_nonfinite: d_x f32 [.., dim], d_first int64 [n_seg+1] (DEVICE, row ranges) -> d_bad int32 [n_seg]: 1 when
 *     a row of the range holds a NaN or infinite element (the CAD side of that test: such a row is nobody's
 *     neighbour and leaves no -1 behind).  sym_pose_batch raises ValueError on either flag, as SciPy's KD-tree does.
 *   cs_corr_assemble: d_desc int64 [n_cfg,5] (DEVICE) = {q_first, n_first, t_first, len, out_first} per
 *     configuration; writes d_src / d_tgt f32 [sum len * k, 3]: query point of d_rows[q_first + i] (d_rows NULL:
 *     row q_first + i) repeated k times against CAD points t_first + d_nn[n_first + i][0..k).  max_len = largest len.
 *     A -1 entry is read as the CAD cloud's row 0 (never an address in front of the buffer); the callers discard
 *     lists that hold one.
 * ---------------------------------------------------------------------------------------- */
int cs_partition_by_label(const int32_t* d_label, const int64_t* d_off, int n_cloud, int64_t* d_order, void* stream);
int cs_cfg_bad(const int32_t* d_nn, int k, const int64_t* d_first, int n_cfg, int32_t* d_bad, void* stream);
int cs_rows_nonfinite(const float* d_x, int dim, const int64_t* d_first, int n_seg, int32_t* d_bad, void* stream);
int cs_corr_assemble(const float* d_xyz0, const float* d_xyz1, const int64_t* d_rows, const int32_t* d_nn, int k,
                     const int64_t* d_desc, int n_cfg, int64_t max_len, float* d_src, float* d_tgt, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training batches (datasets/CategoryDataset.py:121-296 builds one triplet at a time on the host).
 *
 * Fixed-radius pairs.  Replaces utils/preprocess.py:207-228 get_matching_indices (an Open3D KDTreeFlann
 * search_radius_vector_3d per source point, run from a Python loop), as generate_local_pair
 * (datasets/CategoryDataset.py:121-151) calls it.  Segments as cs_knn_feat: problem p searches source segment
 * h_src_seg[p] of (d_src, h_soff) against target segment h_tgt_seg[p] of (d_tgt, h_toff); points f64 [n,3].
 * Pair (i, j) is kept iff d2 < r2 with d2 = ((sx-tx)^2 + (sy-ty)^2) + (sz-tz)^2 in f64 without contraction
 * and r2 = radius * radius.  [O3D-knowledge] Open3D's radius search compares squared distances strictly (a
 * target at exactly r is not returned) and returns the hits sorted by distance; it leaves the order of equal
 * distances unspecified -- here ties are broken by ascending target index.
 * Output CSR over the source rows of all problems (problem-major, rows ascending): d_row_ptr int64 [rows+1];
 * row r's targets (indices LOCAL to the target segment) in ascending (d2, index), at most k_max of them
 * (k_max <= 0: all), like idx[:K] in the reference.
 *   cs_radius_pairs enqueues the search and the row offsets and returns a plan; it does not wait.  The caller
 *   reads the total (d_row_ptr[rows]) to size d_tgt_idx int32 [total] -- the only host wait -- and calls
 *   cs_radius_pairs_fill with the same d_row_ptr while d_src and d_tgt are alive and unchanged, then frees the
 *   plan.  Rows of any length are exact and ordered.
 * ---------------------------------------------------------------------------------------- */
typedef struct cs_radius_plan cs_radius_plan;
int cs_radius_pairs(const double* d_src, const int64_t* h_soff, const double* d_tgt, const int64_t* h_toff,
                    const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, double radius, int k_max,
                    int64_t* d_row_ptr, void* stream, cs_radius_plan** plan);
int cs_radius_pairs_fill(const cs_radius_plan* plan, const int64_t* d_row_ptr, int32_t* d_tgt_idx, void* stream);
void cs_radius_plan_free(cs_radius_plan* plan);

/* Pair sampling of a triplet batch.  Replaces generate_rand_negative_pairs + _hash (utils/preprocess.py:231-259)
 * and the shuffle / [:sample] of generate_local_pair (datasets/CategoryDataset.py:121-151).  d_xyz f32 [n,3] holds
 * the kept CANONICAL points of every cloud (segments h_off); problem p is triplet slot h_slot[p] with base, positive
 * and negative segments h_base_seg[p], h_pos_seg[p], h_neg_seg[p]; its PiP CSR rows are [h_row_base[p],
 * h_row_base[p+1]) of (d_row_ptr, d_tgt_idx) as cs_radius_pairs made them with k_max = 0 (base -> positive).
 * Randomness: u64 = rng(seed, slot, round, stream, ctr) = x of the generator in common.h with itr = 0 and
 *   j = slot << 40 | round << 36 | stream << 32 | ctr, i.e.
 *   x = seed + 0x9E3779B97F4A7C15 * (j + 1)  (mod 2^64);  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;
 *   x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 * and a uniform index below N is floor(u * N) in f64 with u = (x >> 11) * 2^-53.
 *   PiP (lists & 1, stream 0): pair t of the problem (CSR order) gets key (rng(.., 0, t) >> 32) << 32 | t; the
 *     min(sample, n_pos) pairs of smallest key, ascending (ties of the random part by pair index).
 *   PiN (lists & 2, stream 1): n_draw = n_pos candidates; candidate t = (index(rng(.., 1, 2t), N0),
 *     index(rng(.., 1, 2t+1), N1)); dropped when it is a positive pair (d2 < r2 in f64, the PiP test itself --
 *     exactly membership in the uncapped PiP set) or when sqrt((dx*dx + dy*dy) + dz*dz) <= 0.1 in f32 (NumPy's
 *     np.linalg.norm on the f32 clouds, CategoryDataset.py:141-145); the first `sample` survivors in draw order.
 *   NiN (lists & 2, stream 2): the same on base x negative, excluding only the pair (0, 0).
 * d_pip / d_pin / d_nin int32 [n_prob * sample, 2]: problem p's pairs at rows [p * sample, ...), indices local to
 * the segments.  d_counts int32 [n_prob, 4] = {n_pos, PiP, PiN, NiN} (entries of lists not asked for are left
 * alone).  PiN / NiN need only the row offsets, so they may run before the caller's host wait for the total.
 * 1 <= sample <= 4096, 0 <= round < 16, slot < 2^24.  No waits, no float atomics: results are bit-identical. */
int cs_sample_pairs(const float* d_xyz, const int64_t* h_off, const int32_t* h_base_seg, const int32_t* h_pos_seg,
                    const int32_t* h_neg_seg, const int32_t* h_slot, int n_prob, const int64_t* h_row_base,
                    const int64_t* d_row_ptr, const int32_t* d_tgt_idx, int lists, uint64_t seed, int round,
                    double radius, int sample, int32_t* d_pip, int32_t* d_pin, int32_t* d_nin, int32_t* d_counts,
                    void* stream);

/* Rigid transform of the train-mode augmentation in f64.  Replaces np.matmul(R, pc[:, :, None])[:, :, 0] + T of
 * random_rotation (utils/preprocess.py:73-86) and apply_transform (:39-48) in CategoryDataset.py:229-241:
 * out = the segments h_seg[p] of d_xyz (f32 [n,3], widened exactly), concatenated problem-major, each mapped by
 * the row-major 4x4 d_T[p] (f64 [n_prob,16]) as x' = ((r00 x + r01 y) + r02 z) + t0 per coordinate, no
 * contraction.  (The reference's matmul order depends on the BLAS)  Quantise with cs_voxelize_f64. */
int cs_transform_f64(const float* d_xyz, const int64_t* h_off, const int32_t* h_seg, int n_prob, const double* d_T,
                     double* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Metric-learning loss on feature pairs: the FCGF-form contrastive loss that the PiP / PiN / NiN lists
 * of a training batch feed.  The reference ships the pair lists and no loss: this is the specification.
 *
 * One call evaluates up to CS_PAIR_LOSS_MAX_TERMS terms over n_mat distinct feature matrices d_mat[m] (f32
 * [h_rows[m], C] with leading dimension h_ld[m] >= C, 1 <= C <= 256).  Term t pairs rows of matrix h_a[t] (A) with
 * rows of matrix h_b[t] (B) through d_pairs[t] (int32 [h_npairs[t], 2]: row of A, row of B; at most 2^22 pairs; rows
 * out of range are a caller error that is not detected), with kind h_kind[t], margin h_margin[t] in [0, 16] and weight
 * h_weight[t] in [0, 1024].  Several terms may name the same matrix.  h_npairs[t] = 0 is legal: the term is 0 and
 * contributes no gradient.  PRECONDITION: every feature row has norm <= 8 (the network's rows are unit vectors), so
 * d <= 16; rows outside it (or non-finite) give meaningless numbers but no fault.
 * Arithmetic (every operation one IEEE f32 operation unless it says f64; no contraction):
 *   pair p = (i, j): diff_k = A[i][k] - B[j][k];  s = 0, s = s + diff_k * diff_k for k ascending;  d = sqrt(s);
 *     h = max(d - m, 0) for PULL, max(m - d, 0) for PUSH;  l_p = h * h.
 *   value: S_t = sum_p (uint64)((double)l_p * 2^32) (cast truncates), an exact 64-bit integer sum (l_p <= 2^8, so
 *     S_t <= 2^8 * 2^32 * 2^22 = 2^62);  L_t = w * (double)S_t * 2^-32 / P in f64, 0 when P = 0.
 *     d_term_loss f64 [n_term] = L_t, d_total f32 [1] = (float)(sum_t L_t), summed in f64 in term order.
 *   gradient: r_t = (float)((double)w / P).  A pair with h > 0 and d > 0: a = (h + h) * r_t; u_k = diff_k / d;
 *     e_k = a * u_k (negated for PUSH); row i of A's matrix gets +e_k, row j of B's gets -e_k, each entering a 64-bit
 *     integer accumulator as (int64)((double)e_k * 2^44) (cast truncates toward zero; |e_k| <= 32 w / P, so an
 *     accumulator stays below 32 * 1024 * 2^44 = 2^59 even if every pair of a term hits one row).  All terms'
 *     contributions to one matrix land in ONE output: d_grad[m] f32 [h_rows[m], C], leading dimension h_ld_grad[m],
 *     element = (float)((double)acc * 2^-44) * g with g = d_grad_up[0] read on the device.  Every element is written
 *     (zeros where nothing contributes).
 * Integer sums: the results do not depend on the order of the pairs, the launch shape or the run.  No host waits.
 * Refused arguments (status < 0, cs_last_error) leave the outputs untouched.
 * ---------------------------------------------------------------------------------------- */
#define CS_PAIR_LOSS_MAX_TERMS 8
#define CS_PAIR_PULL 0
#define CS_PAIR_PUSH 1
int cs_pair_loss_fwd(int n_mat, const float* const* d_mat, const int64_t* h_rows, const int32_t* h_ld, int C,
                     int n_term, const int32_t* h_a, const int32_t* h_b, const int32_t* h_kind, const float* h_margin,
                     const double* h_weight, const int32_t* const* d_pairs, const int64_t* h_npairs,
                     double* d_term_loss, float* d_total, void* stream);
int cs_pair_loss_bwd(int n_mat, const float* const* d_mat, const int64_t* h_rows, const int32_t* h_ld, int C,
                     int n_term, const int32_t* h_a, const int32_t* h_b, const int32_t* h_kind, const float* h_margin,
                     const double* h_weight, const int32_t* const* d_pairs, const int64_t* h_npairs,
                     const float* d_grad_up, float* const* d_grad, const int32_t* h_ld_grad, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hardest negatives in feature space: for every anchor row of a query cloud, the feature-nearest row of the
 * problem's target cloud that is not a spatial neighbour of the anchor in the canonical frame.  FCGF trains the
 * contrastive loss of cs_pair_loss_* with such negatives; the reference ships pair lists and no loss: this
 * is the specification.
 *   Features: d_qf f32 [nq, C] with leading dimension ld_q >= C, d_tf likewise with ld_t; 1 <= C <= 256.
 *   Points: d_qxyz / d_txyz f32 [., 3] (contiguous), the canonical points, row-aligned with the features.
 *   Segments and problems: segment tables h_qoff / h_toff, problem p searches target segment h_tseg[p] for the anchors
 *     of query segment h_qseg[p], p < n_prob, as in cs_knn_feat.  A query segment may appear in at most one problem
 *     (otherwise status < 0): an anchor has exactly one problem.
 *   Anchors: d_anchor int32 [A], GLOBAL query rows in any order, duplicates allowed.  An anchor belongs to the problem
 *     whose query segment contains its row; the library finds it on the device from the offsets it uploads once (no
 *     per-problem anchor table).  Anchors live on the device and the call does not wait, so an anchor whose row is
 *     outside [0, h_qoff[last]) or whose segment is in no problem cannot be refused by the status: it is answered
 *     -1 / +inf.
 *   Admissibility: target row j of the problem's target segment is admissible for anchor row i iff
 *     NOT ((dx*dx + dy*dy) + dz*dz) < r*r   with d. = (double)q. - (double)t., every operation one f64 operation,
 *     no contraction, r*r = radius * radius in f64 -- the PiP test of cs_radius_pairs itself.  radius <= 0 admits
 *     every row.
 *   Result: the admissible row of smallest f64 squared feature distance d = 0, d = fma(diff_c, diff_c, d) with
 *     diff_c = (double)q_c - (double)t_c for c ascending from 0 (the canonical k-NN arithmetic); ties go to
 *     the smaller row index.
 *   Outputs: d_idx int32 [A] = that row LOCAL to the target segment, -1 when no row is admissible (an empty target
 *     segment included); d_dist f64 [A], optional = sqrt(d), +inf for -1.  Entry a answers d_anchor[a].
 *   Stream behaviour: everything is enqueued on `stream`; no host waits, no float atomics.  The result does not depend
 *     on the order of the anchors or on the launch shape.  A = 0 and n_prob = 0 are legal.  Refused arguments
 *     (status < 0, cs_last_error) leave the outputs untouched.
 *   Paths: C = 16 ranks on the f16 matrix cores (hi / lo cut of every feature), evaluates the shortlisted rows with
 *     the canonical chain and the exact admissibility test and accepts a winner only when every row that was not
 *     evaluated exactly has a lower bound above the winner's exact distance (a tie counts as not vouched for); the
 *     other anchors, every other C, and every anchor under CS_HARDNEG_MFMA=0 go through the exhaustive kernel.  All
 *     return the same indices and distances.
 *   cs_hardest_stats: out = {anchors answered, of those recomputed exhaustively}, counted only while the environment
 *     variable CS_HARDNEG_STATS=1 (the count synchronises), as cs_knn_shortlist_stats.
 * Profile family "hardneg".
 * ---------------------------------------------------------------------------------------- */
int cs_hardest_negatives(const float* d_qf, int ld_q, const float* d_qxyz, const int64_t* h_qoff, const float* d_tf,
                         int ld_t, const float* d_txyz, const int64_t* h_toff, const int32_t* h_qseg,
                         const int32_t* h_tseg, int n_prob, int C, const int32_t* d_anchor, int64_t A, double radius,
                         int32_t* d_idx, double* d_dist, void* stream);
void cs_hardest_stats(uint64_t out[2], int reset);

/* ------------------------------------------------------------------------------------------
 * cs_icp_batch: batched point-to-point ICP, the refinement behind a global registration.  It follows Open3D's
 * registration_icp with TransformationEstimationPointToPoint(with_scaling = false) and
 * ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration); the reference has no such step, so this comment
 * is the specification (tests/icp_ref.py restates it bit for bit).  Every operation below is ONE IEEE f64 operation
 * unless a fused fma(a, b, c) is written; nothing is contracted.
 *   Problems: problem p < n_prob owns source segment h_src_seg[p] of d_src (f32 [n,3], offsets h_soff) and target segment
 *     h_tgt_seg[p] of d_tgt (offsets h_toff), selected as in cs_chamfer_1dir; segments may be shared between problems.
 *     d_T0 f32 [n_prob,16]: the initial transforms, row-major 4x4 as cs_ransac_batch writes them, widened to f64 (T).
 *   Pose: every round poses the ORIGINAL source rows (x, y, z) with the current T (row c = T_c0..T_c3):
 *       p_c = fma(T_c0, x, fma(T_c1, y, fma(T_c2, z, T_c3)))      -- the chain of cs_chamfer_1dir.
 *     (Open3D transforms the cloud cumulatively and so accumulates the roundings of every iteration; deliberate difference.)
 *   Association: for a source the target row j of its segment with the smallest canonical squared distance
 *       d2 = fma(dz, dz, fma(dy, dy, dx * dx)),  d. = p. - (double)t.,
 *     ties to the smaller row.  The pair is kept iff d2 < max_dist * max_dist, strictly ([O3D-knowledge]: Open3D's
 *     hybrid search keeps a neighbour AT the radius; a strict threshold is the choice cs_ransac_batch made for max_corr).
 *     A source whose distances are all NaN / +inf has no pair.
 *   Evaluation: n_corr = kept pairs; fitness = n_corr / n_src (0 for an empty source segment);
 *     rmse = sqrt(sum_d2 / n_corr) (0 when n_corr = 0), sum_d2 from the fixed-point sum below.
 *   Sums: per problem 17 signed 64-bit integer sums over the kept pairs (p, q = (double) target row), relative to the origin
 *     o_c = 0.5 * (min_c + max_c) of the target segment's bounding box (f32 min / max widened to f64; o = 0 when the segment
 *     is empty or the box is not finite), p' = p - o, q' = q - o:
 *       count;  I(p'_c * 2^s1), I(q'_c * 2^s1) for c = x, y, z;  I((p'_a * q'_b) * 2^s2) for a, b in x, y, z;  I(d2 * 2^s2),
 *     I(v) = (int64) of v clamped to +-2^(61 - eN), truncating toward zero.  With h = max_c 0.5 * (max_c - min_c) (0 like o),
 *     M = h + max_dist = m * 2^eM (frexp: 0.5 <= m < 1; eM clamped to [-100, 400]) and eN the smallest integer with
 *     n_src <= 2^eN:  s1 = 61 - eN - eM,  s2 = 61 - eN - 2 eM.  Every kept pair has |p'_c|, |q'_c| <= M, so no term reaches
 *     the clamp and no sum leaves 2^61.  Integer sums: the same in any order.
 *   Update (one problem, from its sums, n = count): sp_c = (double)Sp_c * 2^-s1, sq_c likewise, mp = sp / n, mq = sq / n;
 *     S_ab = fma(-sp_a, mq_b, (double)Spq_ab * 2^-s2) (the cross-covariance about the means, source index first);
 *     Horn's N from S, its largest eigenvector by horn_qcp with jacobi4 as fallback (corsair_amd/csrc/horn.h, the
 *     RANSAC's solver and selection rules), the quaternion normalised by division, R as in cs_ransac_batch;
 *     pm = mp + o, qm = mq + o, t_a = qm_a - fma(R_a2, pm_2, fma(R_a1, pm_1, R_a0 * pm_0));  T <- U T with
 *       T'_ab = fma(R_a0, T_0b, fma(R_a1, T_1b, R_a2 * T_2b))  (b < 3),
 *       T'_a3 = fma(R_a0, T_03, fma(R_a1, T_13, fma(R_a2, T_23, t_a)));  the last row of T stays that of T0.
 *   Loop: evaluate T0; then repeat { update; evaluate } and stop after the evaluation in which |fitness - previous fitness| <
 *     relative_fitness AND |rmse - previous rmse| < relative_rmse, or after max_iter updates.  A problem stops at once, keeping
 *     its current T, when an evaluation has n_corr < 3 or a non-finite value, or an update would make T non-finite.
 *     max_iter = 0 evaluates T0 only (Open3D's evaluate_registration).
 *   Outputs: d_T f64 [n_prob,16]; d_T32 f32 [n_prob,16], optional = d_T cast once at the end; d_fitness, d_rmse f64 and
 *     d_ncorr int32 [n_prob] of the LAST evaluation (the one of the returned T); d_iters int32 [n_prob] = updates applied;
 *     d_corr int32, optional, one entry per source row of every problem, problem-major (problem p starts at the sum of the
 *     source counts of the problems before it): the target row LOCAL to its segment of the last evaluation, -1 = no pair.
 *   Independence: a problem's result depends on that problem alone -- not on its batch neighbours, on the order of the
 *     source rows inside its segment, on the launch shape or on the run.
 *   Empty source or target segment: answered with fitness 0, rmse 0, T = T0, 0 iterations.  n_prob = 0 is legal.
 *   Refused (CS_ERR_INVALID): NULL tables or outputs, negative segment ids or sizes, max_dist <= 0 or not finite, NaN
 *     thresholds; (CS_ERR_UNSUPPORTED): max_iter outside [0, 1000], a segment of 2^31 rows or more.
 *   Stream behaviour: everything is enqueued on `stream`, max_iter + 1 rounds; convergence is a per-problem device flag on
 *     which the workgroups of a finished problem leave -- no host wait (CS_ICP_STATS=1 adds one at the end).  Scratch comes
 *     from the calling thread's pool; no float atomics.
 *   Paths: the association ranks by |t|^2 - 2 p.t on the f16 matrix cores over the image cs_chamfer_1dir uses (built once
 *     per call), evaluates the rows of a lane's best tiles with the canonical chain keeping (distance, row), and accepts a
 *     result only when it lies STRICTLY below the smallest unevaluated tile minimum minus the error budget; workgroups it
 *     cannot vouch for, or with coordinates outside the f16 range (|c| >= 60), are recomputed by the exhaustive kernel,
 *     which is the whole path under CS_ICP_F16=0.  Both return the same bits.
 *   cs_icp_stats: out = {256-source workgroups answered by the f16 path, of those recomputed}, summed over the rounds,
 *     counted only while CS_ICP_STATS=1.
 * Profile family "icp".
 * ---------------------------------------------------------------------------------------- */
int cs_icp_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const int64_t* h_toff,
                 const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, const float* d_T0, double max_dist,
                 int max_iter, double relative_fitness, double relative_rmse, double* d_T, float* d_T32,
                 double* d_fitness, double* d_rmse, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream);
void cs_icp_stats(uint64_t out[2], int reset);

/* ------------------------------------------------------------------------------------------
 * cs_icp_plane_batch: cs_icp_batch with Open3D's TransformationEstimationPointToPlane in the place of the point-to-point
 * estimation (tests/icp_plane_ref.py restates it bit for bit).  The arguments are those of cs_icp_batch plus
 * d_tgt_normal f32 [rows of d_tgt, 3], the normal of every target row (cs_estimate_normals, or the caller's own; they need
 * not be unit vectors and their sign does not matter).  Problems, pose chain, association (both paths, the strict
 * voucher, CS_ICP_F16, CS_ICP_STATS / cs_icp_stats), evaluation (rmse from the POINT distances d2, as [O3D-knowledge]
 * Open3D's evaluation has it for every estimation), loop, stop rule, outputs, independence, empty-segment answers, refusals
 * (+ a NULL d_tgt_normal while a target row exists) and stream behaviour are those of cs_icp_batch: the same code.  What
 * differs is the sums and the update.
 *   Per kept pair, with o, M, eM, eN of cs_icp_batch: p' = p - o, n = (double) normal row of the matched target,
 *     e = p - q, r = fma(e_z, n_z, fma(e_y, n_y, e_x * n_x)), a = p' x n with a_x = fma(p'_y, n_z, -(p'_z * n_y)),
 *     a_y = fma(p'_z, n_x, -(p'_x * n_z)), a_z = fma(p'_x, n_y, -(p'_y * n_x)), J = (a_x, a_y, a_z, n_x, n_y, n_z).
 *   Sums: 29 signed 64-bit integers: count; I((J_i * J_j) * 2^s) for i <= j, row-major (21); I((J_i * r) * 2^s) (6);
 *     I(d2 * 2^s2).  Each product is rounded to f64 first; I clamps to +-2^(61 - eN) and truncates.  With b = 61 - eN the
 *     exponents s are, for i, j < 3 (rot x rot) b - 2 eM - 3, for i < 3 <= j (rot x trans) b - eM - 2, for 3 <= i, j
 *     (trans x trans) b - 1, for J_i r with i < 3 b - 2 eM - 2 and with i >= 3 b - eM - 1: a kept pair has |p'_c| <= M,
 *     |r| < max_dist <= M and, for unit normals, |n_c| <= 1, each class carries one bit for the roundings, no term reaches
 *     the clamp and no sum leaves 2^61; the clamp keeps that true for any normals.
 *   Update: A_ij = (double)sum * 2^-s (symmetric 6x6), b_i likewise; A x = -b by an unpivoted Cholesky, columns j = 0..5:
 *       d = A_jj, then d = fma(-L_jk, L_jk, d) for k < j;  L_jj = sqrt(d);
 *       L_ij (i > j) = (A_ij, then fma(-L_ik, L_jk, .) for k < j) / L_jj;
 *       y_i = (-b_i, then fma(-L_ik, y_k, .) for k < i) / L_ii;   x_i (i = 5..0) = (y_i, then fma(-L_ki, x_k, .) for
 *       k = i+1..5) / L_ii.
 *     The quaternion (1, 0.5 x_0, 0.5 x_1, 0.5 x_2) is normalised by division and turned into R as in cs_ransac_batch (the
 *     Cayley rotation; [O3D-knowledge] Open3D composes Rz Ry Rx of the three solved angles and solves by LDLT);
 *     t_a = (x_(3+a) + o_a) - fma(R_a2, o_2, fma(R_a1, o_1, R_a0 * o_0));  T <- U T by cs_icp_batch's chain.
 *   A problem stops at once, keeping T, when an evaluation has n_corr < 6 (3 for cs_icp_batch) or a non-finite value, when
 *     a pivot d is not finite or not greater than 2^-30 * A_jj, or when the update would make T non-finite.
 * Profile family "icp".
 * ---------------------------------------------------------------------------------------- */
int cs_icp_plane_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                       const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                       const float* d_T0, double max_dist, int max_iter, double relative_fitness, double relative_rmse,
                       double* d_T, float* d_T32, double* d_fitness, double* d_rmse, int32_t* d_iters, int32_t* d_ncorr,
                       int32_t* d_corr, void* stream);

/* ------------------------------------------------------------------------------------------
 * cs_icp_plane_robust_batch: cs_icp_plane_batch with a robust kernel on the point-to-plane residual, the RobustKernel
 * argument of Open3D's TransformationEstimationPointToPlane (tests/icp_robust_ref.py restates it bit for bit).
 * The arguments are those of cs_icp_plane_batch plus `kernel` (CS_ICP_KERNEL_*), `kernel_scale` (k) and one more optional
 * output, d_wfitness f64 [n_prob].  Everything not said here -- problems, pose chain, association on both paths, evaluation,
 * loop, stop rules, outputs, independence, empty segments, stream behaviour -- is cs_icp_plane_batch's: the same code.
 *   Weight of a kept pair, from r of cs_icp_plane_batch, a = |r|, k = kernel_scale, every operation ONE IEEE f64 operation
 *   ([O3D-knowledge]: Open3D's HuberLoss, CauchyLoss and TukeyLoss::Weight as remembered; not checked against Open3D):
 *       L2:      w = 1
 *       Huber:   w = (a <= k) ? 1 : k / a
 *       Cauchy:  q = r / k;  w = 1 / (1 + q * q)
 *       Tukey:   if (!(a < k)) w = 0;  else { q = r / k;  e = 1 - q * q;  w = e * e; }
 *     and a w that is NaN becomes 0.  (Open3D's GM and L1 kernels are left out on purpose: their weights, k / (k + r^2)^2
 *     with k < 1 and 1 / |r|, are not bounded by 1 and the bound below would not hold.)
 *   Sums: 30 signed 64-bit integers, the 29 of cs_icp_plane_batch and one more.  Each of the 27 products J_i * J_j and
 *     J_i * r is rounded to f64 as there, THEN multiplied by w (one more rounding), then scaled by its class's power of two,
 *     clamped to +-2^(61 - eN) and truncated.  The count and I(d2 * 2^s2) stay unweighted: fitness, rmse and n_corr are
 *     Open3D's evaluation, the numbers cs_icp_plane_batch returns for the same pose.  The 30th sum is I(w * 2^(61 - eN)).
 *     Bound: 0 <= w <= 1 and rounding is monotone, so |fl(x * w)| <= |x|: no weighted term is larger than the unweighted
 *     term that cs_icp_plane_batch bounds, and the 30th sum has at most 2^eN terms of at most 2^(61 - eN).  Nothing leaves
 *     2^61, and the clamp keeps that true for any input.
 *   d_wfitness = ((double)sum_w * 2^-(61 - eN)) / n_src of the last evaluation: the weighted inlier share (0 for an empty
 *     source segment; equal to the fitness with L2).
 *   Update and stop rules: cs_icp_plane_batch's on the weighted A and b.  When every weight is 0 (Tukey with every
 *     |r| >= k) A is exactly zero, the first pivot fails cs_icp_plane_batch's pivot rule and the problem stops after that
 *     evaluation: T = T0 when it is the first, 0 updates, wfitness 0.
 *   kernel = CS_ICP_KERNEL_L2 runs cs_icp_plane_batch's code and returns its bits; kernel_scale is ignored then.
 *   Refused (CS_ERR_INVALID) in addition: kernel outside 0..3; kernel_scale not finite or <= 0 while kernel != L2.
 * Profile family "icp".
 * ---------------------------------------------------------------------------------------- */
#define CS_ICP_KERNEL_L2 0
#define CS_ICP_KERNEL_HUBER 1
#define CS_ICP_KERNEL_CAUCHY 2
#define CS_ICP_KERNEL_TUKEY 3
int cs_icp_plane_robust_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                              const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                              const float* d_T0, double max_dist, int max_iter, double relative_fitness,
                              double relative_rmse, int kernel, double kernel_scale, double* d_T, float* d_T32,
                              double* d_fitness, double* d_rmse, double* d_wfitness, int32_t* d_iters, int32_t* d_ncorr,
                              int32_t* d_corr, void* stream);

/* ------------------------------------------------------------------------------------------
 * cs_icp_scale_batch: cs_icp_batch (d_tgt_normal = NULL) or cs_icp_plane_batch (d_tgt_normal != NULL) with one more unknown,
 * an isotropic scale of the source: Open3D's TransformationEstimationPointToPoint(with_scaling = true) for the point
 * estimation; the plane estimation with a scale has no Open3D counterpart (tests/icp_scale_ref.py restates both
 * bit for bit).  The arguments are those of cs_icp_plane_batch plus scale_min, scale_max and the output d_scale f64 [n_prob].
 * Problems, pose chain, association (both paths, the strict voucher, CS_ICP_F16, CS_ICP_STATS / cs_icp_stats), evaluation,
 * loop, stop criteria, outputs, independence, empty-segment answers (scale 1), refusals and stream behaviour are those of
 * cs_icp_batch: the same code.  T then carries s R in its upper block.  The association only ever sees POSED points
 * p = T x: the f16 range test (|p_c| < 60), the voucher and its error budget (a function of |p| and of the largest |t|) are
 * evaluated on p, whatever T produced it, so nothing there assumes a rotation and both paths still return the same bits.
 * Every operation below is ONE IEEE f64 operation unless a fused fma(a, b, c) is written.
 *   Point + scale.  18 sums: the 17 of cs_icp_batch and I(pp * 2^(s2 - 2)), pp = fma(p'_z, p'_z, fma(p'_y, p'_y, p'_x * p'_x))
 *     <= 3 M^2 < 2^(2 eM + 2), so no term reaches the clamp.  sp, sq, mp, mq, S, R as in cs_icp_batch, then
 *       den = (double)Spp * 2^-(s2 - 2), then den = fma(-sp_a, mp_a, den) for a = x, y, z;
 *       num = R_00 * S_00, then num = fma(R_ab, S_ab, num) for the other eight (a, b), row-major;   s_u = num / den;
 *       t_a = fma(-s_u, fma(R_a2, pm_2, fma(R_a1, pm_1, R_a0 * pm_0)), qm_a);   U = [s_u * R_ab | t]
 *     (Umeyama's fit with R from Horn's quaternion).  The problem stops when an evaluation has n_corr < 3.
 *   Plane + scale.  The Jacobian gets a seventh column J_6 = fma(p'_z, n_z, fma(p'_y, n_y, p'_x * n_x)) (the derivative of
 *     the residual by sigma in p <- (1 + sigma) R p' + t'), |J_6| <= sqrt(3) M < 2 M like a rotational column.  37 sums: count;
 *     I((J_i * J_j) * 2^s) for i <= j < 7, row-major (28); I((J_i * r) * 2^s) (7); I(d2 * 2^s2).  A column is rotational for
 *     i < 3 or i = 6, translational otherwise, and the exponents of cs_icp_plane_batch apply by class: both rotational
 *     b - 2 eM - 3, one of them b - eM - 2, none b - 1, J_i r b - 2 eM - 2 (rotational) or b - eM - 1.  The 7x7 system is
 *     solved by cs_icp_plane_batch's Cholesky sequence with 7 in the place of 6 and its pivot rule on all seven pivots;
 *       s_u = 1 + x_6;  R the Cayley rotation of (x_0, x_1, x_2);
 *       t_a = fma(-s_u, fma(R_a2, o_2, fma(R_a1, o_1, R_a0 * o_0)), x_(3+a) + o_a);   U = [s_u * R_ab | t],
 *     the map x -> s_u R (x - o) + o + t'.  The problem stops when an evaluation has n_corr < 7.
 *   T <- U T by cs_icp_batch's chain in both.
 *   Scale: d_scale[p] starts at 1 and becomes s_u * d_scale[p] with every applied update: the factor this call added to T0.
 *     A problem stops at once, keeping T and its scale, the update NOT applied, when den is not finite or not > 0 (point),
 *     when s_u is not finite or not > 0, or when s_u * d_scale[p] is not inside [scale_min, scale_max].  The interval is the
 *     guard against the collapse of a scaled ICP started far from the truth, which shrinks the source onto one target point
 *     while the rmse falls.  d_iters counts applied updates only.
 *   Refused (CS_ERR_INVALID) in addition, before anything is launched: bounds that are not finite, scale_min <= 0,
 *     scale_min > 1, scale_max < 1; a NULL d_scale.
 * Profile family "icp".
 * ---------------------------------------------------------------------------------------- */
int cs_icp_scale_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                       const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                       const float* d_T0, double max_dist, int max_iter, double relative_fitness, double relative_rmse,
                       double scale_min, double scale_max, double* d_T, float* d_T32, double* d_fitness, double* d_rmse,
                       double* d_scale, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream);

/* ------------------------------------------------------------------------------------------
 * cs_icp_gicp_batch: cs_icp_batch with a plane-to-plane estimation, Generalized ICP (Segal, Haehnel, Thrun, RSS 2009;
 * [O3D-knowledge] Open3D's registration_generalized_icp / TransformationEstimationForGeneralizedICP as remembered, not
 * checked against Open3D) in the place of the point-to-point estimation (tests/gicp_ref.py restates it bit for
 * bit).  The arguments are those of cs_icp_plane_batch plus d_src_normal f32 [rows of d_src, 3], the normal of every source
 * row in the source's OWN frame, `epsilon` and one more optional output, d_mrmse f64 [n_prob].  Problems, pose chain,
 * association (both paths, the strict voucher, CS_ICP_F16, CS_ICP_STATS / cs_icp_stats), evaluation (fitness and rmse from
 * the POINT distances d2), loop, stop criteria, outputs, independence, empty-segment answers (mrmse 0), and stream behaviour
 * are those of cs_icp_batch: the same code.  What differs is the sums and the update.  Every operation below is ONE IEEE f64
 * operation unless a fused fma(a, b, c) is written; only + - * / sqrt fma appear.
 *   Covariance of a row with normal n: C(n) = I - g n n^T, g = (1 - epsilon) / nn, nn = fma(n_z, n_z, fma(n_y, n_y, n_x * n_x))
 *     ([O3D-knowledge] Open3D's Rx diag(epsilon, 1, 1) Rx^T, Rx taking e_1 onto the normal, written without building Rx: valid
 *     for a normal of any length and either sign).  A normal with a non-finite component, or with nn zero or not finite, is
 *     replaced by n = 0, g = 0: C = I, the row is weighted isotropically.  1 - epsilon is computed once.
 *   Per kept pair, with o, M, eM, eN of cs_icp_batch: p' = p - o, e = p - q, n = (double) normal row of the matched
 *     target, s = (double) normal row of the source, m = A s with A the upper 3 x 3 block of the round's T:
 *       m_c = fma(T_c0, s_x, fma(T_c1, s_y, T_c2 * s_z))        -- the pose chain without the translation.
 *     Normalising m by m . m means a similarity T0 only ROTATES the source covariance (deliberate difference: Open3D forms
 *     T C_s T^T, which also scales it).  With g_t, g_s the gains of n and m, a_i = g_t * n_i, b_i = g_s * m_i:
 *       Mc = C(n) + C(m):  Mc_ii = fma(-b_i, m_i, fma(-a_i, n_i, 2)),  Mc_ij (i < j) = fma(-b_i, m_j, -(a_i * n_j));
 *     its eigenvalues lie in [2 epsilon, 2].  W = Mc^-1 by the adjugate over the determinant:
 *       c00 = fma(M11, M22, -(M12 * M12)),  c01 = fma(M02, M12, -(M01 * M22)),  c02 = fma(M01, M12, -(M02 * M11)),
 *       c11 = fma(M00, M22, -(M02 * M02)),  c12 = fma(M01, M02, -(M00 * M12)),  c22 = fma(M00, M11, -(M01 * M01)),
 *       det = fma(M02, c02, fma(M01, c01, M00 * c00)),  id = 1 / det,  W_ij = W_ji = c_ij * id;   |W|_2 <= 1 / (2 epsilon).
 *     u = W e: u_i = fma(W_i2, e_z, fma(W_i1, e_y, W_i0 * e_x)).  The Jacobian of p <- p + omega x p' + t is
 *     J = [-[p']x | I], three residual rows per pair; with x(p', v) = (fma(p'_y, v_z, -(p'_z * v_y)),
 *     fma(p'_z, v_x, -(p'_x * v_z)), fma(p'_x, v_y, -(p'_y * v_x))) the blocks of J^T W J and J^T W e are
 *       trans x trans: W;   rot x trans: K, column j of K = x(p', column j of W);
 *       rot x rot: row i of RR = x(p', row i of K), of which the entries j >= i are used;   J^T W e = (x(p', u), u).
 *     (Deliberate difference: Open3D builds residual rows with W^(1/2); its normal equations are these same J^T Mc^-1 J and
 *     J^T Mc^-1 e, without a matrix square root.)
 *   Sums: 30 signed 64-bit integers, in cs_icp_plane_batch's layout: count; the 21 entries i <= j, row-major, of the 6 x 6
 *     matrix [RR K; K^T W]; the 6 entries of (x(p', u), u); I(d2 * 2^s2); I(mc * 2^s), mc = fma(e_z, u_z, fma(e_y, u_y,
 *     e_x * u_x)), the Mahalanobis cost.  I clamps to +-2^(61 - eN) and truncates.  With eW the smallest integer with
 *     1 / (2 epsilon) <= 2^eW (-1 .. 9) and b = 61 - eN - eW the exponents are cs_icp_plane_batch's with that b: rot x rot
 *     b - 2 eM - 3, rot x trans b - eM - 2, trans x trans b - 1, x(p', u) b - 2 eM - 2, u b - eM - 1, and mc shares
 *     b - 2 eM - 2.  |p'_c| <= M, |p'| <= sqrt(3) M, |e| < max_dist <= M and |W|_2 <= 2^eW give |K_ij| < 2^(eM + 1 + eW),
 *     |RR_ij| <= 3 M^2 2^eW < 2^(2 eM + 2 + eW), |u_i| < 2^(eM + eW), |x(p', u)_i| < 2^(2 eM + 1 + eW), mc < 2^(2 eM + eW);
 *     each class carries one bit for the roundings, so no term reaches the clamp and no sum leaves 2^61 -- for normals of
 *     any length, since only their directions enter.  The clamp keeps the sums defined for any input.
 *   Update: cs_icp_plane_batch's, the same code: A and b from the sums, A x = -b by the unpivoted Cholesky sequence, the
 *     Cayley rotation of (x_0, x_1, x_2), t about o, T <- U T.
 *   A problem stops at once, keeping T, when an evaluation has n_corr < 6 or a non-finite value, when a pivot d is not
 *     finite or not greater than 2^-30 * A_jj, or when the update would make T non-finite.  The pivot floor is
 *     cs_icp_plane_batch's, kept on purpose: A >= (1/2) G and A_jj <= G_jj / (2 epsilon) for the point-to-point normal
 *     matrix G of the same pairs, so a pivot's share of its diagonal entry is at least epsilon (>= 2^-10) times the share
 *     the geometry gives G, and the floor only cuts geometry shares below 2^-20; a translational A_jj is at least n / 2 and
 *     is carried to n units of 2^-(60 - eN - eW), relative 2^-(59 - eN - eW), which stays 2^7 below the floor for segments
 *     of up to 2^13 sources at the smallest epsilon.  A single plane is NOT singular here: in the plane's
 *     directions the pairs pull with weight 1/2 like a point-to-point estimation, so the pivot rule does not fire and the
 *     problem runs to its criteria.
 *   d_mrmse = sqrt(sm / n_corr), sm = (double)sum_mc * 2^-s, of the last evaluation; 0 when n_corr = 0 or sm <= 0
 *     ([O3D-knowledge] Open3D's ComputeRMSE of this estimation).  It takes no part in the stop criteria.
 *   Refused (CS_ERR_INVALID) in addition to what cs_icp_plane_batch refuses: a NULL d_src_normal while a source row exists;
 *     epsilon not finite or outside [2^-10, 1] (Open3D's default 1e-3 is inside; epsilon = 1 makes every W = I / 2).
 *   Robust kernels and a scale are out of scope for this estimation.
 * Profile family "icp".
 * ---------------------------------------------------------------------------------------- */
int cs_icp_gicp_batch(const float* d_src, const float* d_src_normal, const int64_t* h_soff, const float* d_tgt,
                      const float* d_tgt_normal, const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg,
                      int n_prob, const float* d_T0, double max_dist, int max_iter, double relative_fitness,
                      double relative_rmse, double epsilon, double* d_T, float* d_T32, double* d_fitness, double* d_rmse,
                      double* d_mrmse, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream);

/* ------------------------------------------------------------------------------------------
 * cs_estimate_normals: one surface normal per row from the k nearest rows of the row's own segment, the semantics of
 * [O3D-knowledge] Open3D's PointCloud::estimate_normals(KDTreeSearchParamKNN(k)): the eigenvector of the smallest
 * eigenvalue of the neighbourhood's covariance.  The reference has no such step, so this comment is the specification
 * (tests/normals_ref.py restates it bit for bit).  Every operation is ONE IEEE f64 operation or an explicit fma; nothing is
 * contracted; only + - * / sqrt fma appear (no transcendental function, so a Python restatement can match every bit).
 *   d_xyz f32 [n,3]; h_off int64 [n_seg + 1] host offsets; d_normal f32 [n,3].
 *   Neighbours of row i of a segment of sn rows: the m = min(k, sn) rows j of the SAME segment with the smallest
 *     (d2, j), d2 = fma(dz, dz, fma(dy, dy, dx * dx)), d. = (double)x_j. - (double)x_i., ties to the smaller row, the row
 *     itself included ([O3D-knowledge]: a k-NN query of a cloud's own point returns that point first).  A row whose d2 is
 *     NaN or +inf is never a neighbour, so fewer than m may be found; m' = the number found.  k in [3, 32].
 *   m' < 3: the normal is (0, 0, 1) ([O3D-knowledge]: Open3D's answer for fewer than three neighbours).
 *   Scatter matrix about the query row, over the neighbours in (d2, j) order: u = (double)x_j - (double)x_i;
 *     s_a = s_a + u_a;  C_ab = fma(u_a, u_b, C_ab) (a <= b);  then S_ab = fma(-(s_a / m'), s_b, C_ab) (a <= b, mirrored).
 *     ([O3D-knowledge]: Open3D accumulates the raw second moments about the origin; about the query row the cancellation
 *     is between neighbour-sized numbers.)
 *   Eigenvector: jacobi3 (corsair_amd/csrc/horn.h: cyclic Jacobi, 5 sweeps, jacobi4's rotation) on S; the column of the
 *     smallest diagonal entry, ties to the smaller column; divided by sqrt(fma(e_z, e_z, fma(e_y, e_y, e_x * e_x))); negated
 *     when its component of largest magnitude (the first such on ties) is negative ([O3D-knowledge]: Open3D leaves the sign
 *     to a later orientation step; point-to-plane ICP does not see it).  A non-finite S, a zero or non-finite length or a
 *     non-finite component gives (0, 0, 1).  One cast to f32.
 *     Exactly degenerate inputs have defined answers: rows of one plane z = const give (0, 0, 1); rows of one line along x
 *     give (0, 1, 0) (two zero eigenvalues, the smaller column); m' copies of one point give (1, 0, 0).
 *   Independence: a row's normal depends on its segment alone -- not on batch neighbours, the launch shape or the run --
 *     and on the ORDER of the rows inside the segment only through exact distance ties (which tied row enters the list, and
 *     the order of the sums among tied rows).
 *   n_seg = 0 and empty segments are legal.  Refused (CS_ERR_INVALID): a NULL offset table, a negative count, offsets that
 *     decrease, NULL d_xyz or d_normal while a row exists; (CS_ERR_UNSUPPORTED): k outside [3, 32], a segment of 2^31 rows
 *     or more.  (cs_knn_feat cannot serve this: its KNN_MAXK is 8, and it ranks features, not coordinates.)
 *   Paths, the same bits.  The exhaustive f64 scan of the row's own segment, staged through LDS, one thread
 *     per row with its neighbour list in registers, is the DEFINITION of the neighbour list and the whole path under
 *     CS_NORMALS_GRID=0 (read per call).  Otherwise a segment of more than 1024 rows is ranked on a cell grid
 *     (corsair_amd/csrc/cellgrid.h): the cell size c = 1.5 sqrt(k A / (pi n)) comes on the device from the segment's bounding
 *     box (A its surface area, n its rows; min / max are exact and order-free), every row probes the 27 cells around its
 *     own, and its list is accepted only when its k-th d2 lies STRICTLY below c^2 (1 - 2^-30) -- every row the 27 cells do
 *     not hold is then strictly farther, roundings of floor(x / c) and of the distance chain included (the argument is in
 *     normals.hip), so no unseen row can enter or tie.  Rows that are not accepted are compacted into a list (an integer
 *     counter; the order of the list reaches no output) and recomputed by the exhaustive scan, one wave per row.
 *     Segments with a bounding box of zero area (copies of one point, a single row, rows of one line) or one that is not
 *     finite, segments so far from the origin that a cell index would leave the 16-bit range, and segments of at most
 *     1024 rows go straight to the exhaustive kernel.  Everything is enqueued on `stream`; no host wait (CS_NORMALS_STATS=1
 *     adds one at the end); the atomics are integer (the table's compare-and-swap, the list's counter).
 * Profile family "normals".
 * ---------------------------------------------------------------------------------------- */
int cs_estimate_normals(const float* d_xyz, const int64_t* h_off, int n_seg, int k, float* d_normal, void* stream);

/* ------------------------------------------------------------------------------------------
 * cs_estimate_normals_hybrid: cs_estimate_normals with the neighbours of [O3D-knowledge] Open3D's
 * KDTreeSearchParamHybrid(radius, max_nn): the at most max_nn nearest rows inside the radius (DESIGN 15;
 * tests/normals_hybrid_ref.py restates it bit for bit).  d_xyz, h_off, n_seg, d_normal and stream are cs_estimate_normals'.
 *   Neighbours of row i: the rows j of the SAME segment with d2 < radius * radius (one f64 product; d2 is
 *     cs_estimate_normals' chain fma(dz, dz, fma(dy, dy, dx * dx)) on the coordinates widened to f64).  STRICT, the
 *     project's convention for every threshold ([O3D-knowledge]: Open3D's radius search keeps a point AT the radius; no
 *     measured input can tell the two apart, an integer lattice can).  Of those, the min(max_nn, found) smallest by
 *     (d2, j), ties to the smaller row, the row itself included.  A NaN or inf d2 is never a neighbour (also when
 *     radius * radius overflows to +inf: then every finite d2 passes and the call is cs_estimate_normals(k = max_nn)).
 *     max_nn in [3, 32]; radius finite and > 0.  A radius whose square underflows to 0 finds nothing.
 *   Everything after the neighbour list is cs_estimate_normals' -- the same code (nrm_finish, normals.hip): fewer than three
 *     neighbours give (0, 0, 1); the scatter about the query row in (d2, j) order, jacobi3, the selection, sign and
 *     degenerate rules, the one cast.  Independence as stated there.
 *   n_seg = 0 and empty segments are legal, and so is every n_seg and segment size cs_estimate_normals accepts.  Refused:
 *     what cs_estimate_normals refuses (max_nn in the place of k), and (CS_ERR_INVALID) a radius that is NaN, infinite or
 *     <= 0.
 *   Paths, the same bits:
 *     the exhaustive scan, cs_estimate_normals' kernel with the radius test added: the definition, the whole path under
 *       CS_NORMALS_GRID=0 (read per call), and the path of every segment of at most 512 rows (one LDS stage of the scan)
 *       and of a radius of 1e300 or more;
 *     the cell grid (corsair_amd/csrc/cellgrid.h, shared with cs_radius_pairs): cells of radius (1 + 2^-10), rows sorted
 *       by (segment, cell), an open-addressing table of the cells' ranges, every row probes the 27 cells around its own --
 *       complete for d2 < radius^2 by the argument in cellgrid.h, roundings of floor(x / cell) and of the distance chain
 *       included -- and keeps its list in registers, inserting by the full (d2, j) pair since candidates come in no
 *       particular order.  Cells clamp to the 16-bit key range: exact for any coordinates, only slower for far-out rows.
 *       The 16-bit segment field of the key means the grid is built per chunk of 65 535 segments.
 *   Everything is enqueued on `stream`; no host wait; the only atomics are the table's integer compare-and-swap, whose
 *     order reaches no output.
 *   cs_normals_stats: out = {rows answered by a grid path, of those recomputed by the exhaustive scan}, counted only while
 *     CS_NORMALS_STATS=1.  The hybrid grid is complete and recomputes nothing.
 * Profile family "normals", one scope per call.
 * ---------------------------------------------------------------------------------------- */
int cs_estimate_normals_hybrid(const float* d_xyz, const int64_t* h_off, int n_seg, double radius, int max_nn,
                               float* d_normal, void* stream);
void cs_normals_stats(uint64_t out[2], int reset);

/* ------------------------------------------------------------------------------------------
 * cs_fgr_batch: Fast Global Registration (Zhou, Park, Koltun, ECCV 2016) on fixed correspondence lists, the second
 * estimator beside cs_ransac_batch.  It follows [O3D-knowledge] Open3D's registration_fgr_based_on_correspondence
 * (FastGlobalRegistrationOption: division_factor, tuple_scale, maximum_correspondence_distance = mu_floor,
 * iteration_number, maximum_tuple_count, tuple_test), as remembered and not checked against an installation; where the
 * project's habits differ they hold (DESIGN 17 lists the differences).  This comment is the specification and
 * tests/fgr_ref.py restates it bit for bit.  Every operation below is ONE IEEE f64 operation, evaluated in the order the
 * parentheses give (sums without parentheses from left to right), unless a fused fma(a, b, c) is written; nothing is
 * contracted.
 *   Problems: cs_ransac_batch's layout -- d_src, d_tgt f32 [M,3], pair i = (src_i, tgt_i), problem p owns the m pairs
 *     [h_off[p], h_off[p+1]).
 *   Frame: lo_c / hi_c = fminf / fmaxf of coordinate c over the source rows of the problem (NaN loses), cs_c =
 *     0.5 * ((double)lo_c + (double)hi_c); ct likewise from the target rows.  d2 of a row r of a side with midpoint c:
 *     d. = (double)r. - c., d2 = (dx*dx + dy*dy) + dz*dz;  g = sqrt(max d2 over all rows of both sides).
 *     q^_c = ((double)src_c - cs_c) / g,  p^_c = ((double)tgt_c - ct_c) / g.
 *     The frame is DEGENERATE when m = 0, a lo or hi is not finite, any d2 is NaN, or g is 0 or not finite.
 *   Tuple test (tuple_test != 0): trial t = 0, 1, ... < 100 m draws i_j = rng(seed, t, j) for j = 0, 1, 2 by
 *     cs_ransac_batch's generator and multiply-shift (not keyed by the problem, like the RANSAC's).  For an edge (a, b):
 *     ls = sqrt((dx*dx + dy*dy) + dz*dz) of d = q^_a - q^_b, lt likewise of p^_a - p^_b.  The trial passes iff
 *     ls * tuple_scale < lt && lt * tuple_scale < ls for its edges (i_0,i_1), (i_1,i_2), (i_2,i_0) -- strict, so a repeated
 *     index fails.  The working list is the pairs i_0, i_1, i_2 of each of the first max_tuple passing trials in trial order,
 *     duplicates kept; n_tuple = trials kept.  Trials are chunked over lanes, but the list is a function of the trial order
 *     alone.  tuple_test = 0: the working list is all m pairs in order and n_tuple = -1.  A degenerate frame has an empty
 *     working list (n_tuple = 0 with the test on).
 *   A problem with a degenerate frame or a working list of n < 10 pairs is answered with the IDENTITY and 0 updates.
 *   Optimisation: T^ = identity (3x4), mu = 1.  For itr = 0 .. iteration_number - 1, per working pair (from its ORIGINAL
 *     q^: the pose-chain rule of cs_icp_batch, written with single operations here):
 *       q_c = ((T^_c0 * q^_x + T^_c1 * q^_y) + T^_c2 * q^_z) + T^_c3;   e = q - p^;   r2 = (e_x*e_x + e_y*e_y) + e_z*e_z;
 *       w = (mu / (r2 + mu))^2 (one division, one product);   wq_c = w * q_c;
 *       x = q x e:  x_x = q_y*e_z - q_z*e_y,  x_y = q_z*e_x - q_x*e_z,  x_z = q_x*e_y - q_y*e_x.
 *     16 signed 64-bit integer sums of I(v * 2^s), I = clamp to +-2^(61 - eN) (NaN to the lower clamp), then truncation
 *     toward zero; eN the smallest integer with n <= 2^eN, b = 61 - eN:
 *       [0] w, s = b;  [1..3] wq_c, s = b - 2;  [4..9] wq_a * q_b for (a,b) = xx, xy, xz, yy, yz, zz, s = b - 4;
 *       [10..12] w * e_c, s = b - 3;  [13..15] w * x_c, s = b - 5.
 *     The bounds behind the exponents (|q| <= 4) are derived in corsair_amd/csrc/fgr.hip and DESIGN 17; the clamp keeps the
 *     sums defined for any T^.  Each sum is converted back as (double)sum * 2^-s.
 *     Normal equations of r = q + omega x q + t - p^ in x = (omega, t), J = [-[q]x | I]:  A x = -b with
 *       A = [[Sxx' , [Swq]x], [. , Sw I]],  Sxx' = (Syy+Szz, -Sxy, -Sxz; ., Sxx+Szz, -Syz; ., ., Sxx+Syy) from the six
 *       second-moment sums, [v]x = (0, -v_z, v_y; v_z, 0, -v_x; -v_y, v_x, 0),  b = (sums 13..15, sums 10..12);
 *     solved by cs_icp_plane_batch's unpivoted Cholesky with its pivot rule (d > 2^-30 A_jj, finite).  R of the quaternion
 *     (1, 0.5 x_0, 0.5 x_1, 0.5 x_2) normalised by division, t = (x_3, x_4, x_5), T^ <- U T^ by cs_icp_batch's chain.  A failed
 *     pivot or a non-finite new T^ stops the problem, which keeps the T^ it had.  After the update of iteration itr:
 *     if itr % 4 == 0 && mu > mu_floor then mu <- mu / division_factor.
 *   Result (a problem that was not answered with the identity): R = R^,
 *       t_a = (g * t^_a + ct_a) - ((R_a0 * cs_0 + R_a1 * cs_1) + R_a2 * cs_2);  last row (0, 0, 0, 1).
 *   Outputs: d_T f32 [n_prob,16] = the f64 result cast once; d_T64 f64 [n_prob,16], optional; d_inliers int32 and d_rmse
 *     f64 [n_prob] as cs_ransac_batch evaluates a hypothesis, of the returned f64 transform over ALL m pairs: d2 by its
 *     fma chain, inlier iff d2 < max_corr * max_corr, rmse = sqrt((sum of (uint64)(d2 * 2^k) * 2^-k) / inliers), 0 without an
 *     inlier, k = 61 - eM - ex with m <= 2^eM and max_corr^2 = f 2^ex (frexp; ex at least -900, 1024 when not finite);
 *     d_iters int32 [n_prob] = updates applied; d_ntuple int32 [n_prob].
 *   Independence: a problem's result depends on that problem alone -- not on its batch neighbours, the launch shape or
 *     the run; with the tuple test off it does not depend on the order of its pairs either.
 *   Empty problems are legal (identity, 0 inliers), so is n_prob = 0.
 *   Refused (CS_ERR_INVALID): NULL table or outputs (d_T64 may be NULL), a negative segment, max_corr or mu_floor not
 *     positive and finite, division_factor <= 1, tuple_scale outside (0, 1), max_tuple < 1; (CS_ERR_UNSUPPORTED):
 *     iteration_number outside [0, 1000], max_tuple above 65536, a problem of 2^31 pairs or more.
 *   Stream behaviour: one launch on `stream`, one persistent workgroup per problem, no host wait; the table of normalised
 *     pairs (f64, 48 bytes per pair of the call) and, with the test on, the working lists (48 bytes x 3 max_tuple per
 *     problem) come from the calling thread's pool.  No float atomics.
 * Profile family "fgr".
 * ---------------------------------------------------------------------------------------- */
int cs_fgr_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, int n_prob, double max_corr,
                 double mu_floor, double division_factor, int iteration_number, int tuple_test, double tuple_scale,
                 int max_tuple, uint64_t seed, float* d_T, double* d_T64, int32_t* d_inliers, double* d_rmse,
                 int32_t* d_iters, int32_t* d_ntuple, void* stream);

/* ------------------------------------------------------------------------------------------
 * cs_orient_normals: flips normals so that they point away from (away = 1) or towards (away = 0) a view point per
 * segment -- [O3D-knowledge] Open3D's orient_normals_towards_camera_location with the sense selectable -- or, with
 * d_view = NULL, the segment's centroid.  cs_estimate_normals' sign rule depends on the pose and FPFH is not invariant to a
 * flipped normal, so cs_fpfh's callers orient first.  tests/fpfh_ref.py restates this comment bit for bit.
 *   d_xyz f32 [n,3]; h_off int64 [n_seg + 1] host offsets; d_view f64 [n_seg,3] device or NULL; d_normal f32 [n,3] in/out.
 *   Per row:  d = (double)x - v (one f64 subtraction per coordinate),  s = fma(n_z, d_z, fma(n_y, d_y, n_x * d_x)) on the
 *     normal widened to f64; the three components are negated when s < 0 (away = 1) or s > 0 (away = 0).  A zero or NaN s
 *     keeps the normal (so do NaN normals, rows and view points).
 *   The centroid (d_view = NULL) is exact and free of the rows' order: over the rows of the segment whose three coordinates
 *     are finite and below 2^15 in magnitude, S_c = sum of the integers (int64)rint(x_c * 2^16) (round to nearest even; each
 *     below 2^31 in magnitude, fewer than 2^31 rows: the 64-bit sum cannot overflow), cnt = their number, and
 *     v_c = ((double)S_c / (double)cnt) * 2^-16 (the conversions round to nearest even).  A segment without such a row keeps
 *     its normals.  A permuted segment gives the permuted answer, bit for bit.
 *   n_seg = 0 and empty segments are legal.  Refused (CS_ERR_INVALID): a NULL offset table, a negative count, offsets that
 *     decrease, an `away` other than 0 / 1, NULL d_xyz or d_normal while a row exists; (CS_ERR_UNSUPPORTED): a segment of
 *     2^31 rows or more.  No host wait; the only atomics are the integer sums.  Profile family "orient".
 * ---------------------------------------------------------------------------------------- */
int cs_orient_normals(const float* d_xyz, const int64_t* h_off, int n_seg, const double* d_view, int away,
                      float* d_normal, void* stream);

/* ------------------------------------------------------------------------------------------
 * cs_fpfh: Fast Point Feature Histograms (Rusu, Blodow, Beetz, ICRA 2009), 33 values per row, after [O3D-knowledge]
 * Open3D's ComputeFPFHFeature as remembered and not checked against an installation; where the project's habits differ
 * they hold (DESIGN 21 lists the differences).  This comment is the specification and tests/fpfh_ref.py restates it bit for
 * bit.  Every operation is ONE IEEE f64 operation in the order the parentheses give, or an explicit fma; nothing is
 * contracted; only + - * / sqrt floor fma and comparisons appear.
 *   d_xyz f32 [n,3]; d_normal f32 [n,3] (oriented: cs_orient_normals); h_off int64 [n_seg + 1] host offsets;
 *   d_fpfh f32 [n,33].  Coordinates and normals are widened to f64 first.
 *   Neighbours of row i: the rows j != i of the SAME segment with d2 < radius * radius (one f64 product), STRICT;
 *     (dx, dy, dz) = p_j - p_i, d2 = fma(dz, dz, fma(dy, dy, dx * dx)) -- cs_estimate_normals_hybrid's chain.  Of those the
 *     min(max_nn - 1, found) smallest by (d2, j) ([O3D-knowledge]: Open3D's hybrid search returns the row itself first and
 *     max_nn counts it).  A NaN or inf d2 never qualifies.  max_nn in [4, 128]; radius finite and > 0.  m_i = their number.
 *   Pair (i, j), len = sqrt(d2), dot(a, b) = (a_x * b_x + a_y * b_y) + a_z * b_z,
 *     cross(a, b) = (a_y * b_z - a_z * b_y, a_z * b_x - a_x * b_z, a_x * b_y - a_y * b_x):
 *     a1 = dot(n_i, dp) / len, a2 = dot(n_j, dp) / len.  |a1| < |a2|: n1 = n_j, n2 = n_i, dp = -dp, f2 = -a2 (Open3D's
 *     acos(|a1|) > acos(|a2|) without the acos); otherwise n1 = n_i, n2 = n_j, f2 = a1.
 *     v = cross(dp, n1), vl = sqrt(dot(v, v)), v = v / vl (three divisions), w = cross(n1, v), f1 = dot(v, n2),
 *     x = dot(n1, n2), y = dot(w, n2); f0 is the angle of (x, y).
 *     Degenerate -- len = 0, vl = 0 or not finite, or one of f1, f2, x, y not finite (NaN normals arrive here) -- the
 *     pair goes to bins 5 / 5 / 5 (Open3D's answer, all features 0).
 *   Bins, 11 per feature, 33 counters: f0 -> its bin, f1 -> 11 + its bin, f2 -> 22 + its bin.
 *     f1, f2: floor((11 * (f + 1)) * 0.5) clamped to [0, 10].
 *     f0: the number of boundaries theta_m = -pi + 2 pi m / 11 (m = 1..10) that are not above the angle, with no
 *       transcendental function: corsair_amd/csrc/fpfh_bounds.h (tools/gen_fpfh_bounds.py) tabulates (c_m, s_m) =
 *       (cos theta_m, sin theta_m) as f64 literals and THOSE numbers are the specification; t_m = fma(c_m, y, -(s_m * x)).
 *       x = y = 0: bin 5.  Otherwise y < 0: the number of m in 1..5 with t_m >= 0; else 5 + the number of m in 6..10 with
 *       t_m >= 0.  DELIBERATE DIFFERENCE: y = -0 with x < 0 gives bin 10 like y = +0 (atan2 gives -pi there, bin 0).
 *   SPFH: spfh_b(i) = (double)count_b(i) * (100.0 / (double)m_i), zeros when m_i = 0.  DELIBERATE DIFFERENCE: Open3D adds
 *     100 / m_i once per pair.
 *   FPFH: acc_b = 0 (33), sum_g = 0 (3).  For the neighbours j of i in (d2, j) order, skipping d2 == 0, for b = 0..32 in
 *     order: val = spfh_b(j) / d2;  acc_b = acc_b + val;  sum_(b / 11) = sum_(b / 11) + val.  Then
 *     out_b = acc_b * (100.0 / sum_(b / 11)) when sum_(b / 11) != 0 (a NaN sum counts as != 0), else acc_b; then
 *     out_b = out_b + spfh_b(i); one cast to f32.
 *   Independence: a row's descriptor depends on its segment alone -- not on batch neighbours, the launch shape or the run
 *     -- and on the ORDER of the rows inside the segment only through exact distance ties.
 *   n_seg = 0 and empty segments are legal.  Refused (CS_ERR_INVALID): a NULL offset table, a negative count, offsets that
 *     decrease, NULL arrays while a row exists, a radius that is NaN, infinite or <= 0; (CS_ERR_UNSUPPORTED): max_nn
 *     outside [4, 128], a segment of 2^31 rows or more.
 *   Paths, the same bits: the exhaustive scan of the row's segment is the definition, the whole path under CS_FPFH_GRID=0
 *     (read per call) and the path of every segment of at most 512 rows (cs_estimate_normals_hybrid's convention) and of a
 *     radius of 1e150 or more.  Otherwise the cell grid of cs_estimate_normals_hybrid (the same code: cells of
 *     radius (1 + 2^-10), rows sorted by (segment, cell), complete for d2 < radius^2 by the argument in cellgrid.h).  A
 *     ball larger than the on-chip list is ranked in parts (fpfh.hip) with the same result.
 *   Everything is enqueued on `stream`; no host wait (CS_FPFH_STATS=1 adds one at the end); the only atomics are integer.
 *   cs_fpfh_stats: out = {neighbours found (the sum of m_i), rows whose on-chip list was ranked in parts}, counted only
 *     while CS_FPFH_STATS=1.  CS_FPFH_PASS=1 (read per call) is a timing diagnostic for tools/fpfh_bench.py: the call stops
 *     after the SPFH pass and d_fpfh is NOT written.
 * Profile family "fpfh", one scope per call.
 * ---------------------------------------------------------------------------------------- */
int cs_fpfh(const float* d_xyz, const float* d_normal, const int64_t* h_off, int n_seg, double radius, int max_nn,
            float* d_fpfh, void* stream);
void cs_fpfh_stats(uint64_t out[2], int reset);

/* ------------------------------------------------------------------------------------------
 * Scan cleaning: the two outlier filters of [O3D-knowledge] Open3D, remove_statistical_outlier(nb_neighbors,
 * std_ratio) and remove_radius_outlier(nb_points, radius), as remembered and not checked against an installation; where the
 * project's habits differ they hold.  The reference has no such step, so these comments are the specification and
 * tests/outlier_ref.py restates them bit for bit.  Every operation is ONE IEEE f64 operation in the order the parentheses
 * give, or an explicit fma; nothing is contracted; only + - * / sqrt fma rint, scalings by powers of two, integer
 * arithmetic and comparisons appear.  Common to the three calls: d_xyz f32 [n,3]; h_off int64 [n_seg + 1] host offsets;
 * neighbours are rows of the SAME segment; d2 = fma(dz, dz, fma(dy, dy, dx * dx)), d. = (double)x_j. - (double)x_i.
 * (cs_estimate_normals' chain); every threshold is STRICT; a NaN or +inf d2 is never a neighbour.  n_seg = 0 and empty
 * segments are legal.  Refused by all three (CS_ERR_INVALID): a NULL offset table, a negative count, offsets that decrease,
 * a NULL array while a row exists; (CS_ERR_UNSUPPORTED): a segment of 2^31 rows or more.  Everything is enqueued on
 * `stream`; no host wait (CS_OUTLIER_STATS=1 adds one at the end of cs_knn_mean_dist); the only atomics are integer.
 * Profile family "outlier", one scope per call.
 *
 * cs_knn_mean_dist: d_mean f64 [n]; k in [2, 32] (else CS_ERR_UNSUPPORTED).
 *   Row i: among the rows j of its segment with d2 < +inf, itself included (d2 = 0; [O3D-knowledge]: the average Open3D
 *     forms counts the point itself), the c = min(k, found) smallest d2, d2_(0) <= d2_(1) <= ...;
 *     mean_i = (((+0 + sqrt(d2_(0))) + sqrt(d2_(1))) + ...) / (double)c.
 *     Rows that tie in d2 contribute equal terms: the value is a function of the multiset of the row's d2 values and does
 *     not depend on the order of the rows inside the segment, on batch neighbours, the launch shape or the run.
 *   A row with a non-finite coordinate finds nothing (c = 0) and gets the quiet NaN 0x7ff8000000000000.
 *   Paths, the same bits: the exhaustive scan of the row's segment (cs_estimate_normals' kernel with a list of d2 alone) is
 *     the definition, the whole path under CS_OUTLIER_GRID=0 (read per call) and the path of every segment of at most 1024
 *     rows.  Otherwise cs_estimate_normals' cell grid (the same code: the cell from the segment's bounding box, the 27
 *     cells, the voucher): a list is accepted only when its k-th d2 lies strictly below c^2 (1 - 2^-30); every other row is
 *     compacted into a list and recomputed by the scan, one wave per row; segments the device keeps off the grid (a box
 *     of zero area or one that is not finite, a cell index at the clamp) are answered by the exhaustive kernel.
 *
 * cs_outlier_statistical: d_mean f64 [n] (cs_knn_mean_dist's); std_ratio finite and >= 0 (else CS_ERR_INVALID);
 *   d_keep u8 [n] (0 / 1); d_stat f64 [n_seg,4] = (n_valid, mu, sigma, tau) per segment, written for empty segments too.
 *   The VALID rows of a segment are those with 0 <= mean_i < +inf (cs_knn_mean_dist writes no negative mean; a caller's
 *     own is treated like a NaN one); n_valid = their number.
 *   M = the maximum of the valid means (exact and free of the order).  M = f 2^e with f in [0.5, 1) (frexp), and
 *     s = min(31 - e, 1023): the minimum keeps 2^s inside the f64 range for M < 2^-992, where the integers below are
 *     smaller than 2^31 and the statistic coarser; no distance between f32 rows comes near.  M = 0: s = 31.
 *   q_i = (uint64)rint(mean_i * 2^s) (round to nearest even; the scaling by a power of two is exact), at most 2^31.
 *   Three unsigned 64-bit integer sums over the valid rows: S1 = sum q_i, S2lo = sum (q_i^2 mod 2^32),
 *     S2hi = sum floor(q_i^2 / 2^32); each stays below 2^63 for fewer than 2^31 rows.
 *   With n = n_valid, in this order:
 *     mu = ((double)S1 / (double)n) * 2^-s when n >= 1 and M > 0, else 0;
 *     sigma (the sample deviation): when n >= 2 and M > 0, in unsigned 128-bit integers S2 = S2hi * 2^32 + S2lo,
 *       D = n * S2 - S1 * S1 (not negative; below 2^124), dhi = floor(D / 2^64), dlo = D mod 2^64,
 *       dd = (double)dhi * 2^64 + (double)dlo,  den = (double)n * (double)(n - 1),  sigma = sqrt(dd / den) * 2^-s; else 0;
 *     tau = fma(std_ratio, sigma, mu).
 *     The conversions of 64-bit integers round to nearest even; the scalings by 2^-s are exact unless the result is
 *     subnormal, where they round once.
 *   keep_i = mean_i > 0 && mean_i < tau ([O3D-knowledge]: Open3D also drops a row whose average is 0, e.g. one of k or more
 *     copies of a point).  A NaN mean is dropped.  M = 0 gives mu = sigma = tau = 0 and keeps nothing.
 *   The four values are a pure function of the multiset of the segment's means: a permuted segment gives the permuted mask
 *     and the SAME d_stat, bit for bit, on any launch shape (the integer sums commute; so does the maximum).
 *
 * cs_outlier_radius: radius finite and > 0, nb_points >= 0 (else CS_ERR_INVALID); d_count int32 [n]; d_keep u8 [n] or NULL.
 *   count_i = the number of rows j of the segment, itself included, with d2 < radius * radius (one f64 product);
 *     keep_i = count_i > nb_points ([O3D-knowledge]: Open3D's rule, whose radius search also returns the point itself; it
 *     keeps a point AT the radius, which no measured input can tell apart and an integer lattice can).
 *   A row with a non-finite coordinate gets 0.  A radius whose square overflows to +inf counts the segment's finite rows;
 *     one whose square underflows to 0 counts nothing.
 *   Paths, the same bits: the exhaustive scan is the definition, the whole path under CS_OUTLIER_GRID=0, the path of every
 *     segment of at most 512 rows and of a radius of 1e300 or more; otherwise cs_estimate_normals_hybrid's cell grid (the
 *     same code: cells of radius (1 + 2^-10), complete for d2 < radius^2 by the argument in cellgrid.h).
 *
 * cs_outlier_stats: out = {rows answered by a grid path, of those recomputed by the exhaustive scan}, counted only while
 *   CS_OUTLIER_STATS=1 (read per call).  The radius grid is complete and recomputes nothing.
 * ---------------------------------------------------------------------------------------- */
int cs_knn_mean_dist(const float* d_xyz, const int64_t* h_off, int n_seg, int k, double* d_mean, void* stream);
int cs_outlier_statistical(const double* d_mean, const int64_t* h_off, int n_seg, double std_ratio, uint8_t* d_keep,
                           double* d_stat, void* stream);
int cs_outlier_radius(const float* d_xyz, const int64_t* h_off, int n_seg, double radius, int nb_points, int32_t* d_count,
                      uint8_t* d_keep, void* stream);
void cs_outlier_stats(uint64_t out[2], int reset);

/* ------------------------------------------------------------------------------------------
 * Scan clustering: DBSCAN per segment, [O3D-knowledge] Open3D's cluster_dbscan(eps, min_points) as remembered
 * and not checked against an installation, and the mask of the largest cluster.  The reference has no such step, so these
 * comments are the specification and tests/dbscan_ref.py restates them.  As in the block above: every operation is ONE IEEE
 * f64 operation in the order given, or an explicit fma; nothing is contracted; every threshold is STRICT.  d_xyz f32 [n,3];
 * h_off int64 [n_seg + 1] host offsets; neighbours are rows of the SAME segment; d2 is cs_outlier_radius' chain,
 * d2 = fma(dz, dz, fma(dy, dy, dx * dx)) with d. = (double)x_j. - (double)x_i.; a NaN or +inf d2 is never a neighbour.
 * n_seg = 0 and empty segments are legal.  Everything is enqueued on `stream`; no host wait (CS_DBSCAN_STATS=1 adds one at
 * the end of cs_dbscan); the only atomics are integer.  Profile family "cluster", one scope per call.
 *
 * cs_dbscan: eps finite and > 0, min_points >= 1 (else CS_ERR_INVALID); d_label int32 [n]; d_count int32 [n] or NULL.
 *   Also refused (CS_ERR_INVALID): a NULL offset table, a negative count, offsets that decrease, a NULL d_xyz or d_label
 *   while a row exists; (CS_ERR_UNSUPPORTED): a segment of 2^31 rows or more.
 *   r2 = eps * eps (one f64 product).
 *   count_i = the number of rows j of the segment, itself included, with d2 < r2: exactly cs_outlier_radius' count (the
 *     same kernels).  d_count, when given, receives it.
 *   Row i is a CORE row when count_i >= min_points ([O3D-knowledge]: Open3D's and scikit-learn's rule, the point itself
 *     counted; with min_points = nb_points + 1 it is cs_outlier_radius' keep rule).
 *   Two core rows are LINKED when d2 < r2; a CLUSTER is a connected component of the core rows under that relation.
 *   The clusters of a segment are numbered 0, 1, ... in ascending order of their smallest core row (local to the segment).
 *   A non-core row with at least one core row inside d2 < r2 is a BORDER row: it takes the label of the core neighbour with
 *     the smallest (d2, local row index), compared as a pair.  THIS IS A DELIBERATE DIFFERENCE: [O3D-knowledge] Open3D and
 *     scikit-learn give a border row to whichever cluster reaches it first in their visit order, which depends on the
 *     order of the rows; the rule here depends on no order except through exact ties of d2.
 *   Every other row gets -1: noise, and every row with a non-finite coordinate (its count is 0).
 *   A permuted segment gives the same core set and the same partition of the core rows; a border row's cluster can differ
 *     only at an exact tie of d2 between core rows of two clusters; the cluster NUMBERS follow the smallest rows.  The
 *     result is a function of the segment alone: batch neighbours, the stream, the launch shape and the run do not reach it.
 *   An eps whose square overflows to +inf links every finite row of the segment to every other; one whose square underflows
 *     to 0 finds nothing, not even the row itself: count = 0, nothing is core, every label is -1.
 *   Paths, the same values: the exhaustive scan of the row's segment (cs_outlier_radius' kernel shape) is the definition,
 *     the whole path under CS_DBSCAN_GRID=0 (read per call), the path of every segment of at most 512 rows and of an eps of
 *     1e150 or more; otherwise cs_estimate_normals_hybrid's cell grid (the same code: cells of eps (1 + 2^-10), complete for
 *     d2 < r2 by the argument in cellgrid.h).  The components come from a lock-free union-find (dbscan.hip): whatever the
 *     order in which the threads run, its trees are the components and each root is the component's smallest row.
 *
 * cs_cluster_largest: d_label int32 [n] (cs_dbscan's); d_keep u8 [n] (0 / 1); d_stat int32 [n_seg,3] per segment, written
 *   for empty segments too.  Refused as above; a NULL d_stat with n_seg > 0, a NULL d_label or d_keep while a row exists.
 *   A label outside [0, rows of the segment) is treated as -1 (no cluster).
 *   size(c) = the number of rows of the segment with label c, core and border rows alike.
 *   d_stat = (the number of c with size(c) > 0, the c of the largest size -- of equal sizes the smallest c --, that size);
 *     (0, -1, 0) for a segment without a cluster.  keep_i = label_i is that c.
 *   Integer atomics only (counts, a maximum, a sum): the same values on any launch shape.
 *
 * cs_dbscan_stats: out = {rows answered by the grid path, border rows}, counted only while CS_DBSCAN_STATS=1 (read per call).
 * ---------------------------------------------------------------------------------------- */
int cs_dbscan(const float* d_xyz, const int64_t* h_off, int n_seg, double eps, int min_points, int32_t* d_label,
              int32_t* d_count, void* stream);
int cs_cluster_largest(const int32_t* d_label, const int64_t* h_off, int n_seg, uint8_t* d_keep, int32_t* d_stat,
                       void* stream);
void cs_dbscan_stats(uint64_t out[2], int reset);

/* ------------------------------------------------------------------------------------------
 * Support-plane segmentation: the dominant plane of every segment by RANSAC, [O3D-knowledge] Open3D's
 * segment_plane(distance_threshold, ransac_n, num_iterations) as remembered and not checked against an installation; where
 * the project's habits differ they hold (the list is at the end).  The reference has no such step, so this comment is the
 * specification and tests/plane_ref.py restates it bit for bit.  As in the blocks above: every operation is ONE IEEE f64
 * operation in the order given, or an explicit fma; nothing is contracted; only + - * / sqrt fma rint, scalings by powers of
 * two, integer arithmetic and comparisons appear; every threshold is STRICT.  d_xyz f32 [n,3]; h_off int64 [n_seg + 1] host
 * offsets; p_i = row i as f64; a segment has m rows with local indices 0 .. m - 1.
 *
 * cs_segment_plane: dist finite and > 0, iters in [1, 65536] (else CS_ERR_INVALID); d_plane f64 [n_seg,4]; d_stat int32
 *   [n_seg,8]; d_inlier u8 [n] (0 / 1).  Also refused (CS_ERR_INVALID): a NULL offset table, a negative count, offsets that
 *   decrease, a NULL d_plane or d_stat with n_seg > 0, a NULL d_xyz or d_inlier while a row exists; (CS_ERR_UNSUPPORTED): a
 *   segment of 2^31 rows or more.  n_seg = 0 and empty segments are legal; an empty segment writes the NO-PLANE row.
 *   Stage 1, the hypotheses.  thr2 = dist * dist.  For t = 0 .. iters - 1:
 *     i_j = rng_index(seed, t, j, m), j = 0, 1, 2 (corsair_amd/csrc/common.h: the generator of cs_ransac_batch's samples;
 *       the draws depend on (seed, t, j, m) alone, not on the segment's place in the batch);
 *     e1 = p_i1 - p_i0, e2 = p_i2 - p_i0;
 *     n_x = fma(e1_y, e2_z, -(e1_z * e2_y)), n_y = fma(e1_z, e2_x, -(e1_x * e2_z)), n_z = fma(e1_x, e2_y, -(e1_y * e2_x));
 *     nn = fma(n_z, n_z, fma(n_y, n_y, n_x * n_x)), bound = thr2 * nn.
 *     The hypothesis is VALID when 0 < nn < +inf and 0 < bound < +inf: repeated rows, collinear rows, a non-finite sample and
 *       a threshold that under- or overflows are invalid and count 0.
 *     Row q is an inlier of t when, with u = p_q - p_i0 and s = fma(u_z, n_z, fma(u_y, n_y, u_x * n_x)), s * s < bound (no
 *       square root, no division; a NaN is false, so a row with a non-finite coordinate is never an inlier).
 *     count_t = the inliers of t.  The best hypothesis has the largest count, ties to the SMALLEST t.
 *     A segment without a valid hypothesis, or with a best count below 3, has NO PLANE: its d_plane row is zero, its d_stat row
 *       (0, -1, 0, 0, 0, 0, 0, rows_finite), its d_inlier rows 0.  rows_finite = the rows whose three coordinates are finite.
 *   Stage 2, the refit, free of the order of the rows.  A = the stage-1 inliers of the best t, o = p_i0 of that t, u = p - o.
 *     M = the largest |u_a| over A and the three axes (exact and order-free).  M = 0: the refit is skipped.
 *     M = f 2^e with f in [0.5, 1) (frexp), sh = min(15 - e, 1023); q_a = (int64)rint(u_a * 2^sh), |q_a| <= 2^15.
 *     Nine signed 64-bit sums over A: S_a, and S_ab (a <= b) of q_a q_b; each stays below 2^62 for fewer than 2^31 rows.
 *     With n = |A|, in signed 128-bit integers C_ab = n S_ab - S_a S_b (magnitude below 2^93), converted by
 *       cs_outlier_statistical's rule for its D: the magnitude as (double)hi * 2^64 + (double)lo (hi, lo its upper and lower
 *       64 bits), the sign applied afterwards; mirrored.
 *     jacobi3 (corsair_amd/csrc/horn.h) on C; e = the column of the smallest diagonal entry, ties to the smaller column,
 *       as cs_estimate_normals selects it; len2 = fma(e_z, e_z, fma(e_y, e_y, e_x * e_x)).
 *     When the refit is skipped, or len2 is zero or not finite (which a non-finite component makes it): the final plane is
 *       the sampled one, n_a = n_a / sqrt(nn) and c = o, refit = 0.
 *     Otherwise n_a = e_a / sqrt(len2), c_a = o_a + ((double)S_a / (double)n) * 2^-sh, refit = 1.
 *   Stage 3, final inliers, sides, orientation.  For every finite row: u = p - c, s = fma(u_z, n_z, fma(u_y, n_y, u_x * n_x)),
 *     inlier = s * s < thr2; n_pos, n_neg = the finite rows that are no inliers with s > 0, with s < 0.
 *     n_neg > n_pos: n is negated and the two counts swap.  n_neg = n_pos: cs_estimate_normals' sign rule, the component of
 *       largest magnitude (the first such on ties) is made positive (the counts are equal, a swap changes nothing).
 *     d = -fma(c_z, n_z, fma(c_y, n_y, c_x * n_x)).  d_plane = (n_x, n_y, n_z, d): the normal points to the side most rows
 *       are on, and n_neg counts what lies beyond the plane.
 *     d_stat = (1, best t, count of stage 1, refit, final count, n_pos, n_neg, rows_finite); d_inlier = the final mask.
 *   Independence: the result is a function of (the segment's rows in their order, dist, iters, seed).  The order of the rows
 *     enters through the draws only; batch neighbours, the stream, the launch shape and the run do not reach the result, and
 *     stages 2 and 3 depend on the SET A alone (integer sums and an exact maximum).
 *   Differences from [O3D-knowledge] Open3D: the number of hypotheses is fixed (no probabilistic early exit); thresholds are
 *     strict; the refit is a fixed-point covariance about a sampled row with a resolution of 2^-15 of the inliers' extent
 *     (tests/test_plane_cpu.py bounds its angle to the float fit); the returned inliers are those of the REFITTED plane;
 *     ransac_n is 3.
 *   Kernels (plane.hip): the count of 256 hypotheses x one slice of CS_PLANE_SLICE rows (read per call, default 1024) per
 *     workgroup with one integer atomicAdd per thread, then per-row passes and one thread per segment.  Everything is enqueued
 *     on `stream`; no host wait; the only atomics are integer.  Profile family "plane", one scope per call.
 * ---------------------------------------------------------------------------------------- */
int cs_segment_plane(const float* d_xyz, const int64_t* h_off, int n_seg, double dist, int iters, uint64_t seed,
                     double* d_plane, int32_t* d_stat, uint8_t* d_inlier, void* stream);

/* ------------------------------------------------------------------------------------------
 * Feature-matching RANSAC: the third correspondence estimator, beside cs_ransac_batch and cs_fgr_batch, after
 * [O3D-knowledge] Open3D's registration_ransac_based_on_feature_matching(mutual_filter, max_correspondence_distance,
 * ransac_n, [CorrespondenceCheckerBasedOnEdgeLength(similarity), CorrespondenceCheckerBasedOnDistance(distance)]) as
 * remembered and not checked against an installation; where the project's habits differ they hold (the list is at the end).
 * The reference has no such step, so these comments are the specification and tests/featmatch_ref.py restates them bit for
 * bit.  As in the blocks above: every operation is ONE IEEE f64 operation in the order given (sums without parentheses from
 * left to right), or an explicit fma; nothing is contracted; only + - * / sqrt fma, scalings by powers of two, integer
 * arithmetic and comparisons appear; every threshold is STRICT unless >= is written; a comparison with a NaN is false.
 * Everything is enqueued on `stream`; scratch comes from the calling thread's pool; no host wait, no cooperative launch, no
 * flag a thread waits on; the only atomics are integer; every loop is bounded by an argument or a segment's rows.  Profile
 * family "featmatch", one scope per call.
 *
 * cs_corr_mutual: the correspondences of n_pair (query, CAD) pairs from two 1-NN lists.
 *   d_nn_fwd int32 [N0]: the local CAD row of every query row (cs_knn_feat's d_idx at k = 1); d_nn_bwd int32 [N1]: the local
 *     query row of every CAD row (the same call with the roles of the segments swapped; NULL allowed when mutual = 0);
 *     d_xyz0 f32 [N0,3], d_xyz1 f32 [N1,3]; h_off0, h_off1 int64 [n_pair + 1] host offsets of the pairs' segments, n0 and n1
 *     rows; d_src, d_tgt f32 [N0,3] (neither may alias an input); d_m int32 [n_pair]; d_stat int32 [n_pair,2].
 *   Query row i (local) of a pair is VALID when 0 <= nn_fwd[i] < n1 (a -1 entry -- a non-finite descriptor, an empty CAD -- is
 *     never a match) and MUTUAL when it is valid and nn_bwd[nn_fwd[i]] == i.  c = the number of mutual rows.
 *   mutual = 1 and c >= 3 * ransac_n: the mutual rows are kept.  mutual = 1 and c < 3 * ransac_n: [O3D-knowledge] Open3D's
 *     fallback, decided on the device -- the valid rows are kept and d_stat says so.  mutual = 0: the valid rows are kept.
 *   The kept rows in ascending i (a STABLE compaction) fill the slots h_off0[p], h_off0[p] + 1, ...: d_src = xyz0[i],
 *     d_tgt = xyz1[nn_fwd[i]], both copied bit for bit.  d_m[p] = their number.  The capacity of a pair is its n0 slots, so
 *     the host needs no count; the slots past d_m[p] are written with +0.
 *   d_stat[p] = (c with mutual = 1, the number of valid rows with mutual = 0;  1 when the fallback was taken, else 0).
 *   n_pair = 0, empty queries and empty CADs are legal.  Refused (CS_ERR_INVALID): a NULL offset table, a negative count,
 *     offsets that decrease, ransac_n outside [1, 2^20], mutual other than 0 / 1, NULL d_m or d_stat with n_pair > 0, a NULL
 *     array that a row needs; (CS_ERR_UNSUPPORTED): a segment of 2^31 rows or more.
 *   One workgroup per pair: a count pass, then a block scan over its rows.
 *
 * cs_ransac_fm_batch: d_src, d_tgt f32 [M,3], pair i = (s_i, q_i) widened to f64; problem p owns the slots
 *   [h_off[p], h_off[p+1]) (cs_corr_mutual's layout; h_off int64 [n_prob + 1] on the host) of which the first
 *   m = min(max(d_m[p], 0), capacity) hold pairs; d_m int32 [n_prob] on the device, NULL = every list is full.
 *   max_corr finite and > 0; ransac_n = n in {3, 4}; edge_similarity in [0, 1], 0 = the edge checker is off; check_distance
 *   0 = the distance checker is off; 1 <= iterations < 2^31; d_T f64 [n_prob,4,4]; d_stat int32 [n_prob,4]; d_rmse f64 [n_prob].
 *   thr2 = max_corr * max_corr, sim2 = edge_similarity * edge_similarity, each formed once.
 *   Hypothesis t = 0 .. iterations - 1 of a problem with m >= n:
 *     Sampling: i_j = rng_index(seed, t, j, m), j = 0 .. n - 1 (corsair_amd/csrc/common.h: the generator of cs_ransac_batch and
 *       cs_segment_plane; the draws depend on (seed, t, j, m) alone).  Draws are with replacement.
 *     Edge-length checker (edge_similarity > 0), before the fit: for every a < b < n, with e = s_ia - s_ib and
 *       f = q_ia - q_ib, ls2 = fma(e_z, e_z, fma(e_y, e_y, e_x * e_x)), lt2 likewise of f:
 *       ls2 >= sim2 * lt2 && lt2 >= sim2 * ls2, else t is INVALID.  No square root is taken; a repeated draw passes (0 >= 0).
 *     Fit, the formulas of cs_ransac_batch's hypothesis kernel with plain divisions: per axis
 *       cs_c = ((0 + s_i0c) + s_i1c + ...) / (double)n, ct_c likewise;  S_xy = fma(ds_x, dt_y, S_xy) from S = 0 over j in order,
 *       ds = s_ij - cs, dt = q_ij - ct;  Horn's N from S;  the eigenvector by horn_qcp (corsair_amd/csrc/horn.h) ALONE: a fit it
 *       declines makes t INVALID (there is no Jacobi fallback here);  qn = sqrt(qw*qw + qx*qx + qy*qy + qz*qz), q = q / qn (four
 *       divisions);  R from q as cs_ransac_batch forms it;  t_a = ct_a - (R_a0 * cs_0 + R_a1 * cs_1 + R_a2 * cs_2).
 *       A fit with a value of R or t that is not finite makes t INVALID.
 *     Distance: the project's canonical chain of the posed source (cs_ransac_batch's count),
 *       p_c = fma(R_c2, s_z, fma(R_c1, s_y, fma(R_c0, s_x, t_c))),  d_c = p_c - q_c,  d2 = fma(d_z, d_z, fma(d_y, d_y, d_x * d_x)).
 *     Distance checker (check_distance != 0), after the fit: d2 < thr2 for every sampled pair, else t is INVALID.
 *     Count: count_t = the pairs i < m of the problem with d2 < thr2.  Invalid hypotheses count nothing and never win.
 *   Best: the largest count; ties go to the SMALLEST t (cs_segment_plane's rule: a u64 maximum of count << 32 | ~t).
 *     m < n, no valid hypothesis, or a best count < n: found = 0, d_T = the identity, d_stat = (0, -1, 0, n_valid),
 *     d_rmse = 0 (cs_ransac_batch answers a problem of fewer than ransac_n pairs the same way).
 *     Otherwise d_T = (R | t; 0 0 0 1) of the best hypothesis in f64 -- there is NO refit over the inliers -- and
 *     d_stat = (1, t_best, count, n_valid), n_valid = the hypotheses that passed the checkers and the fit.
 *   d_rmse = sqrt(((double)E * 2^-k) / (double)count), E = the unsigned 64-bit INTEGER sum over the inliers of the best
 *     hypothesis of (uint64)(d2 * 2^k) (one product, truncation), k = 61 - eM - ex with eM the smallest integer with
 *     m <= 2^eM and thr2 = f 2^ex, f in [0.5, 1) (frexp; ex at least -900, 1024 when thr2 is not finite).  A fixed-point sum:
 *     it depends on the SET of inliers alone, not on any order or launch shape.
 *   A max_corr whose square overflows to +inf counts every pair with a finite d2; one whose square underflows to 0 counts
 *     nothing.  Rows with a NaN or infinite coordinate are never inliers and invalidate the hypotheses that sample them.
 *   Independence: the result of a problem is a function of its pairs in their order, the parameters and the seed alone.  Batch
 *     neighbours, the capacity behind m, the stream, the launch shape (CS_FM_SLICE, CS_FM_CHUNK) and the run do not reach it.
 *   n_prob = 0 and empty problems are legal.  Refused (CS_ERR_INVALID): a NULL offset table, a negative count, offsets that
 *     decrease, max_corr not positive and finite, edge_similarity outside [0, 1] (a NaN too), iterations < 1, NULL outputs with
 *     n_prob > 0, NULL d_src or d_tgt while a slot exists; (CS_ERR_UNSUPPORTED): ransac_n outside {3, 4}, a problem of 2^31
 *     slots or more, iterations >= 2^31.
 *   Differences from [O3D-knowledge] Open3D, deliberate: the number of hypotheses is FIXED (no confidence-based early exit, as
 *     cs_segment_plane decided); the tie rule (the smallest t; Open3D keeps the first best of an unordered parallel loop);
 *     thresholds are strict (the edge checker's >= is Open3D's); the counter-based generator; NO final refit over the inliers
 *     (the ICP stage follows); the winner is ranked by its inlier count alone (Open3D compares fitness, then rmse); a fit that
 *     horn_qcp declines is dropped.
 *   Kernels (featmatch.hip), per chunk of CS_FM_CHUNK hypotheses (default 8192, read per call, rounded up to a multiple of
 *     256 and shrunk so that the lists of a call stay below 256 MiB): one lane per hypothesis appends the valid ones to the
 *     problem's list through one integer atomicAdd (the order of the list reaches nothing); the count of 256 listed hypotheses
 *     x one slice of CS_FM_SLICE pairs (default 1024, read per call) per workgroup with one integer atomicAdd per lane; the
 *     u64 atomicMax.  Then one thread per problem and one pass over the rows.  The same bits for every value of both variables.
 * ---------------------------------------------------------------------------------------- */
int cs_corr_mutual(const int32_t* d_nn_fwd, const int32_t* d_nn_bwd, const float* d_xyz0, const int64_t* h_off0,
                   const float* d_xyz1, const int64_t* h_off1, int n_pair, int ransac_n, int mutual, float* d_src,
                   float* d_tgt, int32_t* d_m, int32_t* d_stat, void* stream);
int cs_ransac_fm_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, const int32_t* d_m, int n_prob,
                       double max_corr, int ransac_n, double edge_similarity, int check_distance, int64_t iterations,
                       uint64_t seed, double* d_T, int32_t* d_stat, double* d_rmse, void* stream);

/* ------------------------------------------------------------------------------------------
 * The compatibility-graph correspondence estimator: a pose from a correspondence list whose inlier share is a few
 * per cent, by searching the graph of pairwise length-compatible correspondences instead of sampling it (the family of
 * spectral matching, Leordeanu and Hebert 2005, and SC2-PCR, Chen et al. 2022, as remembered from the papers; the list of
 * differences is at the end).  The reference has no such step, so this comment is the specification and tests/sc2_ref.py
 * restates it bit for bit.  As in the blocks above: every operation is ONE IEEE f64 operation in the order given (sums
 * without parentheses from left to right), or an explicit fma; nothing is contracted; every threshold is STRICT; a comparison
 * with a NaN is false.  Everything is enqueued on `stream`; scratch comes from the calling thread's pool; no host wait, no
 * cooperative launch, no flag a thread waits on; the only atomics are integer; every loop is bounded by an argument or a
 * problem's rows.  Profile family "sc2", one scope per call.
 *
 * cs_sc2_batch: d_src, d_tgt f32 [M,3], pair i = (s_i, q_i) widened to f64; problem p owns the slots [h_off[p], h_off[p+1])
 *   (cs_ransac_fm_batch's layout; h_off int64 [n_prob + 1] on the host) of which the first m = min(max(d_m[p], 0), capacity)
 *   hold pairs; d_m int32 [n_prob] on the device, NULL = every list is full.  compat_dist (tau) and max_corr finite and > 0;
 *   n_seeds >= 0, 0 = every row is a seed; k_consensus = K in [2, 64].  d_T f64 [n_prob,4,4]; d_stat int32 [n_prob,6]; d_rmse
 *   f64 [n_prob]; d_inlier u8 [h_off[n_prob]] or NULL.  tau2 = tau * tau and thr2 = max_corr * max_corr, each formed once.
 *   a. Compatibility of the rows i != j, both FINITE (all six coordinates): with e = s_i - s_j and f = q_i - q_j,
 *        ls2 = fma(e_z, e_z, fma(e_y, e_y, e_x * e_x)), lt2 likewise of f, a = (ls2 + lt2) - tau2,
 *        c_ij = ls2 > 0 && lt2 > 0 && (a < 0 || a * a < 4.0 * (ls2 * lt2)).
 *      This is | |e| - |f| | < tau without a square root (square twice; a < 0 is the case in which the first squaring is
 *      not an equivalence).  It is symmetric in i and j to the bit (e and f change sign, the squares do not), so the matrix
 *      may be built from one triangle.  Two matches of one source point (ls2 = 0, as k-NN lists have them) or onto one target
 *      point (lt2 = 0) are never compatible.  c_ii = 0.  A row that is not finite is compatible with nothing.  A tau whose
 *      square overflows to +inf makes every two finite rows with ls2 > 0, lt2 > 0 and a finite ls2 + lt2 compatible; one
 *      whose square underflows to 0 leaves the comparison a * a < 4 (ls2 * lt2) as its rounding decides it.
 *   b. Degrees and seeds: deg_i = sum_j c_ij.  The seeds are the rows of rank < S under the key (deg_i << 32) | ~i (~i: the
 *      32-bit complement), the largest key first: the largest degree, ties to the SMALLEST row.  S = m with n_seeds = 0,
 *      else min(n_seeds, m).  The seed of rank r is hypothesis r.
 *   c. Second-order count of a seed s and a row j with c_sj = 1: sc_sj = the rows k with c_sk = 1 and c_jk = 1
 *      (popcount(row_s & row_j)).
 *   d. Consensus set A_s: s and the min(K, deg_s) rows j with c_sj = 1 of the largest key (sc_sj << 32) | ~j (ties to the
 *      smallest row).  |A_s| < 3 makes the seed INVALID.
 *   e. Fit over A_s, its rows taken in ASCENDING ROW INDEX, cs_ransac_fm_batch's fit formulas at n = |A_s|: the centroids by
 *      the left-to-right sum from 0 divided by (double)n, S_xy by fma in that order, Horn's N, horn_qcp ALONE (a fit it
 *      declines makes the seed INVALID), the same normalisation, R and t.  A value of R or t that is not finite makes the
 *      seed INVALID.
 *   f. Count: count_r = the pairs i < m with d2 < thr2, d2 by the canonical chain of the posed source (cs_ransac_fm_batch).
 *   g. Best: the largest count; ties go to the SMALLEST rank (a u64 maximum of count << 32 | ~r).  m < 3, no valid seed, or a
 *      best count < 3: found = 0, d_T = the identity, d_stat = (0, -1, 0, n_valid, -1, 0), d_rmse = 0.  Otherwise
 *      d_T = (R | t; 0 0 0 1) of the best seed -- there is NO refit over the inliers, the ICP stage follows -- and
 *      d_stat = (1, the seed's row, count, n_valid, its rank, its degree), n_valid = the valid seeds.  d_rmse follows
 *      cs_ransac_fm_batch's fixed-point rule (the same k, the same truncation).  d_inlier = the best pose's mask (d2 < thr2)
 *      over the first m slots of the problem and 0 in the slots behind them and in every slot of a problem without a pose;
 *      slots before h_off[0] are written with 0.
 *   Rows with a NaN or infinite coordinate are compatible with nothing and never inliers.  A max_corr whose square overflows
 *     counts every pair with a finite d2; one whose square underflows counts nothing.
 *   h. Independence: the result of a problem is a function of its pairs in their order and of the parameters alone.  Batch
 *      neighbours, the capacity behind m, the stream, the launch shape (CS_SC2_CHUNK_BYTES, CS_SC2_SLICE, CS_SC2_SPAN) and the
 *      run do not reach it.  A permutation of the pairs permutes the matrix, the degrees and the second-order counts with
 *      it; it enters the result through the ~i tie keys (which of several rows of one degree is a seed and of which rank,
 *      which of several rows of one count joins A_s, which of two seeds of one count wins) and through the order of the
 *      fit's sums (the last bits of R and t) only.
 *   n_prob = 0, empty problems and m < 3 are legal.  Refused (CS_ERR_INVALID): a NULL offset table, a negative count, offsets
 *     that decrease, compat_dist or max_corr not positive and finite, n_seeds < 0, NULL d_T, d_stat or d_rmse with
 *     n_prob > 0, NULL d_src or d_tgt while a slot exists; (CS_ERR_UNSUPPORTED): k_consensus outside [2, 64], a problem of
 *     more than 32 768 slots (its bit matrix is 128 MiB; the message advises a smaller k_nn).  The checks come before any
 *     device work.
 *   Memory: one bit per ordered pair, sized by the CAPACITY, which the host knows (8 B x capacity x ceil(capacity / 64)).  A
 *     call whose matrices exceed CS_SC2_CHUNK_BYTES (read per call, default 256 MiB) runs in chunks of whole consecutive
 *     problems, never fewer than one, with the same bits.  The checks and the planner stand in corsair_amd/csrc/sc2_plan.h.
 *   Differences from SC2-PCR and spectral matching, deliberate: NO eigenvector -- seeds are ranked by the integer degree;
 *     no non-maximum suppression among the seeds; ONE consensus stage instead of two; an UNWEIGHTED fit; a HARD compatibility
 *     instead of a soft one; the winner is ranked by its inlier count; NO final refit over the inliers.
 *   Kernels (sc2.hip), per chunk: the matrix build (a lane owns a row and walks 64 wave-uniform rows per word; one triangle
 *     and its transpose; CS_SC2_SPAN word columns per wave, default 8), the degrees by integer atomicAdd, the rank by
 *     counting larger keys, one wave per seed for the second-order counts and the K best, one thread per seed for the fit,
 *     the count of 256 seeds x one slice of CS_SC2_SLICE pairs (default 1024) per workgroup, the u64 atomicMax.  The same
 *     bits for every value of the three variables.
 * ---------------------------------------------------------------------------------------- */
int cs_sc2_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, const int32_t* d_m, int n_prob,
                 double compat_dist, double max_corr, int n_seeds, int k_consensus, double* d_T, int32_t* d_stat,
                 double* d_rmse, uint8_t* d_inlier, void* stream);

/* ------------------------------------------------------------------------------------------
 * Point-pair-feature voting: a pose of a scene against a model from oriented points alone, with no descriptor
 * and no correspondence list (Drost, Ulrich, Navab and Ilic, CVPR 2010, as remembered from the paper; the list of
 * differences is at the end).  The reference has no such step, so this comment is the specification and tests/ppf_ref.py
 * restates it bit for bit.  Every operation is ONE IEEE f64 operation in the order the parentheses give; an fma appears only
 * where fma( is written (step h); nothing is contracted; only + - * / sqrt fma, casts and comparisons appear; a comparison
 * with a NaN is false.  Everything is enqueued on `stream`; scratch comes from the calling thread's pool; no host wait, no
 * cooperative launch, no flag a thread waits on; the only atomics are integer; every loop is bounded by an argument or a
 * segment's rows.  Profile family "ppf", one scope per call.
 *
 * cs_ppf_batch: d_scene, d_scene_normal f32 [rows,3] with host offsets h_soff; d_model, d_model_normal f32 [rows,3] with host
 *   offsets h_moff; problem p < n_prob pairs scene segment h_scene_seg[p] with model segment h_model_seg[p], selected as in
 *   cs_icp_batch; segments may be shared between problems.  h_dist_step f64 [n_prob] on the host: one distance step per
 *   problem; max_dist: the verification radius; ref_step >= 1; n_cand in [1, 64].  Outputs, all on the device: d_T, d_Tinv
 *   f64 [n_prob,4,4]; d_stat int32 [n_prob,8]; d_rmse f64 [n_prob]; d_cand_T f64 [n_prob,n_cand,4,4]; d_cand_stat int32
 *   [n_prob,n_cand,4].  Normals must be ORIENTED (cs_orient_normals); they need not be unit vectors.
 *   Row: x = the coordinates and N = the normal, widened to f64.  nn = sqrt((N_0 * N_0 + N_1 * N_1) + N_2 * N_2).  The row is
 *     VALID when its six values are finite and nn > 0; then u = (N_0 / nn, N_1 / nn, N_2 / nn).  An invalid row is no
 *     reference, takes part in no pair and stands in no table; step h counts it when its coordinates are finite.
 *   b. Local frame of a valid row: the rotation that takes u to +x, I + [v]x + [v]x^2 / (1 + c) with v = u cross x and
 *      c = u_0, written out: k = 1.0 + u_0; when k >= 2^-20, with w = (u_1 * u_2) / k:
 *        row0 = (u_0, u_1, u_2),  row1 = (-u_1, 1.0 - (u_1 * u_1) / k, -w),  row2 = (-u_2, -w, 1.0 - (u_2 * u_2) / k);
 *      otherwise (u within 1.4e-3 rad of -x) the half turn about y: row0 = (-1, 0, 0), row1 = (0, 1, 0), row2 = (0, 0, -1).
 *      The frame of the row is p -> R (p - x).
 *   a. Feature of the ordered pair (i, j), i != j, of two valid rows of ONE segment: d = x_j - x_i (three subtractions),
 *      len = sqrt((d_0 * d_0 + d_1 * d_1) + d_2 * d_2), q = len / dist_step, dot(a, b) = (a_0 * b_0 + a_1 * b_1) + a_2 * b_2,
 *        c1 = dot(u_i, d) / len,  c2 = dot(u_j, d) / len,  c3 = dot(u_i, u_j),
 *        y = (float)dot(row1_i, d),  z = (float)dot(row2_i, d)      -- the in-plane direction of the pair, stored as f32.
 *      The pair is SKIPPED when !(len > 0), when !(q < 64.0), or when y or z is not finite or both are zero (d parallel to
 *      the normal: no in-plane direction).  dbin = (int)q.  An angle has 15 bins of 12 degrees: bin(c) = the number of
 *      k in 1..14 with c <= C_k, C_k = cos(12 k degrees) -- an angle AT a boundary belongs to the bin above it, a cosine
 *      beyond +-1 by a rounding goes to bin 0 or 14.  corsair_amd/csrc/ppf_bounds.h (tools/gen_ppf_bounds.py) tabulates C_k
 *      as f64 literals and THOSE numbers are the specification.  key = ((dbin * 15 + bin(c1)) * 15 + bin(c2)) * 15 + bin(c3).
 *   c. Model table of (model segment, dist_step): every ordered pair of the segment that is not skipped, as the entry
 *      (m_r = i local to the segment, y, z), grouped by key.  A table is built once per chunk (below) for all the problems of
 *      the chunk that share the segment and the step.  The order of the entries inside a key reaches no output.
 *   d. Voting.  The references of a problem are the scene rows r (local to the segment) with r % ref_step == 0; n_ref of
 *      them.  For a valid reference r and every scene row i != r whose pair (r, i) is not skipped, every entry (m_r, ym, zm)
 *      of the table under the pair's key casts ONE vote, an integer increment of the cell m_r * 30 + bin.  With (ys, zs) of
 *      the scene pair, all four f32 values widened:  px = ym * ys + zm * zs,  py = zm * ys - ym * zs  (the complex product of
 *      the model direction and the conjugate of the scene direction; alpha = its angle, the turn about x that takes the
 *      scene pair onto the model pair).  30 bins over [-pi, pi): bin = the number of boundaries theta_m = 2 pi (m - 15) / 30,
 *      m = 1..29, not above alpha, found without a transcendental function: ppf_bounds.h tabulates (c_m, s_m) =
 *      (cos theta_m, sin theta_m), t_m = c_m * py - s_m * px (no fma).  py < 0: the number of m in 1..14 with t_m >= 0; else
 *      15 + the number of m in 16..29 with t_m >= 0.  DELIBERATE DIFFERENCE from atan2, as in cs_fpfh: py = -0 with px < 0
 *      gives bin 29 like py = +0.
 *   e. Peak of a reference: the maximum over its cells with votes > 0 of votes << 32 | ~cell (~: the 32-bit complement): the
 *      most votes, ties to the SMALLEST cell.  An invalid reference and one without a vote have votes = 0.
 *   f. Candidates of a problem: the min(n_cand, n_ref) references of the largest key votes << 32 | ~(r / ref_step), the
 *      largest first (cs_sc2_batch's rank rule): candidate c has rank c.  A candidate with votes = 0 is INVALID.
 *   g. Pose of a valid candidate (reference s with frame Rs, model row m with frame Rm, bin b): Tm^-1 Rx(alpha_b) Ts with
 *      (ca, sa) = (cos alpha_b, sin alpha_b), alpha_b = 2 pi (b - 14.5) / 30 the centre of the bin, tabulated in ppf_bounds.h:
 *        A_0k = Rs_0k,  A_1k = ca * Rs_1k - sa * Rs_2k,  A_2k = sa * Rs_1k + ca * Rs_2k,
 *        R_ak = (Rm_0a * A_0k + Rm_1a * A_1k) + Rm_2a * A_2k,
 *        t_a = x_m,a - ((R_a0 * x_s,0 + R_a1 * x_s,1) + R_a2 * x_s,2).      T = (R | t; 0 0 0 1) maps the SCENE onto the MODEL.
 *   h. Verification of a valid candidate: for every scene row (x, y, z) of the segment with finite coordinates,
 *        P_a = fma(R_a2, z, fma(R_a1, y, fma(R_a0, x, t_a)))   (the canonical chain of the posed source),
 *        d2_j = fma(e_2, e_2, fma(e_1, e_1, e_0 * e_0)),  e = P - x_j,  over EVERY model row j (valid or not; a NaN or
 *        infinite d2 is never the minimum), dmin = the smallest.  The row COUNTS when dmin < max_dist * max_dist (formed
 *        once), strictly.  count = the rows that count; the squared error is the sum of (uint64)(dmin * 2^k) over them,
 *        k = 61 - eM - ex, ns <= 2^eM, max_dist^2 = f 2^ex (cs_sc2_batch's fixed-point rule with the scene rows as m).
 *   i. Winner: the valid candidate of the largest count << 32 | ~rank (ties to the smallest rank).
 *      d_T = its T; d_Tinv = (R^T | ti), ti_a = -((R_0a * t_0 + R_1a * t_1) + R_2a * t_2), maps the model onto the scene;
 *      d_stat = (1, votes, scene row, model row, alpha bin, count, rank, n_ref); d_rmse = sqrt((error * 2^-k) / count), 0 when
 *      count = 0.  d_cand_T[c], d_cand_stat[c] = T and (votes, count, scene row, cell) of candidate c; the identity and
 *      (0, 0, -1, -1) for an invalid candidate and for the slots behind min(n_cand, n_ref).
 *      No valid candidate -- an empty or one-row scene or model, every row invalid, every pair skipped -- : found = 0,
 *      d_T = d_Tinv = the identity, d_stat = (0, 0, -1, -1, -1, 0, -1, n_ref), d_rmse = 0.
 *   Independence: the result of a problem is a function of its two segments and of dist_step, max_dist, ref_step and n_cand
 *     alone.  Batch neighbours, the stream, the launch shape (CS_PPF_CHUNK_BYTES, CS_PPF_ACC) and the run do not reach it.  A
 *     permutation of the rows permutes the tables and the votes with it; it enters the result through the ~ tie keys and
 *     through which rows are references only.
 *   n_prob = 0 and empty segments are legal.  Refused (CS_ERR_INVALID): a negative problem count, a NULL host table, a
 *     negative segment id, offsets that decrease or are negative, a dist_step or max_dist not positive and finite,
 *     ref_step < 1, a NULL output with n_prob > 0, a NULL array while a row exists; (CS_ERR_UNSUPPORTED): n_cand outside
 *     [1, 64], a model segment of more than 4 096 rows (its table of all ordered pairs is 192 MiB; the message advises a
 *     coarser voxel), a scene segment of more than 16 384 rows.  The checks come before any device work.
 *   Memory: a table takes 12 B per ordered pair and 8 B x 216 001 keys.  The accumulator of a reference, model rows x 30 u32
 *     counters, lives in the LDS of its workgroup when the model has at most 1 360 rows (163 200 B of the 160 KiB of a CU) and
 *     in one of 256 zeroed global slabs otherwise; CS_PPF_ACC=global (read per call) sends every problem to the slabs,
 *     CS_PPF_ACC=lds names the default.  The same bits on both paths: both add integers.  A call whose tables and slabs
 *     exceed CS_PPF_CHUNK_BYTES (read per call, default 512 MiB; every problem is counted with a table of its own) runs in
 *     chunks of whole consecutive problems, never fewer than one, with the same bits.  The checks, the accumulator rule and
 *     the planner stand in corsair_amd/csrc/ppf_plan.h.
 *   Differences from Drost et al., deliberate: NO pose clustering and NO averaging of the poses of a cluster -- the
 *     candidates are the best references, each verified by an exhaustive nearest-row count, and the ICP stage follows; the
 *     model is NOT subsampled here (the caller's voxel size does that) and the table holds ALL m^2 pairs; every n-th row is
 *     a reference instead of a random fifth; alpha is binned from the pair of directions at vote time instead of being
 *     stored as an angle.  The raw pose carries the 12 degree resolution of alpha: up to 6 degrees about the normal.
 *   Limits: a flipped normal (a concave part oriented away from the centroid) changes the feature and loses the
 *     votes of its pairs; a symmetric model has several equal peaks and the tie rule picks one; the table grows with m^2.
 * ---------------------------------------------------------------------------------------- */
int cs_ppf_batch(const float* d_scene, const float* d_scene_normal, const int64_t* h_soff, const float* d_model,
                 const float* d_model_normal, const int64_t* h_moff, const int32_t* h_scene_seg, const int32_t* h_model_seg,
                 int n_prob, const double* h_dist_step, double max_dist, int ref_step, int n_cand, double* d_T, double* d_Tinv,
                 int32_t* d_stat, double* d_rmse, double* d_cand_T, int32_t* d_cand_stat, void* stream);

/* ------------------------------------------------------------------------------------------
 * Partial views: a virtual depth camera per segment -- hidden-point removal by a splat z-buffer.  The reference
 * has no such step, so this comment is the specification and tests/view_ref.py restates it bit for bit.  As in the blocks
 * above: every operation is ONE IEEE f64 operation in the order given, or an explicit fma; nothing is contracted; only
 * + - * / floor fma min, comparisons and integer arithmetic appear (min(a, b) = a < b ? a : b); every threshold is STRICT; a
 * comparison with a NaN is false.
 *
 * cs_render_views: d_xyz f32 [n,3]; h_off int64 [n_seg + 1] host offsets; segment s is seen by camera s.  d_cam f64
 *   [n_seg,12] on the device: the rows R | t of the rigid world -> camera map, row c = (R_c0, R_c1, R_c2, t_c); the camera
 *   looks along +z.  width, height in [1, 4096]; focal (pixels), point_size and depth_tol (world units) finite and > 0.
 *   d_visible u8 [n] (0 / 1); d_depth f32 [n_seg, height, width] or NULL; d_stat int32 [n_seg,4].
 *   Per row (x, y, z), widened to f64, of segment s:
 *     P_c = fma(R_c2, z, fma(R_c1, y, fma(R_c0, x, t_c))), c = 0, 1, 2 (the pose chain of cs_ransac_batch's count and of
 *       cs_ransac_fm_batch, restated in the unit); Z = P_2.
 *     The row is IN FRONT when P_0, P_1 and P_2 are finite and Z > 0.  Nothing below is formed for another row.
 *     u = fma(focal, P_0 / Z, 0.5 * width), v = fma(focal, P_1 / Z, 0.5 * height) (width and height converted to f64).
 *     h = min(((0.5 * focal) * point_size) / Z, 16.0): half the side of the row's square in pixels.  The cap of 16 pixels is
 *       part of the semantics: it bounds the work of a row that sits on the lens to 33 x 33 pixels.
 *     Centre pixel: (cu, cv) = (floor(u), floor(v)).  The row is IN FRAME when 0 <= cu < width && 0 <= cv < height, compared
 *       as doubles.
 *     Footprint: the pixel columns floor(u - h) .. floor(u + h) and the rows floor(v - h) .. floor(v + h), each value
 *       clamped AS A DOUBLE to [-1, width] (to [-1, height]) before the conversion to int, then clipped to the image.  A row
 *       that is in front but out of frame still covers what its footprint reaches.
 *   Depth buffer: zbuf[s,y,x] = the minimum Z over the in-front rows of segment s whose footprint covers (x, y), +inf
 *     without one.  Positive finite doubles order as their bit patterns: one u64 atomicMin per covered pixel, order-free.
 *   Visible: in front, in frame, and Z - zbuf[s,cv,cu] < depth_tol.  A row's own footprint holds its centre pixel (floor is
 *     monotonic and h >= 0), so the difference is >= 0.
 *   d_visible = the mask.  d_depth = the buffer converted ONCE to f32 (round to nearest even; +inf stays, a Z above the
 *     largest float becomes +inf).  d_stat[s] = (rows in front, rows in frame, rows visible, pixels whose f64 depth is
 *     finite).
 *   Independence: the result of a segment is a function of the SET of its rows and of its camera.  A permuted segment gives
 *     the permuted mask and the same depth image and stat row, bit for bit; batch neighbours, the stream, the launch shape
 *     (CS_VIEW_CHUNK_BYTES, CS_VIEW_PRECHECK) and the run do not reach it.
 *   Grazing surfaces: a row whose surface is seen at a flat angle can be hidden by a NEIGHBOUR's camera-facing square that
 *     covers its centre pixel from more than depth_tol in front; a square below about one row spacing lets rows of the far
 *     side through between the near ones (tests/test_view_cpu.py).  A depth sensor loses grazing surfaces too.
 *   n_seg = 0 and empty segments are legal: an empty segment has an all-+inf image and a zero stat row.
 *   Refused (CS_ERR_INVALID): a NULL offset table, a negative count, offsets that decrease; focal, point_size or depth_tol
 *     not finite or <= 0; NULL d_cam or d_stat with n_seg > 0; NULL d_xyz or d_visible while a row exists;
 *     (CS_ERR_UNSUPPORTED): width or height outside [1, 4096], a segment of 2^31 rows or more.  The checks come before any
 *     device work.
 *   Differences from [O3D-knowledge] Open3D's hidden_point_removal (Katz's operator: spherical flipping and a convex hull):
 *     no hull; a pinhole image of a fixed resolution decides, so the result depends on width, height, point_size and
 *     depth_tol, and rows outside the image are never visible.
 *   Kernels (view.hip), per chunk of whole segments whose buffers (8 B x height x width each) fit CS_VIEW_CHUNK_BYTES (read
 *     per call, default 256 MiB, never fewer than one segment): a fill, the splat (one lane per row), the resolve (one lane
 *     per row, integer stat atomics) and the export (one lane per pixel).  CS_VIEW_PRECHECK=0 (read per call) drops the read
 *     of a pixel before its atomic; the buffer only decreases, so the read changes no result.  Everything is enqueued on
 *     `stream`; scratch comes from the calling thread's pool; no host wait, no cooperative launch, no flag a thread waits
 *     on; the only atomics are integer.  Profile family "view", one scope per call.
 * ---------------------------------------------------------------------------------------- */
int cs_render_views(const float* d_xyz, const int64_t* h_off, int n_seg, const double* d_cam, int width, int height,
                    double focal, double point_size, double depth_tol, uint8_t* d_visible, float* d_depth, int32_t* d_stat,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Profiling hooks for bench.py: when enabled the library brackets the launches of each named
 * kernel family with hipEvents on the launch stream and accumulates the elapsed time.
 * names: "conv", "ransac_eval", "ransac_pre", "ransac_hyp", "knn", "chamfer", "topk", "symcut",
 * "kmap", "loss", "hardneg", "icp", "normals", "fgr", "chamfer2", "fpfh", "orient", "outlier", "cluster", "plane",
 * "featmatch", "view", "sc2", "ppf".
 * ---------------------------------------------------------------------------------------- */
void cs_prof_enable(int on);
void cs_prof_reset(void);
int cs_prof_get(const char* name, double* total_ms, int64_t* launches);
/* algorithmic work (FLOP) the bracketed launches of the family performed since the last reset */
int cs_prof_get_units(const char* name, double* units);

/* Return the calling thread's cached scratch memory to the HIP runtime.  Scratch is cached per host
 * thread (one stream per thread), so the library may be driven from several threads at once. */
void cs_pool_trim(void);
/* out = {live scratch/handle blocks, blocks freed by a thread other than the one that allocated them,
 * bytes cached by the calling thread}.  A handle (cs_coordmap_free / cs_kernelmap_free) may be dropped on
 * any thread: a foreign block is released with hipFree (device-synchronising), never recycled into the
 * freeing thread's stream-ordered cache. */
void cs_pool_stats(uint64_t out[3]);

/* ------------------------------------------------------------------------------------------
 * TEST HOOKS of the scratch pool (tests/test_gpu_stale_memory.py).  No product path calls them.
 *
 * cs_pool_poison: pattern in 0..255 -- from then on every block the pool hands out, fresh from the driver or cached, on any
 *   host thread, is first filled with that byte over its whole size class; any other value (-1 by convention) turns the
 *   hook off, which is the default.  While the hook is on every allocation waits for the DEVICE, fills the block and waits
 *   for the device again: a cached block may still be read by work queued in stream order, and the library's side streams
 *   are non-blocking, so no stream could order the fill.  Stream overlap is therefore gone in this mode; results are not.
 *   With the hook off the cost is one relaxed atomic load per allocation.  A result that changes with the pattern shows a
 *   kernel that reads scratch (or handle storage) it has not written.
 * cs_pool_poison_stats: out = {blocks, bytes} poisoned since the process started or since the last call with reset != 0.
 * cs_pool_peek: takes a pool block of `bytes` (> 0) as an entry point would, copies its first `bytes` bytes device-to-device
 *   to d_out on `stream` and frees the block again: what a kernel would find in scratch of that size.
 * ---------------------------------------------------------------------------------------- */
void cs_pool_poison(int pattern);
void cs_pool_poison_stats(uint64_t out[2], int reset);
int cs_pool_peek(size_t bytes, uint8_t* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CORSAIR_HIP_H */
