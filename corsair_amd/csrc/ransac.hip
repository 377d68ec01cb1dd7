// Batched correspondence RANSAC on gfx950.
//
// Replaces registration_based_on_corr -> Open3D registration_ransac_based_on_correspondence
// (utils/eval_pose.py:82-100 of the reference; ransac_n = 10, 100 000 iterations, confidence 0.999).
// Semantics: Open3D's loop as executed by ONE thread (iteration order = index order), with the
// global Mersenne twister replaced by a counter-based generator so that iteration i of every
// problem is reproducible anywhere.  Iterations are processed in rounds of growing chunks: [0, 64) (CS_RANSAC_FIRST),
// [64, 512), then doubling -- [512, 1024), [1024, 2048), ... -- up to 16 384 per round.  The first chunk is counted
// exactly (there is no best count to prune against yet); every later one goes through the f16 prefilter.  A round:
//   k_ransac_hyp        one lane per hypothesis: sample ransac_n pairs (packed 32-B rows), closed-form
//                       rigid fit (Horn quaternion; largest eigenpair of the 4x4 matrix from its characteristic
//                       polynomial, horn_qcp, with the Jacobi eigen-solver as per-lane fallback; f64), emit R|t as f64
//                       (Open3D keeps the Matrix4d; the f32 cast happens at the very end, where the
//                       reference casts the result: utils/symmetry.py:274); in a prefiltered round also the
//                       hypothesis' prefilter row (pf_emit_row: 16 f16 coefficients + c_h)
//   k_ransac_prefilter  (from the second chunk on) an UPPER bound of every hypothesis' inlier count on the
//                       f16 matrix cores; hypotheses whose bound is below the carried best cannot
//                       matter and get count 0.  <1, true> = one MFMA per tile (K = 16: a_hi . b_hi',
//                       the dropped term bounded per pair), signs counted by v_add_f32 under
//                       round-toward-minus-infinity; 0.2 % survive.  <2, false> = two MFMAs per tile (K = 32:
//                       a_hi . (b_hi + b_lo)), signs through a v_alignbit history: the whole prefilter with
//                       CS_RANSAC_PF_K=32, and always the SECOND STAGE -- the survivors of the K = 16 bound,
//                       compacted by k_ransac_survivors, go through it (list mode) before the exact count.  See the
//                       block comments above k_ransac_pack16_b0 / the kernel and DESIGN.md ("RANSAC prefilter").
//   k_ransac_count      the exact count in Open3D's arithmetic: the reference hands Open3D f64 points
//                       (utils/eval_pose.py:83-86) and Eigen transforms and compares in double, so the
//                       inlier test is evaluated in f64: a lane owns one hypothesis (R|t in 12 f64
//                       registers), the pairs of a 256-row stage are converted to f64 once and read
//                       from LDS as broadcasts; p = fma(r2,sz, fma(r1,sy, fma(r0,sx, t))), d = p - q,
//                       |d|^2 = fma(dz,dz, fma(dy,dy, dx dx)) < max_corr^2 (the canonical chain, the
//                       oracle's).  Used for all hypotheses of an unfiltered chunk (<false, 64> for a chunk of 64)
//                       and (<true>) for survivor lists longer than 1024 per problem; k_ransac_count_few handles
//                       the usual handful of survivors (same chain, count and fixed-point error in one pass).  These
//                       kernels see ~0.1 % of the (hypothesis, pair) work; the f16 prefilter carries the rest.
//   k_ransac_scan1      one wave per problem replays the chunk in iteration order (prefix max of the
//                       inlier counts -> early-exit bound est_k -> stop position) and lists the
//                       hypotheses that tie for the best count.  When k_ransac_count_few has left their errors it
//                       also picks the best of them: the usual round is hyp -> prefilter -> survivors ->
//                       second-stage prefilter -> count_few -> scan1, six launches.  Otherwise:
//   k_ransac_err        fixed-point squared error (exact integer sums) of those few candidates
//   k_ransac_scan2      best = max count, then min error, then first -- the final state of the
//                       sequential rule "better = more inliers, or equal inliers and smaller rmse"
// The host loop (cs_ransac_batch, at the end of this file) synchronises once per round (one pinned copy of the
// per-problem state); the next round's hypotheses and prefilter are already enqueued at that point.
// Inlier counts and fixed-point errors are integers, so any split of the correspondence range across
// workgroups gives identical sums.
#include <math.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "common.h"
#include "exact_div.h"
#include "horn.h"

namespace cs {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

struct RansacProb {
  int64_t off;
  int32_t m;
  int32_t est_k;
  int32_t best_cnt;
  int32_t best_itr;
  unsigned long long best_err;
  int32_t done;
  int32_t iters;
  // per-chunk scratch written by scan1, read by err / scan2
  int32_t n_cand;
  int32_t chunk_max;
  double best_T[12];
};

// The kernels of a round's front half (hypotheses, f16 rows, prefilter) may run while the previous
// round's scan kernels update est_k / done (cs_ransac_batch): they read the two fields with relaxed
// atomic loads and only use them to skip work -- either value is safe (est_k only shrinks, done only
// rises), the scan kernels decide with the final state.
__device__ __forceinline__ RansacProb prob_view(const RansacProb* probs, int p) {
  RansacProb v = {};
  v.off = probs[p].off;
  v.m = probs[p].m;
  v.est_k = __atomic_load_n(&probs[p].est_k, __ATOMIC_RELAXED);
  v.done = __atomic_load_n(&probs[p].done, __ATOMIC_RELAXED);
  return v;
}

// rng_u64: common.h
__host__ __device__ static inline uint32_t rng_index(uint64_t seed, uint64_t itr, uint64_t j,
                                                     uint32_t m) {
  return (uint32_t)(((rng_u64(seed, itr, j) >> 32) * (uint64_t)m) >> 32);
}

// structure-of-arrays copy of the correspondences: pk[c * total + i], c = sx,sy,sz,qx,qy,qz
// + pair32[i] = (sx, sy, sz, qx | qy, qz, 0, 0): one aligned 32-B sector per pair for the random
// sampling of k_ransac_hyp (two 12-B rows of the caller's arrays would touch two to four lines)
__global__ void k_ransac_pack(const float* __restrict__ src, const float* __restrict__ tgt,
                              int64_t n, float* __restrict__ pk, float4* __restrict__ pair32) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  pair32[2 * i + 0] = make_float4(src[3 * i + 0], src[3 * i + 1], src[3 * i + 2], tgt[3 * i + 0]);
  pair32[2 * i + 1] = make_float4(tgt[3 * i + 1], tgt[3 * i + 2], 0.f, 0.f);
  pk[0 * n + i] = src[3 * i + 0];
  pk[1 * n + i] = src[3 * i + 1];
  pk[2 * n + i] = src[3 * i + 2];
  pk[3 * n + i] = tgt[3 * i + 0];
  pk[4 * n + i] = tgt[3 * i + 1];
  pk[5 * n + i] = tgt[3 * i + 2];
}

// hyp layout: [prob][12][bmax] (structure of arrays), element 4a+b = R[a][b], 4a+3 = t[a]
// RN = ransac_n when it is known at compile time (10: the reference's value; the loops are unrolled and the sampled
// pairs stay in registers between the centroid and the covariance pass), 0 = read it from the argument and read the
// pairs again; inv_n = exact_div_recip(ransac_n)
// Placement table of a round (problem of XCD x, slot i) as a kernel ARGUMENT: the host builds it per round, a
// device copy of it was one hipMemcpyAsync (a blit-kernel launch) per round.  Rounds with more than XCD_SLOTS
// problems per XCD fall back to the device table (xcd_ptr != nullptr).
constexpr int XCD_SLOTS = 64;
struct XcdTab {
  int32_t v[8 * XCD_SLOTS];
};
__device__ __forceinline__ int xcd_problem(const int32_t* __restrict__ xcd_ptr, const XcdTab& tab, int i) {
  return xcd_ptr ? xcd_ptr[i] : tab.v[i];
}

// (defined with the prefilter's operand kernels below)
__device__ __forceinline__ void pf_emit_row(const RansacProb& pr, int p, int h, int bmax, const double (&R)[3][3], double (&t)[3],
                                            const unsigned* __restrict__ stat, const double* __restrict__ sums, double thr2,
                                            double tcap, _Float16* __restrict__ A16, float* __restrict__ c_h);

// centroids = sums / ransac_n, six quotients with one divisor: exact_div.h's multiply-and-correct sequence, which returns the
// IEEE quotient (proof and conditions there), when the host found the divisor admissible (inv_n != 0) and all six sums are in
// the proven range; otherwise (a sum that is 0, subnormal or not finite) the six divisions as before
__device__ __forceinline__ void centroid_div(double (&cs_)[3], double (&ct_)[3], double dn, double inv_n) {
  bool fast = inv_n != 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) fast = fast && exact_div_ok(cs_[a]) && exact_div_ok(ct_[a]);
  if (fast) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      cs_[a] = exact_div(cs_[a], dn, inv_n);
      ct_[a] = exact_div(ct_[a], dn, inv_n);
    }
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      cs_[a] = cs_[a] / dn;
      ct_[a] = ct_[a] / dn;
    }
  }
}

// Five waves per SIMD: the attribute holds the register allocator to that budget for BOTH instantiations -- <10> takes 96
// registers and <0> 94, neither uses scratch (without it <10> takes 107 and runs at four waves).  The budget is not free: a
// change here or in horn.h that needs more registers would spill instead of failing, so check the compiler's resource report
// (-Rpass-analysis=kernel-resource-usage: VGPRs <= 96, ScratchSize 0) after touching either.
template <int RN>
__attribute__((amdgpu_waves_per_eu(5, 5)))
__global__ __launch_bounds__(256) void k_ransac_hyp(const RansacProb* probs,
                                                    const float4* __restrict__ pair32, int it0,
                                                    int bcount, int bmax, int ransac_n, double inv_n,
                                                    uint64_t seed,
                                                    const int32_t* __restrict__ xcd_prob, const XcdTab xcd_tab,
                                                    int slots, int tiles, int force_jacobi,
                                                    double* __restrict__ hyp,
                                                    // prefilter rows of the chunk (A16 != nullptr): pf_emit_row
                                                    const unsigned* __restrict__ pf_stat, const double* __restrict__ pf_sums,
                                                    double thr2, double tcap, _Float16* __restrict__ A16,
                                                    float* __restrict__ c_h, int32_t* __restrict__ cnt_zero) {
  // 1-D grid dealt round-robin to the XCDs: XCD x samples only the problems xcd_prob[x][.], whose
  // correspondences then stay in that XCD's L2 (the sampling is a random gather of 24-B rows)
  const int xcd = blockIdx.x & 7;
  const int item = blockIdx.x >> 3;
  const int slot = item / tiles;
  const int p = xcd_problem(xcd_prob, xcd_tab, xcd * slots + slot);
  if (p < 0) return;
  const int h = (item - slot * tiles) * blockDim.x + threadIdx.x;
  if (h >= bcount) return;
  // the prefilter behind this kernel adds the partial counts of its pair-range splits with atomics: cleared here
  if (cnt_zero) cnt_zero[(int64_t)p * bmax + h] = 0;
  const RansacProb pr = prob_view(probs, p);
  const int itr = it0 + h;
  if (pr.done || itr >= pr.est_k) return;
  const uint32_t m = (uint32_t)pr.m;
  double cs_[3] = {0, 0, 0}, ct_[3] = {0, 0, 0};
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  if (RN > 0) {
    // the ten samples stay in registers between the two passes AS THE f32 VALUES THEY WERE LOADED AS (60 registers)
    float pa[RN > 0 ? RN : 1][6];
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int64_t i = pr.off + rng_index(seed, (uint64_t)itr, (uint64_t)j, m);
      const float4 a = pair32[2 * i], b = pair32[2 * i + 1];  // one 32-B sector
      pa[j][0] = a.x; pa[j][1] = a.y; pa[j][2] = a.z; pa[j][3] = a.w; pa[j][4] = b.x; pa[j][5] = b.y;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        cs_[c] += (double)pa[j][c];
        ct_[c] += (double)pa[j][3 + c];
      }
    }
    centroid_div(cs_, ct_, (double)RN, inv_n);
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      // opaque copies, so that the values are converted to f64 AGAIN here: the compiler otherwise keeps the sixty f64
      // conversions of the first pass alive (120 registers; the kernel then held 164 and ran at three waves per SIMD).
      // Reading the sectors a second time instead was measured slower than the parent (113 vs 105 us per launch).
#pragma unroll
      for (int c = 0; c < 6; ++c) asm volatile("" : "+v"(pa[j][c]));
      const double ds[3] = {(double)pa[j][0] - cs_[0], (double)pa[j][1] - cs_[1], (double)pa[j][2] - cs_[2]};
      const double dt[3] = {(double)pa[j][3] - ct_[0], (double)pa[j][4] - ct_[1], (double)pa[j][5] - ct_[2]};
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) S[x][y] = fma(ds[x], dt[y], S[x][y]);
    }
  } else {
    for (int j = 0; j < ransac_n; ++j) {
      const int64_t i = pr.off + rng_index(seed, (uint64_t)itr, (uint64_t)j, m);
      const float4 a = pair32[2 * i], b = pair32[2 * i + 1];  // one 32-B sector
      cs_[0] += (double)a.x;
      cs_[1] += (double)a.y;
      cs_[2] += (double)a.z;
      ct_[0] += (double)a.w;
      ct_[1] += (double)b.x;
      ct_[2] += (double)b.y;
    }
    centroid_div(cs_, ct_, (double)ransac_n, inv_n);
    for (int j = 0; j < ransac_n; ++j) {
      const int64_t i = pr.off + rng_index(seed, (uint64_t)itr, (uint64_t)j, m);
      const float4 a = pair32[2 * i], b = pair32[2 * i + 1];
      const double ds[3] = {(double)a.x - cs_[0], (double)a.y - cs_[1], (double)a.z - cs_[2]};
      const double dt[3] = {(double)a.w - ct_[0], (double)b.x - ct_[1], (double)b.y - ct_[2]};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) S[a][b] = fma(ds[a], dt[b], S[a][b]);
    }
  }
  double N[4][4], V[4][4];
  N[0][0] = S[0][0] + S[1][1] + S[2][2];
  N[0][1] = S[1][2] - S[2][1];
  N[0][2] = S[2][0] - S[0][2];
  N[0][3] = S[0][1] - S[1][0];
  N[1][1] = S[0][0] - S[1][1] - S[2][2];
  N[1][2] = S[0][1] + S[1][0];
  N[1][3] = S[2][0] + S[0][2];
  N[2][2] = -S[0][0] + S[1][1] - S[2][2];
  N[2][3] = S[1][2] + S[2][1];
  N[3][3] = -S[0][0] - S[1][1] + S[2][2];
  N[1][0] = N[0][1];
  N[2][0] = N[0][2];
  N[3][0] = N[0][3];
  N[2][1] = N[1][2];
  N[3][1] = N[1][3];
  N[3][2] = N[2][3];
  double qv[4];
  if (force_jacobi || !horn_qcp(S, N, qv)) {
    // rare (ill-separated largest eigenvalue): the lanes that need it run the Jacobi solver
    jacobi4(N, V);
    // eigenvector of the largest eigenvalue (ties -> lowest index), selected without dynamic indexing
    double best = N[0][0];
    qv[0] = V[0][0]; qv[1] = V[1][0]; qv[2] = V[2][0]; qv[3] = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
      if (N[c][c] > best) {
        best = N[c][c];
        qv[0] = V[0][c];
        qv[1] = V[1][c];
        qv[2] = V[2][c];
        qv[3] = V[3][c];
      }
    }
  }
  double qw = qv[0], qx = qv[1], qy = qv[2], qz = qv[3];
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw = qw / qn;
  qx = qx / qn;
  qy = qy / qn;
  qz = qz / qn;
  double R[3][3];
  R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  R[0][1] = 2.0 * (qx * qy - qw * qz);
  R[0][2] = 2.0 * (qx * qz + qw * qy);
  R[1][0] = 2.0 * (qx * qy + qw * qz);
  R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
  R[1][2] = 2.0 * (qy * qz - qw * qx);
  R[2][0] = 2.0 * (qx * qz - qw * qy);
  R[2][1] = 2.0 * (qy * qz + qw * qx);
  R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
  double* o = hyp + ((int64_t)p * 12) * bmax + h;
  double tv[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t = ct_[a] - (R[a][0] * cs_[0] + R[a][1] * cs_[1] + R[a][2] * cs_[2]);
    tv[a] = t;
    o[(int64_t)(4 * a + 0) * bmax] = R[a][0];
    o[(int64_t)(4 * a + 1) * bmax] = R[a][1];
    o[(int64_t)(4 * a + 2) * bmax] = R[a][2];
    o[(int64_t)(4 * a + 3) * bmax] = t;
  }
  if (A16) pf_emit_row(pr, p, h, bmax, R, tv, pf_stat, pf_sums, thr2, tcap, A16, c_h);
}

// ------------------------------------------------------------------------------------------------
// Exact inlier counts, f64 (Open3D evaluates Matrix4d * Vector4d and squaredNorm in double).
// grid: x = (hypothesis tile of 256) * splits + split, y = problem; block = 256 lanes = 256 hypotheses.
// A lane keeps its hypothesis in 12 f64 registers and walks the pair range of its split; pairs are
// staged 256 at a time: each thread loads one pair (6 coalesced f32 loads from the SoA copy), converts
// it to f64 once and stores it as one 48-B LDS row, which all lanes then read as broadcasts.
// Canonical chain (oracle/corsair_oracle.c oc_ransac):
//   p_c = fma(r_c2, sz, fma(r_c1, sy, fma(r_c0, sx, t_c))),  d_c = p_c - q_c,
//   |d|^2 = fma(dz, dz, fma(dy, dy, dx dx)),  inlier iff |d|^2 < max_corr^2 (all f64).
// ------------------------------------------------------------------------------------------------
constexpr int RC_CHUNK = 256;   // pairs per LDS stage = threads per workgroup
constexpr int RC_HYP = 256;     // hypotheses per workgroup

__device__ __forceinline__ double residual2_f64(const double (&R)[12], double sx, double sy, double sz,
                                                double qx, double qy, double qz) {
  const double dx = fma(R[2], sz, fma(R[1], sy, fma(R[0], sx, R[3]))) - qx;
  const double dy = fma(R[6], sz, fma(R[5], sy, fma(R[4], sx, R[7]))) - qy;
  const double dz = fma(R[10], sz, fma(R[9], sy, fma(R[8], sx, R[11]))) - qz;
  return fma(dz, dz, fma(dy, dy, dx * dx));
}

// LIST: the hypotheses are the survivors of the prefilter, hlist[p][0 .. n_surv[p]) (any order).
// HPW = hypotheses per workgroup: 256 (one per lane) or 64 (round 5: the FIRST chunk of a call, 64 iterations counted
// exactly before there is a best count to prune against -- lane = hypothesis + 64 x quarter, every quarter (= wave) takes
// every fourth staged pair and the four partial counts meet in the integer atomics the pair-range splits use anyway).
template <bool LIST, int HPW>
__device__ __forceinline__ void ransac_count_tile(double (*lds)[RC_CHUNK][6], const int p, const int tile,
                                                  const int split,
                                                  const RansacProb* __restrict__ probs,
                                                  const float* __restrict__ pk, int64_t total,
                                                  const double* __restrict__ hyp, int it0,
                                                  int bcount, int bmax, int splits, double thr2,
                                                  int32_t* __restrict__ res_cnt,
                                                  const int32_t* __restrict__ hlist,
                                                  const int32_t* __restrict__ n_surv) {
  const RansacProb pr = probs[p];
  if (pr.done) return;
  static_assert(HPW == RC_HYP || (!LIST && HPW == 64), "hypotheses per workgroup");
  constexpr int NPART = RC_HYP / HPW;                     // lanes that share a hypothesis (pair-interleaved)
  const int nlist = LIST ? n_surv[p] : 0;
  if (LIST) {
    if (tile * HPW >= nlist) return;
  } else {
    if (it0 + tile * HPW >= pr.est_k || tile * HPW >= bcount) return;  // whole block beyond the bound
  }
  const int tid = threadIdx.x;
  const int part = tid / HPW;
  const int h = tile * HPW + (tid - part * HPW);          // hypothesis slot of this lane
  const bool mine = LIST ? h < nlist : (h < bcount && it0 + h < pr.est_k);
  const int hsel = LIST ? hlist[(int64_t)p * bmax + min(h, nlist - 1)] : min(h, bmax - 1);
  double R[12];
  {
    const double* hp = hyp + ((int64_t)p * 12) * bmax + hsel;
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = hp[(int64_t)e * bmax];
  }
  const int per = ((pr.m + splits - 1) / splits + RC_CHUNK - 1) / RC_CHUNK * RC_CHUNK;
  const int beg = split * per;
  const int end = min(pr.m, beg + per);
  int cnt = 0;
  // staging registers: the next stage's pair of this thread is in flight while the current stage is
  // evaluated; rows past the range become far-away targets (never inliers)
  float stg[6];
  auto stage_load = [&](int base) {
    const int i = base + tid;
    const int64_t g = pr.off + (i < end ? i : 0);
#pragma unroll
    for (int c = 0; c < 6; ++c) stg[c] = pk[(int64_t)c * total + g];
  };
  auto stage_store = [&](int b, int base) {
    const bool ok = base + tid < end;
#pragma unroll
    for (int c = 0; c < 6; ++c) lds[b][tid][c] = ok ? (double)stg[c] : (c >= 3 ? 1.0e30 : 0.0);
  };
  if (beg < end) {
    stage_load(beg);
    stage_store(0, beg);
  }
  int buf = 0;
  for (int base = beg; base < end; base += RC_CHUNK) {
    __syncthreads();
    const bool more = base + RC_CHUNK < end;
    if (more) stage_load(base + RC_CHUNK);
    const int nrow = min(RC_CHUNK, end - base);
    if (nrow == RC_CHUNK) {
#pragma unroll 4
      for (int j = part; j < RC_CHUNK; j += NPART) {
        const double* q = lds[buf][j];
        cnt += residual2_f64(R, q[0], q[1], q[2], q[3], q[4], q[5]) < thr2 ? 1 : 0;
      }
    } else {
      for (int j = part; j < nrow; j += NPART) {
        const double* q = lds[buf][j];
        cnt += residual2_f64(R, q[0], q[1], q[2], q[3], q[4], q[5]) < thr2 ? 1 : 0;
      }
    }
    if (more) stage_store(buf ^ 1, base + RC_CHUNK);
    buf ^= 1;
  }
  if (mine) {
    if (splits == 1 && NPART == 1)
      res_cnt[(int64_t)p * bmax + hsel] = cnt;
    else
      atomicAdd(&res_cnt[(int64_t)p * bmax + hsel], cnt);   // (res_cnt of the chunk is zero on entry)
  }
}

// grid: x = (hypothesis tile of 256) * splits + split, y = problem.  LIST: the survivor count is only
// known on the device, so a fixed number of tile slots (gridDim.x / splits) strides over the list.
template <bool LIST, int HPW = RC_HYP>
__global__ __launch_bounds__(256) void k_ransac_count(const RansacProb* __restrict__ probs,
                                                      const float* __restrict__ pk, int64_t total,
                                                      const double* __restrict__ hyp, int it0,
                                                      int bcount, int bmax, int splits, double thr2,
                                                      int32_t* __restrict__ res_cnt,
                                                      const int32_t* __restrict__ hlist,
                                                      const int32_t* __restrict__ n_surv) {
  // [buf][j][c]: c = 0..2 source xyz, c = 3..5 target xyz of pair j, f64 (one 48-B row per pair)
  __shared__ __attribute__((aligned(16))) double lds[2][RC_CHUNK][6];
  const int p = blockIdx.y;
  const int tile0 = blockIdx.x / splits;
  const int split = blockIdx.x - tile0 * splits;
  if (LIST) {
    const int nlist = n_surv[p];
    const int tstride = gridDim.x / splits;
    for (int tile = tile0; tile * RC_HYP < nlist; tile += tstride) {
      ransac_count_tile<LIST, HPW>(lds, p, tile, split, probs, pk, total, hyp, it0, bcount, bmax, splits, thr2,
                                   res_cnt, hlist, n_surv);
      __syncthreads();  // the next tile restages LDS
    }
  } else {
    ransac_count_tile<LIST, HPW>(lds, p, tile0, split, probs, pk, total, hyp, it0, bcount, bmax, splits, thr2,
                                 res_cnt, hlist, n_surv);
  }
}

// ------------------------------------------------------------------------------------------------
// Exactness-preserving f16 prefilter.
// Once a problem has a best inlier count, a hypothesis matters only if its own count can reach it
// (otherwise it changes neither the best, nor the early-exit bound, nor the tie set).  The squared
// residual is bilinear in hypothesis and pair quantities,
//   |R s + t - q|^2 = |t|^2 + a . b,   a = [1, 2 R^T t, -2 R, -2 t],  b = [|s|^2 + |q|^2, s, q (x) s, q]   (16 terms)
// The pair side is split into f16 hi + lo, the hypothesis side is rounded to f16 (a_hi): a_hi . b_hi +
// a_hi . b_lo (K = 32) is two v_mfma_f32_32x32x16_f16 per 32 x 32 tile (16x the f32 matrix rate) whose
// accumulator INPUT holds |t|^2 - (thr^2 + eps_h): the sign of the result says whether the pair is
// within the INFLATED threshold.  eps_h bounds |d~^2 - d^2| (pf_emit_row) -- including the dropped
// (a - a_hi) . b, bounded per hypothesis with the per-problem maxima of |b_k| -- so the sign count is an
// UPPER bound of the exact inlier count.  Hypotheses whose bound is below the carried best get count
// 0, the few survivors go through the exact f64 kernels: results are unchanged bit for bit.
// (The K = 48 form with a_lo . b_hi has a ~2.5x tighter eps_h but 3 MFMAs per tile: measured slower
// end to end, DESIGN.md "What was tried".)
// ------------------------------------------------------------------------------------------------
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
constexpr int PF_K = 16;        // halfs per hypothesis row (32 B): a_hi, used by both MFMAs
constexpr int PF_PITCH = 40;    // halfs per pair row, K = 32 form (80 B = 5 slots of 16 B: conflict-free ds_read_b128)
constexpr int PF_PITCH1 = 24;   // halfs per pair row, K = 16 form (48 B = 3 slots: rows 0..15 start in 16 different slots of 4 banks)
__host__ __device__ constexpr int pf_pitch(int nm) { return nm == 2 ? PF_PITCH : PF_PITCH1; }
constexpr int PF_ROWS = 192;    // pairs per LDS stage (6 MFMA row tiles)
constexpr int PF_NG = 2;        // 32-hypothesis groups per wave (LDS fragments are reused NG times)
constexpr int PF_HYP = 4 * 32 * PF_NG;  // hypotheses per workgroup
constexpr int PF_STAT = 17;     // per-problem statistics of the pair image: smax, max |b_k| (k = 0..15)
constexpr float PF_SMAX = 128.0f;       // point norm above which a problem bypasses the prefilter
                                        // (f16 range: |s|^2 + |q|^2 and q (x) s must stay below 65504)

// f64 -> f16 through f32 (v_cvt_f32_f64 + v_cvt_f16_f32).  gfx950 has no direct conversion: `(_Float16)double` is a
// ~25-instruction integer sequence, and the prefilter's operand kernels make 16 - 32 of them per hypothesis and per pair (a sixth
// of k_ransac_hyp's instructions).  The two roundings can differ from the single one by one f16 ulp in rare ties; nothing
// below assumes a correctly rounded value -- every bound is computed from the value this function RETURNS (|x - f16_of(x)|),
// and its relative error 2^-11 + 2^-24 sits inside the constants' slack (2.002 for 2 sqrt(1.001), 1.0005).
__device__ __forceinline__ _Float16 f16_of(double v) { return (_Float16)(float)v; }

__device__ __forceinline__ void split16(double v, _Float16* hi, _Float16* lo) {
  const _Float16 h = f16_of(v);
  *hi = h;
  *lo = f16_of(v - (double)h);
}

// rows of problem p in the f16 pair image: m rounded up to whole LDS stages
__host__ __device__ static inline int64_t pf_padded(int64_t m) { return (m + PF_ROWS - 1) / PF_ROWS * PF_ROWS; }

// pair side: 80-B rows [bh(0..15) | bl(0..15) | 8 x 0] in exactly the layout the prefilter keeps in LDS
// (a stage is one contiguous 15-KiB copy); every problem is padded to whole stages with rows whose d~^2
// is +60000 (never counted).  stat[p] = {largest point norm, max |b_k| (k = 0..15)} of problem p as
// float bit patterns (non-negative floats order like their bits), rounded up.
// grid: x = blocks over the rows of a problem (grid-stride), y = problem; off16[p] = first row.
// Per-problem sums of the source and target points (mu = sum / m is evaluated with the same expression by every consumer).  The prefilter works in coordinates CENTRED per problem, s' = s - mu_s, q' = q - mu_q: the residual is the same,
// R s' + t' - q' = R s + t - q with t' = t + R mu_s - mu_q (pf_emit_row), but every magnitude the error bounds scale with
// -- smax, W, |t'| = |c'_t - R c'_s| with c' the centroids of the ten sampled points in centred coordinates -- shrinks to the
// spread of the problem's points.  The part-to-part problems of split_corr (utils/symmetry.py:145-179: a leg against a leg)
// sit far from the origin; without the centring 30 % of their hypotheses exceeded the |t| cap of the K = 16 form.
__global__ __launch_bounds__(256) void k_ransac_pair_sums(const RansacProb* __restrict__ probs, const float* __restrict__ src,
                                                          const float* __restrict__ tgt, double* __restrict__ sums,
                                                          unsigned* __restrict__ stat, unsigned long long* __restrict__ chk_stats) {
  // ONE workgroup per problem and a fixed reduction order: the means -- and with them the prefilter's survivor sets -- are
  // the same in every run (an atomic accumulation made the survivor counts of otherwise identical runs differ by 1e-4)
  __shared__ double red[4][6];
  const RansacProb pr = probs[blockIdx.x];
  // the maxima that k_ransac_images accumulates with atomics, and the CS_RANSAC_CHECK totals, start at zero (this kernel
  // precedes both on the stream: no fill launches)
  if (threadIdx.x < PF_STAT) stat[blockIdx.x * PF_STAT + threadIdx.x] = 0u;
  if (blockIdx.x == 0 && threadIdx.x < 4) chk_stats[threadIdx.x] = 0ull;
  double a[6] = {0, 0, 0, 0, 0, 0};
  // a lane adds its rows j = lane, lane + 256, ... in that order; the loads of SUMS_U rows are issued together (the loop is
  // bound by the latency of its strided loads: one workgroup walks a whole problem)
  constexpr int SUMS_U = 8;
  for (int j0 = threadIdx.x; j0 < pr.m; j0 += 256 * SUMS_U) {
    float v[SUMS_U][6];
#pragma unroll
    for (int u = 0; u < SUMS_U; ++u) {
      const int j = j0 + 256 * u;
      const int64_t i = pr.off + (j < pr.m ? j : j0);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[u][c] = src[3 * i + c];
        v[u][3 + c] = tgt[3 * i + c];
      }
    }
#pragma unroll
    for (int u = 0; u < SUMS_U; ++u) {
      if (j0 + 256 * u < pr.m) {
#pragma unroll
        for (int c = 0; c < 6; ++c) a[c] += (double)v[u][c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a[c] += __shfl_xor(a[c], off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = a[c];
  }
  __syncthreads();
  // what is stored is the MEAN (the six f64 divisions were made by every hypothesis and every pair row that read the sums)
  if (threadIdx.x < 6) {
    const double sum = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    const double v = sum / (double)(pr.m > 0 ? pr.m : 1);
    sums[blockIdx.x * 6 + threadIdx.x] = (v == v && fabs(v) < 1.0e30) ? v : 0.0;   // non-finite input: no centring (the rows are rejected by their norm)
  }
}
__device__ __forceinline__ void pf_centre(const double* __restrict__ sums, int p, int m, double (&mu)[6]) {
  (void)m;
#pragma unroll
  for (int c = 0; c < 6; ++c) mu[c] = sums[p * 6 + c];
}

// The centred bilinear row of one pair, b = (|s|^2 + |q|^2, s, q (x) s, q), and the pair's magnitude test -- ONE definition for
// k_ransac_images and k_ransac_pack16_b0, whose rows must agree.  Returns max(|s|, |q|) rounded up to f32 (1.0000002: the f32
// norm may round down); NaN when a coordinate is not finite.  A pair is in f16 range iff the value is <= PF_SMAX.
__device__ __forceinline__ float pf_pair_row(float s0, float s1, float s2, float q0, float q1, float q2, const double (&mu)[6],
                                             double (&b)[16]) {
  const double sx = s0 - mu[0], sy = s1 - mu[1], sz = s2 - mu[2];
  const double qx = q0 - mu[3], qy = q1 - mu[4], qz = q2 - mu[5];
  const double ss = sx * sx + sy * sy + sz * sz, qq = qx * qx + qy * qy + qz * qz;
  b[0] = ss + qq;
  b[1] = sx; b[2] = sy; b[3] = sz;
  b[4] = qx * sx; b[5] = qx * sy; b[6] = qx * sz;
  b[7] = qy * sx; b[8] = qy * sy; b[9] = qy * sz;
  b[10] = qz * sx; b[11] = qz * sy; b[12] = qz * sz;
  b[13] = qx; b[14] = qy; b[15] = qz;
  return 1.0000002f * (float)sqrt(fmax(ss, qq));
}

// First pass over the pairs of a call: the packed copies (k_ransac_pack's pk and pair32), the per-problem statistics and the
// rows [bh | bl | pad] of the K = 32 form (B32, PF_PITCH halfs: the prefilter's image with CS_RANSAC_PF_K=32, the second
// stage's otherwise; null with CS_RANSAC_STAGE2=0) from one read of src / tgt and one evaluation of the centred bilinear
// row b and its hi / lo split.  The rows of the K = 16 form need the problem's smax: k_ransac_pack16_b0 below.
static_assert(PF_PITCH == 40 && PF_PITCH1 == 24, "k_ransac_images / k_ransac_pack16_b0 write 5 / 3 pieces of 16 B per row");
__global__ __launch_bounds__(256) void k_ransac_images(const RansacProb* __restrict__ probs,
                                                       const int64_t* __restrict__ off16,
                                                       const float* __restrict__ src,
                                                       const float* __restrict__ tgt,
                                                       const double* __restrict__ sums, int64_t n,
                                                       float* __restrict__ pk, float4* __restrict__ pair32,
                                                       _Float16* __restrict__ B32, unsigned* __restrict__ stat) {
  __shared__ float red[4][PF_STAT];
  const RansacProb pr = probs[blockIdx.y];
  double mu[6];
  pf_centre(sums, blockIdx.y, pr.m, mu);
  const int mpad = (int)pf_padded(pr.m);
  float mx[PF_STAT];
#pragma unroll
  for (int k = 0; k < PF_STAT; ++k) mx[k] = 0.f;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < mpad; j += gridDim.x * blockDim.x) {
    union {
      _Float16 h[PF_PITCH];
      uint4 v[5];
    } row;
#pragma unroll
    for (int k = 0; k < 5; ++k) row.v[k] = make_uint4(0u, 0u, 0u, 0u);
    if (j < pr.m) {
      const int64_t i = pr.off + j;
      const float fs[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
      const float fq[3] = {tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2]};
      pair32[2 * i + 0] = make_float4(fs[0], fs[1], fs[2], fq[0]);
      pair32[2 * i + 1] = make_float4(fq[1], fq[2], 0.f, 0.f);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pk[c * n + i] = fs[c];
        pk[(3 + c) * n + i] = fq[c];
      }
      double b[16];
      float mag = pf_pair_row(fs[0], fs[1], fs[2], fq[0], fq[1], fq[2], mu, b);
      // out of f16 range (or NaN): a finite (zero) row; smax then marks the problem's hypotheses unusable
      const bool ok = mag <= PF_SMAX;
      if (!(mag == mag)) mag = INFINITY;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        _Float16 hi = (_Float16)0.0f, lo = (_Float16)0.0f;
        if (ok) {
          split16(b[k], &hi, &lo);
          mx[1 + k] = fmaxf(mx[1 + k], __double2float_ru(fabs(b[k])));
        }
        row.h[k] = hi;
        row.h[16 + k] = lo;
      }
      mx[0] = fmaxf(mx[0], mag);
    } else {
      row.h[0] = (_Float16)60000.0f;  // pairs with a_0 = 1
    }
    const int64_t r = off16[blockIdx.y] + j;
    if (B32) {
      uint4* dst = reinterpret_cast<uint4*>(B32 + r * PF_PITCH);
#pragma unroll
      for (int k = 0; k < PF_PITCH / 8; ++k) dst[k] = row.v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < PF_STAT; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = mx[k];
  }
  __syncthreads();
  if (threadIdx.x < PF_STAT) {
    const int k = threadIdx.x;
    const float m = fmaxf(fmaxf(red[0][k], red[1][k]), fmaxf(red[2][k], red[3][k]));
    if (m > 0.f) atomicMax(&stat[blockIdx.y * PF_STAT + k], __float_as_uint(m));
  }
}

// K = 16 form (round 4), second pass over the pairs (needs the problem's smax, which the first pass produces): rows
// [bh | pad] (PF_PITCH1 halfs) -- the matrix pipe then evaluates a_hi . b_hi only, and what it drops, a_hi . b_lo, is bounded
// PER PAIR and taken out of the pair's constant term b_0 (a_0 = 1 exactly), so the sign test stays an upper bound.  The
// kernel writes WHOLE rows (a 2-byte update of rows another kernel wrote was a read-modify-write in memory).  The constant
// term of every pair is   b_0' = round_down_f16( b_0 - E_p ),   E_p = (1 + 2^-10) sum_{k=1..15} A_k |b_k - hi(b_k)|,
// with A_k an upper bound of |a_hi_k| over all USABLE hypotheses of the problem:
//   k = 4..12  (a = -2 R):          |a| <= 2 sqrt(1 + max|E|) <= 2.002   (pf_emit_row requires max|E| < 1e-3)
//   k = 1..3, 13..15 (2 R^T t, -2 t): |a| <= 2 |t| sqrt(1 + max|E|) with |t| <= tcap * smax: pf_emit_row CHECKS that and
//     marks the other hypotheses unusable (they survive to the exact kernels).  |t| = |c_t - R c_s| can reach 2 smax, but
//     both centroids are means of ten points of a centred object: on the bench clouds |t| / smax has median 0.2 and
//     99.99 % of the hypotheses are below 0.8, so tcap = 0.75 (PF_TCAP) costs 1e-4 of them and shrinks E_p 2.7x
// The constant term is also CENTRED: b_0 - beta with beta = smax^2 (b_0 = |s|^2 + |q|^2 lies in [0, 2 smax^2]); the
// hypothesis side adds beta to its accumulator input.  f16 is finer near zero: the round-down costs ~6e-5 instead of 2.4e-4.
// and |a_hi| <= |a| (1 + 2^-11).  Then  sum_k a_hi_k b'_k  <=  sum_k a_hi_k (b_hi_k + b_lo_k)  for every usable hypothesis:
// the one-MFMA value is never above what the K = 32 form computes exactly, i.e. every pair the K = 32 form counts is
// counted -- the count stays an UPPER bound (pf_emit_row's eps_h covers the rest as before).  The price is a looser
// bound: E_p is ~1e-3 for unit-sized objects (2.5 % of thr^2 = 0.04), the rounding of b_0 another ~2.4e-4 on average.
__global__ __launch_bounds__(256) void k_ransac_pack16_b0(const RansacProb* __restrict__ probs,
                                                          const int64_t* __restrict__ off16,
                                                          const float4* __restrict__ pair32,
                                                          const double* __restrict__ sums,
                                                          const unsigned* __restrict__ stat, double tcap,
                                                          _Float16* __restrict__ B16) {
  const RansacProb pr = probs[blockIdx.y];
  double mu[6];
  pf_centre(sums, blockIdx.y, pr.m, mu);
  const double smax = (double)__uint_as_float(stat[blockIdx.y * PF_STAT]);
  // smax out of range (a point norm above PF_SMAX, or not finite): the problem bypasses the prefilter, every hypothesis is
  // unusable; its rows keep the plain b_0 and are zero where the pair itself is out of range.  Otherwise every pair is in range.
  const bool bypass = !(smax <= (double)PF_SMAX);
  const double beta = smax * smax;
  const double a_rot = 2.002 * (1.0 + 0x1p-11), a_t = 2.0 * tcap * smax * 1.0005 * (1.0 + 0x1p-11);
  const int mpad = (int)pf_padded(pr.m);
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < mpad; j += gridDim.x * blockDim.x) {
    union {
      _Float16 h[PF_PITCH1];
      uint4 v[3];
    } row;
#pragma unroll
    for (int k = 0; k < 3; ++k) row.v[k] = make_uint4(0u, 0u, 0u, 0u);
    if (j < pr.m) {
      const int64_t i = pr.off + j;
      const float4 pa = pair32[2 * i], pb = pair32[2 * i + 1];   // the pair as k_ransac_images packed it: (sx, sy, sz, qx | qy, qz)
      double b[16];
      const float mag = pf_pair_row(pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, mu, b);
      if (bypass) {
        if (mag <= PF_SMAX) {   // (false for NaN)
#pragma unroll
          for (int k = 0; k < 16; ++k) row.h[k] = f16_of(b[k]);
        }
      } else {
        double e_t = 0.0, e_rot = 0.0;
#pragma unroll
        for (int k = 1; k < 16; ++k) {
          const _Float16 hi = f16_of(b[k]);
          row.h[k] = hi;
          const double lo = fabs(b[k] - (double)hi);
          if (k >= 4 && k <= 12) e_rot += lo; else e_t += lo;
        }
        const double ep = (1.0 + 0x1p-10) * (a_rot * e_rot + a_t * e_t);
        // round toward -inf into f16: RNE first, one ulp down when that landed above
        const double v = (b[0] - beta) - ep - 0x1p-40 * (fabs(b[0]) + beta + ep);   // (the f64 roundings of the terms themselves)
        _Float16 h = f16_of(v);
        if ((double)h > v) {
          unsigned short u = __builtin_bit_cast(unsigned short, h);
          // next representable value below: magnitude down for positive values, up for negative ones (+0 -> -min subnormal)
          u = (u & 0x8000u) ? (unsigned short)(u + 1) : (u == 0 ? (unsigned short)0x8001u : (unsigned short)(u - 1));
          h = __builtin_bit_cast(_Float16, u);
        }
        row.h[0] = h;
      }
    } else {
      row.h[0] = (_Float16)60000.0f;  // pairs with a_0 = 1
    }
    uint4* dst = reinterpret_cast<uint4*>(B16 + (off16[blockIdx.y] + j) * PF_PITCH1);
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = row.v[k];
  }
}

// hypothesis side: row = a_hi(0..15) (f16 roundings of a) and the accumulator input
//   c_h = |t|^2 - (thr^2 + eps_h).
// eps_h >= |d~^2 - d^2| where d^2 is what the exact (f64) kernels compute and d~^2 the f16 pipeline
// c_h + sum_k a_hi_k (b_hi_k + b_lo_k):
//   * 32 products, exact in f32; their accumulation rounds (or truncates) at most 33 times relative
//     to sum_k |a_k b_k| <= sqrt(3) (|s| + |q| + |t|)^2 =: sqrt(3) W            <= 33 * 2^-23 * sqrt(3) W
//   * the residuals of the hi+lo splits of b                            <= 2^-22 * sqrt(3) W + 2^-25 (2 W + 59)
//   * (the exact kernels evaluated d^2 in f32 when this budget was set:   <= 2^-20 W; they are f64 now and
//      the term is kept as slack)
//   => < 8.3e-6 W + 1.8e-6; charged 2.5e-5 W + 6e-6 (3x margin).  The accumulation term assumes one ulp per
//   addition; measured, the two chained MFMAs are within 2.3 ulp in total (tools/ubench/mfma_err.hip,
//   4e8 results), so the charge is ~30x the observed error.  CS_RANSAC_CHECK runs validate the bound.
//   * the dropped (a - a_hi) . b                      <= sum_k |a_k - a_hi_k| max_pairs |b_k|   (stat[p])
//   * |R s|^2 = |s|^2 only up to the orthonormality defect E = R^T R - I:    <= 3 max|E| smax^2
// with W <= (2 smax + |t|)^2.  A hypothesis outside the f16 range (or not finite) gets c_h = -inf and
// a zero row: every pair counts, it always survives to the exact kernel.
// Prefilter row of one hypothesis (R, t): 16 f16 coefficients + the f32 constant c_h (see k_ransac_prefilter).  Called by
// k_ransac_hyp while R and t are still in registers.
__device__ __forceinline__ void pf_emit_row(const RansacProb& pr, int p, int h, int bmax, const double (&R)[3][3], double (&t)[3],
                                            const unsigned* __restrict__ stat, const double* __restrict__ sums, double thr2,
                                            double tcap, _Float16* __restrict__ A16, float* __restrict__ c_h) {
  // the pair image is in centred coordinates: t' = t + R mu_s - mu_q (see k_ransac_pair_sums); the f64 rounding of these
  // nine operations (<= 1e-15 (|t| + |mu|)) sits far inside the 6e-6 of eps
  {
    double mu[6];
    pf_centre(sums, p, pr.m, mu);
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = t[a] + (R[a][0] * mu[0] + R[a][1] * mu[1] + R[a][2] * mu[2]) - mu[3 + a];
  }
  const double smax = (double)__uint_as_float(stat[p * PF_STAT]);
  const double tt = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
  const double tn = sqrt(tt);
  double a[16];
  a[0] = 1.0;
#pragma unroll
  for (int b = 0; b < 3; ++b) a[1 + b] = 2.0 * (R[0][b] * t[0] + R[1][b] * t[1] + R[2][b] * t[2]);
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int b = 0; b < 3; ++b) a[4 + 3 * x + b] = -2.0 * R[x][b];
#pragma unroll
  for (int x = 0; x < 3; ++x) a[13 + x] = -2.0 * t[x];
  double dev = 0.0;
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int y = 0; y < 3; ++y) {
      const double e = R[0][x] * R[0][y] + R[1][x] * R[1][y] + R[2][x] * R[2][y] - (x == y ? 1.0 : 0.0);
      dev = fmax(dev, fabs(e));
    }
  bool usable = smax <= (double)PF_SMAX && tn <= 4.0 * (double)PF_SMAX && dev < 1.0e-3;
  // K = 16 form: the per-pair bound of the dropped a_hi . b_lo (k_ransac_pack16_b0) assumes |t| <= 2.002 smax
  // (tcap > 0) and its constant term is centred by beta = smax^2, which comes back through c_h
  if (tcap > 0.0) usable = usable && tn <= tcap * smax;
  usable = usable && thr2 < 3.0e4;   // the padding rows (b_0 = 60000) must stay positive: c_h > -60000
  const double beta = tcap > 0.0 ? smax * smax : 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) usable = usable && fabs(a[k]) < 6.0e4;  // false for NaN
  union {
    _Float16 h[PF_K];
    uint4 v[2];
  } row;
  double drop = 0.0;  // sum_k |a_k - a_hi_k| max |b_k|
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const _Float16 hi = usable ? f16_of(a[k]) : (_Float16)0.0f;
    row.h[k] = hi;
    if (usable) drop += fabs(a[k] - (double)hi) * (double)__uint_as_float(stat[p * PF_STAT + 1 + k]);
  }
  uint4* dst = reinterpret_cast<uint4*>(A16 + ((int64_t)p * bmax + h) * PF_K);
  dst[0] = row.v[0];
  dst[1] = row.v[1];
  const double w = 2.0 * smax + tn;
  const double eps = 2.5e-5 * w * w + 6.0e-6 + 3.0 * dev * smax * smax + 1.000001 * drop;
  // rounded towards -inf so that the f32 value never tightens the test
  // unusable: a zero row and c_h = -1, so every row (padding included) counts and the hypothesis survives.  (FINITE: the
  // round-toward-minus-infinity counters of k_ransac_prefilter<1, true> add the results themselves.)
  c_h[(int64_t)p * bmax + h] = usable ? __double2float_rd((tt + beta) - (thr2 + eps)) : -1.0f;
}

// Upper bounds of the inlier counts.
// grid: 1-D, 8 * slots * tiles * splits workgroups.  Workgroups are dealt round-robin to the 8 XCDs, so
// XCD x = id % 8 is given the problems xcd_prob[x][0..slots) (host: longest-first balancing): all
// workgroups that stream one problem's pair image run on ONE XCD at about the same time and share it
// through that XCD's 4-MiB L2 instead of each pulling it from HBM / Infinity Cache.
// MFMA operand maps (v_mfma_f32_32x32x16_f16): lane l supplies A[row l&31][k = 8(l>>5) .. +8) and
// B[k = 8(l>>5) .. +8)][col l&31]; D as for the f32 shape.  rows = pairs (LDS, shared by the four
// waves), cols = hypotheses (registers, PF_NG groups of 32 per wave).
//
// Staging: a stage is PF_ROWS rows = 15 KiB, contiguous in the pair image, copied global -> LDS by
// 15 LDS-DMA instructions of 1 KiB (global_load_lds_dwordx4: no staging registers, no ds_write); the
// copy of stage s+1 is in flight while stage s is computed.
//
// Inner loop: units k = (row tile t, hypothesis group g), 12 per stage.  K = 32 (<2, false>): the two MFMAs of unit k are
// issued interleaved with the sign extraction (16 x v_alignbit into a per-lane history word, one VALU
// op per pair) of unit k-2, held in another of three rotating accumulator sets: a result is first
// read a whole unit (>= 64 cycles) after the MFMA that wrote it, beyond the 11 wait states the
// hardware requires.  The VALU side is the longer one (v_alignbit_b32 issues every ~4.5 cycles per
// SIMD, tools/ubench/valu_rate.hip: 16 x 4.5 = 72 cycles against 64 for the MFMAs).  The unit is one asm block: the compiler's scheduler does not keep this order
// (it hoists the dependent VALU ops and pays s_nop 10 per unit).
// K = 16 (<1, true>, RTN): the signs are counted by the results THEMSELVES -- under round-toward-minus-infinity (MODE.fp_round)
// and with a counter in [2^63, 2^64), whose ulp is 2^40, `v_add_f32 cnt, acc, cnt` subtracts exactly 2^40 iff acc < 0 for
// any |acc| < 2^40 (tools/ubench/rtn_count.hip: edge cases incl. -0 and denormals) -- one FULL-RATE VALU op per result
// instead of a 4.5-cycle v_alignbit.  Full-rate ops do not overlap with the matrix pipe, but the K = 16 unit has only one
// MFMA: 32 + 16 x 2.3 = 69 cycles against 72+ (tools/ubench/pf_k16_mix.hip: 29.2 vs 32.8 ns per unit per SIMD).
template <int NM, bool RTN>   // NM = MFMAs per unit: 2 = K 32 (a_hi . (b_hi + b_lo)), 1 = K 16 (a_hi . b_hi', k_ransac_images + k_ransac_pack16_b0)
__global__ __launch_bounds__(256) void k_ransac_prefilter(const RansacProb* probs,
                                                          const int64_t* __restrict__ off16,
                                                          const _Float16* __restrict__ B16,
                                                          const _Float16* __restrict__ A16,
                                                          const float* __restrict__ c_h, int it0,
                                                          int bcount, int bmax, int splits,
                                                          const int32_t* __restrict__ xcd_prob,
                                                          const XcdTab xcd_tab, int slots, int tiles,
                                                          int32_t* __restrict__ cnt_up,
                                                          unsigned long long* __restrict__ trace,
                                                          const int32_t* __restrict__ n_list) {
  const unsigned long long t_start = trace ? wall_clock64() : 0ULL;
  const unsigned long long c_start = trace ? __builtin_amdgcn_s_memtime() : 0ULL;
  constexpr int PITCH = pf_pitch(NM);
  constexpr int STAGE_BYTES = PF_ROWS * PITCH * 2;  // 15360 (K 32) / 9216 (K 16)
  constexpr int STAGE_KIB = STAGE_BYTES / 1024;        // 15 LDS-DMA instructions
  static_assert(STAGE_BYTES % 1024 == 0, "a stage must be whole 1-KiB LDS-DMA instructions");
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE_BYTES];
  const int xcd = blockIdx.x & 7;
  const int item = blockIdx.x >> 3;
  const int slot = item / (tiles * splits);
  const int inner = item - slot * (tiles * splits);
  const int p = xcd_problem(xcd_prob, xcd_tab, xcd * slots + slot);
  if (p < 0) return;
  const int tile = inner / splits;
  const int split = inner - tile * splits;
  const RansacProb pr = prob_view(probs, p);
  if (pr.done) return;
  // n_list: the hypotheses are a COMPACT per-problem list of n_list[p] rows (second stage over the survivors: rows
  // compacted by k_ransac_survivors, bmax = its row capacity) instead of the iterations it0 .. it0 + bcount of a chunk
  if (n_list) bcount = min(n_list[p], bmax);
  const int ek_rel = n_list ? 0x7fffffff : pr.est_k - it0;   // hypotheses at or beyond it are past the iteration bound
  if (tile * PF_HYP >= ek_rel || tile * PF_HYP >= bcount) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int col = lane & 31;
  const int h0 = tile * PF_HYP + wave * 32 * PF_NG;
  const bool wave_live = h0 < bcount && h0 < ek_rel;
  f16x8 bop[PF_NG];
  f32x16 cin[PF_NG];
#pragma unroll
  for (int g = 0; g < PF_NG; ++g) {
    // hypotheses past the chunk / bound read a valid row; their result is not stored
    int hh = h0 + 32 * g + col;
    if (hh >= bcount || hh >= ek_rel) hh = wave_live ? h0 : 0;
    const _Float16* row = A16 + ((int64_t)p * bmax + hh) * PF_K + 8 * half;
    bop[g] = *reinterpret_cast<const f16x8*>(row);
    const float c = c_h[(int64_t)p * bmax + hh];
#pragma unroll
    for (int r = 0; r < 16; ++r) cin[g][r] = c;
    asm volatile("" : "+v"(cin[g]));  // keep the 16 copies resident instead of re-splatting per tile
  }
  const int mpad = (int)pf_padded(pr.m);
  const int per = ((mpad / PF_ROWS + splits - 1) / splits) * PF_ROWS;
  const int beg = split * per;
  const int end = min(mpad, beg + per);
  static_assert(RTN == (NM == 1), "two forms: <1, true> = K 16 with the add-based sign count, <2, false> = K 32 with the sign history");
  unsigned bits[PF_NG];
  int cnt[PF_NG];
  constexpr float RTN_C0 = 0x1p64f - 0x1p40f;   // 2^64 - 2^40: all 24 significand bits set, ulp 2^40
  float fc[PF_NG][2];
#pragma unroll
  for (int g = 0; g < PF_NG; ++g) {
    bits[g] = 0u;
    cnt[g] = 0;
    fc[g][0] = RTN_C0;
    fc[g][1] = RTN_C0;
  }
  const char* gsrc = reinterpret_cast<const char*>(B16 + off16[p] * PITCH) + lane * 16;
  auto issue_stage = [&](int b, int base) {
    const char* g = gsrc + (int64_t)base * (PITCH * 2);
#pragma unroll
    for (int i = 0; i < (STAGE_KIB + 3) / 4; ++i) {
      const int piece = wave + 4 * i;  // wave-uniform
      if (piece < STAGE_KIB)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(g + piece * 1024),
            (__attribute__((address_space(3))) void*)(lds + b * STAGE_BYTES + piece * 1024), 16, 0, 0);
    }
  };
  static_assert(PF_NG == 2 && PF_ROWS == 192, "the unrolled schedule below is written for 12 units per stage");
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 S0, S1 = zero16, S2 = zero16;  // +0: the first two (dummy) extractions shift in zeros
#define PF_UNIT2(DST, SRC, G, A, COUNT) \
  asm volatile( \
      "v_mfma_f32_32x32x16_f16 %0, %2, %4, %6\n\t" \
      "v_alignbit_b32 %1, %1, %7, 31\n\t" \
      "v_alignbit_b32 %1, %1, %8, 31\n\t" \
      "v_alignbit_b32 %1, %1, %9, 31\n\t" \
      "v_alignbit_b32 %1, %1, %10, 31\n\t" \
      "v_alignbit_b32 %1, %1, %11, 31\n\t" \
      "v_alignbit_b32 %1, %1, %12, 31\n\t" \
      "v_alignbit_b32 %1, %1, %13, 31\n\t" \
      "v_alignbit_b32 %1, %1, %14, 31\n\t" \
      "v_mfma_f32_32x32x16_f16 %0, %3, %5, %0\n\t" \
      "v_alignbit_b32 %1, %1, %15, 31\n\t" \
      "v_alignbit_b32 %1, %1, %16, 31\n\t" \
      "v_alignbit_b32 %1, %1, %17, 31\n\t" \
      "v_alignbit_b32 %1, %1, %18, 31\n\t" \
      "v_alignbit_b32 %1, %1, %19, 31\n\t" \
      "v_alignbit_b32 %1, %1, %20, 31\n\t" \
      "v_alignbit_b32 %1, %1, %21, 31\n\t" \
      "v_alignbit_b32 %1, %1, %22, 31" \
      : "=&v"(DST), "+v"(bits[G]) \
      : "v"(A[0]), "v"(A[1]), "v"(bop[G]), "v"(bop[G]), \
        "v"(cin[G]), "v"(SRC[0]), "v"(SRC[1]), "v"(SRC[2]), "v"(SRC[3]), "v"(SRC[4]), "v"(SRC[5]), \
        "v"(SRC[6]), "v"(SRC[7]), "v"(SRC[8]), "v"(SRC[9]), "v"(SRC[10]), "v"(SRC[11]), \
        "v"(SRC[12]), "v"(SRC[13]), "v"(SRC[14]), "v"(SRC[15])); \
  if (COUNT) cnt[G] += __popc(bits[G]);
#define PF_UNITR(DST, SRC, G, GC, A) \
  asm volatile( \
      "v_mfma_f32_32x32x16_f16 %0, %3, %4, %5\n\t" \
      "v_add_f32 %1, %6, %1\n\t" \
      "v_add_f32 %2, %7, %2\n\t" \
      "v_add_f32 %1, %8, %1\n\t" \
      "v_add_f32 %2, %9, %2\n\t" \
      "v_add_f32 %1, %10, %1\n\t" \
      "v_add_f32 %2, %11, %2\n\t" \
      "v_add_f32 %1, %12, %1\n\t" \
      "v_add_f32 %2, %13, %2\n\t" \
      "v_add_f32 %1, %14, %1\n\t" \
      "v_add_f32 %2, %15, %2\n\t" \
      "v_add_f32 %1, %16, %1\n\t" \
      "v_add_f32 %2, %17, %2\n\t" \
      "v_add_f32 %1, %18, %1\n\t" \
      "v_add_f32 %2, %19, %2\n\t" \
      "v_add_f32 %1, %20, %1\n\t" \
      "v_add_f32 %2, %21, %2" \
      : "=&v"(DST), "+v"(fc[GC][0]), "+v"(fc[GC][1]) \
      : "v"(A[0]), "v"(bop[G]), \
        "v"(cin[G]), "v"(SRC[0]), "v"(SRC[1]), "v"(SRC[2]), "v"(SRC[3]), "v"(SRC[4]), "v"(SRC[5]), \
        "v"(SRC[6]), "v"(SRC[7]), "v"(SRC[8]), "v"(SRC[9]), "v"(SRC[10]), "v"(SRC[11]), \
        "v"(SRC[12]), "v"(SRC[13]), "v"(SRC[14]), "v"(SRC[15]));
#define PF_UNIT(DST, SRC, G, A, COUNT)            \
  if constexpr (NM == 2) {                        \
    PF_UNIT2(DST, SRC, G, A, COUNT)               \
  }
#define PF_LOAD(A, TILE)                                                                          \
  {                                                                                               \
    const _Float16* arow_ = reinterpret_cast<const _Float16*>(lds + buf * STAGE_BYTES) +          \
                            ((TILE) * 32 + col) * PITCH + 8 * half;                               \
    _Pragma("unroll") for (int m = 0; m < NM; ++m) A[m] =                                         \
        *reinterpret_cast<const f16x8*>(arow_ + 16 * m);                                          \
  }
  if (beg < end) issue_stage(0, beg);
  // f32 rounding toward -inf from here on (MODE[1:0]); nothing below depends on round-to-nearest: the MFMA results may
  // come out one ulp lower, which can only add to the count
  if constexpr (RTN) asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 2");
  const unsigned long long t_loop = trace ? wall_clock64() : 0ULL;
  unsigned long long t_wait_dma = 0, t_wait_bar = 0;
  int buf = 0;
  for (int base = beg; base < end; base += PF_ROWS) {
    // this wave's pieces of the stage have landed; after the barrier everybody's have, and everybody
    // has finished reading the other buffer, which the next copy overwrites
    const unsigned long long tw0 = trace ? wall_clock64() : 0ULL;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long tw1 = trace ? wall_clock64() : 0ULL;
    __builtin_amdgcn_s_barrier();
    if (trace) {
      const unsigned long long tw2 = wall_clock64();
      t_wait_dma += tw1 - tw0;
      t_wait_bar += tw2 - tw1;
    }
    if (base + PF_ROWS < end) issue_stage(buf ^ 1, base + PF_ROWS);
    if constexpr (RTN) {
      if (wave_live) {
        // TWO accumulator sets: S0 always holds group 0, S1 group 1; unit k = (tile k / 2, group k % 2) writes its group's
        // set and adds the OTHER set = the results of unit k - 1 into that group's counters.  Between the MFMA of unit
        // k - 1 and the first read of its results lie its own 16 adds and the MFMA of unit k: 17 instructions, beyond
        // the 11 wait states an 8-pass MFMA needs.  (A third set as in the v_alignbit schedule costs 16 VGPRs: 142, three
        // waves per SIMD.)
        f16x8 aX[2], aY[2];
        PF_LOAD(aX, 0)
        PF_LOAD(aY, 1)
        PF_UNITR(S0, S1, 0, 1, aX)
        PF_UNITR(S1, S0, 1, 0, aX)
        PF_LOAD(aX, 2)
        PF_UNITR(S0, S1, 0, 1, aY)
        PF_UNITR(S1, S0, 1, 0, aY)
        PF_LOAD(aY, 3)
        PF_UNITR(S0, S1, 0, 1, aX)
        PF_UNITR(S1, S0, 1, 0, aX)
        PF_LOAD(aX, 4)
        PF_UNITR(S0, S1, 0, 1, aY)
        PF_UNITR(S1, S0, 1, 0, aY)
        PF_LOAD(aY, 5)
        PF_UNITR(S0, S1, 0, 1, aX)
        PF_UNITR(S1, S0, 1, 0, aX)
        PF_UNITR(S0, S1, 0, 1, aY)
        PF_UNITR(S1, S0, 1, 0, aY)
      }
    } else if (wave_live) {
      // unit k writes set k % 3 and extracts set (k + 1) % 3 = unit k-2 = (tile t-1, same group);
      // 32 fresh sign bits are counted whenever tile t-1 is odd
      f16x8 aX[2], aY[2];
      PF_LOAD(aX, 0)
      PF_LOAD(aY, 1)
      PF_UNIT(S0, S1, 0, aX, true)
      PF_UNIT(S1, S2, 1, aX, true)
      PF_LOAD(aX, 2)
      PF_UNIT(S2, S0, 0, aY, false)
      PF_UNIT(S0, S1, 1, aY, false)
      PF_LOAD(aY, 3)
      PF_UNIT(S1, S2, 0, aX, true)
      PF_UNIT(S2, S0, 1, aX, true)
      PF_LOAD(aX, 4)
      PF_UNIT(S0, S1, 0, aY, false)
      PF_UNIT(S1, S2, 1, aY, false)
      PF_LOAD(aY, 5)
      PF_UNIT(S2, S0, 0, aX, true)
      PF_UNIT(S0, S1, 1, aX, true)
      PF_UNIT(S1, S2, 0, aY, false)
      PF_UNIT(S2, S0, 1, aY, false)
    }
    buf ^= 1;
  }
#undef PF_UNIT
#undef PF_UNITR
#undef PF_UNIT2
#undef PF_LOAD
  if (trace && lane == 0) {
    unsigned hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    unsigned long long* o = trace + ((size_t)blockIdx.x * 4 + wave) * 4;
    o[0] = t_start;
    o[1] = (t_wait_dma << 32) | t_wait_bar;
    o[2] = wall_clock64();
    // shader-clock cycles of this wave's lifetime in the top bits (with o[2] - o[0] at 100 MHz: the
    // in-kernel clock), placement in the low bits
    o[3] = ((__builtin_amdgcn_s_memtime() - c_start) << 24) | ((unsigned long long)(xcc & 0xf) << 20) |
           (hwid & 0xfffff);
    (void)t_loop;
  }
  if (!wave_live || beg >= end) return;
  // drain: the asm blocks hide their MFMAs from the compiler's hazard recognizer
  asm volatile("s_nop 15\n\ts_nop 15" : "+v"(S1), "+v"(S2));
  if constexpr (RTN) {
    // the last unit (group 1) is the only one not counted yet
#pragma unroll
    for (int r = 0; r < 16; ++r) asm volatile("v_add_f32 %0, %1, %0" : "+v"(fc[1][r & 1]) : "v"(S1[r]));
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0" ::: "memory");
#pragma unroll
    for (int g = 0; g < PF_NG; ++g)   // (C0 - fc) is count * 2^40 exactly: both operands are multiples of 2^40 below 2^64
      cnt[g] = (int)((RTN_C0 - fc[g][0]) * 0x1p-40f) + (int)((RTN_C0 - fc[g][1]) * 0x1p-40f);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) bits[0] = __builtin_amdgcn_alignbit(bits[0], __float_as_uint(S1[r]), 31);
    cnt[0] += __popc(bits[0]);
#pragma unroll
    for (int r = 0; r < 16; ++r) bits[1] = __builtin_amdgcn_alignbit(bits[1], __float_as_uint(S2[r]), 31);
    cnt[1] += __popc(bits[1]);
  }
#pragma unroll
  for (int g = 0; g < PF_NG; ++g) {
    const int c = cnt[g] + __shfl_xor(cnt[g], 32);
    const int h = h0 + 32 * g + col;
    if (half == 0 && h < bcount && h < ek_rel) {
      if (splits == 1)
        cnt_up[(int64_t)p * bmax + h] = c;
      else
        atomicAdd(&cnt_up[(int64_t)p * bmax + h], c);
    }
  }
}

constexpr int PF_S2_CAP = 1024;   // rows per problem of the second stage's compact list (= the largest list the few-survivor kernel takes)
// What the second stage needs of a survivor, written by k_ransac_survivors itself when the stage runs (s2.A16s != nullptr):
// A16s[p][slot] = A16[p][h], c_hs = c_h - beta (the K = 32 image is not centred by beta: (c - beta) in double is exact, and
// narrowing toward -inf never tightens the test; an unusable hypothesis -- c_h = -1, zero row -- stays negative: every row
// counts again), its counter cleared.
struct Stage2Rows {
  const _Float16* A16;
  const float* c_h;
  const unsigned* stat;
  double tcap;
  _Float16* A16s;
  float* c_hs;
  int32_t* cnt2;
};
// Survivors: hypotheses whose upper bound reaches the carried best count.  The others get count 0.
__global__ void k_ransac_survivors(const RansacProb* __restrict__ probs, const int32_t* __restrict__ cnt_up,
                                   int it0, int bcount, int bmax, int32_t* __restrict__ res_cnt,
                                   unsigned long long* __restrict__ err_by_h,
                                   int32_t* __restrict__ hlist, int32_t* __restrict__ n_surv, const Stage2Rows s2) {
  const int p = blockIdx.y;
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= bcount) return;
  const RansacProb pr = probs[p];
  if (pr.done || it0 + h >= pr.est_k) return;
  res_cnt[(int64_t)p * bmax + h] = 0;
  if (cnt_up[(int64_t)p * bmax + h] >= pr.best_cnt) {
    const int slot = atomicAdd(&n_surv[p], 1);
    hlist[(int64_t)p * bmax + slot] = h;
    err_by_h[(int64_t)p * bmax + h] = 0;  // accumulated by k_ransac_count_few
    if (s2.A16s && slot < PF_S2_CAP) {
      const uint4* src = reinterpret_cast<const uint4*>(s2.A16 + ((int64_t)p * bmax + h) * PF_K);
      uint4* dst = reinterpret_cast<uint4*>(s2.A16s + ((int64_t)p * PF_S2_CAP + slot) * PF_K);
      dst[0] = src[0];
      dst[1] = src[1];
      const double smax = (double)__uint_as_float(s2.stat[p * PF_STAT]);
      const double beta = s2.tcap > 0.0 ? smax * smax : 0.0;   // the double pf_emit_row added
      s2.c_hs[(int64_t)p * PF_S2_CAP + slot] = __double2float_rd((double)s2.c_h[(int64_t)p * bmax + h] - beta);
      s2.cnt2[(int64_t)p * PF_S2_CAP + slot] = 0;
    }
  }
}

// ---- second stage (round 4): the K = 16 bound leaves 3 - 4x the survivors of the K = 32 bound; the survivors of a round --
// a compact list of ~16 hypotheses per problem -- go through the K = 32 form (a_hi . (b_hi + b_lo), same a_hi rows, same
// eps_h) before they are counted exactly.  1.5 % of the matrix work of a first-stage launch.
// The list is not compacted again: k_ransac_count_few skips the entries whose K = 32 bound is below the carried best count.

// Debug check (CS_RANSAC_CHECK=1): the bound must dominate the exact count of every hypothesis.
__global__ void k_ransac_check_bound(const RansacProb* __restrict__ probs, const int32_t* __restrict__ exact,
                                     const int32_t* __restrict__ cnt_up, int it0, int bcount, int bmax,
                                     unsigned long long* __restrict__ stats) {
  const int p = blockIdx.y;
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= bcount) return;
  const RansacProb pr = probs[p];
  if (pr.done || it0 + h >= pr.est_k) return;
  const int e = exact[(int64_t)p * bmax + h], u = cnt_up[(int64_t)p * bmax + h];
  if (e > u) atomicAdd(&stats[0], 1ULL);
  atomicAdd(&stats[1], 1ULL);
  atomicAdd(&stats[2], (unsigned long long)(u - e > 0 ? u - e : 0));
}

// Debug check of the SECOND stage (CS_RANSAC_CHECK=1): the K = 32 bound of every compacted survivor must dominate its exact
// count too (violations and comparisons go to the same counters as the first stage's).
__global__ void k_ransac_check_bound2(const RansacProb* __restrict__ probs, const int32_t* __restrict__ exact,
                                      const int32_t* __restrict__ hlist, const int32_t* __restrict__ n_surv, int bmax,
                                      const int32_t* __restrict__ cnt2, unsigned long long* __restrict__ stats) {
  const int p = blockIdx.y;
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (probs[p].done || slot >= min(n_surv[p], PF_S2_CAP)) return;
  const int e = exact[(int64_t)p * bmax + hlist[(int64_t)p * bmax + slot]], u = cnt2[(int64_t)p * PF_S2_CAP + slot];
  if (e > u) atomicAdd(&stats[0], 1ULL);
  atomicAdd(&stats[1], 1ULL);
  atomicAdd(&stats[2], (unsigned long long)(u - e > 0 ? u - e : 0));
}

// Exact counts (and fixed-point errors) when only a handful of hypotheses survive the prefilter (the
// normal case: ~2 per problem and round).  The MFMA list kernel above needs a 128-hypothesis tile per
// workgroup and costs ~110 us per round even for two survivors.  Here the pair range of a problem is
// split over gridDim.x workgroups, each walks its slice once per survivor with the canonical f64
// chain; integer partial sums are combined with atomics (exact, order-free).
// grid: x = pair slice, y = problem, z = survivor slot (strided).  res_cnt / err_by_h of the survivors
// are zero on entry.
__global__ __launch_bounds__(256) void k_ransac_count_few(const RansacProb* __restrict__ probs,
                                                          const float* __restrict__ pk, int64_t total,
                                                          const double* __restrict__ hyp, int bmax,
                                                          double thr2, double scale,
                                                          int32_t* __restrict__ res_cnt,
                                                          unsigned long long* __restrict__ err_by_h,
                                                          const int32_t* __restrict__ hlist,
                                                          const int32_t* __restrict__ n_surv, int list_stride,
                                                          // second stage (cnt2 != nullptr): entry c of the first-stage list is
                                                          // skipped when its K = 32 bound is below the best
                                                          const int32_t* __restrict__ cnt2) {
  const int p = blockIdx.y;
  const RansacProb pr = probs[p];
  if (pr.done) return;
  const int nlist = n_surv[p];
  // entries beyond the capacity of the compact list were not looked at by the second stage: they pass unfiltered
  auto next_entry = [&](int c) {
    if (cnt2)
      while (c < nlist && c < PF_S2_CAP && cnt2[(int64_t)p * PF_S2_CAP + c] < pr.best_cnt) c += gridDim.z;
    return c;
  };
  int c = next_entry(blockIdx.z);
  if (c >= nlist) return;
  const int tid = threadIdx.x;
  const int per = (pr.m + gridDim.x - 1) / gridDim.x;
  const int i0 = blockIdx.x * per, i1 = min(pr.m, i0 + per);
  if (i0 >= i1) return;
  // this thread's pairs stay in registers across the survivors (slices are short: m / gridDim.x / 256)
  constexpr int MAXP = 8;
  const bool in_regs = per <= 256 * MAXP;
  float ps[MAXP][6];
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < MAXP; ++j) {
      const int i = i0 + tid + 256 * j;
      const int64_t g = pr.off + (i < i1 ? i : i0);
#pragma unroll
      for (int c = 0; c < 6; ++c) ps[j][c] = pk[(int64_t)c * total + g];
      if (i >= i1) ps[j][3] = 1.0e30f;  // far-away target: never an inlier
    }
  }
  // the next survivor's hypothesis is requested before the current one is evaluated: list entry -> twelve strided f64
  // loads are two dependent trips to L2 (~2 us), as long as the 8 x 22 f64 operations per thread they feed
  int hn = hlist[(int64_t)p * list_stride + c];
  double Rn[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) Rn[e] = hyp[((int64_t)p * 12 + e) * bmax + hn];
  for (; c < nlist;) {
    const int h = hn;
    double R[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = Rn[e];
    c = next_entry(c + gridDim.z);
    if (c < nlist) {
      hn = hlist[(int64_t)p * list_stride + c];
#pragma unroll
      for (int e = 0; e < 12; ++e) Rn[e] = hyp[((int64_t)p * 12 + e) * bmax + hn];
    }
    int cnt = 0;
    unsigned long long err = 0;  // fixed-point squared error of the inliers (exact integer sum, as k_ransac_err)
    auto one = [&](float sx, float sy, float sz, float qx, float qy, float qz) {
      const double d2 = residual2_f64(R, (double)sx, (double)sy, (double)sz, (double)qx, (double)qy, (double)qz);
      if (d2 < thr2) {
        ++cnt;
        err += (unsigned long long)(d2 * scale);
      }
    };
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < MAXP; ++j) one(ps[j][0], ps[j][1], ps[j][2], ps[j][3], ps[j][4], ps[j][5]);
    } else {
      for (int i = i0 + tid; i < i1; i += 256) {
        const int64_t g = pr.off + i;
        one(pk[0 * total + g], pk[1 * total + g], pk[2 * total + g], pk[3 * total + g], pk[4 * total + g],
            pk[5 * total + g]);
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      cnt += __shfl_xor(cnt, off);
      err += __shfl_xor(err, off);
    }
    if ((tid & 63) == 0 && cnt) {
      atomicAdd(&res_cnt[(int64_t)p * bmax + h], cnt);
      atomicAdd(&err_by_h[(int64_t)p * bmax + h], err);
    }
  }
}

// est_k implied by a best inlier count c (Open3D: log(1 - confidence) / log(1 - ratio^n))
__device__ __forceinline__ int est_bound(int c, int m, int ransac_n, double log_1mc, int est_k0) {
  const double ratio = fmin(1.0, (double)c / (double)m);
  double pw = 1.0;
  for (int j = 0; j < ransac_n; ++j) pw = pw * ratio;
  const double den = log(1.0 - pw);
  if (den < 0.0) {  // den == 0: (inliers/M)^n below 2^-53 -> no finite bound
    const double est = log_1mc / den;
    if (est < (double)est_k0) return (int)ceil(est);
  }
  return est_k0;
}

// One wave per problem: sequential-semantics replay of the chunk from the inlier counts alone.
__global__ __launch_bounds__(256) void k_ransac_scan1(RansacProb* probs, int n_prob,
                                                     const int32_t* __restrict__ res_cnt, int it0,
                                                     int bcount, int bmax, int ransac_n,
                                                     int max_iter, double log_1mc,
                                                     int32_t* __restrict__ cand, int* n_active,
                                                     // fused k_ransac_scan2 (err_by_h != nullptr: k_ransac_count_few left the
                                                     // error of every survivor, so no k_ransac_err has to run in between)
                                                     const unsigned long long* __restrict__ err_by_h,
                                                     const double* __restrict__ hyp, int32_t* __restrict__ next_nsurv,
                                                     int* __restrict__ next_nactive) {
  // The chunk's counts are staged in LDS by all four waves (coalesced), then wave 0 replays them: lane l
  // owns the contiguous segment [l seg, (l+1) seg).  Element h of lane l sits at h + l, which spreads
  // the lanes' same-offset reads over the banks.
  extern __shared__ int32_t lcnt[];
  const int p = blockIdx.x;
  if (err_by_h && threadIdx.x == 0) {   // what k_ransac_scan2 clears for the next round (the other parity's counters)
    next_nsurv[p] = 0;
    if (p == 0) *next_nactive = 0;
  }
  RansacProb pr = probs[p];
  if (pr.done) return;
  const int seg = (bcount + 63) / 64;
  {
    const int32_t* g = res_cnt + (int64_t)p * bmax;
    for (int h = threadIdx.x; h < bcount; h += 256) lcnt[h + h / seg] = g[h];
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const int32_t* cnt = lcnt + lane;  // cnt[h] for h in this lane's segment
  const int s0 = lane * seg, s1 = min(bcount, s0 + seg);
  // 1. exclusive prefix max of the counts over lanes, seeded with the carried best
  int lmax = 0;
  for (int h = s0; h < s1; ++h)
    if (it0 + h < pr.est_k) lmax = max(lmax, cnt[h]);
  int incl = lmax;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl = max(incl, o);
  }
  int pre = __shfl_up(incl, 1);
  if (lane == 0) pre = 0;
  pre = max(pre, pr.best_cnt);
  // 2. first position where the loop of the reference would stop
  int stop = 0x7fffffff;
  {
    int cur = pre;
    int ek = cur > pr.best_cnt ? est_bound(cur, pr.m, ransac_n, log_1mc, pr.est_k) : pr.est_k;
    for (int h = s0; h < s1; ++h) {
      if (it0 + h >= ek) {
        stop = h;
        break;
      }
      const int c = cnt[h];
      if (c > cur) {
        cur = c;
        ek = est_bound(cur, pr.m, ransac_n, log_1mc, pr.est_k);
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) stop = min(stop, __shfl_xor(stop, off));
  if (stop > bcount) stop = bcount;
  // 3. best count over the evaluated prefix, new bound
  int cmax = 0;
  for (int h = s0; h < min(s1, stop); ++h) cmax = max(cmax, cnt[h]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
  int new_ek = pr.est_k;
  if (cmax > pr.best_cnt) new_ek = est_bound(cmax, pr.m, ransac_n, log_1mc, pr.est_k);
  // 4. candidates: evaluated hypotheses that tie for the best count (ascending order)
  int ncand = 0;
  // fused scan2: the sequential rule "take candidate c if the count rose or its error is strictly below the best so far" ends
  // at the FIRST candidate (ascending hypothesis) of the smallest error, provided the count rose or that error is below
  // the carried one -- a lexicographic (error, hypothesis) minimum over the lanes' segments
  unsigned long long e_min = ~0ULL;
  int h_min = 0x7fffffff;
  if (cmax > 0 && cmax >= pr.best_cnt) {
    if (err_by_h) {
      for (int h = s0; h < min(s1, stop); ++h)
        if (cnt[h] == cmax) {
          const unsigned long long e = err_by_h[(int64_t)p * bmax + h];
          if (e < e_min) {   // strict: the earlier hypothesis keeps a tie
            e_min = e;
            h_min = h;
          }
        }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long eo = __shfl_xor(e_min, off);
        const int ho = __shfl_xor(h_min, off);
        if (eo < e_min || (eo == e_min && ho < h_min)) {
          e_min = eo;
          h_min = ho;
        }
      }
    } else {
      int mine = 0;
      for (int h = s0; h < min(s1, stop); ++h) mine += cnt[h] == cmax;
      int incl2 = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl2, off);
        if (lane >= off) incl2 += o;
      }
      int pos = incl2 - mine;
      ncand = __shfl(incl2, 63);
      for (int h = s0; h < min(s1, stop); ++h)
        if (cnt[h] == cmax) cand[(int64_t)p * bmax + pos++] = h;
    }
  }
  if (lane == 0) {
    const int consumed = it0 + stop;
    pr.est_k = new_ek;
    pr.n_cand = ncand;
    pr.chunk_max = cmax;
    if (consumed >= pr.est_k || consumed >= max_iter) {
      pr.done = 1;
      pr.iters = consumed < max_iter ? consumed : max_iter;
    } else {
      atomicAdd(n_active, 1);
    }
    if (err_by_h && h_min != 0x7fffffff && (cmax > pr.best_cnt || e_min < pr.best_err)) {
      pr.best_cnt = cmax;
      pr.best_err = e_min;
      pr.best_itr = it0 + h_min;
      for (int c = 0; c < 12; ++c) pr.best_T[c] = hyp[((int64_t)p * 12 + c) * bmax + h_min];
    }
    // (unfused: best_* are updated by scan2; keep everything else)
    probs[p] = pr;
  }
}

// Fixed-point squared error of the candidate hypotheses: grid (slots, problems).
__global__ __launch_bounds__(256) void k_ransac_err(const RansacProb* __restrict__ probs,
                                                    const float* __restrict__ pk, int64_t total,
                                                    const double* __restrict__ hyp, int bmax,
                                                    const int32_t* __restrict__ cand, double thr2,
                                                    double scale,
                                                    unsigned long long* __restrict__ cand_err) {
  __shared__ unsigned long long red[256];
  const int p = blockIdx.y;
  const RansacProb pr = probs[p];
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < pr.n_cand; c += gridDim.x) {
    const int h = cand[(int64_t)p * bmax + c];
    const double* hp = hyp + ((int64_t)p * 12) * bmax + h;
    double R[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = hp[(int64_t)e * bmax];
    unsigned long long err = 0;
    for (int i = tid; i < pr.m; i += 256) {
      const int64_t g = pr.off + i;
      const double d2 = residual2_f64(R, (double)pk[0 * total + g], (double)pk[1 * total + g],
                                      (double)pk[2 * total + g], (double)pk[3 * total + g],
                                      (double)pk[4 * total + g], (double)pk[5 * total + g]);
      if (d2 < thr2) err += (unsigned long long)(d2 * scale);
    }
    red[tid] = err;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid == 0) cand_err[(int64_t)p * bmax + c] = red[0];
    __syncthreads();
  }
}

// cand_err is indexed by candidate slot (k_ransac_err) or, when by_h is set, by hypothesis
// (k_ransac_count_few computed the error of every survivor along with its count)
__global__ void k_ransac_scan2(RansacProb* probs, int n_prob, const double* __restrict__ hyp,
                               const int32_t* __restrict__ cand,
                               const unsigned long long* __restrict__ cand_err, int by_h, int it0,
                               int bmax, int32_t* __restrict__ next_nsurv, int* __restrict__ next_nactive) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  // last kernel of a round: clear the survivor / activity counters the NEXT round accumulates into (the other
  // parity's: this round's are still to be copied to the host) -- a hipMemsetAsync per round before
  next_nsurv[p] = 0;
  if (p == 0) *next_nactive = 0;
  RansacProb pr = probs[p];
  if (pr.n_cand <= 0) return;
  bool changed = false;
  int best_h = -1;
  for (int c = 0; c < pr.n_cand; ++c) {
    const unsigned long long e = cand_err[(int64_t)p * bmax + (by_h ? cand[(int64_t)p * bmax + c] : c)];
    if (pr.chunk_max > pr.best_cnt || e < pr.best_err) {
      pr.best_cnt = pr.chunk_max;
      pr.best_err = e;
      best_h = cand[(int64_t)p * bmax + c];
      changed = true;
    }
  }
  pr.n_cand = 0;
  if (changed) {
    pr.best_itr = it0 + best_h;
    for (int c = 0; c < 12; ++c) pr.best_T[c] = hyp[((int64_t)p * 12 + c) * bmax + best_h];
  }
  probs[p] = pr;
}

__global__ void k_ransac_finish(const RansacProb* __restrict__ probs, int n_prob, double scale,
                                float* __restrict__ T, int32_t* __restrict__ inliers,
                                double* __restrict__ rmse, int32_t* __restrict__ iters) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  const RansacProb pr = probs[p];
  float* o = T + (int64_t)p * 16;
  if (pr.best_cnt > 0) {
    for (int c = 0; c < 12; ++c) o[c] = (float)pr.best_T[c];  // the reference's T_est.astype(np.float32)
  } else {
    for (int c = 0; c < 12; ++c) o[c] = (c % 5 == 0) ? 1.f : 0.f;
  }
  o[12] = 0.f;
  o[13] = 0.f;
  o[14] = 0.f;
  o[15] = 1.f;
  if (inliers) inliers[p] = pr.best_cnt;
  if (rmse)
    rmse[p] = pr.best_cnt > 0 ? sqrt(((double)pr.best_err / scale) / (double)pr.best_cnt) : 0.0;
  if (iters) iters[p] = pr.iters;
}

}  // namespace cs

using namespace cs;

namespace {
// prefilter diagnostics: {bound violations, hypotheses checked, sum of (bound - exact)} from
// CS_RANSAC_CHECK runs, {survivors, hypotheses evaluated} always
std::atomic<unsigned long long> g_pf_stats[5];  // zero-initialised (static storage)

// page-locked host staging buffer of the calling thread (grown on demand, freed at thread exit)
struct PinnedScratch {
  char* p = nullptr;
  size_t n = 0;
  ~PinnedScratch() {
    if (p) (void)hipHostFree(p);
  }
};
thread_local PinnedScratch t_pinned;
char* pinned_scratch(size_t bytes) {
  if (t_pinned.n < bytes) {
    if (t_pinned.p) (void)hipHostFree(t_pinned.p);
    t_pinned.p = nullptr;
    t_pinned.n = 0;
    void* q = nullptr;
    if (hipHostMalloc(&q, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    t_pinned.p = static_cast<char*>(q);
    t_pinned.n = bytes;
  }
  return t_pinned.p;
}

// Largest chunk of iterations per round.  One workgroup = 128 hypotheses x all pairs of a problem
// (~100 us), 1536 workgroups are resident: chunks of 16384 give >= 8 "waves" of workgroups for a
// 32-query batch, so the partially filled last wave costs ~10 % instead of ~33 % at 4096.
constexpr int BMAX = 16384;
// K = 16 form: largest |t| / smax a hypothesis may have to go through the prefilter; the others are counted exactly
// (k_ransac_pack16_b0 has the measurement behind the value).  The K = 32 form has no cap: its kernels get tcap = 0.
constexpr double PF_TCAP = 0.75;
// Survivors per problem up to which k_ransac_count_few does the exact counts; longer lists go to k_ransac_count<true>.
// (K = 32 prefilter: 32 / 64 / 128 / 256 measured, 128 the fastest by ~1 %.  The K = 16 form leaves 3 - 4x the survivors,
// ~16 per problem and round on the chair shape: the list kernel -- one workgroup of 256 hypothesis lanes per problem --
// then ran in every fourth round at 670 us.)
constexpr int FEW_MAX = 1024;

// The environment knobs of cs_ransac_batch.  All of them are read HERE, once per call: tests flip them between calls
// of one process, so none is cached.  INTEGRATION.md lists them.
struct Options {
  bool prefilter;          // CS_RANSAC_PREFILTER=0: exact-only RANSAC (the reference path of the identity tests)
  bool check;              // CS_RANSAC_CHECK=1: verify the bound against the exact count of EVERY hypothesis (slow; tests)
  int pf_nm;               // CS_RANSAC_PF_K=32: 2 = the two-MFMA form a_hi . (b_hi + b_lo); default 16: 1 = one MFMA,
                           // a_hi . b_hi' with the dropped term bounded per pair.  Same results (the exact kernels decide)
  bool stage2;             // CS_RANSAC_STAGE2=0: no K = 32 second stage on the survivors of the K = 16 form
  int first_chunk;         // CS_RANSAC_FIRST=<n>: iterations counted exactly before the prefilter starts (default 64)
  int force_jacobi;        // CS_RANSAC_JACOBI=1: every hypothesis through the Jacobi eigen-solver (the fallback of horn_qcp;
                           // the oracle's oc_rigid_fit_force_jacobi is its counterpart)
  bool overlap;            // CS_RANSAC_OVERLAP=0: every round on the caller's stream
  int trace_it0;           // CS_PF_TRACE=<it0>: per-workgroup trace of the prefilter launch of the round starting at it0
  const char* trace_file;  // (-1 = off), written to CS_PF_TRACE_FILE (tools/pf_trace.py)
};
Options read_options() {
  const char* pf = getenv("CS_RANSAC_PREFILTER");
  const char* ck = getenv("CS_RANSAC_CHECK");
  const char* k = getenv("CS_RANSAC_PF_K");
  const char* s2 = getenv("CS_RANSAC_STAGE2");
  const char* first = getenv("CS_RANSAC_FIRST");
  const char* jac = getenv("CS_RANSAC_JACOBI");
  const char* ov = getenv("CS_RANSAC_OVERLAP");
  const char* tr = getenv("CS_PF_TRACE");
  const char* trf = getenv("CS_PF_TRACE_FILE");
  Options o;
  o.prefilter = !(pf && pf[0] == '0');
  o.check = ck && ck[0] == '1';
  o.pf_nm = (k && atoi(k) == 32) ? 2 : 1;
  o.stage2 = !(s2 && s2[0] == '0');
  // The unfiltered chunk costs its hypotheses x ALL pairs in f64 (0.31 ms per 48-problem call at 256, twice per chair step);
  // with 64 the second chunk, [64, 512), is already prefiltered -- against the best of 64 hypotheses instead of 256, which
  // lets a few more of its hypotheses through to the exact kernels.  Results are the sequential loop's either way.
  // Clamped: a first chunk above BMAX would index the BMAX-sized scratch out of range, 0 would never advance the chunk loop.
  o.first_chunk = ((std::min(std::max(first ? atoi(first) : 64, 64), BMAX) + 63) / 64) * 64;
  o.force_jacobi = jac && atoi(jac) != 0;
  o.overlap = !(ov && ov[0] == '0');
  o.trace_it0 = tr ? atoi(tr) : -1;
  o.trace_file = trf ? trf : "/tmp/pf_trace.bin";
  return o;
}

// Every device buffer of a call, and the views of the buffers that exist once per round parity.
struct Scratch {
  int n_prob = 0;
  // per-round state in ONE block, so a round ends with one device->host copy (into pinned memory):
  // [RansacProb x n_prob | 2 x { n_surv int32 x n_prob (padded to 8 B) | n_active int32 (8 B) }]: the counters
  // exist once per round parity, the last scan kernel of a round clears the set of the next round
  size_t st_probs = 0, st_surv = 0, st_cnt = 0, st_bytes = 0;
  PoolBuf<char> state;
  char* h_state = nullptr;                 // the thread's pinned staging buffer (not owned)
  PoolBuf<float> pk;                       // SoA copy of the correspondences
  PoolBuf<float4> pair32;                  // 32-B rows for the sampling
  PoolBuf<double> hyp;                     // hypotheses (f64 R|t), one set per round parity
  PoolBuf<int32_t> res_cnt, cand;
  PoolBuf<unsigned long long> cand_err;
  // prefilter: f16 pair image (every problem padded to whole LDS stages), hypothesis rows, bounds, survivor lists
  PoolBuf<int64_t> off16;
  PoolBuf<_Float16> B16, A16;
  PoolBuf<float> c_h;
  PoolBuf<int32_t> cnt_up, hlist;
  PoolBuf<unsigned> pf_stat;
  PoolBuf<double> pf_sums;
  // second stage: K = 32 image, the compacted rows of the survivors, their bounds
  PoolBuf<_Float16> B32, A16s;
  PoolBuf<float> c_hs;
  PoolBuf<int32_t> cnt2;
  PoolBuf<int32_t> exact_dbg;              // CS_RANSAC_CHECK
  PoolBuf<unsigned long long> chk_stats;
  PoolBuf<int32_t> xcd_buf;                // placement tables, one per round parity (8 x n_prob entries each)
  PoolBuf<unsigned long long> trace;       // CS_PF_TRACE
  size_t trace_cap = 1;

  bool alloc(int n, int64_t tot1, int64_t rows16, int pf_nm, bool pf, bool stage2, bool check, bool tracing) {
    n_prob = n;
    st_probs = sizeof(RansacProb) * (size_t)n;
    st_surv = ((sizeof(int32_t) * (size_t)n + 7) / 8) * 8;
    st_cnt = st_surv + 8;
    st_bytes = st_probs + 2 * st_cnt;
    h_state = pinned_scratch(st_bytes);
    const size_t nb = (size_t)n * BMAX, ns2 = (size_t)n * PF_S2_CAP;
    if (tracing) trace_cap = (size_t)8 * n * 64 * 16 * 16;
    return h_state && state.alloc(st_bytes) && pk.alloc((size_t)tot1 * 6) && pair32.alloc((size_t)tot1 * 2) &&
           hyp.alloc(2 * nb * 12) && res_cnt.alloc(nb) && cand.alloc(nb) && cand_err.alloc(nb) && off16.alloc(n + 1) &&
           B16.alloc(pf ? (size_t)rows16 * pf_pitch(pf_nm) : 8) && A16.alloc(pf ? 2 * nb * PF_K : 8) &&
           c_h.alloc(pf ? 2 * nb : 1) && cnt_up.alloc(pf ? 2 * nb : 1) && hlist.alloc(pf ? nb : 1) &&
           pf_stat.alloc((size_t)n * PF_STAT) && pf_sums.alloc((size_t)n * 6) &&
           B32.alloc(stage2 ? (size_t)rows16 * PF_PITCH : 8) && A16s.alloc(stage2 ? ns2 * PF_K : 8) &&
           c_hs.alloc(stage2 ? ns2 : 1) && cnt2.alloc(stage2 ? ns2 : 1) &&
           exact_dbg.alloc(check ? nb : 1) && chk_stats.alloc(4) && xcd_buf.alloc((size_t)16 * n) && trace.alloc(trace_cap);
  }
  RansacProb* probs() const { return reinterpret_cast<RansacProb*>(state.p); }
  // counters of a round parity, device and host copy
  int32_t* nsurv(int par) const { return reinterpret_cast<int32_t*>(state.p + st_probs + par * st_cnt); }
  int* nactive(int par) const { return reinterpret_cast<int*>(state.p + st_probs + par * st_cnt + st_surv); }
  const int32_t* h_nsurv(int par) const { return reinterpret_cast<const int32_t*>(h_state + st_probs + par * st_cnt); }
  int h_nactive(int par) const { return *reinterpret_cast<const int*>(h_state + st_probs + par * st_cnt + st_surv); }
  // buffers of a round parity
  double* hyp_of(int par) const { return hyp.p + (size_t)par * n_prob * 12 * BMAX; }
  _Float16* A16_of(int par) const { return A16.p + (size_t)par * n_prob * BMAX * PF_K; }
  float* c_h_of(int par) const { return c_h.p + (size_t)par * n_prob * BMAX; }
  int32_t* cnt_up_of(int par) const { return cnt_up.p + (size_t)par * n_prob * BMAX; }
  int32_t* xcd_of(int par) const { return xcd_buf.p + (size_t)par * 8 * n_prob; }
};

struct Event {
  hipEvent_t e = nullptr;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
};
// an error return must not hand the scratch buffers back to the pool while a side stream still uses
// them; on the normal path the final wait on the main stream is already ordered behind its events
struct SideDrain {
  hipStream_t st = nullptr;
  bool clean = false;
  ~SideDrain() {
    if (st && !clean) (void)hipStreamSynchronize(st);
  }
};

// The front half of one round, as enqueued: what the back half needs to know about it.
struct Front {
  int it0 = 0, b = 0, par = 0;
  bool pf = false, on_side = false;
  // placement of the round's prefilter launch (the second stage of the back half uses the same)
  XcdTab xtab;
  const int32_t* xcd_prob = nullptr;
  int pslots = 1;
};

// One cs_ransac_batch call: arguments, options, scratch, streams and the state carried from round to round.
struct RansacCall {
  int n_prob = 0, ransac_n = 0, max_iter = 0, m_max = 0;
  uint64_t seed = 0;
  int64_t total = 0, tot1 = 1;
  double thr2 = 0.0, scale = 0.0, log_1mc = 0.0, tcap = 0.0;
  Options opt;
  bool pf_alloc = false, stage2 = false, check = false;   // what the options come to for THIS call
  std::vector<RansacProb> hp;                             // host copy of the per-problem state, as of the last read-back
  std::vector<int64_t> h_off16;
  std::vector<int32_t> h_xcd[2];
  Scratch sc;                                             // (declared before the drains: they are destroyed first)
  Event round_done, front_done[2], hyp_done[2];
  hipStream_t s = nullptr, side = nullptr, side_hyp = nullptr;
  SideDrain side_drain, side_hyp_drain;
  int max_surv_prev = 1 << 30;  // survivors per problem in the previous prefiltered round (unknown: many)
  unsigned long long tot_surv = 0, tot_eval = 0;
  size_t trace_n = 0;

  int init(const int64_t* h_off, int n, double max_corr, int rn, int iters, double confidence, uint64_t sd, hipStream_t st);
  int setup(const float* d_src, const float* d_tgt);
  int open_streams();
  bool prefiltered(int it0) const { return pf_alloc && it0 >= opt.first_chunk; }
  // chunks: [0, first) counted exactly, [first, 512) in one piece, then doubling ([512, 1024), [1024, 2048), ...) up to BMAX
  int chunk_of(int it0) const {
    const int b = it0 < opt.first_chunk ? opt.first_chunk : it0 < 512 ? 512 - it0 : (it0 < BMAX ? it0 : BMAX);
    return b > max_iter - it0 ? max_iter - it0 : b;
  }
  // pair-range splits of the exact count of a whole chunk: enough workgroups for 256 CUs x several waves; the
  // correspondence range is split when the chunk is small (integer partial sums combine exactly)
  int chunk_splits(int tiles) const {
    int splits = (int)(4096 / ((int64_t)n_prob * tiles > 0 ? (int64_t)n_prob * tiles : 1));
    if (splits < 1) splits = 1;
    if (splits > 16) splits = 16;
    while (splits > 1 && m_max / splits < 4 * RC_CHUNK) --splits;
    return splits;
  }
  int place(int it0, int par, int* live);
  Front enqueue_front(int it0, int par, hipStream_t st);
  int back_half(const Front& cur);
  int count_chunk(const Front& cur, double eval_pairs);
  int count_survivors(const Front& cur, bool* err_known);
  bool read_back(const Front& cur);
  int finish(float* d_T, int32_t* d_inliers, double* d_rmse, int32_t* d_iters);
};

// Problem table, derived constants, options and scratch.
int RansacCall::init(const int64_t* h_off, int n, double max_corr, int rn, int iters, double confidence, uint64_t sd,
                     hipStream_t st) {
  n_prob = n;
  ransac_n = rn;
  max_iter = iters;
  seed = sd;
  s = st;
  total = h_off[n_prob] - h_off[0];
  tot1 = total ? total : 1;
  hp.resize(n_prob);
  h_off16.assign(n_prob + 1, 0);
  for (int p = 0; p < n_prob; ++p) {
    int64_t m = h_off[p + 1] - h_off[p];
    CS_REQUIRE(m >= 0 && m < (1LL << 24), CS_ERR_INVALID,
               "cs_ransac_batch: bad segment %d (a problem holds fewer than 2^24 correspondences)", p);
    RansacProb& pr = hp[p];
    memset(&pr, 0, sizeof(pr));
    pr.off = h_off[p];
    pr.m = (int32_t)m;
    pr.est_k = max_iter;
    pr.best_itr = -1;
    // Open3D returns the default (identity) result when there are fewer pairs than ransac_n
    pr.done = m < ransac_n ? 1 : 0;
    if (m > m_max) m_max = (int)m;
    h_off16[p + 1] = h_off16[p] + pf_padded(m);
  }
  // squared threshold (Open3D: max_correspondence_distance * max_correspondence_distance in double) and
  // the power-of-two fixed-point scale of the inlier error: terms d^2 * scale < 2^38, so the u64 sum over
  // a problem's (< 2^24) pairs cannot overflow and is exact in any order
  thr2 = max_corr * max_corr;
  int ex = 0;
  (void)frexp(thr2, &ex);
  scale = ldexp(1.0, 38 - ex);
  log_1mc = log(1.0 - confidence);  // -inf when confidence == 1: never exits early
  opt = read_options();
  // the prefilter needs pairs and at least one iteration behind the exactly counted first chunk
  pf_alloc = opt.prefilter && total > 0 && max_iter > opt.first_chunk;
  stage2 = pf_alloc && opt.pf_nm == 1 && opt.stage2;
  check = pf_alloc && opt.check;   // (no prefiltered round, nothing to check)
  tcap = opt.pf_nm == 2 ? 0.0 : PF_TCAP;
  const bool ok = sc.alloc(n_prob, tot1, h_off16[n_prob] ? h_off16[n_prob] : 1, opt.pf_nm, pf_alloc, stage2, check,
                           opt.trace_it0 >= 0);
  CS_REQUIRE(ok, CS_ERR_HIP, "cs_ransac_batch: scratch allocation failed");
  return CS_OK;
}

// Uploads the problem table and builds what every round reads: the packed pairs and, for the prefilter, the pair sums
// and the f16 images.
int RansacCall::setup(const float* d_src, const float* d_tgt) {
  // problems + zeroed counters in one upload (h_state is page-locked and not read before the first round ends)
  memset(sc.h_state, 0, sc.st_bytes);
  memcpy(sc.h_state, hp.data(), sc.st_probs);
  CS_HIP_CHECK(hipMemcpyAsync(sc.state.p, sc.h_state, sc.st_bytes, hipMemcpyHostToDevice, s));
  RansacProb* const d_probs = sc.probs();
  if (pf_alloc) {
    // three launches: means (+ cleared statistics) -> packed pairs, K = 32 image and the per-problem maxima -> (K = 16) the
    // one-MFMA image, whose constant term takes the per-pair bound of the dropped term and needs the problem's smax.  The
    // first two read src / tgt once each, the third the packed pairs.
    int pblocks = (int)ceil_div(m_max > 0 ? m_max : 1, 256);
    if (pblocks > 64) pblocks = 64;
    const dim3 pgrid((unsigned)pblocks, (unsigned)n_prob);
    CS_HIP_CHECK(hipMemcpyAsync(sc.off16.p, h_off16.data(), sizeof(int64_t) * (n_prob + 1),
                                hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ransac_pair_sums, dim3((unsigned)n_prob), dim3(256), 0, s, d_probs, d_src, d_tgt, sc.pf_sums.p,
                       sc.pf_stat.p, sc.chk_stats.p);
    hipLaunchKernelGGL(k_ransac_images, pgrid, dim3(256), 0, s, d_probs, sc.off16.p, d_src, d_tgt, sc.pf_sums.p, total,
                       sc.pk.p, sc.pair32.p, opt.pf_nm == 2 ? sc.B16.p : (stage2 ? sc.B32.p : nullptr), sc.pf_stat.p);
    if (opt.pf_nm == 1)
      hipLaunchKernelGGL(k_ransac_pack16_b0, pgrid, dim3(256), 0, s,
                         d_probs, sc.off16.p, sc.pair32.p, sc.pf_sums.p, sc.pf_stat.p, tcap, sc.B16.p);
    CS_LAUNCH_CHECK();
  } else if (total > 0) {   // no prefilter in this call: the packed pairs alone
    hipLaunchKernelGGL(k_ransac_pack, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s,
                       d_src, d_tgt, total, sc.pk.p, sc.pair32.p);
    CS_LAUNCH_CHECK();
  }
  if (opt.trace_it0 >= 0) CS_HIP_CHECK(hipMemsetAsync(sc.trace.p, 0, sizeof(unsigned long long) * sc.trace_cap, s));
  return CS_OK;
}

// Events and the two side streams of the pipelined rounds (see cs_ransac_batch).
int RansacCall::open_streams() {
  for (Event* ev : {&round_done, &front_done[0], &front_done[1], &hyp_done[0], &hyp_done[1]})
    CS_HIP_CHECK(hipEventCreateWithFlags(&ev->e, hipEventDisableTiming));
  side = opt.overlap ? side_stream() : nullptr;
  // the hypotheses of a side-stream front half go to a THIRD stream: those of round i+2 are enqueued when round i
  // is known (their buffers, one set per parity, are free then) and run UNDER the prefilter of round i+1 instead of
  // behind it on the same stream (f64 vector work beside f16 matrix work)
  side_hyp = side ? side_stream(1) : nullptr;
  side_drain.st = side;
  side_hyp_drain.st = side_hyp;
  return CS_OK;
}

// Deals the problems that are live at iteration it0 to the 8 XCDs, longest first onto the least loaded XCD (host only).
// h_xcd[par] becomes the table [xcd][slot] -> problem (-1 = empty); returns the slots per XCD.
int RansacCall::place(int it0, int par, int* live) {
  std::vector<int> order;
  for (int p = 0; p < n_prob; ++p)
    if (!hp[p].done && hp[p].est_k > it0) order.push_back(p);
  *live = (int)order.size();
  std::sort(order.begin(), order.end(), [&](int a, int c) { return hp[a].m > hp[c].m; });
  std::vector<std::vector<int>> lists(8);
  int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int p : order) {
    int best = 0;
    for (int x = 1; x < 8; ++x)
      if (load[x] < load[best]) best = x;
    lists[best].push_back(p);
    load[best] += pf_padded(hp[p].m);
  }
  int pslots = 1;
  for (int x = 0; x < 8; ++x) pslots = std::max(pslots, (int)lists[x].size());
  std::vector<int32_t>& tab = h_xcd[par];
  tab.assign((size_t)8 * pslots, -1);
  for (int x = 0; x < 8; ++x)
    for (size_t i = 0; i < lists[x].size(); ++i) tab[(size_t)x * pslots + i] = lists[x][i];
  return pslots;
}

// Front half of the round that starts at it0: hypotheses (with their prefilter rows) and, from the second chunk on, the
// prefilter.  Independent of the carried best, so it may be enqueued on `st` = the side stream before the previous
// round is known; its skip tests read est_k / done while they may be updated (prob_view), and its placement is built
// from the state one round earlier: finished problems cost a few empty workgroups.
Front RansacCall::enqueue_front(int it0, int par, hipStream_t st) {
  Front f;
  f.it0 = it0;
  f.b = chunk_of(it0);
  f.par = par;
  f.pf = prefiltered(it0);
  f.on_side = st != s;
  const int b = f.b;
  int live = 0;
  f.pslots = place(it0, par, &live);
  const int pslots = f.pslots;
  // stream of the hypothesis kernel: the third stream for a prefiltered front half on the side stream
  hipStream_t sh = (f.on_side && f.pf && side_hyp) ? side_hyp : st;
  // the table travels as a kernel argument; rounds with more than XCD_SLOTS problems per XCD copy it to the device
  if (pslots <= XCD_SLOTS) {
    memcpy(f.xtab.v, h_xcd[par].data(), sizeof(int32_t) * 8 * pslots);
  } else {
    (void)hipMemcpyAsync(sc.xcd_of(par), h_xcd[par].data(), sizeof(int32_t) * 8 * pslots, hipMemcpyHostToDevice, sh);
    f.xcd_prob = sc.xcd_of(par);
  }
  RansacProb* const d_probs = sc.probs();
  _Float16* A16_r = f.pf ? sc.A16_of(par) : nullptr;
  float* c_h_r = f.pf ? sc.c_h_of(par) : nullptr;
  int32_t* cnt_up_r = f.pf ? sc.cnt_up_of(par) : nullptr;
  const int ptiles = (b + PF_HYP - 1) / PF_HYP;
  // 1024 workgroups are resident (4 per CU): split the pair range until there are >= 8 rounds of
  // workgroups, as long as a workgroup keeps >= 8 stages
  int psplits = (int)((8 * 1024 + (int64_t)live * ptiles - 1) / std::max<int64_t>((int64_t)live * ptiles, 1));
  if (psplits < 1) psplits = 1;
  if (psplits > 16) psplits = 16;
  while (psplits > 1 && m_max / psplits < 8 * PF_ROWS) --psplits;
  {
    ProfScope prof("ransac_hyp", sh);
    const int htiles = (b + 255) / 256;
    // the prefilter adds the partial counts of its pair-range splits with atomics: the hypothesis kernel clears them
    int32_t* fz = psplits > 1 ? cnt_up_r : nullptr;
    const auto kernel = ransac_n == 10 ? k_ransac_hyp<10> : k_ransac_hyp<0>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(8 * pslots * htiles)), dim3(256), 0, sh, d_probs,
                       sc.pair32.p, it0, b, BMAX, ransac_n, exact_div_recip((double)ransac_n), seed, f.xcd_prob, f.xtab, pslots, htiles, opt.force_jacobi,
                       sc.hyp_of(par), sc.pf_stat.p, sc.pf_sums.p, thr2, tcap, A16_r, c_h_r, fz);
  }
  if (f.pf) {
    if (sh != st) {   // the prefilter (side stream) follows the hypotheses (third stream)
      (void)hipEventRecord(hyp_done[par].e, sh);
      (void)hipStreamWaitEvent(st, hyp_done[par].e, 0);
    }
    ProfScope prof("ransac_pre", st);  // work units are added by the back half (state known there)
    const unsigned nblk = (unsigned)(8 * pslots * ptiles * psplits);
    unsigned long long* tr = (opt.trace_it0 == it0) ? sc.trace.p : nullptr;
    const auto kernel = opt.pf_nm == 2 ? k_ransac_prefilter<2, false> : k_ransac_prefilter<1, true>;
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(256), 0, st, d_probs, sc.off16.p, sc.B16.p, A16_r, c_h_r, it0, b, BMAX,
                       psplits, f.xcd_prob, f.xtab, pslots, ptiles, cnt_up_r, tr, (const int32_t*)nullptr);
    if (tr) trace_n = (size_t)nblk * 16;
  }
  if (f.on_side) (void)hipEventRecord(front_done[par].e, st);
  return f;
}

// Exact count of EVERY hypothesis of an unfiltered chunk (the first of a call, or all of them without the prefilter).
int RansacCall::count_chunk(const Front& cur, double eval_pairs) {
  const int b = cur.b;
  const int hpw = b <= 64 ? 64 : RC_HYP;      // hypotheses per workgroup
  const int tiles = (b + hpw - 1) / hpw;
  const int splits = chunk_splits(tiles);
  if (splits > 1 || hpw != RC_HYP)  // partial counts (pair-range splits, lane quarters) are combined with integer atomics
    CS_HIP_CHECK(hipMemset2DAsync(sc.res_cnt.p, sizeof(int32_t) * BMAX, 0, sizeof(int32_t) * b, n_prob, s));
  ProfScope prof("ransac_eval", s, 30.0 * eval_pairs);
  const dim3 grid((unsigned)(tiles * splits), (unsigned)n_prob);
  const auto kernel = hpw == 64 ? k_ransac_count<false, 64> : k_ransac_count<false, RC_HYP>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, sc.probs(), sc.pk.p, tot1, sc.hyp_of(cur.par), cur.it0, b, BMAX,
                     splits, thr2, sc.res_cnt.p, (const int32_t*)nullptr, (const int32_t*)nullptr);
  return CS_OK;
}

// Prefiltered round: the hypotheses whose bound reaches the carried best are listed, go through the K = 32 bound (second
// stage) and are counted exactly.  *err_known: their fixed-point errors are in cand_err (by hypothesis) as well.
int RansacCall::count_survivors(const Front& cur, bool* err_known) {
  const int it0 = cur.it0, b = cur.b;
  RansacProb* const d_probs = sc.probs();
  const double* hyp_r = sc.hyp_of(cur.par);
  const int32_t* cnt_up_r = sc.cnt_up_of(cur.par);
  int32_t* const d_nsurv = sc.nsurv(cur.par);   // cleared by the previous round's last scan kernel (or the upload)
  // This round's survivor counts are not known on the host: the previous round's pick the kernels (each is exact for
  // any count).  The first prefiltered round has no previous count, but a chunk of b <= FEW_MAX cannot leave more.
  const int surv_cap = std::min(max_surv_prev, b);
  const bool few = max_surv_prev <= FEW_MAX || b <= FEW_MAX;
  // the second stage runs when the few-survivor kernel will; its rows are written by the survivors kernel itself
  const bool run_s2 = stage2 && few && surv_cap <= PF_S2_CAP;
  Stage2Rows s2rows{};
  if (run_s2) {
    s2rows.A16 = sc.A16_of(cur.par);
    s2rows.c_h = sc.c_h_of(cur.par);
    s2rows.stat = sc.pf_stat.p;
    s2rows.tcap = tcap;
    s2rows.A16s = sc.A16s.p;
    s2rows.c_hs = sc.c_hs.p;
    s2rows.cnt2 = sc.cnt2.p;
  }
  hipLaunchKernelGGL(k_ransac_survivors, dim3((unsigned)((b + 255) / 256), (unsigned)n_prob), dim3(256), 0, s, d_probs,
                     cnt_up_r, it0, b, BMAX, sc.res_cnt.p, sc.cand_err.p, sc.hlist.p, d_nsurv, s2rows);
  {
    ProfScope prof("ransac_eval", s);
    if (few) {
      if (run_s2) {
        // K = 32 bound of the survivors (rows compacted by k_ransac_survivors): one small prefilter launch over all pairs,
        // with the placement of the round's first stage.  Tiles for the WHOLE capacity: workgroups past a problem's list
        // leave at once.  k_ransac_count_few then skips the entries whose bound is below the best.
        const int s2tiles = std::max(1, (std::min(b, PF_S2_CAP) + PF_HYP - 1) / PF_HYP);
        int s2splits = 8;
        while (s2splits > 1 && m_max / s2splits < 8 * PF_ROWS) --s2splits;
        hipLaunchKernelGGL((k_ransac_prefilter<2, false>), dim3((unsigned)(8 * cur.pslots * s2tiles * s2splits)), dim3(256),
                           0, s, d_probs, sc.off16.p, sc.B32.p, sc.A16s.p, sc.c_hs.p, 0, PF_S2_CAP, PF_S2_CAP, s2splits,
                           cur.xcd_prob, cur.xtab, cur.pslots, s2tiles, sc.cnt2.p, (unsigned long long*)nullptr, d_nsurv);
      }
      // pair slices short enough for a thread to keep its pairs in registers across the survivors (8 per thread)
      int fslices = 8;
      while (fslices < 32 && m_max > fslices * 2048) fslices *= 2;
      // survivor slots per (slice, problem): a workgroup loads its pairs once and walks its share of the survivors, so
      // FEW slots amortise the load (chair, same box: 2 / 4 / 8 / 16 slots -> 1 431 / 1 454 / 1 424 / 1 370 queries/s)
      const int fslots = surv_cap <= 256 ? 4 : 8;
      hipLaunchKernelGGL(k_ransac_count_few, dim3((unsigned)fslices, (unsigned)n_prob, (unsigned)fslots), dim3(256), 0, s,
                         d_probs, sc.pk.p, tot1, hyp_r, BMAX, thr2, scale, sc.res_cnt.p, sc.cand_err.p, sc.hlist.p, d_nsurv,
                         BMAX, run_s2 ? sc.cnt2.p : (const int32_t*)nullptr);
      *err_known = true;
    } else {
      // few hypotheses, so the pair range is split finely
      int lsplits = 16;
      while (lsplits > 1 && m_max / lsplits < RC_CHUNK) --lsplits;
      const int ltiles = std::min((b + RC_HYP - 1) / RC_HYP, 4);  // tile slots; the kernel strides over longer lists
      hipLaunchKernelGGL(k_ransac_count<true>, dim3((unsigned)(ltiles * lsplits), (unsigned)n_prob), dim3(256), 0, s,
                         d_probs, sc.pk.p, tot1, hyp_r, it0, b, BMAX, lsplits, thr2, sc.res_cnt.p, sc.hlist.p, d_nsurv);
    }
  }
  if (check) {   // both bounds against the exact count of every hypothesis of the chunk
    const int tiles = (b + RC_HYP - 1) / RC_HYP;
    const int splits = chunk_splits(tiles);
    CS_HIP_CHECK(hipMemset2DAsync(sc.exact_dbg.p, sizeof(int32_t) * BMAX, 0, sizeof(int32_t) * b, n_prob, s));
    hipLaunchKernelGGL(k_ransac_count<false>, dim3((unsigned)(tiles * splits), (unsigned)n_prob), dim3(256), 0, s,
                       d_probs, sc.pk.p, tot1, hyp_r, it0, b, BMAX, splits, thr2, sc.exact_dbg.p, (const int32_t*)nullptr,
                       (const int32_t*)nullptr);
    hipLaunchKernelGGL(k_ransac_check_bound, dim3((unsigned)((b + 255) / 256), (unsigned)n_prob), dim3(256), 0, s,
                       d_probs, sc.exact_dbg.p, cnt_up_r, it0, b, BMAX, sc.chk_stats.p);
    if (run_s2)
      hipLaunchKernelGGL(k_ransac_check_bound2, dim3(PF_S2_CAP / 256, (unsigned)n_prob), dim3(256), 0, s, d_probs,
                         sc.exact_dbg.p, sc.hlist.p, d_nsurv, BMAX, sc.cnt2.p, sc.chk_stats.p);
  }
  return CS_OK;
}

// Back half of a round, on the caller's stream: exact counts (of the whole chunk, or of the prefilter's survivors), then the
// replay of the chunk in iteration order -- the sequential RANSAC state (best, est_k, done) advances here.
int RansacCall::back_half(const Front& cur) {
  const int it0 = cur.it0, b = cur.b;
  // algorithmic work of this chunk (hp is the state before it): 30 FLOP per (evaluated hypothesis,
  // correspondence) (transform 18 + squared distance 8 + compare/accumulate) -- for the
  // exact count and for the prefilter alike (its matrix pipe executes 32 or 64 per pair: bench.py reports both)
  double eval_pairs = 0.0;
  for (int p = 0; p < n_prob; ++p) {
    if (hp[p].done) continue;
    const int nh = std::min(hp[p].est_k - it0, b);
    if (nh > 0) {
      eval_pairs += (double)nh * (double)hp[p].m;
      tot_eval += (unsigned long long)nh;
    }
  }
  bool err_known = false;  // the fixed-point errors of all candidates are already in cand_err (by hypothesis)
  if (!cur.pf) {
    if (int rc = count_chunk(cur, eval_pairs)) return rc;
  } else {
    prof_add_units("ransac_pre", 30.0 * eval_pairs);   // the units of the launch the front half bracketed
    if (int rc = count_survivors(cur, &err_known)) return rc;
  }
  static const hipError_t scan1_lds = hipFuncSetAttribute(
      reinterpret_cast<const void*>(k_ransac_scan1), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
  CS_REQUIRE(scan1_lds == hipSuccess, CS_ERR_HIP, "cs_ransac_batch: cannot reserve LDS for k_ransac_scan1");
  RansacProb* const d_probs = sc.probs();
  const double* hyp_r = sc.hyp_of(cur.par);
  int32_t* const next_nsurv = sc.nsurv(cur.par ^ 1);
  int* const next_nactive = sc.nactive(cur.par ^ 1);
  // scan1 replays the chunk and lists the candidates that tie for the best count.  When k_ransac_count_few has left the
  // error of every survivor it also picks the best of them; otherwise (unfiltered chunk, long survivor list) the errors
  // of the candidates are computed by k_ransac_err and k_ransac_scan2 picks.
  hipLaunchKernelGGL(k_ransac_scan1, dim3((unsigned)n_prob), dim3(256), sizeof(int32_t) * (b + 64), s, d_probs, n_prob,
                     sc.res_cnt.p, it0, b, BMAX, ransac_n, max_iter, log_1mc, sc.cand.p, sc.nactive(cur.par),
                     err_known ? sc.cand_err.p : (const unsigned long long*)nullptr, hyp_r, next_nsurv, next_nactive);
  if (!err_known) {
    hipLaunchKernelGGL(k_ransac_err, dim3(8, (unsigned)n_prob), dim3(256), 0, s, d_probs, sc.pk.p,
                       tot1, hyp_r, BMAX, sc.cand.p, thr2, scale, sc.cand_err.p);
    hipLaunchKernelGGL(k_ransac_scan2, dim3((unsigned)ceil_div(n_prob, 64)), dim3(64), 0, s,
                       d_probs, n_prob, hyp_r, sc.cand.p, sc.cand_err.p, 0, it0, BMAX, next_nsurv, next_nactive);
  }
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// The round's state has arrived in h_state: survivor bookkeeping, then hp becomes the state after the round.
// Returns whether any problem is still active.
bool RansacCall::read_back(const Front& cur) {
  if (cur.pf) {   // (hp is still the state before the round: the problems that were live in it)
    const int32_t* h_surv = sc.h_nsurv(cur.par);
    max_surv_prev = 0;
    for (int p = 0; p < n_prob; ++p)
      if (!hp[p].done) {
        tot_surv += (unsigned long long)h_surv[p];
        if (h_surv[p] > max_surv_prev) max_surv_prev = h_surv[p];
      }
  }
  memcpy(hp.data(), sc.h_state, sc.st_probs);
  return sc.h_nactive(cur.par) != 0;
}

// Trace dump, statistics, results.
int RansacCall::finish(float* d_T, int32_t* d_inliers, double* d_rmse, int32_t* d_iters) {
  if (trace_n) {
    std::vector<unsigned long long> ht(trace_n);
    CS_HIP_CHECK(hipMemcpy(ht.data(), sc.trace.p, sizeof(unsigned long long) * trace_n, hipMemcpyDeviceToHost));
    FILE* f = fopen(opt.trace_file, "wb");
    if (f) {
      fwrite(ht.data(), sizeof(unsigned long long), trace_n, f);
      fclose(f);
    }
  }
  g_pf_stats[3] += tot_surv;
  g_pf_stats[4] += tot_eval;
  if (check) {
    unsigned long long h_stats[4] = {0, 0, 0, 0};
    CS_HIP_CHECK(hipMemcpyAsync(h_stats, sc.chk_stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, s));
    CS_HIP_CHECK(hipStreamSynchronize(s));
    g_pf_stats[0] += h_stats[0];
    g_pf_stats[1] += h_stats[1];
    g_pf_stats[2] += h_stats[2];
    CS_REQUIRE(h_stats[0] == 0, CS_ERR_INTERNAL,
               "cs_ransac_batch: prefilter bound violated for %llu hypotheses", h_stats[0]);
  }
  hipLaunchKernelGGL(k_ransac_finish, dim3((unsigned)ceil_div(n_prob, 64)), dim3(64), 0, s,
                     sc.probs(), n_prob, scale, d_T, d_inliers, d_rmse, d_iters);
  CS_LAUNCH_CHECK();
  CS_HIP_CHECK(hipStreamSynchronize(s));
  side_drain.clean = true;
  side_hyp_drain.clean = true;
  return CS_OK;
}
}  // namespace

extern "C" {

void cs_ransac_prefilter_stats(uint64_t out[5], int reset) {
  for (int i = 0; i < 5; ++i) {
    if (out) out[i] = g_pf_stats[i].load();
    if (reset) g_pf_stats[i].store(0);
  }
}

int cs_ransac_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, int n_prob,
                    double max_corr, int ransac_n, int max_iter, double confidence, uint64_t seed,
                    float* d_T, int32_t* d_inliers, double* d_rmse, int32_t* d_iters,
                    void* stream) {
  CS_REQUIRE(h_off && d_T, CS_ERR_INVALID, "cs_ransac_batch: NULL argument");
  CS_REQUIRE(ransac_n >= 3 && ransac_n <= 64, CS_ERR_INVALID,
             "cs_ransac_batch: ransac_n %d not in [3, 64]", ransac_n);
  CS_REQUIRE(max_corr > 0.0 && max_iter >= 1, CS_ERR_INVALID,
             "cs_ransac_batch: need max_corr > 0 and max_iter >= 1");
  CS_REQUIRE(confidence > 0.0 && confidence <= 1.0, CS_ERR_INVALID,
             "cs_ransac_batch: confidence must be in (0, 1]");
  if (n_prob <= 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const int64_t total = h_off[n_prob] - h_off[0];
  CS_REQUIRE(h_off[0] == 0 && total >= 0, CS_ERR_INVALID, "cs_ransac_batch: bad offsets");
  CS_REQUIRE(total == 0 || (d_src && d_tgt), CS_ERR_INVALID, "cs_ransac_batch: NULL correspondences");
  RansacCall c;
  if (int rc = c.init(h_off, n_prob, max_corr, ransac_n, max_iter, confidence, seed, s)) return rc;
  if (int rc = c.setup(d_src, d_tgt)) return rc;
  if (int rc = c.open_streams()) return rc;

  // A round = front half (hypotheses, f16 rows, prefilter: independent of the carried best) + back half (survivors,
  // exact counts, scans: the sequential RANSAC state), then ONE host wait for the round's state in pinned memory.
  // Streams: the back half always runs on the caller's stream s.  The front half of round i+1 is enqueued BEFORE the host
  // waits for round i: behind it on s while the rounds are short, on the low-priority c.side once rounds i and i+1 are both
  // prefiltered (its hypothesis kernel on c.side_hyp) -- so it fills the GPU while the back half of round i (many small
  // dependent kernels) and the host turnaround run.  s waits for a side-stream front half through front_done[parity].
  Front cur = c.enqueue_front(0, 0, s);
  CS_LAUNCH_CHECK();
  bool side_pending = false;  // the side stream holds work the main stream has not waited for
  int side_par = 0;
  while (true) {
    if (cur.on_side) {
      CS_HIP_CHECK(hipStreamWaitEvent(s, c.front_done[cur.par].e, 0));
      side_pending = false;
    }
    if (int rc = c.back_half(cur)) return rc;
    // the per-problem state (est_k, done), the survivor counts and the activity counter come back in
    // one copy behind a synchronisation the chunk loop needs anyway
    CS_HIP_CHECK(hipMemcpyAsync(c.sc.h_state, c.sc.state.p, c.sc.st_bytes, hipMemcpyDeviceToHost, s));
    CS_HIP_CHECK(hipEventRecord(c.round_done.e, s));
    Front nxt;
    const int it1 = cur.it0 + cur.b;
    const bool have_next = it1 < max_iter;
    if (have_next) {
      // on the side stream once both rounds are prefiltered: before that the rounds are short and the exact count of
      // round i+1 would compete with round i
      nxt = c.enqueue_front(it1, cur.par ^ 1, (c.side && cur.pf && c.prefiltered(it1)) ? c.side : s);
      if (nxt.on_side) {
        side_pending = true;
        side_par = nxt.par;
      }
      CS_LAUNCH_CHECK();
    }
    CS_HIP_CHECK(hipEventSynchronize(c.round_done.e));   // the host's only wait of a round
    const bool active = c.read_back(cur);
    if (!active || !have_next) break;
    cur = nxt;
  }
  // a speculative front half may still be running on the side stream (its workgroups see done = 1 and
  // leave): the scratch buffers go back to the main stream's pool only behind it
  if (side_pending) CS_HIP_CHECK(hipStreamWaitEvent(s, c.front_done[side_par].e, 0));
  return c.finish(d_T, d_inliers, d_rmse, d_iters);
}

}  // extern "C"
