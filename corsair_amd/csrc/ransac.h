// What the RANSAC units share: ransac.hip (sequential replay + host driver), ransac_hyp.hip (hypotheses), ransac_prefilter.hip
// (f16 pair images, prefilter, survivors) and ransac_count.hip (exact f64 counts).  The per-problem state, the placement table,
// the geometry constants the driver sizes buffers and grids with, the canonical residual, the hypothesis-side prefilter row
// (k_ransac_hyp inlines it) and the host launch functions: every kernel is defined once, in one unit, and reached from the driver
// through an ordinary host function that picks the instantiation and launches on the stream it is given.
#pragma once
#include "common.h"

namespace cs {

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

// ---- geometry ----------------------------------------------------------------------------------
// Largest chunk of iterations per round.  One workgroup = 128 hypotheses x all pairs of a problem
// (~100 us), 1536 workgroups are resident: chunks of 16384 give >= 8 "waves" of workgroups for a
// 32-query batch, so the partially filled last wave costs ~10 % instead of ~33 % at 4096.
constexpr int BMAX = 16384;
// exact counts (ransac_count.hip)
constexpr int RC_CHUNK = 256;   // pairs per LDS stage = threads per workgroup
constexpr int RC_HYP = 256;     // hypotheses per workgroup
// prefilter (ransac_prefilter.hip)
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
constexpr int PF_S2_CAP = 1024;   // rows per problem of the second stage's compact list (= the largest list the few-survivor kernel takes)
// K = 16 form: largest |t| / smax a hypothesis may have to go through the prefilter; the others are counted exactly
// (k_ransac_pack16_b0 has the measurement behind the value).  The K = 32 form has no cap: its kernels get tcap = 0.
constexpr double PF_TCAP = 0.75;
// Survivors per problem up to which k_ransac_count_few does the exact counts; longer lists go to k_ransac_count<true>.
// (K = 32 prefilter: 32 / 64 / 128 / 256 measured, 128 the fastest by ~1 %.  The K = 16 form leaves 3 - 4x the survivors,
// ~16 per problem and round on the chair shape: the list kernel -- one workgroup of 256 hypothesis lanes per problem --
// then ran in every fourth round at 670 us.)
constexpr int FEW_MAX = 1024;

// rows of problem p in the f16 pair image: m rounded up to whole LDS stages
__host__ __device__ static inline int64_t pf_padded(int64_t m) { return (m + PF_ROWS - 1) / PF_ROWS * PF_ROWS; }

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

// ---- the canonical residual (oracle/corsair_oracle.c oc_ransac), used by k_ransac_count, k_ransac_count_few, k_ransac_err ----
//   p_c = fma(r_c2, sz, fma(r_c1, sy, fma(r_c0, sx, t_c))),  d_c = p_c - q_c,  |d|^2 = fma(dz, dz, fma(dy, dy, dx dx))
__device__ __forceinline__ double residual2_f64(const double (&R)[12], double sx, double sy, double sz,
                                                double qx, double qy, double qz) {
  const double dx = fma(R[2], sz, fma(R[1], sy, fma(R[0], sx, R[3]))) - qx;
  const double dy = fma(R[6], sz, fma(R[5], sy, fma(R[4], sx, R[7]))) - qy;
  const double dz = fma(R[10], sz, fma(R[9], sy, fma(R[8], sx, R[11]))) - qz;
  return fma(dz, dz, fma(dy, dy, dx * dx));
}

// ---- hypothesis side of the prefilter (the pair side and the bound itself: ransac_prefilter.hip) -----------------------------
// f64 -> f16 through f32 (v_cvt_f32_f64 + v_cvt_f16_f32).  gfx950 has no direct conversion: `(_Float16)double` is a
// ~25-instruction integer sequence, and the prefilter's operand kernels make 16 - 32 of them per hypothesis and per pair (a sixth
// of k_ransac_hyp's instructions).  The two roundings can differ from the single one by one f16 ulp in rare ties; nothing
// below assumes a correctly rounded value -- every bound is computed from the value this function RETURNS (|x - f16_of(x)|),
// and its relative error 2^-11 + 2^-24 sits inside the constants' slack (2.002 for 2 sqrt(1.001), 1.0005).
__device__ __forceinline__ _Float16 f16_of(double v) { return (_Float16)(float)v; }

// the per-problem means of the source and target points (k_ransac_pair_sums): the prefilter works in centred coordinates
__device__ __forceinline__ void pf_centre(const double* __restrict__ sums, int p, double (&mu)[6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) mu[c] = sums[p * 6 + c];
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
    pf_centre(sums, p, mu);
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

// ---- host launch functions, each next to its kernels ---------------------------------------------------------------------------
// The call's problem table and packed pairs, as the launch functions take them.
struct RansacIn {
  RansacProb* probs;
  int n_prob, m_max;
  int64_t tot1;      // pairs of the call (1 when it has none): the stride of pk
  float* pk;         // SoA copy of the correspondences
  float4* pair32;    // 32-B rows for the sampling
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

// ransac_hyp.hip.  A16 != nullptr: a prefiltered round, the hypotheses' prefilter rows are written too
void ransac_launch_pack(const RansacIn& in, const float* src, const float* tgt, hipStream_t s);   // (call without prefilter)
void ransac_launch_hyp(const RansacIn& in, const Front& f, int ransac_n, uint64_t seed, int force_jacobi, double* hyp,
                       const unsigned* pf_stat, const double* pf_sums, double thr2, double tcap, _Float16* A16, float* c_h,
                       int32_t* cnt_zero, hipStream_t s);
// ransac_prefilter.hip.  Set-up of a prefiltered call: k_ransac_pair_sums -> k_ransac_images (B32 may be null) ->
// k_ransac_pack16_b0 (B16 != nullptr: the K = 16 form)
void ransac_launch_images(const RansacIn& in, const int64_t* off16, const float* src, const float* tgt, double* sums,
                          unsigned* stat, unsigned long long* chk_stats, _Float16* B32, _Float16* B16, double tcap,
                          hipStream_t s);
// nm = MFMAs per tile (2: K = 32, 1: K = 16).  n_list == nullptr: the chunk f.it0 .. + f.b, rows of BMAX per problem;
// otherwise the second stage over compact lists of PF_S2_CAP rows.  Returns the number of workgroups.
unsigned ransac_launch_prefilter(int nm, const RansacIn& in, const int64_t* off16, const _Float16* B, const _Float16* A16,
                                 const float* c_h, const Front& f, int tiles, int splits, int32_t* cnt_up,
                                 unsigned long long* trace, const int32_t* n_list, hipStream_t s);
void ransac_launch_survivors(const RansacIn& in, const Front& f, const int32_t* cnt_up, int32_t* res_cnt,
                             unsigned long long* err_by_h, int32_t* hlist, int32_t* n_surv, const Stage2Rows& s2, hipStream_t s);
// CS_RANSAC_CHECK: k_ransac_check_bound and (cnt2 != nullptr) k_ransac_check_bound2
void ransac_launch_check(const RansacIn& in, const Front& f, const int32_t* exact, const int32_t* cnt_up, const int32_t* hlist,
                         const int32_t* n_surv, const int32_t* cnt2, unsigned long long* stats, hipStream_t s);
// ransac_count.hip.  Whole chunk: hpw = hypotheses per workgroup (64 or RC_HYP), grid of tiles x splits per problem
void ransac_launch_count_chunk(const RansacIn& in, const double* hyp, int it0, int b, int hpw, int tiles, int splits,
                               double thr2, int32_t* res_cnt, hipStream_t s);
void ransac_launch_count_list(const RansacIn& in, const double* hyp, int it0, int b, double thr2, int32_t* res_cnt,
                              const int32_t* hlist, const int32_t* n_surv, hipStream_t s);
void ransac_launch_count_few(const RansacIn& in, const double* hyp, double thr2, double scale, int32_t* res_cnt,
                             unsigned long long* err_by_h, const int32_t* hlist, const int32_t* n_surv, int fslots,
                             const int32_t* cnt2, hipStream_t s);
void ransac_launch_err(const RansacIn& in, const double* hyp, const int32_t* cand, double thr2, double scale,
                       unsigned long long* cand_err, hipStream_t s);

}  // namespace cs
