// RANSAC f16 prefilter (see ransac.hip for the round it belongs to): the pair images of a call (k_ransac_pair_sums,
// k_ransac_images, k_ransac_pack16_b0), the bound itself on the matrix cores (k_ransac_prefilter), the compaction of the
// survivors (k_ransac_survivors) and the CS_RANSAC_CHECK kernels.  The hypothesis rows are written by k_ransac_hyp
// (pf_emit_row, ransac.h, with the error budget eps_h).
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
#include <math.h>

#include "ransac.h"

namespace cs {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

__device__ __forceinline__ void split16(double v, _Float16* hi, _Float16* lo) {
  const _Float16 h = f16_of(v);
  *hi = h;
  *lo = f16_of(v - (double)h);
}

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
  // fmax drops a NaN operand: a pair with a NaN on ONE side would pass for the other side's norm, its NaN row would enter
  // the image, and one NaN result ruins the add-based sign counter of k_ransac_prefilter<1, true> for every pair after it.
  // b_0 = ss + qq is NaN as soon as either side is.
  return 1.0000002f * (float)sqrt(b[0] == b[0] ? fmax(ss, qq) : b[0]);
}

// pair side: 80-B rows [bh(0..15) | bl(0..15) | 8 x 0] in exactly the layout the prefilter keeps in LDS
// (a stage is one contiguous 15-KiB copy); every problem is padded to whole stages with rows whose d~^2
// is +60000 (never counted).  stat[p] = {largest point norm, max |b_k| (k = 0..15)} of problem p as
// float bit patterns (non-negative floats order like their bits), rounded up.
// grid: x = blocks over the rows of a problem (grid-stride), y = problem; off16[p] = first row.
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
  pf_centre(sums, blockIdx.y, mu);
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
  pf_centre(sums, blockIdx.y, mu);
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

void ransac_launch_images(const RansacIn& in, const int64_t* off16, const float* src, const float* tgt, double* sums,
                          unsigned* stat, unsigned long long* chk_stats, _Float16* B32, _Float16* B16, double tcap,
                          hipStream_t s) {
  // three launches: means (+ cleared statistics) -> packed pairs, K = 32 image and the per-problem maxima -> (K = 16) the
  // one-MFMA image, whose constant term takes the per-pair bound of the dropped term and needs the problem's smax.  The
  // first two read src / tgt once each, the third the packed pairs.
  int pblocks = (int)ceil_div(in.m_max > 0 ? in.m_max : 1, 256);
  if (pblocks > 64) pblocks = 64;
  const dim3 pgrid((unsigned)pblocks, (unsigned)in.n_prob);
  hipLaunchKernelGGL(k_ransac_pair_sums, dim3((unsigned)in.n_prob), dim3(256), 0, s, in.probs, src, tgt, sums, stat, chk_stats);
  hipLaunchKernelGGL(k_ransac_images, pgrid, dim3(256), 0, s, in.probs, off16, src, tgt, sums, in.tot1, in.pk, in.pair32, B32,
                     stat);
  if (B16)
    hipLaunchKernelGGL(k_ransac_pack16_b0, pgrid, dim3(256), 0, s, in.probs, off16, in.pair32, sums, stat, tcap, B16);
}

unsigned ransac_launch_prefilter(int nm, const RansacIn& in, const int64_t* off16, const _Float16* B, const _Float16* A16,
                                 const float* c_h, const Front& f, int tiles, int splits, int32_t* cnt_up,
                                 unsigned long long* trace, const int32_t* n_list, hipStream_t s) {
  const unsigned nblk = (unsigned)(8 * f.pslots * tiles * splits);
  const int it0 = n_list ? 0 : f.it0, b = n_list ? PF_S2_CAP : f.b, bmax = n_list ? PF_S2_CAP : BMAX;
  const auto kernel = nm == 2 ? k_ransac_prefilter<2, false> : k_ransac_prefilter<1, true>;
  hipLaunchKernelGGL(kernel, dim3(nblk), dim3(256), 0, s, in.probs, off16, B, A16, c_h, it0, b, bmax, splits, f.xcd_prob,
                     f.xtab, f.pslots, tiles, cnt_up, trace, n_list);
  return nblk;
}

void ransac_launch_survivors(const RansacIn& in, const Front& f, const int32_t* cnt_up, int32_t* res_cnt,
                             unsigned long long* err_by_h, int32_t* hlist, int32_t* n_surv, const Stage2Rows& s2, hipStream_t s) {
  hipLaunchKernelGGL(k_ransac_survivors, dim3((unsigned)((f.b + 255) / 256), (unsigned)in.n_prob), dim3(256), 0, s, in.probs,
                     cnt_up, f.it0, f.b, BMAX, res_cnt, err_by_h, hlist, n_surv, s2);
}

void ransac_launch_check(const RansacIn& in, const Front& f, const int32_t* exact, const int32_t* cnt_up, const int32_t* hlist,
                         const int32_t* n_surv, const int32_t* cnt2, unsigned long long* stats, hipStream_t s) {
  hipLaunchKernelGGL(k_ransac_check_bound, dim3((unsigned)((f.b + 255) / 256), (unsigned)in.n_prob), dim3(256), 0, s, in.probs,
                     exact, cnt_up, f.it0, f.b, BMAX, stats);
  if (cnt2)
    hipLaunchKernelGGL(k_ransac_check_bound2, dim3(PF_S2_CAP / 256, (unsigned)in.n_prob), dim3(256), 0, s, in.probs, exact,
                       hlist, n_surv, BMAX, cnt2, stats);
}
}  // namespace cs
