// What the k-NN units (knn.h: knn.hip, knn_exact.hip, knn_f16.hip), topk.hip, chamfer.hip, hardneg.hip and two ICP units
// (icp_assoc.hip: the kernels' side, icp.hip: the driver's) share: the matrix-core operand types, the f16 hi / lo cut, the
// KNF_* scan of 16-d features, the host helpers of their drivers, and the two kernels that two of them launch (each defined
// once, in one unit, and reached from the other through an ordinary host function).  The scan of 3-d points that
// chamfer.hip and the ICP units share is chf_rank.h, on top of this header.
#pragma once
#include <stdlib.h>

#include <atomic>
#include <vector>

#include "common.h"

namespace cs {

using f64x4 = __attribute__((ext_vector_type(4))) double;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ void knf_split(float v, _Float16* hi, _Float16* lo) {
  const _Float16 h = (_Float16)v;
  *hi = h;
  *lo = (_Float16)(v - (float)h);
}

// ------------------------------------------------------------------------------------------
// The f16 matrix-core shortlist scan of 16-d features, shared by k_knn_f16 (knn_f16.hip) and k_hn_f16 (hardneg.hip):
// operand rows, the LDS stage, the tile's fragments and MFMAs, the lane's ranked list and its threshold, the error
// budget.  The kernels differ only in what they do with a value below the threshold.
//   value v~ = f32(|t|^2) + sum of the 48 products th.(-2qh) + tl.(-2qh) + th.(-2ql), accumulated in f32 by three
//   v_mfma_f32_32x32x16_f16, stands for v = |t|^2 - 2 q.t = d - |q|^2.
//   rows = targets (LDS, staged by LDS-DMA from a 112-B-pitch f16 image), cols = queries (registers): a lane owns one
//   query and 16 of a tile's 32 target rows; the two lanes of a query (lane, lane ^ 32) own disjoint halves.
// Error budget: 48 f32 accumulation steps and the dropped lo*lo products relative to sum |terms| <= |q|^2 + |t|^2, the
// hi + lo split residuals, the f32 rounding of |t|^2 -- together < 2^-17 (|q|^2 + |t|^2_max); charged KNF_EPS_REL.
// Outside |q|^2, |t|^2_max < KNF_RANGE the f16 operands may overflow: nothing is trusted there.
// ------------------------------------------------------------------------------------------
constexpr int KNF_PITCH = 56;   // halfs per image row (112 B): conflict-free ds_read_b128 fragments
constexpr int KNF_ROWS = 192;   // target rows per LDS stage (6 MFMA row tiles, 21 KiB)
constexpr int KNF_STAGE_BYTES = KNF_ROWS * KNF_PITCH * 2;  // 21504
constexpr int KNF_STAGE_KIB = KNF_STAGE_BYTES / 1024;
static_assert(KNF_STAGE_BYTES % 1024 == 0, "a stage is copied in 1-KiB pieces");
constexpr double KNF_EPS_REL = 0x1.0p-15;
constexpr double KNF_RANGE = 1.0e8;

// image row of one target: [th(16) | tl(16) | th(16) | 0(8)]; returns |t|^2 (f64 fma chain)
__device__ __forceinline__ double knf_pack_target_row(const float* __restrict__ f, _Float16* __restrict__ dst) {
  union {
    _Float16 h[KNF_PITCH];
    uint4 v[7];
  } row;
  double n2 = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    _Float16 hi, lo;
    knf_split(f[c], &hi, &lo);
    row.h[c] = hi;
    row.h[16 + c] = lo;
    row.h[32 + c] = hi;
    n2 = fma((double)f[c], (double)f[c], n2);
  }
#pragma unroll
  for (int c = 48; c < KNF_PITCH; ++c) row.h[c] = (_Float16)0.0f;
  uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma unroll
  for (int c = 0; c < 7; ++c) d4[c] = row.v[c];
  return n2;
}

// operand row of one query: [-2 qh(16) | -2 qh(16) | -2 ql(16)] (scaling by 2 is exact in f16 below the range limit);
// returns |q|^2 (f64 fma chain)
__device__ __forceinline__ double knf_pack_query_row(const float* __restrict__ f, _Float16* __restrict__ dst) {
  union {
    _Float16 h[48];
    uint4 v[6];
  } row;
  double n2 = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    _Float16 hi, lo;
    knf_split(-2.0f * f[c], &hi, &lo);
    row.h[c] = hi;
    row.h[16 + c] = hi;
    row.h[32 + c] = lo;
    n2 = fma((double)f[c], (double)f[c], n2);
  }
  uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma unroll
  for (int c = 0; c < 6; ++c) d4[c] = row.v[c];
  return n2;
}

// max |t|^2 of a segment (error budget of the verification): wave maximum, then an unsigned maximum of the bit patterns
// of non-negative floats -- an integer atomic, the same in any order
__device__ __forceinline__ void knf_seg_max(float mx, unsigned* __restrict__ seg_bits) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(seg_bits, __float_as_uint(mx));
}

// LDS-DMA of one stage (KNF_ROWS image rows from row `base`) into stage buffer b: wave w of the four copies the 1-KiB
// pieces w, w + 4, ...  gimg = first image row of the segment + 16 * lane bytes.  The caller orders the data
// (s_waitcnt vmcnt(0) by every wave, then a barrier: common.h, lds_dma16).
__device__ __forceinline__ void knf_issue_dma(const char* gimg, unsigned lds_base, int wave, int b, int base) {
  const char* gp = gimg + (int64_t)base * (KNF_PITCH * 2);
#pragma unroll
  for (int i = 0; i < (KNF_STAGE_KIB + 3) / 4; ++i) {
    const int piece = wave + 4 * i;
    if (piece < KNF_STAGE_KIB) lds_dma16(gp + piece * 1024, lds_base + b * KNF_STAGE_BYTES + piece * 1024);
  }
}

// fragments of 32-row tile t of a stage: A operands of the lane's row (t * 32 + col), and the accumulator input = |t|^2 of
// the 16 rows this lane owns: (r & 3) + 8 (r >> 2) + 4 half.  tn = the stage's |t|^2 (KNF_ROWS floats, 16-B aligned).
__device__ __forceinline__ void knf_load_tile(const char* stage, const float* tn, int t, int col, int half,
                                              f16x8 (&a)[3], f32x16& c16) {
  const _Float16* arow = reinterpret_cast<const _Float16*>(stage) + (t * 32 + col) * KNF_PITCH + 8 * half;
#pragma unroll
  for (int m = 0; m < 3; ++m) a[m] = *reinterpret_cast<const f16x8*>(arow + 16 * m);
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    const float4 v = *reinterpret_cast<const float4*>(&tn[t * 32 + 8 * q4 + 4 * half]);
    c16[4 * q4 + 0] = v.x; c16[4 * q4 + 1] = v.y; c16[4 * q4 + 2] = v.z; c16[4 * q4 + 3] = v.w;
  }
}
// stage row of result element r of a tile (the row id of the value d[r])
__device__ __forceinline__ int knf_result_row(int t, int half, int r) { return t * 32 + 4 * half + (r & 3) + 8 * (r >> 2); }

// the lo parts: d = hi.hi (given) + lo.hi + hi.lo
__device__ __forceinline__ f32x16 knf_mfma_lo(const f16x8 (&a)[3], const f16x8 (&b)[3], f32x16 d) {
  d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], b[1], d, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2], b[2], d, 0, 0, 0);
}

// ordered insertion of (cd, ci) into the lane's ascending list; strict <: an equal value keeps the earlier entry
template <int KK>
__device__ __forceinline__ void knf_insert(float (&bd)[KK], int32_t (&bi)[KK], float cd, int32_t ci) {
  bool carry = false;  // once placed, the displaced tail shifts down unconditionally
#pragma unroll
  for (int s2 = 0; s2 < KK; ++s2) {
    if (carry || cd < bd[s2]) {
      carry = true;
      const float td = bd[s2];
      const int32_t ti = bi[s2];
      bd[s2] = cd;
      bi[s2] = ci;
      cd = td;
      ci = ti;
    }
  }
}
// the two lanes of a query scan disjoint halves of every tile: either one's KK-th value bounds the query's KK-th best
__device__ __forceinline__ float knf_pair_min(float t) { return fminf(t, __shfl_xor(t, 32)); }

// canonical squared distance of a 16-d query (f64) and a target row: one fma chain, columns ascending
__device__ __forceinline__ double knf_chain16(const double (&q)[16], const float* __restrict__ tp) {
  double d = 0.0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const double diff = q[e] - (double)tp[e];
    d = fma(diff, diff, d);
  }
  return d;
}

template <typename T>
static int upload(PoolBuf<T>& buf, const std::vector<T>& host, hipStream_t s) {
  if (!buf.alloc(host.size())) return CS_ERR_HIP;
  if (!host.empty())
    CS_HIP_CHECK(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(T),
                                hipMemcpyHostToDevice, s));
  // pageable source: the runtime has staged the bytes when the call returns
  return CS_OK;
}

// Environment switches are read once per call, in each family's read_options(): tests flip them between the
// calls of one process, so none is cached.  INTEGRATION.md lists them.
inline bool env_first_is(const char* name, char c) {
  const char* e = getenv(name);
  return e && e[0] == c;
}

// out[i] = sum_c X[i, c]^2, one f64 fma chain per row (k_row_norms, topk.hip).  Launch only: the caller's
// CS_LAUNCH_CHECK covers it.
void row_norms(const float* d_x, int64_t n, int d, double* d_out, hipStream_t s);

// *host_out = number of non-zero entries of flag[0, n) (k_count_flags, knn.hip).  Waits for the stream: only the
// statistics switches call it.  `who` prefixes the error text.
int count_flagged(const int32_t* d_flag, int64_t n, unsigned long long* host_out, hipStream_t s, const char* who);

// the body of every cs_*_stats getter: {items answered by the fast path, of those recomputed by its fallback}
inline void read_stats(std::atomic<unsigned long long> (&stats)[2], uint64_t out[2], int reset) {
  for (int i = 0; i < 2; ++i) {
    if (out) out[i] = stats[i].load();
    if (reset) stats[i].store(0);
  }
}

}  // namespace cs
