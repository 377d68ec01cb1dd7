// Scan cleaning: the mean distance to the k nearest rows of a row's own segment, the statistical filter on
// those means, and the count of rows inside a radius.  The specifications are the comments of cs_knn_mean_dist,
// cs_outlier_statistical and cs_outlier_radius in include/corsair_hip.h; tests/outlier_ref.py restates them bit for bit.
//
// The definitions (k_out_mean, k_out_count) are normals.hip's exhaustive scan: one thread per row, 256 rows of one segment
// per workgroup, the segment staged through LDS 512 rows at a time.  Both results are functions of the MULTISET of the
// row's d2 values -- tied rows contribute equal terms -- so the ranked list holds d2 only, no row indices: 2 KC list
// registers where k_normals holds 3 KC, and an insertion that needs no tie rule.
// The grid paths probe the sorted cell grid that normals.hip builds (normals_grid.h, cg_probe of cellgrid.h): the radius
// count on the hybrid grid (complete by cellgrid.h's argument), the mean distance on the bounding-box grid with the k-NN
// voucher (the argument above nrm_seg_of in normals.hip: a list whose k-th d2 lies strictly inside cov2 is the scan's);
// rows the voucher refuses go to a redo list that k_out_mean_redo answers by the scan, one wave per row.
// The radius count (k_out_count, k_out_count_grid), the work list and the offset check stand in outlier_count.h, which
// dbscan.hip includes too: the count is cs_dbscan's first pass.
#include <math.h>

#include <algorithm>
#include <vector>

#include "cellgrid.h"
#include "nn_common.h"
#include "normals_grid.h"
#include "outlier_count.h"

namespace cs {
namespace {

constexpr int OUT_REDO_BLOCKS = 2048;

// A segment of fewer rows than this goes to the exhaustive mean-distance kernel: NRM_KNN_GRID_MIN of normals.hip (two LDS
// stages of the scan), taken over as it is (OUT_GRID_MIN, the radius count's, is in outlier_count.h).  Not tuned.
constexpr int OUT_KNN_GRID_MIN = 2 * OUT_TT + 1;

// d enters the ascending list; d < bd[KC - 1] is the caller's test.  Equal values are interchangeable: no tie rule.
template <int KC>
__device__ __forceinline__ void out_insert(double (&bd)[KC], double d) {
  bd[KC - 1] = d;
#pragma unroll
  for (int s = KC - 1; s >= 1; --s) {
    const bool sw = bd[s] < bd[s - 1];
    const double lo = sw ? bd[s] : bd[s - 1], hi = sw ? bd[s - 1] : bd[s];
    bd[s - 1] = lo;
    bd[s] = hi;
  }
}

// mean = (((+0 + sqrt(d2_0)) + sqrt(d2_1)) + ...) / (double)c over the c = min(k, found) smallest d2, ascending; NaN for c = 0
template <int KC>
__device__ __forceinline__ double out_mean(const double (&bd)[KC], int k) {
  double sum = 0.0;
  int c = 0;
#pragma unroll
  for (int s = 0; s < KC; ++s) {
    if (s < k && bd[s] < INFINITY) {
      sum = sum + sqrt(bd[s]);
      ++c;
    }
  }
  return c ? sum / (double)c : __longlong_as_double(0x7ff8000000000000LL);
}

// gate (optional): the workgroups of a segment that the grid answers (gate[wk.seg].cell > 0) leave at once.
template <int KC>
__global__ __launch_bounds__(OUT_ROWS) void k_out_mean(const OutWork* __restrict__ work, const float* __restrict__ xyz,
                                                       int k, double* __restrict__ mean,
                                                       const NrmSeg* __restrict__ gate) {
  __shared__ float t_lds[OUT_TT * 3];
  const OutWork wk = work[blockIdx.x];
  if (gate && gate[wk.seg].cell > 0.0) return;
  const int tid = threadIdx.x;
  const int row = wk.r0 + tid;
  const bool active = row < wk.sn;
  const float* seg = xyz + wk.seg0 * 3;
  double x = 0, y = 0, z = 0;
  if (active) {
    x = (double)seg[3 * (int64_t)row + 0];
    y = (double)seg[3 * (int64_t)row + 1];
    z = (double)seg[3 * (int64_t)row + 2];
  }
  double bd[KC];
#pragma unroll
  for (int s = 0; s < KC; ++s) bd[s] = INFINITY;
  for (int tbase = 0; tbase < wk.sn; tbase += OUT_TT) {
    const int tcount = min(OUT_TT, wk.sn - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * 3; i += OUT_ROWS) t_lds[i] = seg[(int64_t)tbase * 3 + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) {
      const double d = out_d2(t_lds + 3 * j, x, y, z);
      if (d < bd[KC - 1]) out_insert<KC>(bd, d);   // false for NaN and +inf: never a neighbour
    }
  }
  if (active) mean[wk.seg0 + row] = out_mean<KC>(bd, k);
}

// ---- the grid paths --------------------------------------------------------------------------------------------------
// One thread per sorted row of the chunk (k_normals_grid's shape: the lanes of a wave probe the same cells); the answer goes
// back to the row's own place.  A list of fewer than k entries below the segment's cov2 is not accepted (the voucher) and
// the row goes to the redo list; stats (optional) counts the rows of grid segments.
template <int KC>
__global__ __launch_bounds__(OUT_ROWS) void k_out_mean_grid(CellTable tb, const float* __restrict__ sxyz,
                                                            const int32_t* __restrict__ sj,
                                                            const uint64_t* __restrict__ skeys, int64_t m_total,
                                                            const int64_t* __restrict__ off,
                                                            const NrmSeg* __restrict__ segs, int k,
                                                            double* __restrict__ mean, int32_t* __restrict__ redo,
                                                            unsigned* __restrict__ redo_count,
                                                            unsigned long long* __restrict__ stats) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= m_total) return;
  const int p = (int)(skeys[m] >> 48);
  const NrmSeg sg = segs[p];
  if (!(sg.cell > 0.0)) return;
  if (stats) {   // one atomic per wave
    const unsigned long long mask = __ballot(1);
    if ((int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(&stats[0], (unsigned long long)__popcll(mask));
  }
  const double x = (double)sxyz[3 * m], y = (double)sxyz[3 * m + 1], z = (double)sxyz[3 * m + 2];
  double bd[KC];
#pragma unroll
  for (int s = 0; s < KC; ++s) bd[s] = INFINITY;
  cg_probe<3>(
      tb, sxyz, p, x, y, z, sg.cell, sg.r2, [&](const float* t) { return out_d2(t, x, y, z); },
      [&](double d, int32_t) {
        if (d < bd[KC - 1]) out_insert<KC>(bd, d);
      });
  bool full = false;
#pragma unroll
  for (int s = 0; s < KC; ++s)
    if (s == k - 1) full = bd[s] < INFINITY;
  if (!full) {
    redo[atomicAdd(redo_count, 1u)] = (int32_t)m;   // at most m_total entries: every row is listed at most once
    return;
  }
  mean[off[p] + sj[m]] = out_mean<KC>(bd, k);
}

// The rows of the redo list, one wave per row, by the exhaustive scan of the row's segment (k_normals_redo's staging): lane l
// ranks the rows l, l + 64, ... into its own ascending list.  The 64 lists are then merged by extraction: k times, the
// wave takes the minimum of the lists' heads, adds its square root to the sum -- out_mean's chain, the terms in ascending
// order of d2 -- and the first lane that holds it drops its head.  No list leaves the registers.  A fixed-size launch:
// the workgroups beyond the count leave at once.
template <int KC>
__global__ __launch_bounds__(64) void k_out_mean_redo(const int32_t* __restrict__ redo,
                                                      const unsigned* __restrict__ redo_count,
                                                      const float* __restrict__ sxyz, const int32_t* __restrict__ sj,
                                                      const uint64_t* __restrict__ skeys, const float* __restrict__ xyz,
                                                      const int64_t* __restrict__ off, int k, double* __restrict__ mean,
                                                      unsigned long long* __restrict__ stats) {
  __shared__ float t_lds[OUT_TT * 3];
  const unsigned count = *redo_count;
  const int lane = threadIdx.x;
  if (stats && blockIdx.x == 0 && lane == 0) atomicAdd(&stats[1], (unsigned long long)count);
  for (unsigned u = blockIdx.x; u < count; u += gridDim.x) {
    const int32_t m = redo[u];
    const int p = (int)(skeys[m] >> 48);
    const int64_t seg0 = off[p];
    const int sn = (int)(off[p + 1] - seg0);
    const float* seg = xyz + seg0 * 3;
    const double x = (double)sxyz[3 * (int64_t)m], y = (double)sxyz[3 * (int64_t)m + 1], z = (double)sxyz[3 * (int64_t)m + 2];
    double bd[KC];
#pragma unroll
    for (int s = 0; s < KC; ++s) bd[s] = INFINITY;
    for (int tbase = 0; tbase < sn; tbase += OUT_TT) {
      const int tcount = min(OUT_TT, sn - tbase);
      __syncthreads();
      for (int i = lane; i < tcount * 3; i += 64) t_lds[i] = seg[(int64_t)tbase * 3 + i];
      __syncthreads();
      for (int j = lane; j < tcount; j += 64) {
        const double d = out_d2(t_lds + 3 * j, x, y, z);
        if (d < bd[KC - 1]) out_insert<KC>(bd, d);   // false for NaN and +inf: never a neighbour
      }
    }
    double sum = 0.0;
    int c = 0;
    for (int t = 0; t < k; ++t) {
      double mn = bd[0];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double other = __shfl_xor(mn, o);
        mn = other < mn ? other : mn;
      }
      if (!(mn < INFINITY)) break;   // the same in every lane: fewer than k rows were found
      sum = sum + sqrt(mn);
      ++c;
      const unsigned long long holders = __ballot(bd[0] == mn);
      if (lane == __ffsll((long long)holders) - 1) {
#pragma unroll
        for (int s = 0; s + 1 < KC; ++s) bd[s] = bd[s + 1];
        bd[KC - 1] = INFINITY;
      }
    }
    if (lane == 0) mean[seg0 + sj[m]] = c ? sum / (double)c : __longlong_as_double(0x7ff8000000000000LL);
  }
}

// ---- the statistic ---------------------------------------------------------------------------------------------------
// acc = five u64 per segment, zeroed by the caller: [0] the bit pattern of M (non-negative doubles order like their bits),
// [1] n_valid, [2] S1, [3] S2lo, [4] S2hi.  Integer atomics only: the same values for any order and launch shape.
constexpr int OUT_ACC = 5;

__device__ __forceinline__ bool out_valid(double m) { return m >= 0.0 && m < INFINITY; }   // false for NaN

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(OUT_ROWS) void k_out_max(const OutWork* __restrict__ work, const double* __restrict__ mean,
                                                      unsigned long long* __restrict__ acc) {
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  const double m = row < wk.sn ? mean[wk.seg0 + row] : -1.0;
  const bool ok = out_valid(m);
  unsigned long long bits = ok ? (unsigned long long)__double_as_longlong(m + 0.0) : 0ull;   // -0 + 0 = +0
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(bits, o);
    bits = other > bits ? other : bits;
  }
  const unsigned long long cnt = (unsigned long long)__popcll(__ballot(ok));
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicMax(&acc[OUT_ACC * (int64_t)wk.seg + 0], bits);
    atomicAdd(&acc[OUT_ACC * (int64_t)wk.seg + 1], cnt);
  }
}

// s = min(31 - e, 1023) for M = f 2^e, f in [0.5, 1); 31 for M = 0
__device__ __forceinline__ int out_shift(double M) {
  int e = 0;
  if (M > 0.0) frexp(M, &e);
  return min(31 - e, 1023);
}

__global__ __launch_bounds__(OUT_ROWS) void k_out_sums(const OutWork* __restrict__ work, const double* __restrict__ mean,
                                                       unsigned long long* __restrict__ acc) {
  const OutWork wk = work[blockIdx.x];
  unsigned long long* a = acc + OUT_ACC * (int64_t)wk.seg;
  const int s = out_shift(__longlong_as_double((long long)a[0]));
  const int row = wk.r0 + threadIdx.x;
  const double m = row < wk.sn ? mean[wk.seg0 + row] : -1.0;
  const bool ok = out_valid(m);
  const unsigned long long q = ok ? (unsigned long long)rint(ldexp(m, s)) : 0ull;   // <= 2^31
  const unsigned long long q2 = q * q;                                               // <= 2^62
  const unsigned long long s1 = wave_sum(q), lo = wave_sum(q2 & 0xffffffffull), hi = wave_sum(q2 >> 32);
  if ((threadIdx.x & 63) == 0 && (s1 | lo | hi)) {
    atomicAdd(&a[2], s1);
    atomicAdd(&a[3], lo);
    atomicAdd(&a[4], hi);
  }
}

// One thread per segment: (n_valid, mu, sigma, tau) by the header's sequence.
__global__ void k_out_finish(const unsigned long long* __restrict__ acc, int n_seg, double std_ratio,
                             double* __restrict__ stat) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_seg) return;
  const unsigned long long* a = acc + OUT_ACC * (int64_t)p;
  const double M = __longlong_as_double((long long)a[0]);
  const unsigned long long n = a[1], S1 = a[2], S2lo = a[3], S2hi = a[4];
  const int s = out_shift(M);
  double mu = 0.0, sigma = 0.0;
  if (n >= 1 && M > 0.0) mu = ldexp((double)S1 / (double)n, -s);
  if (n >= 2 && M > 0.0) {
    const unsigned __int128 S2 = ((unsigned __int128)S2hi << 32) + (unsigned __int128)S2lo;
    const unsigned __int128 D = (unsigned __int128)n * S2 - (unsigned __int128)S1 * (unsigned __int128)S1;
    const unsigned long long dhi = (unsigned long long)(D >> 64), dlo = (unsigned long long)D;
    const double dd = (double)dhi * 0x1.0p64 + (double)dlo;   // split by hand: no library conversion of 128 bits
    const double den = (double)n * (double)(n - 1);
    sigma = ldexp(sqrt(dd / den), -s);
  }
  stat[4 * (int64_t)p + 0] = (double)n;
  stat[4 * (int64_t)p + 1] = mu;
  stat[4 * (int64_t)p + 2] = sigma;
  stat[4 * (int64_t)p + 3] = fma(std_ratio, sigma, mu);
}

__global__ __launch_bounds__(OUT_ROWS) void k_out_keep(const OutWork* __restrict__ work, const double* __restrict__ mean,
                                                       const double* __restrict__ stat, uint8_t* __restrict__ keep) {
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  if (row >= wk.sn) return;
  const double tau = stat[4 * (int64_t)wk.seg + 3];
  const double m = mean[wk.seg0 + row];
  keep[wk.seg0 + row] = (m > 0.0 && m < tau) ? 1 : 0;   // false for a NaN mean
}

// ---- host ------------------------------------------------------------------------------------------------------------
std::atomic<unsigned long long> g_outlier_stats[2];

void launch_mean(const OutWork* d_work, size_t n_work, const float* d_xyz, int k, double* d_mean, const NrmSeg* gate,
                 hipStream_t s) {
  const dim3 grid((unsigned)n_work), block(OUT_ROWS);
  if (k <= 8)
    hipLaunchKernelGGL(k_out_mean<8>, grid, block, 0, s, d_work, d_xyz, k, d_mean, gate);
  else if (k <= 16)
    hipLaunchKernelGGL(k_out_mean<16>, grid, block, 0, s, d_work, d_xyz, k, d_mean, gate);
  else
    hipLaunchKernelGGL(k_out_mean<32>, grid, block, 0, s, d_work, d_xyz, k, d_mean, gate);
}

template <int KC>
void launch_mean_grid(const NrmGrid& gr, const float* d_xyz, int k, double* d_mean, int32_t* redo, unsigned* redo_count,
                      unsigned long long* stats, hipStream_t s) {
  hipLaunchKernelGGL(k_out_mean_grid<KC>, dim3((unsigned)ceil_div(gr.m_total, OUT_ROWS)), dim3(OUT_ROWS), 0, s, gr.table(),
                     (const float*)gr.sxyz.p, (const int32_t*)gr.sj.p, (const uint64_t*)gr.skeys.p, gr.m_total,
                     (const int64_t*)gr.doff.p, (const NrmSeg*)gr.segs.p, k, d_mean, redo, redo_count, stats);
  hipLaunchKernelGGL(k_out_mean_redo<KC>, dim3(OUT_REDO_BLOCKS), dim3(64), 0, s, (const int32_t*)redo,
                     (const unsigned*)redo_count, (const float*)gr.sxyz.p, (const int32_t*)gr.sj.p,
                     (const uint64_t*)gr.skeys.p, d_xyz, (const int64_t*)gr.doff.p, k, d_mean, stats);
}

// The grid path over one chunk of segments (normals_grid.h); every launch is enqueued on s, nothing waits.
// knn: the mean distance (the segments' cells come from their boxes, rows the voucher refuses are recomputed, and the
// exhaustive kernel runs gated over every segment of grid_min rows or more: the workgroups of a segment on the grid leave
// at once); else the radius count.
int grid_chunk(bool knn, const float* d_xyz, const int64_t* h_off, int n_seg, int grid_min, double cell, double r2, int k,
               double* d_mean, int nb_points, int32_t* d_count, uint8_t* d_keep, unsigned long long* d_stats,
               hipStream_t s) {
  const char* who = knn ? "cs_knn_mean_dist: scratch allocation failed" : "cs_outlier_radius: scratch allocation failed";
  NrmGrid gr;
  int rc = nrm_grid_build(gr, d_xyz, h_off, n_seg, grid_min, knn ? k : 0, cell, r2, s, who);
  if (rc) return rc;
  if (!knn) {
    hipLaunchKernelGGL(k_out_count_grid, dim3((unsigned)ceil_div(gr.m_total, OUT_ROWS)), dim3(OUT_ROWS), 0, s, gr.table(),
                       (const float*)gr.sxyz.p, (const int32_t*)gr.sj.p, (const uint64_t*)gr.skeys.p, gr.m_total,
                       (const int64_t*)gr.doff.p, (const NrmSeg*)gr.segs.p, nb_points, d_count, d_keep);
    CS_LAUNCH_CHECK();
    return CS_OK;
  }
  PoolBuf<int32_t> redo(gr.m_total);
  PoolBuf<unsigned> redo_count(1);
  CS_REQUIRE(redo.p && redo_count.p, CS_ERR_HIP, "%s", who);
  CS_HIP_CHECK(hipMemsetAsync(redo_count.p, 0, sizeof(unsigned), s));
  if (k <= 8)
    launch_mean_grid<8>(gr, d_xyz, k, d_mean, redo.p, redo_count.p, d_stats, s);
  else if (k <= 16)
    launch_mean_grid<16>(gr, d_xyz, k, d_mean, redo.p, redo_count.p, d_stats, s);
  else
    launch_mean_grid<32>(gr, d_xyz, k, d_mean, redo.p, redo_count.p, d_stats, s);
  CS_LAUNCH_CHECK();
  std::vector<OutWork> work;   // the exhaustive kernel for the segments the device kept off the grid
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    if (sn >= grid_min) push_work(work, h_off[sg], sn, sg);
  }
  PoolBuf<OutWork> dwork;
  rc = upload(dwork, work, s);
  if (rc) return rc;
  launch_mean(dwork.p, work.size(), d_xyz, k, d_mean, gr.segs.p, s);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// the chunks of a call that hold a segment of grid_min rows or more, one grid_chunk each
int grid_chunks(bool knn, const float* d_xyz, const int64_t* h_off, int n_seg, int grid_min, double cell, double r2, int k,
                double* d_mean, int nb_points, int32_t* d_count, uint8_t* d_keep, unsigned long long* d_stats,
                hipStream_t s) {
  for (int sg0 = 0; sg0 < n_seg;) {
    bool any = false;
    const int sg1 = next_chunk(h_off, n_seg, sg0, grid_min, &any);
    if (any) {
      const int rc = grid_chunk(knn, d_xyz, h_off + sg0, sg1 - sg0, grid_min, cell, r2, k, d_mean, nb_points, d_count,
                                d_keep, d_stats, s);
      if (rc) return rc;
    }
    sg0 = sg1;
  }
  return CS_OK;
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_knn_mean_dist(const float* d_xyz, const int64_t* h_off, int n_seg, int k, double* d_mean, void* stream) {
  int64_t rows = 0;
  int rc = check_segments("cs_knn_mean_dist", h_off, n_seg, &rows);
  if (rc) return rc;
  CS_REQUIRE(k >= 2 && k <= 32, CS_ERR_UNSUPPORTED, "cs_knn_mean_dist: k outside [2, 32]");
  if (rows == 0) return CS_OK;
  CS_REQUIRE(d_xyz && d_mean, CS_ERR_INVALID, "cs_knn_mean_dist: NULL argument");
  const bool use_grid = !env_first_is("CS_OUTLIER_GRID", '0');
  const bool want_stats = use_grid && env_first_is("CS_OUTLIER_STATS", '1');
  std::vector<OutWork> work;
  int64_t grid_rows = 0;
  double flop = 0.0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    flop += 8.0 * (double)sn * (double)sn;   // the definition's work, whichever path answers
    if (use_grid && sn >= OUT_KNN_GRID_MIN)
      grid_rows += sn;
    else
      push_work(work, h_off[sg], sn, sg);
  }
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<OutWork> dwork;
  if (!work.empty()) {
    rc = upload(dwork, work, s);
    if (rc) return rc;
  }
  PoolBuf<unsigned long long> dstats;
  if (want_stats && grid_rows > 0) {
    CS_REQUIRE(dstats.alloc(2), CS_ERR_HIP, "cs_knn_mean_dist: scratch allocation failed");
    CS_HIP_CHECK(hipMemsetAsync(dstats.p, 0, 2 * sizeof(unsigned long long), s));
  }
  {
    ProfScope prof("outlier", s, flop);
    if (!work.empty()) {
      launch_mean(dwork.p, work.size(), d_xyz, k, d_mean, nullptr, s);
      CS_LAUNCH_CHECK();
    }
    if (grid_rows > 0) {
      rc = grid_chunks(true, d_xyz, h_off, n_seg, OUT_KNN_GRID_MIN, 0.0, 0.0, k, d_mean, 0, nullptr, nullptr, dstats.p, s);
      if (rc) return rc;
    }
  }
  if (dstats.p) {
    unsigned long long h[2] = {0, 0};
    CS_HIP_CHECK(download_async(h, dstats.p, sizeof(h), s));
    CS_HIP_CHECK(download_sync(s));
    g_outlier_stats[0] += h[0];
    g_outlier_stats[1] += h[1];
  }
  return CS_OK;
}

int cs_outlier_statistical(const double* d_mean, const int64_t* h_off, int n_seg, double std_ratio, uint8_t* d_keep,
                           double* d_stat, void* stream) {
  int64_t rows = 0;
  int rc = check_segments("cs_outlier_statistical", h_off, n_seg, &rows);
  if (rc) return rc;
  CS_REQUIRE(std_ratio >= 0.0 && std_ratio <= 1.7976931348623157e308, CS_ERR_INVALID,
             "cs_outlier_statistical: std_ratio must be finite and >= 0");
  if (n_seg == 0) return CS_OK;
  CS_REQUIRE(d_stat, CS_ERR_INVALID, "cs_outlier_statistical: NULL argument");
  CS_REQUIRE(rows == 0 || (d_mean && d_keep), CS_ERR_INVALID, "cs_outlier_statistical: NULL argument");
  std::vector<OutWork> work;
  for (int sg = 0; sg < n_seg; ++sg) push_work(work, h_off[sg], h_off[sg + 1] - h_off[sg], sg);
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<OutWork> dwork;
  PoolBuf<unsigned long long> acc((size_t)OUT_ACC * n_seg);
  CS_REQUIRE(acc.p, CS_ERR_HIP, "cs_outlier_statistical: scratch allocation failed");
  if (!work.empty()) {
    rc = upload(dwork, work, s);
    if (rc) return rc;
  }
  CS_HIP_CHECK(hipMemsetAsync(acc.p, 0, (size_t)OUT_ACC * n_seg * sizeof(unsigned long long), s));
  ProfScope prof("outlier", s, 8.0 * (double)rows);
  const dim3 grid((unsigned)work.size()), block(OUT_ROWS);
  if (!work.empty()) {
    hipLaunchKernelGGL(k_out_max, grid, block, 0, s, (const OutWork*)dwork.p, d_mean, acc.p);
    hipLaunchKernelGGL(k_out_sums, grid, block, 0, s, (const OutWork*)dwork.p, d_mean, acc.p);
  }
  hipLaunchKernelGGL(k_out_finish, dim3((unsigned)ceil_div(n_seg, 256)), dim3(256), 0, s,
                     (const unsigned long long*)acc.p, n_seg, std_ratio, d_stat);
  if (!work.empty())
    hipLaunchKernelGGL(k_out_keep, grid, block, 0, s, (const OutWork*)dwork.p, d_mean, (const double*)d_stat, d_keep);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

int cs_outlier_radius(const float* d_xyz, const int64_t* h_off, int n_seg, double radius, int nb_points, int32_t* d_count,
                      uint8_t* d_keep, void* stream) {
  int64_t rows = 0;
  int rc = check_segments("cs_outlier_radius", h_off, n_seg, &rows);
  if (rc) return rc;
  CS_REQUIRE(radius > 0.0 && radius <= 1.7976931348623157e308, CS_ERR_INVALID,
             "cs_outlier_radius: radius must be positive and finite");
  CS_REQUIRE(nb_points >= 0, CS_ERR_INVALID, "cs_outlier_radius: negative nb_points");
  if (rows == 0) return CS_OK;
  CS_REQUIRE(d_xyz && d_count, CS_ERR_INVALID, "cs_outlier_radius: NULL argument");
  const double r2 = radius * radius;   // +inf for a radius above 1.3e154: every finite d2 passes; 0 below 1.5e-162: none
  const double cell = radius * (1.0 + 1.0 / 1024.0);   // a little larger than the radius (cellgrid.h)
  // (a cell size near the top of the f64 range could round up to +inf: such a radius bounds nothing, the scan serves it)
  const bool use_grid = !env_first_is("CS_OUTLIER_GRID", '0') && radius < 1e300;
  const bool want_stats = use_grid && env_first_is("CS_OUTLIER_STATS", '1');
  std::vector<OutWork> work;
  int64_t grid_rows = 0;
  double flop = 0.0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    if (use_grid && sn >= OUT_GRID_MIN) {
      grid_rows += sn;
      flop += 8.0 * 27.0 * (double)sn;   // nominal: the cells' occupancy is not known on the host
    } else {
      push_work(work, h_off[sg], sn, sg);
      flop += 8.0 * (double)sn * (double)sn;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<OutWork> dwork;
  if (!work.empty()) {
    rc = upload(dwork, work, s);
    if (rc) return rc;
  }
  ProfScope prof("outlier", s, flop);
  if (!work.empty()) {
    hipLaunchKernelGGL(k_out_count, dim3((unsigned)work.size()), dim3(OUT_ROWS), 0, s, (const OutWork*)dwork.p, d_xyz, r2,
                       nb_points, d_count, d_keep);
    CS_LAUNCH_CHECK();
  }
  if (grid_rows > 0) {
    rc = grid_chunks(false, d_xyz, h_off, n_seg, OUT_GRID_MIN, cell, r2, 0, nullptr, nb_points, d_count, d_keep, nullptr, s);
    if (rc) return rc;
  }
  if (want_stats) g_outlier_stats[0] += (unsigned long long)grid_rows;   // the radius grid is complete: none recomputed
  return CS_OK;
}

void cs_outlier_stats(uint64_t out[2], int reset) { read_stats(g_outlier_stats, out, reset); }

}  // extern "C"
