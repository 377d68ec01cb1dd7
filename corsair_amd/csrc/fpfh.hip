// Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009) and the orientation of normals they need.  The
// specifications are the comments of cs_orient_normals and cs_fpfh in include/corsair_hip.h; tests/fpfh_ref.py restates
// them bit for bit.
//
// cs_fpfh, one wave per row in both passes:
//   k_fpfh_spfh  the lanes split the candidate rows -- the whole segment (GRID = false, the definition) or the nine cell
//                columns around the row (GRID = true; the three cells of a column are neighbours in key order, so a column
//                is ONE range of the sorted rows) -- and append those inside the radius to an LDS list of FP_CAP entries.
//                fp_compact ranks every entry by counting the entries with a smaller (d2, row) pair (all distinct) and
//                writes the first max_nn - 1 to their ranks: the truncated list, in order, with no sort network.  A list
//                about to overflow is compacted the same way and goes on filling (the max_nn - 1 smallest of a union are
//                among the max_nn - 1 smallest of its parts), so a ball of any size gives the exhaustive answer.  Then
//                lane t bins the pair (row, t-th neighbour) into an LDS histogram (integer atomics) and the wave writes
//                the 33 counts (uint8: at most 127 neighbours), the count m and the ordered list (12 B an entry).
//   k_fpfh_sum   lane b < 33 owns bin b and walks the row's list; a neighbour's 33 counts are one contiguous read.  The
//                three group sums are chains over (neighbour, bin) in that order: the values of a turn of neighbours go
//                through LDS and lane g < 3 adds group g's in order.
// No kernel keeps anything but integers in atomics; no output depends on the order of any of them.
#include <math.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "fpfh_bounds.h"
#include "nn_common.h"
#include "normals_grid.h"

namespace cs {
namespace {

constexpr int FP_CAP = 256;          // LDS list entries of a wave (3 KB)
constexpr int FP_MAX_NN = 128;
constexpr int FP_BINS = 33;
constexpr int FP_TURN = 4;            // neighbours per turn of k_fpfh_sum
// the exhaustive scan serves a segment of fewer rows: normals.hip's convention (one LDS stage of its scan)
constexpr int FP_GRID_MIN = 513;
constexpr int64_t FP_LAUNCH_ROWS = 1LL << 30;   // rows (= workgroups) of one launch

__constant__ double c_bounds[10][2] = {CS_FPFH_BOUNDS};

// ---- cs_orient_normals ------------------------------------------------------------------------------------------------
constexpr int OR_ROWS = 256;
constexpr double OR_SCALE = 65536.0;   // 2^16
constexpr float OR_LIMIT = 32768.0f;   // 2^15

struct OrWork {
  int64_t seg0;   // first row of the segment (global)
  int32_t sn;     // rows of the segment
  int32_t r0;     // first row of this workgroup, local to the segment
  int32_t seg;    // the segment
  int32_t pad;
};

// sums[seg] = {sum x, sum y, sum z, count} over the rows with three finite coordinates below 2^15 in magnitude, each
// coordinate as the integer rint(x * 2^16): below 2^31 in magnitude, fewer than 2^31 rows, so the 64-bit sums are exact.
__global__ __launch_bounds__(OR_ROWS) void k_orient_sums(const OrWork* __restrict__ work, const float* __restrict__ xyz,
                                                         unsigned long long* __restrict__ sums) {
  const OrWork wk = work[blockIdx.x];
  const int row = wk.r0 + (int)threadIdx.x;
  long long v[4] = {0, 0, 0, 0};
  if (row < wk.sn) {
    const float* t = xyz + (wk.seg0 + row) * 3;
    const float x = t[0], y = t[1], z = t[2];
    if (fabsf(x) < OR_LIMIT && fabsf(y) < OR_LIMIT && fabsf(z) < OR_LIMIT) {   // false for NaN and inf
      v[0] = (long long)rint((double)x * OR_SCALE);
      v[1] = (long long)rint((double)y * OR_SCALE);
      v[2] = (long long)rint((double)z * OR_SCALE);
      v[3] = 1;
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[c] += __shfl_xor(v[c], o);
  }
  if ((threadIdx.x & 63) == 0 && v[3] != 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) atomicAdd(&sums[4 * (int64_t)wk.seg + c], (unsigned long long)v[c]);
  }
}

__global__ __launch_bounds__(OR_ROWS) void k_orient_apply(const OrWork* __restrict__ work, const float* __restrict__ xyz,
                                                          const double* __restrict__ view,
                                                          const unsigned long long* __restrict__ sums, int away,
                                                          float* __restrict__ normal) {
  const OrWork wk = work[blockIdx.x];
  const int row = wk.r0 + (int)threadIdx.x;
  if (row >= wk.sn) return;
  double v0, v1, v2;
  if (view) {
    v0 = view[3 * (int64_t)wk.seg];
    v1 = view[3 * (int64_t)wk.seg + 1];
    v2 = view[3 * (int64_t)wk.seg + 2];
  } else {
    const long long cnt = (long long)sums[4 * (int64_t)wk.seg + 3];
    if (cnt == 0) return;
    const double dc = (double)cnt;
    v0 = ((double)(long long)sums[4 * (int64_t)wk.seg] / dc) * (1.0 / OR_SCALE);
    v1 = ((double)(long long)sums[4 * (int64_t)wk.seg + 1] / dc) * (1.0 / OR_SCALE);
    v2 = ((double)(long long)sums[4 * (int64_t)wk.seg + 2] / dc) * (1.0 / OR_SCALE);
  }
  const float* t = xyz + (wk.seg0 + row) * 3;
  float* n = normal + (wk.seg0 + row) * 3;
  const double d0 = (double)t[0] - v0, d1 = (double)t[1] - v1, d2 = (double)t[2] - v2;
  const float n0 = n[0], n1 = n[1], n2 = n[2];
  const double s = fma((double)n2, d2, fma((double)n1, d1, (double)n0 * d0));
  if (away ? s < 0.0 : s > 0.0) {
    n[0] = -n0;
    n[1] = -n1;
    n[2] = -n2;
  }
}

// ---- cs_fpfh ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fp_bin11(double f) {
  const double t = floor((11.0 * (f + 1.0)) * 0.5);
  return t < 0.0 ? 0 : (t > 10.0 ? 10 : (int)t);
}

// the number of boundaries theta_m (m = 1..10) not above the angle of (x, y); x and y finite (the header's rule)
__device__ __forceinline__ int fp_bin_angle(double x, double y) {
  if (x == 0.0 && y == 0.0) return 5;
  const int m0 = y < 0.0 ? 0 : 5;
  int b = m0;
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const double c = c_bounds[m0 + u][0], s = c_bounds[m0 + u][1];
    b += fma(c, y, -(s * x)) >= 0.0 ? 1 : 0;
  }
  return b;
}

// The three bins of the pair (i, j): p = the rows, n = their normals, (dx, dy, dz) = p_j - p_i, d2 its chain.
__device__ __forceinline__ void fp_pair(const double (&ni)[3], const double (&nj)[3], double dx, double dy, double dz,
                                        double d2, int& b0, int& b1, int& b2) {
  b0 = b1 = b2 = 5;
  const double len = sqrt(d2);
  if (!(len > 0.0)) return;
  const double a1 = ((ni[0] * dx + ni[1] * dy) + ni[2] * dz) / len;
  const double a2 = ((nj[0] * dx + nj[1] * dy) + nj[2] * dz) / len;
  const bool sw = fabs(a1) < fabs(a2);
  const double p0 = sw ? nj[0] : ni[0], p1 = sw ? nj[1] : ni[1], p2 = sw ? nj[2] : ni[2];   // n1
  const double q0 = sw ? ni[0] : nj[0], q1 = sw ? ni[1] : nj[1], q2 = sw ? ni[2] : nj[2];   // n2
  if (sw) {
    dx = -dx;
    dy = -dy;
    dz = -dz;
  }
  const double f2 = sw ? -a2 : a1;
  double v0 = dy * p2 - dz * p1, v1 = dz * p0 - dx * p2, v2 = dx * p1 - dy * p0;
  const double vl = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  if (!(vl > 0.0 && vl <= 1.7976931348623157e308)) return;
  v0 = v0 / vl;
  v1 = v1 / vl;
  v2 = v2 / vl;
  const double w0 = p1 * v2 - p2 * v1, w1 = p2 * v0 - p0 * v2, w2 = p0 * v1 - p1 * v0;
  const double f1 = (v0 * q0 + v1 * q1) + v2 * q2;
  const double x = (p0 * q0 + p1 * q1) + p2 * q2;
  const double y = (w0 * q0 + w1 * q1) + w2 * q2;
  if (!(isfinite(f1) && isfinite(f2) && isfinite(x) && isfinite(y))) return;
  b0 = fp_bin_angle(x, y);
  b1 = fp_bin11(f1);
  b2 = fp_bin11(f2);
}

// The cnt list entries are ranked by (d2, row) and the first K written to their ranks; returns min(cnt, K).  Called by the
// whole wave (the workgroup) with a uniform cnt <= FP_CAP.
__device__ __forceinline__ int fp_compact(double* l_d, int* l_j, int cnt, int K, int lane) {
  __syncthreads();
  double d[FP_CAP / 64];
  int j[FP_CAP / 64], rk[FP_CAP / 64];
#pragma unroll
  for (int u = 0; u < FP_CAP / 64; ++u) {
    const int e = lane + 64 * u;
    d[u] = e < cnt ? l_d[e] : INFINITY;
    j[u] = e < cnt ? l_j[e] : 0x7fffffff;
    rk[u] = 0;
  }
  for (int t = 0; t < cnt; ++t) {
    const double dt = l_d[t];
    const int jt = l_j[t];
#pragma unroll
    for (int u = 0; u < FP_CAP / 64; ++u) rk[u] += (dt < d[u] || (dt == d[u] && jt < j[u])) ? 1 : 0;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < FP_CAP / 64; ++u) {
    if (lane + 64 * u < cnt && rk[u] < K) {
      l_d[rk[u]] = d[u];
      l_j[rk[u]] = j[u];
    }
  }
  __syncthreads();
  return min(cnt, K);
}

// every lane offers one candidate (ok = it is a neighbour); cnt stays uniform
__device__ __forceinline__ void fp_offer(bool ok, double d2, int j, double* l_d, int* l_j, int& cnt, int K, int lane,
                                         int& overflow) {
  if (cnt + 64 > FP_CAP) {
    cnt = fp_compact(l_d, l_j, cnt, K, lane);
    overflow = 1;
  }
  const unsigned long long mask = __ballot(ok);
  if (ok) {
    const int pos = cnt + __popcll(mask & ((1ULL << lane) - 1ULL));
    l_d[pos] = d2;
    l_j[pos] = j;
  }
  cnt += __popcll(mask);
}

struct FpOut {
  uint8_t* cnt8;     // [rows, 33] SPFH counts
  int32_t* mcount;   // [rows] neighbours
  int64_t* base;     // [rows] first row of the row's segment, relative to the call's first row
  double* list_d;    // [rows, K] the neighbours' d2, ascending by (d2, row)
  int32_t* list_j;   // [rows, K] their rows, local to the segment
  unsigned long long* stats;   // optional {neighbours, rows whose list was compacted before the end}
};

// GRID: workgroup u = sorted row m0 + u of the chunk (rows of segments off the grid leave at once); off = the chunk's
// offsets.  Otherwise workgroup u = row u0 + u of the exhaustive segments' rows: ex_off[n_ex + 1] their prefix sums,
// ex_seg0[n_ex] their first rows (global).  g0 = the call's first row.
template <bool GRID>
__global__ __launch_bounds__(64) void k_fpfh_spfh(CellTable tb, const float* __restrict__ sxyz,
                                                  const int32_t* __restrict__ sj, const uint64_t* __restrict__ skeys,
                                                  const int64_t* __restrict__ off, const NrmSeg* __restrict__ segs,
                                                  const int64_t* __restrict__ ex_off, const int64_t* __restrict__ ex_seg0,
                                                  int n_ex, int64_t u0, const float* __restrict__ xyz,
                                                  const float* __restrict__ normal, int64_t g0, double r2, int K,
                                                  FpOut out) {
  __shared__ double l_d[FP_CAP];
  __shared__ int l_j[FP_CAP];
  __shared__ int hist[FP_BINS];
  const int lane = threadIdx.x;
  const int64_t u = u0 + blockIdx.x;
  int64_t seg0;
  int i, sn = 0, p = 0;
  double cell = 0.0;
  if (GRID) {
    p = (int)(skeys[u] >> 48);
    const NrmSeg sg = segs[p];
    if (!(sg.cell > 0.0)) return;
    cell = sg.cell;
    seg0 = off[p];
    i = sj[u];
  } else {
    int lo = 0, hi = n_ex;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (ex_off[mid] <= u) lo = mid; else hi = mid;
    }
    seg0 = ex_seg0[lo];
    sn = (int)(ex_off[lo + 1] - ex_off[lo]);
    i = (int)(u - ex_off[lo]);
  }
  const float* seg = xyz + seg0 * 3;
  const float* nseg = normal + seg0 * 3;
  const double x = (double)seg[3 * (int64_t)i], y = (double)seg[3 * (int64_t)i + 1], z = (double)seg[3 * (int64_t)i + 2];
  int cnt = 0, overflow = 0;
  if (GRID) {
    // lane c < 27 looks up cell c = 3 * column + (dz + 1); a column's cells are consecutive keys: one range
    int32_t cb = 0x7fffffff, ce = 0;
    if (lane < 27) {
      const int cx = cg_cell(x, cell) + (lane / 9) - 1, cy = cg_cell(y, cell) + ((lane / 3) % 3) - 1;
      const int cz = cg_cell(z, cell) + (lane % 3) - 1;
      int32_t b, e;
      if (cg_lookup(tb, p, cx, cy, cz, b, e)) {
        cb = b;
        ce = e;
      }
    }
    for (int col = 0; col < 9; ++col) {
      const int32_t b = min(min(__shfl(cb, 3 * col), __shfl(cb, 3 * col + 1)), __shfl(cb, 3 * col + 2));
      const int32_t e = max(max(__shfl(ce, 3 * col), __shfl(ce, 3 * col + 1)), __shfl(ce, 3 * col + 2));
      for (int64_t mb = b; mb < e; mb += 64) {
        const int64_t mm = mb + lane;
        bool ok = false;
        double d = 0.0;
        int jj = 0;
        if (mm < e && mm != u) {
          const float* t = sxyz + 3 * mm;
          const double dx = (double)t[0] - x, dy = (double)t[1] - y, dz = (double)t[2] - z;
          d = fma(dz, dz, fma(dy, dy, dx * dx));
          ok = d < r2;   // false for NaN and, r2 being finite here, for +inf
          if (ok) jj = sj[mm];
        }
        fp_offer(ok, d, jj, l_d, l_j, cnt, K, lane, overflow);
      }
    }
  } else {
    for (int jb = 0; jb < sn; jb += 64) {
      const int jj = jb + lane;
      bool ok = false;
      double d = 0.0;
      if (jj < sn && jj != i) {
        const float* t = seg + 3 * (int64_t)jj;
        const double dx = (double)t[0] - x, dy = (double)t[1] - y, dz = (double)t[2] - z;
        d = fma(dz, dz, fma(dy, dy, dx * dx));
        ok = d < r2 && d <= 1.7976931348623157e308;   // NaN and +inf never qualify
      }
      fp_offer(ok, d, jj, l_d, l_j, cnt, K, lane, overflow);
    }
  }
  const int m = fp_compact(l_d, l_j, cnt, K, lane);
  if (lane < FP_BINS) hist[lane] = 0;
  __syncthreads();
  const double ni[3] = {(double)nseg[3 * (int64_t)i], (double)nseg[3 * (int64_t)i + 1], (double)nseg[3 * (int64_t)i + 2]};
  const int64_t orow = seg0 - g0 + i;
  for (int t = lane; t < m; t += 64) {
    const int j = l_j[t];
    const double d = l_d[t];
    const float* tj = seg + 3 * (int64_t)j;
    const float* nn = nseg + 3 * (int64_t)j;
    const double nj[3] = {(double)nn[0], (double)nn[1], (double)nn[2]};
    int b0, b1, b2;
    fp_pair(ni, nj, (double)tj[0] - x, (double)tj[1] - y, (double)tj[2] - z, d, b0, b1, b2);
    atomicAdd(&hist[b0], 1);
    atomicAdd(&hist[11 + b1], 1);
    atomicAdd(&hist[22 + b2], 1);
    out.list_d[orow * K + t] = d;
    out.list_j[orow * K + t] = j;
  }
  __syncthreads();
  if (lane < FP_BINS) out.cnt8[orow * FP_BINS + lane] = (uint8_t)hist[lane];
  if (lane == 0) {
    out.mcount[orow] = m;
    out.base[orow] = seg0 - g0;
    if (out.stats) {
      atomicAdd(&out.stats[0], (unsigned long long)m);
      if (overflow) atomicAdd(&out.stats[1], 1ULL);
    }
  }
}

// workgroup u = row u0 + u of the call; lane b < 33 owns bin b (the lanes above mirror bin 32 and write nothing)
__global__ __launch_bounds__(64) void k_fpfh_sum(int64_t u0, int K, const uint8_t* __restrict__ cnt8,
                                                 const int32_t* __restrict__ mcount, const int64_t* __restrict__ base,
                                                 const double* __restrict__ list_d, const int32_t* __restrict__ list_j,
                                                 float* __restrict__ fpfh) {
  __shared__ __attribute__((aligned(16))) double v_lds[FP_TURN][36];
  const int lane = threadIdx.x;
  const int b = lane < FP_BINS ? lane : FP_BINS - 1;
  const int slot = 12 * (b / 11) + b % 11;
  const int64_t u = u0 + blockIdx.x;
  const int m = mcount[u];
  const int64_t sb = base[u];
  // Four neighbours a turn.  Every lane adds its own bin's values; the group sums are chains over (neighbour, bin), so
  // the turn's values go through LDS (a group's 11 at a 16-byte boundary) and lane g < 3 adds group g's in order.  A
  // neighbour at d2 == 0 and the entries past the list's end contribute val = +0: x + 0 == x for every x these sums can
  // hold (none is -0), which is the header's "skipped".
  // (measured: with the 11 values of a group fetched by every lane through shuffles this pass took 2.67 ms at the bench
  // shape, and 3.46 ms with six more shuffles a neighbour: the cross-lane moves bound it)
  double acc = 0.0, sum = 0.0;
  for (int t0 = 0; t0 < m; t0 += FP_TURN) {
#pragma unroll
    for (int q = 0; q < FP_TURN; ++q) {
      const int t = t0 + q;
      double val = 0.0;
      if (t < m) {
        const double d2 = list_d[u * K + t];
        if (d2 != 0.0) {
          const int64_t jr = sb + list_j[u * K + t];
          const int mj = mcount[jr];
          const double spfh = mj > 0 ? (double)cnt8[jr * FP_BINS + b] * (100.0 / (double)mj) : 0.0;
          val = spfh / d2;
        }
      }
      acc = acc + val;
      if (lane < FP_BINS) v_lds[q][slot] = val;
    }
    __syncthreads();
    if (lane < 3) {
#pragma unroll
      for (int q = 0; q < FP_TURN; ++q) {
#pragma unroll
        for (int k = 0; k < 11; ++k) sum = sum + v_lds[q][12 * lane + k];
      }
    }
    __syncthreads();
  }
  sum = __shfl(sum, b / 11);
  if (sum != 0.0) acc = acc * (100.0 / sum);
  const double own = m > 0 ? (double)cnt8[u * FP_BINS + b] * (100.0 / (double)m) : 0.0;
  acc = acc + own;
  if (lane < FP_BINS) fpfh[u * FP_BINS + lane] = (float)acc;
}

std::atomic<unsigned long long> g_fpfh_stats[2];

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_orient_normals(const float* d_xyz, const int64_t* h_off, int n_seg, const double* d_view, int away,
                      float* d_normal, void* stream) {
  CS_REQUIRE(h_off, CS_ERR_INVALID, "cs_orient_normals: NULL offset table");
  CS_REQUIRE(n_seg >= 0, CS_ERR_INVALID, "cs_orient_normals: negative segment count");
  CS_REQUIRE(away == 0 || away == 1, CS_ERR_INVALID, "cs_orient_normals: away must be 0 or 1");
  std::vector<OrWork> work;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    CS_REQUIRE(h_off[sg] >= 0 && sn >= 0, CS_ERR_INVALID, "cs_orient_normals: bad segment %d", sg);
    CS_REQUIRE(sn < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_orient_normals: segment %d has 2^31 rows or more", sg);
    for (int64_t r = 0; r < sn; r += OR_ROWS) work.push_back(OrWork{h_off[sg], (int32_t)sn, (int32_t)r, sg, 0});
  }
  if (work.empty()) return CS_OK;
  CS_REQUIRE(d_xyz && d_normal, CS_ERR_INVALID, "cs_orient_normals: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<OrWork> dwork;
  const int rc = upload(dwork, work, s);
  if (rc) return rc;
  PoolBuf<unsigned long long> sums;
  ProfScope prof("orient", s, 0.0);
  if (!d_view) {
    CS_REQUIRE(sums.alloc(4 * (size_t)n_seg), CS_ERR_HIP, "cs_orient_normals: scratch allocation failed");
    CS_HIP_CHECK(hipMemsetAsync(sums.p, 0, 4 * (size_t)n_seg * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_orient_sums, dim3((unsigned)work.size()), dim3(OR_ROWS), 0, s, dwork.p, d_xyz, sums.p);
  }
  hipLaunchKernelGGL(k_orient_apply, dim3((unsigned)work.size()), dim3(OR_ROWS), 0, s, dwork.p, d_xyz, d_view,
                     (const unsigned long long*)sums.p, away, d_normal);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

int cs_fpfh(const float* d_xyz, const float* d_normal, const int64_t* h_off, int n_seg, double radius, int max_nn,
            float* d_fpfh, void* stream) {
  CS_REQUIRE(h_off, CS_ERR_INVALID, "cs_fpfh: NULL offset table");
  CS_REQUIRE(n_seg >= 0, CS_ERR_INVALID, "cs_fpfh: negative segment count");
  CS_REQUIRE(max_nn >= 4 && max_nn <= FP_MAX_NN, CS_ERR_UNSUPPORTED, "cs_fpfh: max_nn outside [4, 128]");
  CS_REQUIRE(radius > 0.0 && radius <= 1.7976931348623157e308, CS_ERR_INVALID,
             "cs_fpfh: radius must be positive and finite");
  const double r2 = radius * radius;   // +inf for a radius above 1.3e154: every finite distance passes
  const double cell = radius * (1.0 + 1.0 / 1024.0);
  const bool use_grid = !env_first_is("CS_FPFH_GRID", '0') && radius < 1e150;   // the grid kernel wants a finite r2
  const bool want_stats = env_first_is("CS_FPFH_STATS", '1');
  const bool first_pass_only = env_first_is("CS_FPFH_PASS", '1');   // timing diagnostic: d_fpfh is not written
  const int K = max_nn - 1;
  std::vector<int64_t> ex_off(1, 0), ex_seg0;
  int64_t grid_rows = 0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    CS_REQUIRE(h_off[sg] >= 0 && sn >= 0, CS_ERR_INVALID, "cs_fpfh: bad segment %d", sg);
    CS_REQUIRE(sn < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_fpfh: segment %d has 2^31 rows or more", sg);
    if (sn == 0) continue;
    if (use_grid && sn >= FP_GRID_MIN) {
      grid_rows += sn;
      continue;
    }
    ex_seg0.push_back(h_off[sg]);
    ex_off.push_back(ex_off.back() + sn);
  }
  const int64_t g0 = n_seg > 0 ? h_off[0] : 0;
  const int64_t rows = n_seg > 0 ? h_off[n_seg] - g0 : 0;
  if (rows == 0) return CS_OK;
  CS_REQUIRE(d_xyz && d_normal && d_fpfh, CS_ERR_INVALID, "cs_fpfh: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const char* who = "cs_fpfh: scratch allocation failed";
  PoolBuf<uint8_t> cnt8((size_t)rows * FP_BINS);
  PoolBuf<int32_t> mcount(rows), list_j((size_t)rows * K);
  PoolBuf<int64_t> base(rows);
  PoolBuf<double> list_d((size_t)rows * K);
  PoolBuf<unsigned long long> dstats;
  CS_REQUIRE(cnt8.p && mcount.p && list_j.p && base.p && list_d.p, CS_ERR_HIP, "%s", who);
  if (want_stats) {
    CS_REQUIRE(dstats.alloc(2), CS_ERR_HIP, "%s", who);
    CS_HIP_CHECK(hipMemsetAsync(dstats.p, 0, 2 * sizeof(unsigned long long), s));
  }
  CS_HIP_CHECK(hipMemsetAsync(mcount.p, 0, (size_t)rows * sizeof(int32_t), s));   // k_fpfh_sum trusts every count
  const FpOut out{cnt8.p, mcount.p, base.p, list_d.p, list_j.p, dstats.p};
  {
    // nominal work: 27 cells' candidates are not known on the host; a pair costs about 100 f64 operations
    ProfScope prof("fpfh", s, 100.0 * (double)rows * (double)K);
    const int n_ex = (int)ex_seg0.size();
    if (n_ex > 0) {
      PoolBuf<int64_t> d_exoff, d_exseg0;
      int rc = upload(d_exoff, ex_off, s);
      if (!rc) rc = upload(d_exseg0, ex_seg0, s);
      if (rc) return rc;
      for (int64_t u0 = 0; u0 < ex_off.back(); u0 += FP_LAUNCH_ROWS) {
        const unsigned nb = (unsigned)std::min<int64_t>(FP_LAUNCH_ROWS, ex_off.back() - u0);
        hipLaunchKernelGGL(k_fpfh_spfh<false>, dim3(nb), dim3(64), 0, s, CellTable{}, nullptr, nullptr, nullptr, nullptr,
                           nullptr, d_exoff.p, d_exseg0.p, n_ex, u0, d_xyz, d_normal, g0, r2, K, out);
      }
      CS_LAUNCH_CHECK();
    }
    if (grid_rows > 0) {
      // the chunks of the call that hold a segment on the grid (normals.hip's chunking)
      for (int sg0 = 0; sg0 < n_seg;) {
        int sg1 = sg0;
        bool any = false;
        while (sg1 < n_seg && sg1 - sg0 < NRM_CHUNK_SEGS && (sg1 == sg0 || h_off[sg1 + 1] - h_off[sg0] <= NRM_CHUNK_ROWS)) {
          any = any || h_off[sg1 + 1] - h_off[sg1] >= FP_GRID_MIN;
          ++sg1;
        }
        if (any) {
          NrmGrid gr;
          const int rc = nrm_grid_build(gr, d_xyz, h_off + sg0, sg1 - sg0, FP_GRID_MIN, 0, cell, r2, s, who);
          if (rc) return rc;
          for (int64_t u0 = 0; u0 < gr.m_total; u0 += FP_LAUNCH_ROWS) {
            const unsigned nb = (unsigned)std::min<int64_t>(FP_LAUNCH_ROWS, gr.m_total - u0);
            hipLaunchKernelGGL(k_fpfh_spfh<true>, dim3(nb), dim3(64), 0, s, gr.table(), gr.sxyz.p, gr.sj.p, gr.skeys.p,
                               gr.doff.p, gr.segs.p, nullptr, nullptr, 0, u0, d_xyz, d_normal, g0, r2, K, out);
          }
          CS_LAUNCH_CHECK();
        }
        sg0 = sg1;
      }
    }
    for (int64_t u0 = 0; u0 < rows && !first_pass_only; u0 += FP_LAUNCH_ROWS) {
      const unsigned nb = (unsigned)std::min<int64_t>(FP_LAUNCH_ROWS, rows - u0);
      hipLaunchKernelGGL(k_fpfh_sum, dim3(nb), dim3(64), 0, s, u0, K, cnt8.p, mcount.p, base.p, list_d.p, list_j.p,
                         d_fpfh + g0 * FP_BINS);
    }
    CS_LAUNCH_CHECK();
  }
  if (dstats.p) {
    unsigned long long h[2] = {0, 0};
    CS_HIP_CHECK(download_async(h, dstats.p, sizeof(h), s));
    CS_HIP_CHECK(download_sync(s));
    g_fpfh_stats[0] += h[0];
    g_fpfh_stats[1] += h[1];
  }
  return CS_OK;
}

void cs_fpfh_stats(uint64_t out[2], int reset) { read_stats(g_fpfh_stats, out, reset); }

}  // extern "C"
