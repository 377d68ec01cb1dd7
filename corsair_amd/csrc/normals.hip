// Surface normals from the k nearest rows of a point's own segment, or from the at most max_nn nearest inside
// a radius.  The specifications are the comments of cs_estimate_normals and cs_estimate_normals_hybrid in
// include/corsair_hip.h; tests/normals_ref.py and tests/normals_hybrid_ref.py restate them bit for bit.
//
// The definition (k_normals): one thread per row, 256 rows of one segment per workgroup: the segment is staged through LDS
// 512 rows at a time (k_icp_exact's pattern) and every thread keeps its KC best (distance, row) in registers, sorted, with
// a fully unrolled insertion; then (nrm_finish) the scatter matrix over the first m of them in list order, jacobi3, the
// selection and sign rules, one cast to f32.  No atomics, no scratch memory beyond the work list.
// The grid paths (k_normals_grid, below) build the same list from the 27 cells around a row (cellgrid.h, shared with
// pairs.hip) and hand it to the same nrm_finish; what they cannot prove complete is recomputed by the scan.
#include <hipcub/hipcub.hpp>
#include <math.h>

#include <algorithm>
#include <vector>

#include "cellgrid.h"
#include "horn.h"
#include "nn_common.h"
#include "normals_grid.h"

namespace cs {
namespace {

constexpr int NRM_ROWS = 256;   // rows per workgroup
constexpr int NRM_TT = 512;     // segment rows per LDS stage

struct NrmWork {
  int64_t seg0;   // first row of the segment (global)
  int32_t sn;     // rows of the segment
  int32_t r0;     // first row of this workgroup, local to the segment
};

// Everything after the neighbour list, for cs_estimate_normals and cs_estimate_normals_hybrid alike: the scatter matrix
// about the query row (x, y, z) over the first m list entries in list order, jacobi3, the selection, sign and degenerate
// rules, one cast to f32 into o[0..2].  seg = first row of the segment; bi = rows local to it, -1 = empty slot.
template <int KC>
__device__ __forceinline__ void nrm_finish(const float* __restrict__ seg, double x, double y, double z,
                                           const int (&bi)[KC], int m, float* __restrict__ o) {
  int cnt = 0;
  double s0 = 0, s1 = 0, s2 = 0, c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
#pragma unroll
  for (int s = 0; s < KC; ++s) {
    if (s < m && bi[s] >= 0) {
      const float* t = seg + 3 * (int64_t)bi[s];
      const double u0 = (double)t[0] - x, u1 = (double)t[1] - y, u2 = (double)t[2] - z;
      s0 = s0 + u0;
      s1 = s1 + u1;
      s2 = s2 + u2;
      c00 = fma(u0, u0, c00);
      c01 = fma(u0, u1, c01);
      c02 = fma(u0, u2, c02);
      c11 = fma(u1, u1, c11);
      c12 = fma(u1, u2, c12);
      c22 = fma(u2, u2, c22);
      ++cnt;
    }
  }
  double n0 = 0.0, n1 = 0.0, n2 = 1.0;
  if (cnt >= 3) {
    const double dm = (double)cnt;
    const double q0 = -(s0 / dm), q1 = -(s1 / dm), q2 = -(s2 / dm);
    double a[3][3], v[3][3];
    a[0][0] = fma(q0, s0, c00);
    a[0][1] = fma(q0, s1, c01);
    a[0][2] = fma(q0, s2, c02);
    a[1][1] = fma(q1, s1, c11);
    a[1][2] = fma(q1, s2, c12);
    a[2][2] = fma(q2, s2, c22);
    a[1][0] = a[0][1];
    a[2][0] = a[0][2];
    a[2][1] = a[1][2];
    const bool fin = isfinite(a[0][0]) && isfinite(a[0][1]) && isfinite(a[0][2]) && isfinite(a[1][1]) &&
                     isfinite(a[1][2]) && isfinite(a[2][2]);
    if (fin) {
      jacobi3(a, v);
      // eigenvector of the smallest eigenvalue (ties -> lowest column); selected value by value: no indexed access
      const double w0 = a[0][0], w1 = a[1][1], w2 = a[2][2];
      const double v00 = v[0][0], v10 = v[1][0], v20 = v[2][0], v01 = v[0][1], v11 = v[1][1], v21 = v[2][1];
      const double v02 = v[0][2], v12 = v[1][2], v22 = v[2][2];
      const bool c1 = w1 < w0;
      const double best = c1 ? w1 : w0;
      const bool c2 = w2 < best;
      double e0 = c2 ? v02 : (c1 ? v01 : v00);
      double e1 = c2 ? v12 : (c1 ? v11 : v10);
      double e2 = c2 ? v22 : (c1 ? v21 : v20);
      const double len = sqrt(fma(e2, e2, fma(e1, e1, e0 * e0)));
      if (isfinite(len) && len > 0.0) {
        e0 = e0 / len;
        e1 = e1 / len;
        e2 = e2 / len;
        // the component of largest magnitude (the first one on ties) is positive
        double big = fabs(e0), lead = e0;
        if (fabs(e1) > big) { big = fabs(e1); lead = e1; }
        if (fabs(e2) > big) { big = fabs(e2); lead = e2; }
        if (lead < 0.0) {
          e0 = -e0;
          e1 = -e1;
          e2 = -e2;
        }
        if (isfinite(e0) && isfinite(e1) && isfinite(e2)) {
          n0 = e0;
          n1 = e1;
          n2 = e2;
        }
      }
    }
  }
  o[0] = (float)n0;
  o[1] = (float)n1;
  o[2] = (float)n2;
}

// KC = list capacity (8, 16 or 32 >= k).  Rows arrive in ascending order and enter on a strict <, behind every entry with
// an equal distance: the list is the KC smallest by (distance, row), and its first m entries are the m smallest.
// RAD: the hybrid search's exhaustive path -- only rows with d < r2 enter (cs_estimate_normals_hybrid's definition).
// gate (optional): the workgroups of a segment that the k-NN grid path answers (gate[work_seg[b]].cell > 0) leave at once.
template <int KC, bool RAD>
__global__ __launch_bounds__(NRM_ROWS) void k_normals(const NrmWork* __restrict__ work, const float* __restrict__ xyz,
                                                      int k, double r2, float* __restrict__ normal,
                                                      const NrmSeg* __restrict__ gate,
                                                      const int32_t* __restrict__ work_seg) {
  __shared__ float t_lds[NRM_TT * 3];
  if (gate && gate[work_seg[blockIdx.x]].cell > 0.0) return;
  const NrmWork wk = work[blockIdx.x];
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
  int bi[KC];
#pragma unroll
  for (int s = 0; s < KC; ++s) {
    bd[s] = INFINITY;
    bi[s] = -1;
  }
  for (int tbase = 0; tbase < wk.sn; tbase += NRM_TT) {
    const int tcount = min(NRM_TT, wk.sn - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * 3; i += NRM_ROWS) t_lds[i] = seg[(int64_t)tbase * 3 + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) {
      const double dx = (double)t_lds[3 * j + 0] - x;
      const double dy = (double)t_lds[3 * j + 1] - y;
      const double dz = (double)t_lds[3 * j + 2] - z;
      const double d = fma(dz, dz, fma(dy, dy, dx * dx));
      if (d < bd[KC - 1] && (!RAD || d < r2)) {   // false for NaN and +inf: never a neighbour
        bd[KC - 1] = d;
        bi[KC - 1] = tbase + j;
#pragma unroll
        for (int s = KC - 1; s >= 1; --s) {
          const bool sw = bd[s] < bd[s - 1];   // strict: behind an equal distance of a smaller row
          const double lo = sw ? bd[s] : bd[s - 1], hi = sw ? bd[s - 1] : bd[s];
          const int li = sw ? bi[s] : bi[s - 1], hi_i = sw ? bi[s - 1] : bi[s];
          bd[s - 1] = lo;
          bd[s] = hi;
          bi[s - 1] = li;
          bi[s] = hi_i;
        }
      }
    }
  }
  if (!active) return;
  nrm_finish<KC>(seg, x, y, z, bi, min(k, wk.sn), normal + (wk.seg0 + row) * 3);
}

// ---- the grid paths (cellgrid.h) -------------------------------------------------------------------------------------
// A chunk = consecutive segments [sg0, sg0 + n_seg) of the call, at most NRM_CHUNK_SEGS of them (the 16-bit segment field
// of the key) and fewer than 2^31 rows; its rows are the consecutive global rows [off[0], off[n_seg]).  off = the chunk's
// n_seg + 1 global offsets on the device.
//
// The k-NN voucher.  A segment's cell size c comes from its bounding box (k_nrm_segs); a row probes the 27 cells around its
// own with the bound r2 = cov2 = c * c * (1 - 2^-30) and its list is ACCEPTED only when it holds k entries, i.e. when its
// k-th d2 lies strictly below cov2.  A row j the probe did not see has a cell index two or more away from the query's in
// some axis (the clamp to the key range is monotone, so this holds for the unclamped floors too); the computed quotients
// x / c then differ by more than 1, each is within 2^-53 relative of the true one and k_nrm_segs keeps |x / c| below
// 32767, so the true quotients differ by more than 1 - 2^-36 and |x_j - x_i| > c (1 - 2^-36) in that axis; the distance
// chain is within 4 * 2^-53 relative of the true sum of squares, so the computed d2_j > c^2 (1 - 2^-34) > cov2 (the
// rounding of c * c and of the product with 1 - 2^-30, 2^-52 together, is far inside the margin).  Every unseen row
// therefore lies strictly above every accepted entry: it can neither enter the list nor tie with it, and the accepted
// list is the exhaustive scan's.  A row that is not accepted is appended to the chunk's redo list (an integer counter;
// the order of the list reaches no output: every listed row writes its own normal only) and k_normals_redo recomputes
// it by the exhaustive scan of its segment.

// the chunk segment of global row g: the last p with off[p] <= g (empty segments share an offset and are skipped)
__device__ __forceinline__ int nrm_seg_of(const int64_t* __restrict__ off, int n_seg, int64_t g) {
  int lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// One workgroup per chunk segment.  Hybrid (k = 0): the call's cell and radius^2 for a segment of grid_min rows or more.
// k-NN (k > 0): the segment's bounding box (exact and order-free: min / max), then
//   c = 1.5 * sqrt(k * A / (pi * n)),  A = the surface area of the box, n = its rows
// -- the side of a square that holds 2.25 k / pi rows of a surface of area A sampled evenly, so that the 27 cells hold the
// k nearest of all but a few rows.  Off the grid: fewer than grid_min rows, a box that is not finite, A = 0
// (copies of one point, rows of one line), and a box so far out that a cell index would reach the clamp.
__global__ __launch_bounds__(256) void k_nrm_segs(const float* __restrict__ xyz, const int64_t* __restrict__ off,
                                                  int grid_min, int k, double cell, double r2,
                                                  NrmSeg* __restrict__ segs) {
  __shared__ float red[2][3][4];
  __shared__ int bad[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t s0 = off[p], sn = off[p + 1] - s0;
  if (sn < grid_min) {
    if (tid == 0) segs[p] = NrmSeg{0.0, 0.0};
    return;
  }
  if (k == 0) {
    if (tid == 0) segs[p] = NrmSeg{cell, r2};
    return;
  }
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int nonfinite = 0;
  for (int64_t j = tid; j < sn; j += 256) {
    const float* t = xyz + (s0 + j) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mn[c] = fminf(mn[c], t[c]);
      mx[c] = fmaxf(mx[c], t[c]);
      nonfinite |= !isfinite(t[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mn[c] = fminf(mn[c], __shfl_xor(mn[c], o));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o));
    }
    if ((tid & 63) == 0) {
      red[0][c][tid >> 6] = mn[c];
      red[1][c][tid >> 6] = mx[c];
    }
  }
  nonfinite = __any(nonfinite);
  if ((tid & 63) == 0) bad[tid >> 6] = nonfinite;
  __syncthreads();
  if (tid != 0) return;
  double ext[3], far = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float lo = fminf(fminf(red[0][c][0], red[0][c][1]), fminf(red[0][c][2], red[0][c][3]));
    const float hi = fmaxf(fmaxf(red[1][c][0], red[1][c][1]), fmaxf(red[1][c][2], red[1][c][3]));
    ext[c] = (double)hi - (double)lo;
    far = fmax(far, fmax(fabs((double)lo), fabs((double)hi)));
  }
  const double area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]);
  const double c = 1.5 * sqrt((double)k * area / (3.141592653589793 * (double)sn));
  const bool ok = !(bad[0] | bad[1] | bad[2] | bad[3]) && area > 0.0 && isfinite(c) && c > 0.0 && far / c < 32000.0;
  segs[p] = ok ? NrmSeg{c, (c * c) * (1.0 - 0x1.0p-30)} : NrmSeg{0.0, 0.0};
}

// key of a row of a grid segment = (chunk segment, cell).  A row of a segment off the grid gets the cell (-32768)^3 of its
// segment, which cg_cell never returns and no probe visits.  vals = the row, local to the chunk.
__global__ void k_nrm_keys(const float* __restrict__ xyz, const int64_t* __restrict__ off, int n_seg, int64_t m_total,
                           const NrmSeg* __restrict__ segs, uint64_t* keys, int32_t* vals) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= m_total) return;
  const int64_t g = off[0] + m;
  const int p = nrm_seg_of(off, n_seg, g);
  const float* t = xyz + 3 * g;
  const double cell = segs[p].cell;
  keys[m] = cell > 0.0 ? pack_key(p, cg_cell((double)t[0], cell), cg_cell((double)t[1], cell), cg_cell((double)t[2], cell))
                       : pack_key(p, -32768, -32768, -32768);
  vals[m] = (int32_t)m;
}

// the sorted rows' coordinates [m_total,3] and their rows local to their segments
__global__ void k_nrm_gather(const float* __restrict__ xyz, const int64_t* __restrict__ off,
                             const uint64_t* __restrict__ skeys, const int32_t* __restrict__ svals, int64_t m_total,
                             float* sxyz, int32_t* sj) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= m_total) return;
  const int64_t g = off[0] + svals[m];
  const float* t = xyz + 3 * g;
  sxyz[3 * m] = t[0];
  sxyz[3 * m + 1] = t[1];
  sxyz[3 * m + 2] = t[2];
  sj[m] = (int32_t)(g - off[(int)(skeys[m] >> 48)]);
}

// (d, j) enters the ascending list by the full (d2, row) pair: the list is the KC smallest of what it was offered, whatever
// the order of the offers.  d is finite; an empty slot (+inf, -1) always gives way.
template <int KC>
__device__ __forceinline__ void nrm_insert_pair(double (&bd)[KC], int (&bi)[KC], double d, int j) {
  if (d > bd[KC - 1] || (d == bd[KC - 1] && j > bi[KC - 1])) return;
  bd[KC - 1] = d;
  bi[KC - 1] = j;
#pragma unroll
  for (int s = KC - 1; s >= 1; --s) {
    const bool sw = bd[s] < bd[s - 1] || (bd[s] == bd[s - 1] && bi[s] < bi[s - 1]);
    const double lo = sw ? bd[s] : bd[s - 1], hi = sw ? bd[s - 1] : bd[s];
    const int li = sw ? bi[s] : bi[s - 1], hi_i = sw ? bi[s - 1] : bi[s];
    bd[s - 1] = lo;
    bd[s] = hi;
    bi[s - 1] = li;
    bi[s] = hi_i;
  }
}

// One thread per sorted row (the lanes of a wave probe the same cells); the normal goes back to the row's own place.
// Candidates arrive in no particular order, so insertion compares the full (d2, row) pair: the list is the KC smallest
// of those below the segment's r2, the exhaustive kernel's list.  KNN: a list of fewer than k entries is not accepted
// (the voucher above) and the row goes to the redo list; stats (optional) counts the rows of grid segments.
template <int KC, bool KNN>
__global__ __launch_bounds__(NRM_ROWS) void k_normals_grid(CellTable tb, const float* __restrict__ sxyz,
                                                           const int32_t* __restrict__ sj,
                                                           const uint64_t* __restrict__ skeys, int64_t m_total,
                                                           const float* __restrict__ xyz,
                                                           const int64_t* __restrict__ off,
                                                           const NrmSeg* __restrict__ segs, int k,
                                                           float* __restrict__ normal, int32_t* __restrict__ redo,
                                                           unsigned* __restrict__ redo_count,
                                                           unsigned long long* __restrict__ stats) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= m_total) return;
  const int p = (int)(skeys[m] >> 48);
  const NrmSeg sg = segs[p];
  if (!(sg.cell > 0.0)) return;
  if (KNN && stats) {   // one atomic per wave
    const unsigned long long mask = __ballot(1);
    if ((int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(&stats[0], (unsigned long long)__popcll(mask));
  }
  const int64_t seg0 = off[p];
  const double x = (double)sxyz[3 * m], y = (double)sxyz[3 * m + 1], z = (double)sxyz[3 * m + 2];
  double bd[KC];
  int bi[KC];
#pragma unroll
  for (int s = 0; s < KC; ++s) {
    bd[s] = INFINITY;
    bi[s] = -1;
  }
  cg_probe<3>(
      tb, sxyz, p, x, y, z, sg.cell, sg.r2,
      [&](const float* t) {
        const double dx = (double)t[0] - x, dy = (double)t[1] - y, dz = (double)t[2] - z;
        return fma(dz, dz, fma(dy, dy, dx * dx));
      },
      [&](double d, int32_t mm) {
        if (d > bd[KC - 1]) return;   // the common case, before the row index is loaded
        nrm_insert_pair<KC>(bd, bi, d, sj[mm]);
      });
  if (KNN) {
    bool full = false;
#pragma unroll
    for (int s = 0; s < KC; ++s)
      if (s == k - 1) full = bi[s] >= 0;
    if (!full) {
      redo[atomicAdd(redo_count, 1u)] = (int32_t)m;
      return;
    }
  }
  nrm_finish<KC>(xyz + seg0 * 3, x, y, z, bi, k, normal + (seg0 + sj[m]) * 3);
}

constexpr int NRM_REDO_BLOCKS = 2048;

// The rows of the redo list, one wave per row, by the exhaustive scan of the row's segment: the segment is staged through
// LDS as in k_normals, lane l ranks the rows l, l + 64, ... (ascending within the lane: k_normals' strict insertion) and
// the 64 lists are merged by the full (d2, row) pair into the KC smallest of the segment -- k_normals' list.  A fixed-size
// launch: the workgroups beyond the count leave at once.
template <int KC>
__global__ __launch_bounds__(64) void k_normals_redo(const int32_t* __restrict__ redo,
                                                     const unsigned* __restrict__ redo_count,
                                                     const float* __restrict__ sxyz, const int32_t* __restrict__ sj,
                                                     const uint64_t* __restrict__ skeys, const float* __restrict__ xyz,
                                                     const int64_t* __restrict__ off, int k, float* __restrict__ normal,
                                                     unsigned long long* __restrict__ stats) {
  __shared__ float t_lds[NRM_TT * 3];
  __shared__ double l_d[64 * KC];
  __shared__ int l_i[64 * KC];
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
    int bi[KC];
#pragma unroll
    for (int s = 0; s < KC; ++s) {
      bd[s] = INFINITY;
      bi[s] = -1;
    }
    for (int tbase = 0; tbase < sn; tbase += NRM_TT) {
      const int tcount = min(NRM_TT, sn - tbase);
      __syncthreads();
      for (int i = lane; i < tcount * 3; i += 64) t_lds[i] = seg[(int64_t)tbase * 3 + i];
      __syncthreads();
      for (int j = lane; j < tcount; j += 64) {
        const double dx = (double)t_lds[3 * j + 0] - x;
        const double dy = (double)t_lds[3 * j + 1] - y;
        const double dz = (double)t_lds[3 * j + 2] - z;
        const double d = fma(dz, dz, fma(dy, dy, dx * dx));
        if (d < bd[KC - 1]) {   // false for NaN and +inf: never a neighbour
          bd[KC - 1] = d;
          bi[KC - 1] = tbase + j;
#pragma unroll
          for (int s = KC - 1; s >= 1; --s) {
            const bool sw = bd[s] < bd[s - 1];
            const double lo = sw ? bd[s] : bd[s - 1], hi = sw ? bd[s - 1] : bd[s];
            const int li = sw ? bi[s] : bi[s - 1], hi_i = sw ? bi[s - 1] : bi[s];
            bd[s - 1] = lo;
            bd[s] = hi;
            bi[s - 1] = li;
            bi[s] = hi_i;
          }
        }
      }
    }
    // merge through LDS: every lane builds the same list from the 64 lists, each read in its ascending order until its
    // first entry that cannot enter (those behind it cannot either)
#pragma unroll
    for (int s = 0; s < KC; ++s) {
      l_d[s * 64 + lane] = bd[s];
      l_i[s * 64 + lane] = bi[s];
      bd[s] = INFINITY;
      bi[s] = -1;
    }
    __syncthreads();
    for (int src = 0; src < 64; ++src) {
#pragma unroll 1
      for (int s = 0; s < KC; ++s) {
        const double d = l_d[s * 64 + src];
        const int j = l_i[s * 64 + src];
        if (j < 0 || d > bd[KC - 1] || (d == bd[KC - 1] && j > bi[KC - 1])) break;
        nrm_insert_pair<KC>(bd, bi, d, j);
      }
    }
    if (lane == 0) nrm_finish<KC>(seg, x, y, z, bi, min(k, sn), normal + (seg0 + sj[m]) * 3);
  }
}

// A segment of fewer rows than this goes to the exhaustive kernel: the sort, the table and the scattered probe cannot pay
// where the scan reads the segment from one LDS stage (hybrid) or from two (k-NN, whose cells are 1.5 times wider and
// whose unvouched rows cost a second scan).  Choices by the kernels' shapes; they have not been tuned.
constexpr int NRM_GRID_MIN = NRM_TT + 1;
constexpr int NRM_KNN_GRID_MIN = 2 * NRM_TT + 1;

std::atomic<unsigned long long> g_normals_stats[2];

template <bool RAD>
void launch_exhaustive(const NrmWork* d_work, size_t n_work, const float* d_xyz, int k, double r2, float* d_normal,
                       hipStream_t s, const NrmSeg* gate = nullptr, const int32_t* work_seg = nullptr) {
  const dim3 grid((unsigned)n_work), block(NRM_ROWS);
  if (k <= 8)
    hipLaunchKernelGGL((k_normals<8, RAD>), grid, block, 0, s, d_work, d_xyz, k, r2, d_normal, gate, work_seg);
  else if (k <= 16)
    hipLaunchKernelGGL((k_normals<16, RAD>), grid, block, 0, s, d_work, d_xyz, k, r2, d_normal, gate, work_seg);
  else
    hipLaunchKernelGGL((k_normals<32, RAD>), grid, block, 0, s, d_work, d_xyz, k, r2, d_normal, gate, work_seg);
}

template <int KC, bool KNN>
void launch_grid(const CellTable& tb, const float* sxyz, const int32_t* sj, const uint64_t* skeys, int64_t m_total,
                 const float* d_xyz, const int64_t* doff, const NrmSeg* segs, int k, float* d_normal, int32_t* redo,
                 unsigned* redo_count, unsigned long long* stats, hipStream_t s) {
  hipLaunchKernelGGL((k_normals_grid<KC, KNN>), dim3((unsigned)ceil_div(m_total, NRM_ROWS)), dim3(NRM_ROWS), 0, s, tb, sxyz,
                     sj, skeys, m_total, d_xyz, doff, segs, k, d_normal, redo, redo_count, stats);
  if (KNN)
    hipLaunchKernelGGL(k_normals_redo<KC>, dim3(NRM_REDO_BLOCKS), dim3(64), 0, s, (const int32_t*)redo,
                       (const unsigned*)redo_count, sxyz, sj, skeys, d_xyz, doff, k, d_normal, stats);
}

// The grid path over one chunk of segments; every launch is enqueued on s, nothing waits.  knn: cs_estimate_normals (the
// segments' cells come from their boxes, rows the voucher refuses are recomputed, and the exhaustive kernel runs gated over
// every segment of grid_min rows or more: the workgroups of a segment on the grid leave at once); else the hybrid search.
int grid_chunk(bool knn, const float* d_xyz, const int64_t* h_off, int n_seg, int grid_min, double cell, double r2, int k,
               float* d_normal, unsigned long long* d_stats, hipStream_t s) {
  const char* who = knn ? "cs_estimate_normals: scratch allocation failed"
                        : "cs_estimate_normals_hybrid: scratch allocation failed";
  NrmGrid gr;
  int rc = nrm_grid_build(gr, d_xyz, h_off, n_seg, grid_min, knn ? k : 0, cell, r2, s, who);
  if (rc) return rc;
  const int64_t m_total = gr.m_total;
  PoolBuf<int32_t> redo(knn ? m_total : 1);
  PoolBuf<unsigned> redo_count(1);
  CS_REQUIRE(redo.p && redo_count.p, CS_ERR_HIP, "%s", who);
  CS_HIP_CHECK(hipMemsetAsync(redo_count.p, 0, sizeof(unsigned), s));
  const CellTable tb = gr.table();
  PoolBuf<float>& sxyz = gr.sxyz;
  PoolBuf<int32_t>& sj = gr.sj;
  PoolBuf<uint64_t>& skeys = gr.skeys;
  PoolBuf<int64_t>& doff = gr.doff;
  PoolBuf<NrmSeg>& segs = gr.segs;
#define NRM_GRID(KC)                                                                                                      \
  (knn ? launch_grid<KC, true>(tb, sxyz.p, sj.p, skeys.p, m_total, d_xyz, doff.p, segs.p, k, d_normal, redo.p,            \
                               redo_count.p, d_stats, s)                                                                  \
       : launch_grid<KC, false>(tb, sxyz.p, sj.p, skeys.p, m_total, d_xyz, doff.p, segs.p, k, d_normal, redo.p,           \
                                redo_count.p, d_stats, s))
  if (k <= 8)
    NRM_GRID(8);
  else if (k <= 16)
    NRM_GRID(16);
  else
    NRM_GRID(32);
#undef NRM_GRID
  CS_LAUNCH_CHECK();
  if (knn) {   // the exhaustive kernel for the segments the device kept off the grid
    std::vector<NrmWork> work;
    std::vector<int32_t> work_seg;
    for (int sg = 0; sg < n_seg; ++sg) {
      const int64_t sn = h_off[sg + 1] - h_off[sg];
      if (sn < grid_min) continue;
      for (int64_t r = 0; r < sn; r += NRM_ROWS) {
        work.push_back(NrmWork{h_off[sg], (int32_t)sn, (int32_t)r});
        work_seg.push_back(sg);
      }
    }
    PoolBuf<NrmWork> dwork;
    PoolBuf<int32_t> dwseg;
    rc = upload(dwork, work, s);
    if (!rc) rc = upload(dwseg, work_seg, s);
    if (rc) return rc;
    launch_exhaustive<false>(dwork.p, work.size(), d_xyz, k, 0.0, d_normal, s, segs.p, dwseg.p);
    CS_LAUNCH_CHECK();
  }
  return CS_OK;
}

// the chunks of a call that hold a segment of grid_min rows or more, one grid_chunk each
int grid_chunks(bool knn, const float* d_xyz, const int64_t* h_off, int n_seg, int grid_min, double cell, double r2, int k,
                float* d_normal, unsigned long long* d_stats, hipStream_t s) {
  for (int sg0 = 0; sg0 < n_seg;) {
    int sg1 = sg0;
    bool any = false;
    while (sg1 < n_seg && sg1 - sg0 < NRM_CHUNK_SEGS && (sg1 == sg0 || h_off[sg1 + 1] - h_off[sg0] <= NRM_CHUNK_ROWS)) {
      any = any || h_off[sg1 + 1] - h_off[sg1] >= grid_min;
      ++sg1;
    }
    if (any) {
      const int rc = grid_chunk(knn, d_xyz, h_off + sg0, sg1 - sg0, grid_min, cell, r2, k, d_normal, d_stats, s);
      if (rc) return rc;
    }
    sg0 = sg1;
  }
  return CS_OK;
}

}  // namespace

int nrm_grid_build(NrmGrid& gr, const float* d_xyz, const int64_t* h_off, int n_seg, int grid_min, int k, double cell,
                   double r2, hipStream_t s, const char* who) {
  const int64_t m_total = h_off[n_seg] - h_off[0];
  gr.m_total = m_total;
  int rc = upload(gr.doff, std::vector<int64_t>(h_off, h_off + n_seg + 1), s);
  if (rc) return rc;
  uint64_t cap = 1024;
  while (cap < (uint64_t)(2 * m_total)) cap <<= 1;
  gr.cap = cap;
  PoolBuf<uint64_t> keys(m_total);
  PoolBuf<int32_t> vals(m_total), svals(m_total);
  gr.segs.alloc(n_seg);
  gr.skeys.alloc(m_total);
  gr.tkeys.alloc(cap);
  gr.sj.alloc(m_total);
  gr.tbeg.alloc(cap);
  gr.tend.alloc(cap);
  gr.sxyz.alloc(3 * (size_t)m_total);
  CS_REQUIRE(gr.segs.p && keys.p && gr.skeys.p && gr.tkeys.p && vals.p && svals.p && gr.sj.p && gr.tbeg.p && gr.tend.p &&
                 gr.sxyz.p,
             CS_ERR_HIP, "%s", who);
  const unsigned g = (unsigned)ceil_div(m_total, 256);
  cellgrid_table_fill(gr.tkeys.p, cap, s);
  hipLaunchKernelGGL(k_nrm_segs, dim3((unsigned)n_seg), dim3(256), 0, s, d_xyz, gr.doff.p, grid_min, k, cell, r2,
                     gr.segs.p);
  hipLaunchKernelGGL(k_nrm_keys, dim3(g), dim3(256), 0, s, d_xyz, gr.doff.p, n_seg, m_total, gr.segs.p, keys.p, vals.p);
  CS_LAUNCH_CHECK();
  size_t tmp_bytes = 0;
  CS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.p, gr.skeys.p, vals.p, svals.p, (int)m_total, 0,
                                                  64, s));
  PoolBuf<char> tmp(tmp_bytes);
  CS_REQUIRE(tmp.p, CS_ERR_HIP, "%s", who);
  CS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.p, gr.skeys.p, vals.p, svals.p, (int)m_total, 0,
                                                  64, s));
  hipLaunchKernelGGL(k_nrm_gather, dim3(g), dim3(256), 0, s, d_xyz, gr.doff.p, gr.skeys.p, svals.p, m_total, gr.sxyz.p,
                     gr.sj.p);
  cellgrid_insert_ranges(gr.skeys.p, m_total, gr.tkeys.p, gr.tbeg.p, gr.tend.p, cap - 1, s);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // namespace cs

using namespace cs;

extern "C" {

int cs_estimate_normals(const float* d_xyz, const int64_t* h_off, int n_seg, int k, float* d_normal, void* stream) {
  CS_REQUIRE(h_off, CS_ERR_INVALID, "cs_estimate_normals: NULL offset table");
  CS_REQUIRE(n_seg >= 0, CS_ERR_INVALID, "cs_estimate_normals: negative segment count");
  CS_REQUIRE(k >= 3 && k <= 32, CS_ERR_UNSUPPORTED, "cs_estimate_normals: k outside [3, 32]");
  const bool use_grid = !env_first_is("CS_NORMALS_GRID", '0');
  const bool want_stats = use_grid && env_first_is("CS_NORMALS_STATS", '1');
  std::vector<NrmWork> work;
  int64_t rows = 0, grid_rows = 0;
  double flop = 0.0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    CS_REQUIRE(h_off[sg] >= 0 && sn >= 0, CS_ERR_INVALID, "cs_estimate_normals: bad segment %d", sg);
    CS_REQUIRE(sn < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_estimate_normals: segment %d has 2^31 rows or more", sg);
    rows += sn;
    flop += 8.0 * (double)sn * (double)sn;   // the definition's work, whichever path answers
    if (use_grid && sn >= NRM_KNN_GRID_MIN) {
      grid_rows += sn;
      continue;
    }
    for (int64_t r = 0; r < sn; r += NRM_ROWS) {
      NrmWork w;
      w.seg0 = h_off[sg];
      w.sn = (int32_t)sn;
      w.r0 = (int32_t)r;
      work.push_back(w);
    }
  }
  if (rows == 0) return CS_OK;
  CS_REQUIRE(d_xyz && d_normal, CS_ERR_INVALID, "cs_estimate_normals: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<NrmWork> dwork;
  if (!work.empty()) {
    const int rc = upload(dwork, work, s);
    if (rc) return rc;
  }
  PoolBuf<unsigned long long> dstats;
  if (want_stats && grid_rows > 0) {
    CS_REQUIRE(dstats.alloc(2), CS_ERR_HIP, "cs_estimate_normals: scratch allocation failed");
    CS_HIP_CHECK(hipMemsetAsync(dstats.p, 0, 2 * sizeof(unsigned long long), s));
  }
  {
    ProfScope prof("normals", s, flop);
    if (!work.empty()) {
      launch_exhaustive<false>(dwork.p, work.size(), d_xyz, k, 0.0, d_normal, s);
      CS_LAUNCH_CHECK();
    }
    if (grid_rows > 0) {
      const int rc = grid_chunks(true, d_xyz, h_off, n_seg, NRM_KNN_GRID_MIN, 0.0, 0.0, k, d_normal, dstats.p, s);
      if (rc) return rc;
    }
  }
  if (dstats.p) {
    unsigned long long h[2] = {0, 0};
    CS_HIP_CHECK(download_async(h, dstats.p, sizeof(h), s));
    CS_HIP_CHECK(download_sync(s));
    g_normals_stats[0] += h[0];
    g_normals_stats[1] += h[1];
  }
  return CS_OK;
}

int cs_estimate_normals_hybrid(const float* d_xyz, const int64_t* h_off, int n_seg, double radius, int max_nn,
                               float* d_normal, void* stream) {
  CS_REQUIRE(h_off, CS_ERR_INVALID, "cs_estimate_normals_hybrid: NULL offset table");
  CS_REQUIRE(n_seg >= 0, CS_ERR_INVALID, "cs_estimate_normals_hybrid: negative segment count");
  CS_REQUIRE(max_nn >= 3 && max_nn <= 32, CS_ERR_UNSUPPORTED, "cs_estimate_normals_hybrid: max_nn outside [3, 32]");
  CS_REQUIRE(radius > 0.0 && radius <= 1.7976931348623157e308, CS_ERR_INVALID,
             "cs_estimate_normals_hybrid: radius must be positive and finite");
  const double r2 = radius * radius;   // +inf for a radius above 1.3e154: every finite distance passes
  const double cell = radius * (1.0 + 1.0 / 1024.0);   // a little larger than the radius (cellgrid.h)
  // (a cell size near the top of the f64 range could round up to +inf: such a radius bounds nothing, the scan serves it)
  const bool use_grid = !env_first_is("CS_NORMALS_GRID", '0') && radius < 1e300;
  const bool want_stats = use_grid && env_first_is("CS_NORMALS_STATS", '1');
  std::vector<NrmWork> work;   // the exhaustive kernel's workgroups
  int64_t rows = 0, grid_rows = 0;
  double flop = 0.0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    CS_REQUIRE(h_off[sg] >= 0 && sn >= 0, CS_ERR_INVALID, "cs_estimate_normals_hybrid: bad segment %d", sg);
    CS_REQUIRE(sn < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_estimate_normals_hybrid: segment %d has 2^31 rows or more", sg);
    rows += sn;
    if (use_grid && sn >= NRM_GRID_MIN) {
      grid_rows += sn;
      flop += 8.0 * 27.0 * (double)max_nn * (double)sn;   // nominal: the cells' occupancy is not known on the host
      continue;
    }
    for (int64_t r = 0; r < sn; r += NRM_ROWS) {
      NrmWork w;
      w.seg0 = h_off[sg];
      w.sn = (int32_t)sn;
      w.r0 = (int32_t)r;
      work.push_back(w);
    }
    flop += 8.0 * (double)sn * (double)sn;
  }
  if (rows == 0) return CS_OK;
  CS_REQUIRE(d_xyz && d_normal, CS_ERR_INVALID, "cs_estimate_normals_hybrid: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<NrmWork> dwork;
  if (!work.empty()) {
    const int rc = upload(dwork, work, s);
    if (rc) return rc;
  }
  ProfScope prof("normals", s, flop);
  if (!work.empty()) {
    launch_exhaustive<true>(dwork.p, work.size(), d_xyz, max_nn, r2, d_normal, s);
    CS_LAUNCH_CHECK();
  }
  if (grid_rows > 0) {
    const int rc = grid_chunks(false, d_xyz, h_off, n_seg, NRM_GRID_MIN, cell, r2, max_nn, d_normal, nullptr, s);
    if (rc) return rc;
  }
  if (want_stats) g_normals_stats[0] += (unsigned long long)grid_rows;   // the hybrid grid is complete: none recomputed
  return CS_OK;
}

void cs_normals_stats(uint64_t out[2], int reset) { read_stats(g_normals_stats, out, reset); }

}  // extern "C"
