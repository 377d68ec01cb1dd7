// Surface normals from the k nearest rows of a point's own segment.  The specification is the comment of
// cs_estimate_normals in include/corsair_hip.h; tests/normals_ref.py restates it bit for bit.
//
// One kernel, one thread per row, 256 rows of one segment per workgroup: the segment is staged through LDS 512 rows at a
// time (k_icp_exact's pattern) and every thread keeps its KC best (distance, row) in registers, sorted, with a fully
// unrolled insertion; then the scatter matrix over the first m of them in list order, jacobi3, the selection and sign
// rules, one cast to f32.  No atomics, no scratch memory beyond the work list.
#include <math.h>

#include <algorithm>
#include <vector>

#include "horn.h"
#include "nn_common.h"

namespace cs {
namespace {

constexpr int NRM_ROWS = 256;   // rows per workgroup
constexpr int NRM_TT = 512;     // segment rows per LDS stage

struct NrmWork {
  int64_t seg0;   // first row of the segment (global)
  int32_t sn;     // rows of the segment
  int32_t r0;     // first row of this workgroup, local to the segment
};

// KC = list capacity (8, 16 or 32 >= k).  Rows arrive in ascending order and enter on a strict <, behind every entry with
// an equal distance: the list is the KC smallest by (distance, row), and its first m entries are the m smallest.
template <int KC>
__global__ __launch_bounds__(NRM_ROWS) void k_normals(const NrmWork* __restrict__ work, const float* __restrict__ xyz,
                                                      int k, float* __restrict__ normal) {
  __shared__ float t_lds[NRM_TT * 3];
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
      if (d < bd[KC - 1]) {   // false for NaN and +inf: never a neighbour
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
  const int m = min(k, wk.sn);
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
  float* o = normal + (wk.seg0 + row) * 3;
  o[0] = (float)n0;
  o[1] = (float)n1;
  o[2] = (float)n2;
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_estimate_normals(const float* d_xyz, const int64_t* h_off, int n_seg, int k, float* d_normal, void* stream) {
  CS_REQUIRE(h_off, CS_ERR_INVALID, "cs_estimate_normals: NULL offset table");
  CS_REQUIRE(n_seg >= 0, CS_ERR_INVALID, "cs_estimate_normals: negative segment count");
  CS_REQUIRE(k >= 3 && k <= 32, CS_ERR_UNSUPPORTED, "cs_estimate_normals: k outside [3, 32]");
  std::vector<NrmWork> work;
  double flop = 0.0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    CS_REQUIRE(h_off[sg] >= 0 && sn >= 0, CS_ERR_INVALID, "cs_estimate_normals: bad segment %d", sg);
    CS_REQUIRE(sn < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_estimate_normals: segment %d has 2^31 rows or more", sg);
    for (int64_t r = 0; r < sn; r += NRM_ROWS) {
      NrmWork w;
      w.seg0 = h_off[sg];
      w.sn = (int32_t)sn;
      w.r0 = (int32_t)r;
      work.push_back(w);
    }
    flop += 8.0 * (double)sn * (double)sn;
  }
  if (work.empty()) return CS_OK;
  CS_REQUIRE(d_xyz && d_normal, CS_ERR_INVALID, "cs_estimate_normals: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<NrmWork> dwork;
  const int rc = upload(dwork, work, s);
  if (rc) return rc;
  ProfScope prof("normals", s, flop);
  const dim3 grid((unsigned)work.size()), block(NRM_ROWS);
  if (k <= 8)
    hipLaunchKernelGGL(k_normals<8>, grid, block, 0, s, dwork.p, d_xyz, k, d_normal);
  else if (k <= 16)
    hipLaunchKernelGGL(k_normals<16>, grid, block, 0, s, dwork.p, d_xyz, k, d_normal);
  else
    hipLaunchKernelGGL(k_normals<32>, grid, block, 0, s, dwork.p, d_xyz, k, d_normal);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
