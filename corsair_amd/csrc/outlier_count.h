// The radius count of cs_outlier_radius (outlier.hip), which is also the first pass of cs_dbscan (dbscan.hip): the work
// list, the distance chain, the exhaustive kernel k_out_count and the grid kernel k_out_count_grid, written once.  Both units
// include this file and each compiles its own copy of the two kernels (an unnamed namespace); the bits are those of the
// header comment of cs_outlier_radius in include/corsair_hip.h whichever unit launches them.
#pragma once
#include <vector>

#include "cellgrid.h"
#include "nn_common.h"
#include "normals_grid.h"

namespace cs {
namespace {

constexpr int OUT_ROWS = 256;   // rows per workgroup
constexpr int OUT_TT = 512;     // segment rows per LDS stage

// A segment of fewer rows than this goes to the exhaustive kernel: NRM_GRID_MIN of normals.hip (one LDS stage of the
// scan), taken over as it is.  It has not been tuned, there or here.
constexpr int OUT_GRID_MIN = OUT_TT + 1;

struct OutWork {
  int64_t seg0;   // first row of the segment (global)
  int32_t sn;     // rows of the segment
  int32_t r0;     // first row of this workgroup, local to the segment
  int32_t seg;    // the segment (of the call, or of the chunk for a gated launch)
  int32_t pad;
};

__device__ __forceinline__ double out_d2(const float* __restrict__ t, double x, double y, double z) {
  const double dx = (double)t[0] - x, dy = (double)t[1] - y, dz = (double)t[2] - z;
  return fma(dz, dz, fma(dy, dy, dx * dx));
}

__global__ __launch_bounds__(OUT_ROWS) void k_out_count(const OutWork* __restrict__ work, const float* __restrict__ xyz,
                                                        double r2, int nb_points, int32_t* __restrict__ count,
                                                        uint8_t* __restrict__ keep) {
  __shared__ float t_lds[OUT_TT * 3];
  const OutWork wk = work[blockIdx.x];
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
  int c = 0;
  for (int tbase = 0; tbase < wk.sn; tbase += OUT_TT) {
    const int tcount = min(OUT_TT, wk.sn - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * 3; i += OUT_ROWS) t_lds[i] = seg[(int64_t)tbase * 3 + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) c += out_d2(t_lds + 3 * j, x, y, z) < r2 ? 1 : 0;   // false for NaN, and for inf < inf
  }
  if (!active) return;
  count[wk.seg0 + row] = c;
  if (keep) keep[wk.seg0 + row] = c > nb_points ? 1 : 0;
}

// the hybrid grid (cells of radius (1 + 2^-10)) is complete for d2 < r2: nothing to vouch for, nothing to redo
__global__ __launch_bounds__(OUT_ROWS) void k_out_count_grid(CellTable tb, const float* __restrict__ sxyz,
                                                             const int32_t* __restrict__ sj,
                                                             const uint64_t* __restrict__ skeys, int64_t m_total,
                                                             const int64_t* __restrict__ off,
                                                             const NrmSeg* __restrict__ segs, int nb_points,
                                                             int32_t* __restrict__ count, uint8_t* __restrict__ keep) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= m_total) return;
  const int p = (int)(skeys[m] >> 48);
  const NrmSeg sg = segs[p];
  if (!(sg.cell > 0.0)) return;
  const double x = (double)sxyz[3 * m], y = (double)sxyz[3 * m + 1], z = (double)sxyz[3 * m + 2];
  int c = 0;
  cg_probe<3>(
      tb, sxyz, p, x, y, z, sg.cell, sg.r2, [&](const float* t) { return out_d2(t, x, y, z); },
      [&](double, int32_t) { ++c; });
  const int64_t g = off[p] + sj[m];
  count[g] = c;
  if (keep) keep[g] = c > nb_points ? 1 : 0;
}

[[maybe_unused]] void push_work(std::vector<OutWork>& work, int64_t seg0, int64_t sn, int seg) {
  for (int64_t r = 0; r < sn; r += OUT_ROWS) work.push_back(OutWork{seg0, (int32_t)sn, (int32_t)r, (int32_t)seg, 0});
}

// checks the offset table; rows = the rows of the call
[[maybe_unused]] int check_segments(const char* who, const int64_t* h_off, int n_seg, int64_t* rows) {
  CS_REQUIRE(h_off, CS_ERR_INVALID, "%s: NULL offset table", who);
  CS_REQUIRE(n_seg >= 0, CS_ERR_INVALID, "%s: negative segment count", who);
  *rows = 0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    CS_REQUIRE(h_off[sg] >= 0 && sn >= 0, CS_ERR_INVALID, "%s: bad segment %d", who, sg);
    CS_REQUIRE(sn < (1LL << 31), CS_ERR_UNSUPPORTED, "%s: segment %d has 2^31 rows or more", who, sg);
    *rows += sn;
  }
  return CS_OK;
}

// The chunks of a call (normals_grid.h): consecutive segments [sg0, sg1), at most NRM_CHUNK_SEGS of them and at most
// NRM_CHUNK_ROWS rows unless one segment alone has more.  Returns sg1; *any = a segment of grid_min rows or more is in it.
[[maybe_unused]] int next_chunk(const int64_t* h_off, int n_seg, int sg0, int grid_min, bool* any) {
  int sg1 = sg0;
  *any = false;
  while (sg1 < n_seg && sg1 - sg0 < NRM_CHUNK_SEGS && (sg1 == sg0 || h_off[sg1 + 1] - h_off[sg0] <= NRM_CHUNK_ROWS)) {
    *any = *any || h_off[sg1 + 1] - h_off[sg1] >= grid_min;
    ++sg1;
  }
  return sg1;
}

}  // namespace
}  // namespace cs
