// The cell grid that pairs.hip (cs_radius_pairs, f64 training clouds) and normals.hip (cs_estimate_normals_hybrid, f32
// rows) share: rows sorted by (problem, cell), an open-addressing table from a cell's key to its [begin, end) range of
// the sorted rows, and the 27-cell probe.
//
// cell = floor(x / c) with c slightly larger than the radius r (the callers use r (1 + 2^-10)).  Completeness of the 27
// cells: a pair with d2 < r2 has |dx| <= r (1 + 2^-50) in every coordinate (the distance chains are within 4 * 2^-53
// relative of the true sum of squares), so the true quotients differ by less than 1 - 2^-11; each computed quotient is
// within 2^-53 relative of the true one, below 2^-37 absolute inside the key range, so the two floors differ by at most
// one.  Cells are clamped to the 16-bit key range: clamping is monotone, so neighbours stay neighbours (or share a
// cell) and the search stays exact for any coordinates, only slower for far-out points.
//
// The kernels that build the table are defined once, in pairs.hip, and reached through the two launchers below.
#pragma once
#include "common.h"

namespace cs {

__device__ __forceinline__ int cg_cell(double x, double cell) {
  double q = floor(x / cell);
  if (!(q >= -32767.0)) q = -32767.0;   // also NaN: such a point never passes d2 < r2
  if (q > 32767.0) q = 32767.0;
  return (int)q;
}

struct CellTable {
  const uint64_t* keys;   // [mask + 1], kEmptyKey = free
  const int32_t* beg;     // first sorted row of the slot's cell
  const int32_t* end;     // one past its last
  uint64_t mask;
};

// The [beg, end) range of the sorted rows of cell (x, y, z) of problem p; false when the cell holds no row or lies outside
// the key range.  cg_probe's lookup, also for callers that walk a cell's rows themselves (fpfh.hip: a wave per query).
__device__ __forceinline__ bool cg_lookup(const CellTable& tb, int p, int x, int y, int z, int32_t& beg, int32_t& end) {
  if (x < -32767 || x > 32767 || y < -32767 || y > 32767 || z < -32767 || z > 32767) return false;
  const uint64_t key = pack_key(p, x, y, z);
  uint64_t slot = hash64(key) & tb.mask;
  uint64_t k;
  while ((k = tb.keys[slot]) != key && k != kEmptyKey) slot = (slot + 1) & tb.mask;
  if (k != key) return false;
  beg = tb.beg[slot];
  end = tb.end[slot];
  return true;
}

// Calls f(d2, m) for every sorted row m of problem p in the 27 cells around (qx, qy, qz) with d2 < r2, in no particular
// order.  rows = the sorted coordinates, STRIDE values of T per row; d2_of(t) is the caller's distance chain from the
// query to the row at t (pairs.hip and normals.hip each keep their own).  NaN and, for a finite r2, inf never pass.
template <int STRIDE, typename T, typename D, typename F>
__device__ __forceinline__ void cg_probe(const CellTable& tb, const T* __restrict__ rows, int p, double qx, double qy,
                                         double qz, double cell, double r2, D&& d2_of, F&& f) {
  const int cx = cg_cell(qx, cell), cy = cg_cell(qy, cell), cz = cg_cell(qz, cell);
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int x = cx + dx, y = cy + dy, z = cz + dz;
        int32_t b, e;
        if (!cg_lookup(tb, p, x, y, z, b, e)) continue;
        for (int32_t m = b; m < e; ++m) {
          const double d2 = d2_of(rows + (int64_t)STRIDE * m);
          if (d2 < r2) f(d2, m);
        }
      }
}

// keys[0, cap) = kEmptyKey (k_cg_table_fill).  Launch only: the caller's launch check covers it.
void cellgrid_table_fill(uint64_t* d_keys, uint64_t cap, hipStream_t s);
// Every run of equal keys of the sorted skeys[0, m_total) (one cell of one problem) is inserted with its [begin, end)
// range (k_cg_insert); cap = mask + 1 is a power of two >= 2 * m_total.  Launch only.
void cellgrid_insert_ranges(const uint64_t* d_skeys, int64_t m_total, uint64_t* d_keys, int32_t* d_beg, int32_t* d_end,
                            uint64_t mask, hipStream_t s);

}  // namespace cs
