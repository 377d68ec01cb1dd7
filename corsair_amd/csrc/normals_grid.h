// The sorted cell grid of a chunk of segments as normals.hip builds it, for the units that probe it:
// normals.hip (cs_estimate_normals, cs_estimate_normals_hybrid) and fpfh.hip (cs_fpfh).  The kernels are defined once, in
// normals.hip; nrm_grid_build enqueues them.
#pragma once
#include "cellgrid.h"

namespace cs {

// what the grid kernels know of a chunk segment (written on the device: no host wait)
struct NrmSeg {
  double cell;   // cell size; 0 = the segment is not on the grid (the exhaustive kernel answers it)
  double r2;     // the probe's strict bound on d2: radius^2 (hybrid), the covered distance squared (k-NN)
};

constexpr int NRM_CHUNK_SEGS = 65535;        // chunk segments 0..65534: (65535, 32767, 32767, 32767) is kEmptyKey
constexpr int64_t NRM_CHUNK_ROWS = 1LL << 30;   // rows of a chunk of more than one segment; one segment (< 2^31) is a chunk

// A chunk = consecutive segments of the call, at most NRM_CHUNK_SEGS of them and fewer than 2^31 rows; its rows are the
// consecutive global rows [off[0], off[n_seg]).  The scratch lives as long as the object.
struct NrmGrid {
  int64_t m_total = 0;
  PoolBuf<int64_t> doff;     // the chunk's n_seg + 1 global offsets
  PoolBuf<NrmSeg> segs;      // [n_seg]
  PoolBuf<uint64_t> skeys;   // [m_total] sorted keys (chunk segment, cell)
  PoolBuf<int32_t> sj;       // [m_total] the sorted rows' rows local to their segments
  PoolBuf<float> sxyz;       // [m_total, 3] the sorted rows' coordinates
  PoolBuf<uint64_t> tkeys;   // the table
  PoolBuf<int32_t> tbeg, tend;
  uint64_t cap = 0;
  CellTable table() const { return CellTable{tkeys.p, tbeg.p, tend.p, cap - 1}; }
};

// Builds the grid of one chunk on s; nothing waits.  k = 0: every segment of grid_min rows or more gets (cell, r2), the
// hybrid rule; k > 0: the segments' cells come from their bounding boxes (k_nrm_segs).  `who` prefixes the error text.
int nrm_grid_build(NrmGrid& g, const float* d_xyz, const int64_t* h_off, int n_seg, int grid_min, int k, double cell,
                   double r2, hipStream_t s, const char* who);

}  // namespace cs
