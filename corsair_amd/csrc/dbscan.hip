// Scan clustering: DBSCAN per segment and the mask of the largest cluster.  The specifications are the comments
// of cs_dbscan and cs_cluster_largest in include/corsair_hip.h; tests/dbscan_ref.py restates them.
//
// A call is cut into the chunks of normals_grid.h and every chunk runs seven steps, all enqueued on the caller's stream:
//   1 count    cs_outlier_radius' count (outlier_count.h: the same kernels), its keep mask = the CORE flag
//   2 init     parent[i] = i
//   3 hook     every core row unites its tree with those of its core neighbours of smaller row index (lock-free)
//   4 compress label = the root of the row's tree (a launch of its own: the trees are final), flag = the row is a root
//   5 scan     one exclusive sum of the flags (hipcub)
//   6 number   label = scan[root] - scan[first row of the segment]: clusters ascend with their smallest core row
//   7 border   a non-core row with a neighbour takes the label of its core neighbour of smallest (d2, row)
// Steps 1, 3 and 7 visit the rows with d2 < r2 and exist in two shapes with the same visitor: the exhaustive scan of the
// row's segment staged through LDS (k_out_count's shape; the definition) and the 27-cell probe of the sorted cell grid that
// normals.hip builds (normals_grid.h, cg_probe of cellgrid.h; complete for d2 < r2 by cellgrid.h's argument).  With k = 0
// nrm_grid_build puts every segment of OUT_GRID_MIN rows or more on the grid (NrmSeg.cell > 0) and no other, so the host's
// split into the two shapes is the device's and no gated launch is needed.
// Inside a chunk every array is indexed by the row local to the chunk; parent, root and the neighbour indices are rows
// local to their SEGMENT (below 2^31).
#include <math.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "cellgrid.h"
#include "nn_common.h"
#include "normals_grid.h"
#include "outlier_count.h"

namespace cs {
namespace {

// ---- the union-find ----------------------------------------------------------------------------------------------------
// par = the parent array of ONE segment, indexed by local row.  Invariants, at every moment of the hook kernel:
//   (a) par[x] <= x, and par[x] only ever decreases: every write is an atomicMin, of a value below the one the writer saw;
//   (b) par[x] is a core row of the same component as x (it was reached from x through parent links and d2 < r2 edges).
// By (a) the links form a forest whose roots are par[x] == x and a walk upwards strictly descends, so db_find ends after at
// most x steps whatever it reads.
// Stale reads: the loads are relaxed and may return an older value of par[x].  By (a) an older value is a LARGER index that
// was x's parent earlier: an older ancestor in the same tree (b).  db_find may therefore return a node that is no longer a
// root, and the halving may write a grandparent that is not the newest: both stay inside the component and keep (a).
// Nothing is decided on a read alone: the only step that joins two trees is the atomicMin in db_unite, whose returned
// value is the true one.
// Connectivity: a link x -> p is only ever replaced by x -> q with q < p where the writer either saw p -> ... -> q
// (halving) or goes on to unite p with q itself (db_unite, below): every link ever observed stays implied by the links
// and the unions still owed by running threads, and when the kernel ends nothing is owed.
// Termination of db_unite: the pair (a, b), a > b, is replaced by (old, b) with old < a read by the atomic, then by their
// roots, which are no larger: max(a, b) strictly decreases on every retry, so a call ends after at most a retries.  No
// thread waits for another: there is no lock, no flag to spin on and no barrier between workgroups; a thread that loses a
// race has been handed a strictly smaller problem by the winner's write.
// When the kernel has ended every tree is a component of the core rows and, by (a), its root is the component's smallest row.
__device__ __forceinline__ int32_t db_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// path halving: x's parent becomes its grandparent, then x = the grandparent
__device__ __forceinline__ int32_t db_find(int32_t* par, int32_t x) {
  for (;;) {
    const int32_t p = db_load(par + x);
    if (p == x) return x;
    const int32_t gp = db_load(par + p);
    if (gp == p) return p;
    atomicMin(par + x, gp);   // gp < p: never raises par[x], also when another thread has lowered it meanwhile
    x = gp;
  }
}

__device__ __forceinline__ void db_unite(int32_t* par, int32_t a, int32_t b) {
  for (;;) {
    a = db_find(par, a);
    b = db_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = atomicMin(par + a, b);   // device scope
    if (old == a) return;                        // a was a root and hangs under b now
    a = old;   // a had a parent already (old < a).  If b < old the write has replaced the link a -> old by a -> b: uniting
               // old with b restores it.  If old <= b nothing was written and (old, b) is the union still owed.
  }
}

// f(d2, j) for every row j < rows of the segment with d2 < r2, ascending in j; every thread of the workgroup calls this
// (the stages are loaded together), the inactive ones visit nothing
template <typename F>
__device__ __forceinline__ void db_scan(const float* __restrict__ seg, int rows, float* t_lds, bool active, double x,
                                        double y, double z, double r2, F&& f) {
  const int tid = threadIdx.x;
  for (int tbase = 0; tbase < rows; tbase += OUT_TT) {
    const int tcount = min(OUT_TT, rows - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * 3; i += OUT_ROWS) t_lds[i] = seg[(int64_t)tbase * 3 + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) {
      const double d = out_d2(t_lds + 3 * j, x, y, z);
      if (d < r2) f(d, tbase + j);   // false for NaN, and for inf < inf
    }
  }
}

__global__ __launch_bounds__(OUT_ROWS) void k_db_init(const OutWork* __restrict__ work, int32_t* __restrict__ parent) {
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  if (row < wk.sn) parent[wk.seg0 + row] = row;
}

// Step 3, the scan.  Only rows below the workgroup's last can have a smaller index than one of its rows.
__global__ __launch_bounds__(OUT_ROWS) void k_db_hook(const OutWork* __restrict__ work, const float* __restrict__ xyz,
                                                      double r2, const uint8_t* __restrict__ core, int32_t* parent) {
  __shared__ float t_lds[OUT_TT * 3];
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  const bool active = row < wk.sn && core[wk.seg0 + row];
  const float* seg = xyz + wk.seg0 * 3;
  double x = 0, y = 0, z = 0;
  if (active) {
    x = (double)seg[3 * (int64_t)row + 0];
    y = (double)seg[3 * (int64_t)row + 1];
    z = (double)seg[3 * (int64_t)row + 2];
  }
  const uint8_t* score = core + wk.seg0;
  int32_t* par = parent + wk.seg0;
  db_scan(seg, min(wk.sn, wk.r0 + OUT_ROWS), t_lds, active, x, y, z, r2, [&](double, int j) {
    if (j < row && score[j]) db_unite(par, row, j);
  });
}

// Step 3, the grid: one thread per sorted row of the chunk (k_out_count_grid's shape)
__global__ __launch_bounds__(OUT_ROWS) void k_db_hook_grid(CellTable tb, const float* __restrict__ sxyz,
                                                           const int32_t* __restrict__ sj,
                                                           const uint64_t* __restrict__ skeys, int64_t m_total,
                                                           const int64_t* __restrict__ off,
                                                           const NrmSeg* __restrict__ segs,
                                                           const uint8_t* __restrict__ core, int32_t* parent) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= m_total) return;
  const int p = (int)(skeys[m] >> 48);
  const NrmSeg sg = segs[p];
  if (!(sg.cell > 0.0)) return;
  const int64_t seg0 = off[p];
  const int row = sj[m];
  if (!core[seg0 + row]) return;
  const double x = (double)sxyz[3 * m], y = (double)sxyz[3 * m + 1], z = (double)sxyz[3 * m + 2];
  const uint8_t* score = core + seg0;
  int32_t* par = parent + seg0;
  cg_probe<3>(
      tb, sxyz, p, x, y, z, sg.cell, sg.r2, [&](const float* t) { return out_d2(t, x, y, z); },
      [&](double, int32_t mm) {
        const int j = sj[mm];
        if (j < row && score[j]) db_unite(par, row, j);
      });
}

// Step 4.  The hook kernel has ended: plain loads, no write to parent.  label = the root (core rows) or -1.
__global__ __launch_bounds__(OUT_ROWS) void k_db_compress(const OutWork* __restrict__ work,
                                                          const uint8_t* __restrict__ core,
                                                          const int32_t* __restrict__ parent, int32_t* __restrict__ label,
                                                          int32_t* __restrict__ flag) {
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  if (row >= wk.sn) return;
  const int64_t g = wk.seg0 + row;
  int32_t root = -1;
  if (core[g]) {
    const int32_t* par = parent + wk.seg0;
    root = row;
    for (int32_t p = par[root]; p != root; p = par[root]) root = p;
  }
  label[g] = root;
  flag[g] = root == row ? 1 : 0;
}

// Step 6: pos = the exclusive sum of flag over the chunk
__global__ __launch_bounds__(OUT_ROWS) void k_db_number(const OutWork* __restrict__ work, const int32_t* __restrict__ pos,
                                                        int32_t* __restrict__ label) {
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  if (row >= wk.sn) return;
  const int32_t root = label[wk.seg0 + row];
  if (root >= 0) label[wk.seg0 + row] = pos[wk.seg0 + root] - pos[wk.seg0];
}

// one atomic per wave
__device__ __forceinline__ void db_count_borders(bool is_border, unsigned long long* stats) {
  const unsigned long long mask = __ballot(is_border);
  if (mask && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1)
    atomicAdd(stats, (unsigned long long)__popcll(mask));
}

// Step 7, the scan.  The core rows' labels are final and only non-core rows are written: label is read and written by
// different rows.  The scan ascends in j, so d < bd alone keeps the smaller row of a tie.
__global__ __launch_bounds__(OUT_ROWS) void k_db_border(const OutWork* __restrict__ work, const float* __restrict__ xyz,
                                                        double r2, const uint8_t* __restrict__ core,
                                                        const int32_t* __restrict__ count, int32_t* label,
                                                        unsigned long long* stats) {
  __shared__ float t_lds[OUT_TT * 3];
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  const bool active = row < wk.sn && !core[wk.seg0 + row] && count[wk.seg0 + row] > 1;
  const float* seg = xyz + wk.seg0 * 3;
  double x = 0, y = 0, z = 0;
  if (active) {
    x = (double)seg[3 * (int64_t)row + 0];
    y = (double)seg[3 * (int64_t)row + 1];
    z = (double)seg[3 * (int64_t)row + 2];
  }
  const uint8_t* score = core + wk.seg0;
  double bd = INFINITY;
  int bj = -1;
  db_scan(seg, wk.sn, t_lds, active, x, y, z, r2, [&](double d, int j) {
    if (score[j] && (bj < 0 || d < bd)) {
      bd = d;
      bj = j;
    }
  });
  if (bj >= 0) label[wk.seg0 + row] = label[wk.seg0 + bj];
  if (stats) db_count_borders(bj >= 0, stats);
}

// Step 7, the grid: the probe visits in no particular order, the full (d2, row) pair decides
__global__ __launch_bounds__(OUT_ROWS) void k_db_border_grid(CellTable tb, const float* __restrict__ sxyz,
                                                             const int32_t* __restrict__ sj,
                                                             const uint64_t* __restrict__ skeys, int64_t m_total,
                                                             const int64_t* __restrict__ off,
                                                             const NrmSeg* __restrict__ segs,
                                                             const uint8_t* __restrict__ core,
                                                             const int32_t* __restrict__ count, int32_t* label,
                                                             unsigned long long* stats) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int bj = -1;
  int64_t seg0 = 0;
  int row = 0;
  if (m < m_total) {
    const int p = (int)(skeys[m] >> 48);
    const NrmSeg sg = segs[p];
    seg0 = off[p];
    row = sj[m];
    if (sg.cell > 0.0 && !core[seg0 + row] && count[seg0 + row] > 1) {
      const double x = (double)sxyz[3 * m], y = (double)sxyz[3 * m + 1], z = (double)sxyz[3 * m + 2];
      const uint8_t* score = core + seg0;
      double bd = INFINITY;
      cg_probe<3>(
          tb, sxyz, p, x, y, z, sg.cell, sg.r2, [&](const float* t) { return out_d2(t, x, y, z); },
          [&](double d, int32_t mm) {
            const int j = sj[mm];
            if (score[j] && (bj < 0 || d < bd || (d == bd && j < bj))) {
              bd = d;
              bj = j;
            }
          });
    }
  }
  if (bj >= 0) label[seg0 + row] = label[seg0 + bj];
  if (stats) db_count_borders(bj >= 0, stats);
}

// ---- the largest cluster -----------------------------------------------------------------------------------------------
// size = one counter per row, zeroed by the caller: the rows of cluster id of a segment are counted at seg0 + id.
__device__ __forceinline__ bool cl_valid(int32_t l, int32_t sn) { return l >= 0 && l < sn; }

__global__ __launch_bounds__(OUT_ROWS) void k_cl_sizes(const OutWork* __restrict__ work, const int32_t* __restrict__ label,
                                                       int32_t* __restrict__ size) {
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  if (row >= wk.sn) return;
  const int32_t l = label[wk.seg0 + row];
  if (cl_valid(l, wk.sn)) atomicAdd(&size[wk.seg0 + l], 1);
}

// acc = two u64 per segment, zeroed by the caller: [0] the maximum of (size << 32 | ~id) over the ids with a row -- the
// largest size, of equal sizes the smallest id -- and [1] the number of such ids.  A maximum and a sum of integers: the
// same values in any order.
__global__ __launch_bounds__(OUT_ROWS) void k_cl_max(const OutWork* __restrict__ work, const int32_t* __restrict__ size,
                                                     unsigned long long* __restrict__ acc) {
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  const int32_t v = row < wk.sn ? size[wk.seg0 + row] : 0;
  unsigned long long key = v > 0 ? ((unsigned long long)v << 32) | (unsigned long long)(0xffffffffu - (unsigned)row) : 0ull;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  const unsigned long long cnt = (unsigned long long)__popcll(__ballot(v > 0));
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicMax(&acc[2 * (int64_t)wk.seg + 0], key);
    atomicAdd(&acc[2 * (int64_t)wk.seg + 1], cnt);
  }
}

// one thread per segment: stat = (clusters, id of the largest, its size); (0, -1, 0) without a cluster
__global__ void k_cl_finish(const unsigned long long* __restrict__ acc, int n_seg, int32_t* __restrict__ stat) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_seg) return;
  const unsigned long long key = acc[2 * (int64_t)p], cnt = acc[2 * (int64_t)p + 1];
  stat[3 * (int64_t)p + 0] = (int32_t)cnt;
  stat[3 * (int64_t)p + 1] = cnt ? (int32_t)(0xffffffffu - (unsigned)(key & 0xffffffffull)) : -1;
  stat[3 * (int64_t)p + 2] = (int32_t)(key >> 32);
}

__global__ __launch_bounds__(OUT_ROWS) void k_cl_keep(const OutWork* __restrict__ work, const int32_t* __restrict__ label,
                                                      const int32_t* __restrict__ stat, uint8_t* __restrict__ keep) {
  const OutWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  if (row >= wk.sn) return;
  const int32_t l = label[wk.seg0 + row];
  keep[wk.seg0 + row] = cl_valid(l, wk.sn) && l == stat[3 * (int64_t)wk.seg + 1] ? 1 : 0;
}

// ---- host --------------------------------------------------------------------------------------------------------------
std::atomic<unsigned long long> g_dbscan_stats[2];

// One chunk: xyz, label and count (or NULL) point at the chunk's first row, off = its n_seg + 1 offsets from that row.
int dbscan_chunk(const float* xyz, const std::vector<int64_t>& off, bool use_grid, double cell, double r2, int min_points,
                 int32_t* label, int32_t* count, unsigned long long* d_stats, hipStream_t s) {
  const char* who = "cs_dbscan: scratch allocation failed";
  const int n_seg = (int)off.size() - 1;
  const int64_t m_total = off[n_seg];
  if (m_total == 0) return CS_OK;
  std::vector<OutWork> all, scan;
  bool grid = false;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = off[sg + 1] - off[sg];
    push_work(all, off[sg], sn, sg);
    if (use_grid && sn >= OUT_GRID_MIN)
      grid = true;
    else
      push_work(scan, off[sg], sn, sg);
  }
  PoolBuf<OutWork> d_all, d_scan;
  int rc = upload(d_all, all, s);
  if (!rc && !scan.empty()) rc = upload(d_scan, scan, s);
  if (rc) return rc;
  PoolBuf<uint8_t> core(m_total);
  PoolBuf<int32_t> parent(m_total), flag(m_total), pos(m_total), own_count;
  if (!count) count = own_count.alloc(m_total) ? own_count.p : nullptr;
  CS_REQUIRE(core.p && parent.p && flag.p && pos.p && count, CS_ERR_HIP, "%s", who);
  NrmGrid gr;
  if (grid) {
    rc = nrm_grid_build(gr, xyz, off.data(), n_seg, OUT_GRID_MIN, 0, cell, r2, s, who);
    if (rc) return rc;
  }
  const dim3 block(OUT_ROWS), g_all((unsigned)all.size()), g_scan((unsigned)scan.size());
  const dim3 g_grid((unsigned)ceil_div(m_total, OUT_ROWS));
  const CellTable tb = gr.table();
  const float* sxyz = gr.sxyz.p;
  const int32_t* sj = gr.sj.p;
  const uint64_t* skeys = gr.skeys.p;
  const int64_t* doff = gr.doff.p;
  const NrmSeg* segs = gr.segs.p;
  // 1 count, 2 init
  if (!scan.empty())
    hipLaunchKernelGGL(k_out_count, g_scan, block, 0, s, (const OutWork*)d_scan.p, xyz, r2, min_points - 1, count, core.p);
  if (grid)
    hipLaunchKernelGGL(k_out_count_grid, g_grid, block, 0, s, tb, sxyz, sj, skeys, m_total, doff, segs, min_points - 1,
                       count, core.p);
  hipLaunchKernelGGL(k_db_init, g_all, block, 0, s, (const OutWork*)d_all.p, parent.p);
  // 3 hook
  if (!scan.empty())
    hipLaunchKernelGGL(k_db_hook, g_scan, block, 0, s, (const OutWork*)d_scan.p, xyz, r2, (const uint8_t*)core.p, parent.p);
  if (grid)
    hipLaunchKernelGGL(k_db_hook_grid, g_grid, block, 0, s, tb, sxyz, sj, skeys, m_total, doff, segs,
                       (const uint8_t*)core.p, parent.p);
  // 4 compress, 5 scan, 6 number
  hipLaunchKernelGGL(k_db_compress, g_all, block, 0, s, (const OutWork*)d_all.p, (const uint8_t*)core.p,
                     (const int32_t*)parent.p, label, flag.p);
  CS_LAUNCH_CHECK();
  size_t tmp_bytes = 0;
  CS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, flag.p, pos.p, (int)m_total, s));
  PoolBuf<char> tmp(tmp_bytes);
  CS_REQUIRE(tmp.p, CS_ERR_HIP, "%s", who);
  CS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, flag.p, pos.p, (int)m_total, s));
  hipLaunchKernelGGL(k_db_number, g_all, block, 0, s, (const OutWork*)d_all.p, (const int32_t*)pos.p, label);
  // 7 border
  if (!scan.empty())
    hipLaunchKernelGGL(k_db_border, g_scan, block, 0, s, (const OutWork*)d_scan.p, xyz, r2, (const uint8_t*)core.p,
                       (const int32_t*)count, label, d_stats);
  if (grid)
    hipLaunchKernelGGL(k_db_border_grid, g_grid, block, 0, s, tb, sxyz, sj, skeys, m_total, doff, segs,
                       (const uint8_t*)core.p, (const int32_t*)count, label, d_stats);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_dbscan(const float* d_xyz, const int64_t* h_off, int n_seg, double eps, int min_points, int32_t* d_label,
              int32_t* d_count, void* stream) {
  int64_t rows = 0;
  int rc = check_segments("cs_dbscan", h_off, n_seg, &rows);
  if (rc) return rc;
  CS_REQUIRE(eps > 0.0 && eps <= 1.7976931348623157e308, CS_ERR_INVALID, "cs_dbscan: eps must be positive and finite");
  CS_REQUIRE(min_points >= 1, CS_ERR_INVALID, "cs_dbscan: min_points must be at least 1");
  if (rows == 0) return CS_OK;
  CS_REQUIRE(d_xyz && d_label, CS_ERR_INVALID, "cs_dbscan: NULL argument");
  const double r2 = eps * eps;   // +inf for an eps above 1.3e154: every finite d2 passes; 0 below 1.5e-162: none
  const double cell = eps * (1.0 + 1.0 / 1024.0);   // a little larger than eps (cellgrid.h)
  const bool use_grid = !env_first_is("CS_DBSCAN_GRID", '0') && eps < 1e150;
  const bool want_stats = env_first_is("CS_DBSCAN_STATS", '1');
  int64_t grid_rows = 0;
  double flop = 0.0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    if (use_grid && sn >= OUT_GRID_MIN) {
      grid_rows += sn;
      flop += 3.0 * 8.0 * 27.0 * (double)sn;   // nominal, three probes: the cells' occupancy is not known on the host
    } else {
      flop += 3.0 * 8.0 * (double)sn * (double)sn;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<unsigned long long> dstats;
  if (want_stats) {
    CS_REQUIRE(dstats.alloc(1), CS_ERR_HIP, "cs_dbscan: scratch allocation failed");
    CS_HIP_CHECK(hipMemsetAsync(dstats.p, 0, sizeof(unsigned long long), s));
  }
  {
    ProfScope prof("cluster", s, flop);
    std::vector<int64_t> off;
    for (int sg0 = 0; sg0 < n_seg;) {
      bool any = false;
      const int sg1 = next_chunk(h_off, n_seg, sg0, OUT_GRID_MIN, &any);
      const int64_t base = h_off[sg0];
      off.clear();
      for (int sg = sg0; sg <= sg1; ++sg) off.push_back(h_off[sg] - base);
      rc = dbscan_chunk(d_xyz + 3 * base, off, use_grid, cell, r2, min_points, d_label + base,
                        d_count ? d_count + base : nullptr, dstats.p, s);
      if (rc) return rc;
      sg0 = sg1;
    }
  }
  if (want_stats) {
    unsigned long long h = 0;
    CS_HIP_CHECK(download_async(&h, dstats.p, sizeof(h), s));
    CS_HIP_CHECK(download_sync(s));
    g_dbscan_stats[0] += (unsigned long long)grid_rows;   // the grid is complete: none recomputed
    g_dbscan_stats[1] += h;
  }
  return CS_OK;
}

int cs_cluster_largest(const int32_t* d_label, const int64_t* h_off, int n_seg, uint8_t* d_keep, int32_t* d_stat,
                       void* stream) {
  int64_t rows = 0;
  int rc = check_segments("cs_cluster_largest", h_off, n_seg, &rows);
  if (rc) return rc;
  if (n_seg == 0) return CS_OK;
  CS_REQUIRE(d_stat, CS_ERR_INVALID, "cs_cluster_largest: NULL argument");
  CS_REQUIRE(rows == 0 || (d_label && d_keep), CS_ERR_INVALID, "cs_cluster_largest: NULL argument");
  const int64_t base = h_off[0];
  const int64_t span = h_off[n_seg] - base;   // the counters cover the rows between the first and the last offset
  std::vector<OutWork> work;
  for (int sg = 0; sg < n_seg; ++sg) push_work(work, h_off[sg] - base, h_off[sg + 1] - h_off[sg], sg);
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<OutWork> dwork;
  PoolBuf<int32_t> size(std::max<int64_t>(span, 1));
  PoolBuf<unsigned long long> acc(2 * (size_t)n_seg);
  CS_REQUIRE(size.p && acc.p, CS_ERR_HIP, "cs_cluster_largest: scratch allocation failed");
  if (!work.empty()) {
    rc = upload(dwork, work, s);
    if (rc) return rc;
    CS_HIP_CHECK(hipMemsetAsync(size.p, 0, (size_t)span * sizeof(int32_t), s));
  }
  CS_HIP_CHECK(hipMemsetAsync(acc.p, 0, 2 * (size_t)n_seg * sizeof(unsigned long long), s));
  ProfScope prof("cluster", s, 4.0 * (double)rows);
  const dim3 grid((unsigned)work.size()), block(OUT_ROWS);
  const int32_t* label = d_label ? d_label + base : nullptr;
  if (!work.empty()) {
    hipLaunchKernelGGL(k_cl_sizes, grid, block, 0, s, (const OutWork*)dwork.p, label, size.p);
    hipLaunchKernelGGL(k_cl_max, grid, block, 0, s, (const OutWork*)dwork.p, (const int32_t*)size.p, acc.p);
  }
  hipLaunchKernelGGL(k_cl_finish, dim3((unsigned)ceil_div(n_seg, 256)), dim3(256), 0, s, (const unsigned long long*)acc.p,
                     n_seg, d_stat);
  if (!work.empty())
    hipLaunchKernelGGL(k_cl_keep, grid, block, 0, s, (const OutWork*)dwork.p, label, (const int32_t*)d_stat, d_keep + base);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

void cs_dbscan_stats(uint64_t out[2], int reset) { read_stats(g_dbscan_stats, out, reset); }

}  // extern "C"
