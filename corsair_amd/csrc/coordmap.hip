// Coordinate maps: hash-indexed COO coordinates (the kernel maps built on them are in kernelmap.hip).
//
// Replaces the coordinate manager of MinkowskiEngine as used by the reference
// (evaluation.py:215-218; model/resunet.py:49-193).  Data layout in HBM:
//   coords  int32 [n,4]  (batch, x, y, z), row order = tensor row order
//   keys    uint64 [cap] open-addressing table (linear probing), cap = pow2 >= 2n, empty = ~0
//   vals    int32  [cap] row index of the key
//   seg     int32  [n_batch + 1] first row of every sample (rows grouped by sample), for the LDS kernel-map builder
// All of it is integer work bound by HBM/L2 latency, not MFMA; the tables of a batch-32 eval
// batch (145k voxels -> 4.7 MB of table) stay L2/Infinity-Cache resident between the insert
// and the 27 probes per output row.
#include <hipcub/hipcub.hpp>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "coordmap.h"

namespace cs {

// ---- the table operations of the insert / emit kernels ------------------------------------------------------------------
__device__ __forceinline__ unsigned long long cas_key(uint64_t* keys, uint64_t slot, uint64_t key) {
  return atomicCAS((unsigned long long*)&keys[slot], (unsigned long long)kEmptyKey, (unsigned long long)key);
}
// Claim or find the slot of `key`: CAS down the probe chain from `slot`.  Returns what the last CAS saw, kEmptyKey (the slot
// was claimed) or key (another row holds it); `slot` is that slot.  tried: the CAS at `slot` has been issued and saw `old`.
__device__ __forceinline__ unsigned long long claim_slot(uint64_t* keys, uint64_t mask, uint64_t key, uint64_t& slot,
                                                         bool tried = false, unsigned long long old = 0) {
  while (true) {
    if (tried) {
      if (old == kEmptyKey || old == key) return old;
      slot = (slot + 1) & mask;
    }
    old = cas_key(keys, slot, key);
    tried = true;
  }
}
// slot of a key that is known to be in the table
__device__ __forceinline__ uint64_t slot_of_present(const uint64_t* keys, uint64_t mask, uint64_t key) {
  uint64_t slot = hash64(key) & mask;
  while (keys[slot] != key) slot = (slot + 1) & mask;
  return slot;
}

// floor division for possibly negative a, b > 0
__device__ __forceinline__ int floor_div(int a, int b) {
  int q = a / b;
  int r = a % b;
  return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q;
}

// floor(a / cell) * cell; cell a power of two (every tensor stride of the ResUNet): a mask instead of the
// ~35-instruction run-time division
__device__ __forceinline__ int floor_to_cell(int a, int cell) {
  return (cell & (cell - 1)) == 0 ? (a & ~(cell - 1)) : floor_div(a, cell) * cell;
}

__global__ void k_fill_table(uint64_t* keys, int32_t* vals, uint64_t cap) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < cap; i += stride) {
    keys[i] = kEmptyKey;
    vals[i] = 0x7fffffff;
  }
}

// Insert key(row) with value = min row index.  cell > 1: key of the coarse cell.
// status[0] |= 1 on out-of-range coordinate; status[1] counts duplicate keys.
__global__ void k_insert(const int32_t* __restrict__ coords, int64_t n, int cell, uint64_t* keys,
                         int32_t* vals, uint64_t mask, int* status) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  int b = coords[4 * i + 0], x = coords[4 * i + 1], y = coords[4 * i + 2], z = coords[4 * i + 3];
  if (cell > 1) {
    x = floor_to_cell(x, cell);
    y = floor_to_cell(y, cell);
    z = floor_to_cell(z, cell);
  }
  if (!coord_in_range(b, x, y, z)) {
    atomicOr(&status[0], 1);
    return;
  }
  uint64_t key = pack_key(b, x, y, z);
  uint64_t slot = hash64(key) & mask;
  const unsigned long long old = claim_slot(keys, mask, key, slot);
  if (old == key) atomicAdd(&status[1], 1);
  atomicMin(&vals[slot], (int32_t)i);
}

// flag[i] = 1 iff row i is the first (minimum) row of its coarse cell.
__global__ void k_flag_first(const int32_t* __restrict__ coords, int64_t n, int cell,
                             const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                             uint64_t mask, int32_t* flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  int b = coords[4 * i + 0];
  int x = floor_to_cell(coords[4 * i + 1], cell);
  int y = floor_to_cell(coords[4 * i + 2], cell);
  int z = floor_to_cell(coords[4 * i + 3], cell);
  int32_t v = hash_lookup(keys, vals, mask, pack_key(b, x, y, z));
  flag[i] = (v == (int32_t)i) ? 1 : 0;
}

// Write coarse coordinates in first-occurrence order and re-point the table at the new rows.
__global__ void k_emit_strided(const int32_t* __restrict__ coords, int64_t n, int cell,
                               const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                               uint64_t* keys, int32_t* vals, uint64_t mask, int32_t* out_coords) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  int b = coords[4 * i + 0];
  int x = floor_to_cell(coords[4 * i + 1], cell);
  int y = floor_to_cell(coords[4 * i + 2], cell);
  int z = floor_to_cell(coords[4 * i + 3], cell);
  int32_t o = pos[i];
  out_coords[4 * o + 0] = b;
  out_coords[4 * o + 1] = x;
  out_coords[4 * o + 2] = y;
  out_coords[4 * o + 3] = z;
  vals[slot_of_present(keys, mask, pack_key(b, x, y, z))] = o;  // exactly one row per key reaches here
}

// ---- all coordinate levels of a batch in one pass (round 5: cs_coordmap_pyramid) -------------------------------------------
// The strided maps of a ResUNet batch (tensor strides 2, 4, 8) used to be a chain c1 -> c2 -> c4 -> c8 of
// insert / flag / scan / host round trip / emit, one link per level and one host wait per link, plus two more waits for the
// per-sample segments: six GPU-idle round trips and ~25 launches per forward.  The unique cells of stride 2^l in
// first-occurrence order are the same whether they are taken from the level below or from the stride-1 rows (the first
// stride-1 row of a coarse cell is also the first row of its finer cell, and every level keeps first-occurrence order), so
// all levels come from the stride-1 coordinates at once: one insert kernel (a thread reads its row once and has its four
// atomics in flight together), one flag kernel, ONE scan (the three flags packed as 21-bit fields of a 64-bit word), one
// emit kernel, the segment tables of all levels, and ONE host wait for the sizes.
constexpr int PYR_MAX_LEVELS = 4;
constexpr int PYR_FIELD = 21;                       // rows < 2^21: three counters in one 64-bit scan element
struct PyrLevel {
  uint64_t* keys;
  int32_t* vals;
  uint64_t mask;
  int32_t* coords;                                  // out (level >= 1)
  int32_t* seg;                                     // [n_batch + 1] or nullptr
  int cell;
};
struct PyrArgs {
  int n_levels;
  PyrLevel lv[PYR_MAX_LEVELS];
  int n_batch;
  int* status;                                      // [0] out of range, [1] duplicates, [2 + l] level l not grouped
  int32_t* counts;                                  // rows of level l (l >= 1)
};

// (the pyramid kernels are only launched for power-of-two cells -- cs_coordmap_pyramid takes the chained path otherwise --:
// a mask, without the division arm of floor_to_cell and the uniform branch around it)
__device__ __forceinline__ int floor_to_cell2(int a, int cell) { return a & ~(cell - 1); }
__device__ __forceinline__ uint64_t pyr_key(int b, int x, int y, int z, int cell) {
  return pack_key(b, floor_to_cell2(x, cell), floor_to_cell2(y, cell), floor_to_cell2(z, cell));
}

__global__ __launch_bounds__(256) void k_pyr_insert(const int32_t* __restrict__ coords, int64_t n, const PyrArgs a) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n) return;
  const int4 c = reinterpret_cast<const int4*>(coords)[i];
  // (the floor cells of an in-range coordinate are in range: |floor(x)| <= 32767 < 32768 needs x > -32768, checked here)
  if (!coord_in_range(c.x, c.y, c.z, c.w)) {
    atomicOr(&a.status[0], 1);
    return;
  }
  uint64_t key[PYR_MAX_LEVELS], slot[PYR_MAX_LEVELS];
  unsigned long long old[PYR_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < PYR_MAX_LEVELS; ++l)
    if (l < a.n_levels) {
      const int cell = a.lv[l].cell;
      // (a floor cell can fall on -32768 when the coordinate itself is in range: refused like cs_coordmap_stride does)
      if (l > 0 && !coord_in_range(c.x, floor_to_cell2(c.y, cell), floor_to_cell2(c.z, cell), floor_to_cell2(c.w, cell)))
        atomicOr(&a.status[0], 1);
      key[l] = pyr_key(c.x, c.y, c.z, c.w, cell);
      slot[l] = hash64(key[l]) & a.lv[l].mask;
      old[l] = cas_key(a.lv[l].keys, slot[l], key[l]);
    }
  // (all first CAS are in flight before any is retried)
#pragma unroll
  for (int l = 0; l < PYR_MAX_LEVELS; ++l)
    if (l < a.n_levels) {
      uint64_t sl = slot[l];   // (a local: with a reference into slot[] the retry loops compile to 50 more instructions)
      old[l] = claim_slot(a.lv[l].keys, a.lv[l].mask, key[l], sl, true, old[l]);
      slot[l] = sl;
      if (l == 0 && old[l] == key[l]) atomicAdd(&a.status[1], 1);   // level 0 keeps every row: a second one is a duplicate
      atomicMin(&a.lv[l].vals[slot[l]], (int32_t)i);
    }
}

// packed flags: bit field l - 1 = 1 iff row i is the first (minimum) row of its level-l cell
__global__ __launch_bounds__(256) void k_pyr_flag(const int32_t* __restrict__ coords, int64_t n, const PyrArgs a,
                                                  unsigned long long* __restrict__ flag) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n) return;
  const int4 c = reinterpret_cast<const int4*>(coords)[i];
  unsigned long long f = 0;
#pragma unroll
  for (int l = 1; l < PYR_MAX_LEVELS; ++l)
    if (l < a.n_levels) {
      const int32_t v = hash_lookup(a.lv[l].keys, a.lv[l].vals, a.lv[l].mask, pyr_key(c.x, c.y, c.z, c.w, a.lv[l].cell));
      if (v == (int32_t)i) f |= 1ULL << (PYR_FIELD * (l - 1));
    }
  flag[i] = f;
}

__global__ __launch_bounds__(256) void k_pyr_emit(const int32_t* __restrict__ coords, int64_t n, const PyrArgs a,
                                                  const unsigned long long* __restrict__ flag,
                                                  const unsigned long long* __restrict__ pos) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long f = flag[i], p = pos[i];
  if (i == n - 1) {
#pragma unroll
    for (int l = 1; l < PYR_MAX_LEVELS; ++l)
      if (l < a.n_levels)
        a.counts[l] = (int32_t)(((p + f) >> (PYR_FIELD * (l - 1))) & ((1ULL << PYR_FIELD) - 1));
  }
  if (!f) return;
  const int4 c = reinterpret_cast<const int4*>(coords)[i];
#pragma unroll
  for (int l = 1; l < PYR_MAX_LEVELS; ++l)
    if (l < a.n_levels && ((f >> (PYR_FIELD * (l - 1))) & 1ULL)) {
      const int cell = a.lv[l].cell;
      const int x = floor_to_cell2(c.y, cell), y = floor_to_cell2(c.z, cell), z = floor_to_cell2(c.w, cell);
      const int32_t o = (int32_t)((p >> (PYR_FIELD * (l - 1))) & ((1ULL << PYR_FIELD) - 1));
      reinterpret_cast<int4*>(a.lv[l].coords)[o] = make_int4(c.x, x, y, z);
      const uint64_t slot = slot_of_present(a.lv[l].keys, a.lv[l].mask, pack_key(c.x, x, y, z));
      a.lv[l].vals[slot] = o;   // exactly one row per key reaches here
    }
}

// The segment rule, for row i of n rows: seg[b] = first row whose batch index is >= b.  Rows must be grouped by ascending
// batch index < n_batch; a row that is not raises *not_grouped (the global-table path then serves the map).
__device__ __forceinline__ void segment_row(const int32_t* coords, int64_t i, int64_t n, int n_batch, int32_t* seg,
                                            int* not_grouped) {
  const int b = coords[4 * i];
  const int prev = i > 0 ? coords[4 * (i - 1)] : -1;
  if (b < prev || b >= n_batch || b < 0) {
    atomicOr(not_grouped, 1);
    return;
  }
  for (int bb = prev + 1; bb <= b; ++bb) seg[bb] = (int32_t)i;
  if (i == n - 1)
    for (int bb = b + 1; bb <= n_batch; ++bb) seg[bb] = (int32_t)n;
}

// per-sample segments of every level in one launch: grid.y = level; rows of level l >= 1 are counted on the device
__global__ __launch_bounds__(256) void k_pyr_segments(const int32_t* __restrict__ coords0, int64_t n0, const PyrArgs a) {
  const int l = blockIdx.y;
  if (l >= a.n_levels || !a.lv[l].seg) return;
  const int32_t* coords = l == 0 ? coords0 : a.lv[l].coords;
  const int64_t n = l == 0 ? n0 : (int64_t)a.counts[l];
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n) return;
  segment_row(coords, i, n, a.n_batch, a.lv[l].seg, &a.status[2 + l]);   // (or more samples than announced)
}

// the segments of one map (the lazy path of maps that did not come from cs_coordmap_pyramid)
__global__ void k_segments(const int32_t* __restrict__ coords, int64_t n, int n_batch,
                           int32_t* __restrict__ seg, int* __restrict__ flags) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  segment_row(coords, i, n, n_batch, seg, flags);
}

// Per-sample segment tables of coordinate maps (computed once, cached on the map): for several maps at once --
// TWO host round trips in total (last batch index of every map; the grouping flags of every map) instead of two per map.
int ensure_segments_many(cs_coordmap* const* maps, int n, hipStream_t s) {
  std::vector<cs_coordmap*> todo;
  for (int i = 0; i < n; ++i) {
    cs_coordmap* m = maps[i];
    if (!m || m->seg_state != 0) continue;
    if (std::find(todo.begin(), todo.end(), m) != todo.end()) continue;
    m->seg_state = -1;  // unavailable unless everything below succeeds
    if (m->n > 0) todo.push_back(m);
  }
  if (todo.empty()) return CS_OK;
  const size_t k = todo.size();
  std::vector<int32_t> last_b(k, -1);
  std::vector<int32_t*> seg(k, nullptr);
  std::vector<int> h_flags(k, 0);      // per map: rows not grouped by sample
  // every HIP error is COLLECTED (no return in the middle of the loops): on failure the blocks allocated so far go
  // back to the pool and the maps return to "not computed" (seg_state 0), so a later call can try again
  hipError_t e = hipSuccess;
  auto keep = [&e](hipError_t r) {
    if (e == hipSuccess && r != hipSuccess) e = r;
  };
  for (size_t i = 0; i < k && e == hipSuccess; ++i)
    keep(download_async(&last_b[i], todo[i]->d_coords + 4 * (todo[i]->n - 1), sizeof(int32_t), s));
  if (e == hipSuccess) keep(download_sync(s));
  PoolBuf<int> flags(k);
  if (e == hipSuccess && !flags.p) e = hipErrorOutOfMemory;
  if (e == hipSuccess) keep(hipMemsetAsync(flags.p, 0, k * sizeof(int), s));
  for (size_t i = 0; i < k && e == hipSuccess; ++i) {
    cs_coordmap* m = todo[i];
    if (last_b[i] < 0 || last_b[i] >= kMaxBatch) continue;   // stays -1: the global-table path serves this map
    const int nb = last_b[i] + 1;
    seg[i] = (int32_t*)pool_alloc((size_t)(nb + 1) * sizeof(int32_t));
    if (!seg[i]) {
      e = hipErrorOutOfMemory;
      break;
    }
    keep(hipMemsetAsync(seg[i], 0, (size_t)(nb + 1) * sizeof(int32_t), s));
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_segments, dim3((unsigned)ceil_div(m->n, 256)), dim3(256), 0, s, m->d_coords, m->n, nb, seg[i], flags.p + i);
    keep(hipGetLastError());
  }
  if (e == hipSuccess) keep(download_async(h_flags.data(), flags.p, k * sizeof(int), s));
  if (e == hipSuccess) keep(download_sync(s));
  for (size_t i = 0; i < k; ++i) {
    cs_coordmap* m = todo[i];
    if (e != hipSuccess) {
      pool_free(seg[i]);          // (nullptr is fine)
      m->seg_state = 0;           // not computed: nothing about this map was learnt
      continue;
    }
    if (!seg[i]) continue;
    if (h_flags[i]) {             // not grouped by sample: global path, seg_state stays -1
      pool_free(seg[i]);
      continue;
    }
    m->d_seg = seg[i];
    m->n_batch = last_b[i] + 1;
    m->seg_state = 1;
  }
  if (e != hipSuccess) {
    set_error("ensure_segments_many: %s", hipGetErrorString(e));
    return CS_ERR_HIP;
  }
  return CS_OK;
}

static uint64_t table_capacity(int64_t n) {
  uint64_t c = 1024;
  while (c < (uint64_t)(2 * n)) c <<= 1;
  return c;
}

static int alloc_table(cs_coordmap* m, int64_t n_keys, hipStream_t s) {
  m->capacity = table_capacity(n_keys);
  m->d_keys = (uint64_t*)pool_alloc(m->capacity * sizeof(uint64_t));
  m->d_vals = (int32_t*)pool_alloc(m->capacity * sizeof(int32_t));
  CS_REQUIRE(m->d_keys && m->d_vals, CS_ERR_HIP, "hash table allocation failed");
  int blocks = (int)(m->capacity / 256 < 2048 ? m->capacity / 256 : 2048);
  hipLaunchKernelGGL(k_fill_table, dim3(blocks), dim3(256), 0, s, m->d_keys, m->d_vals,
                     m->capacity);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// A coordinate map under construction: freed when the scope is left, unless release() hands it to the caller.
struct MapOwner {
  cs_coordmap* m = nullptr;
  explicit MapOwner(cs_coordmap* p = nullptr) : m(p) {}
  MapOwner(const MapOwner&) = delete;
  MapOwner& operator=(const MapOwner&) = delete;
  ~MapOwner() { cs_coordmap_free(m); }
  cs_coordmap* operator->() const { return m; }
  cs_coordmap* release() { return std::exchange(m, nullptr); }
};

}  // namespace cs

using namespace cs;

extern "C" {

int cs_coordmap_create(const int32_t* d_coords, int64_t n, int tensor_stride, void* stream,
                       cs_coordmap** out) {
  CS_REQUIRE(out, CS_ERR_INVALID, "cs_coordmap_create: out is NULL");
  *out = nullptr;
  CS_REQUIRE(n >= 0 && n < (1LL << 30), CS_ERR_INVALID, "cs_coordmap_create: bad row count %lld",
             (long long)n);
  CS_REQUIRE(n == 0 || d_coords, CS_ERR_INVALID, "cs_coordmap_create: coords is NULL");
  CS_REQUIRE(tensor_stride >= 1, CS_ERR_INVALID, "cs_coordmap_create: bad tensor stride");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  ProfScope prof("kmap", s);
  MapOwner m(new cs_coordmap());
  m->n = n;
  m->tensor_stride = tensor_stride;
  const int rc = alloc_table(m.m, n, s);
  if (rc) return rc;
  m->d_coords = (int32_t*)pool_alloc((n ? n : 1) * 4 * sizeof(int32_t));
  PoolBuf<int> status(2);
  CS_REQUIRE(m->d_coords && status.p, CS_ERR_HIP, "coordinate allocation failed");
  int h_status[2] = {0, 0};
  if (n > 0) {
    hipError_t e = hipMemcpyAsync(m->d_coords, d_coords, n * 4 * sizeof(int32_t),
                                  hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(status.p, 0, 2 * sizeof(int), s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_insert, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, m->d_coords,
                         n, 1, m->d_keys, m->d_vals, m->capacity - 1, status.p);
      e = hipGetLastError();
    }
    if (e == hipSuccess)
      e = download_async(h_status, status.p, sizeof(h_status), s);
    if (e == hipSuccess) e = download_sync(s);
    CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_coordmap_create: %s", hipGetErrorString(e));
  }
  CS_REQUIRE(!h_status[0], CS_ERR_RANGE,
             "cs_coordmap_create: coordinate out of the supported range (|x|,|y|,|z| < 32768, 0 <= batch < 65535)");
  CS_REQUIRE(!h_status[1], CS_ERR_DUPLICATE,
             "cs_coordmap_create: %d duplicate coordinate rows (quantise the cloud first)", h_status[1]);
  *out = m.release();
  return CS_OK;
}

int cs_coordmap_stride(const cs_coordmap* in, int stride, void* stream, cs_coordmap** out) {
  CS_REQUIRE(in && out, CS_ERR_INVALID, "cs_coordmap_stride: NULL argument");
  *out = nullptr;
  CS_REQUIRE(stride >= 2, CS_ERR_INVALID, "cs_coordmap_stride: stride must be >= 2");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  ProfScope prof("kmap", s);
  const int64_t n = in->n;
  const int cell = in->tensor_stride * stride;
  MapOwner m(new cs_coordmap());
  m->tensor_stride = cell;
  int rc = alloc_table(m.m, n, s);
  if (rc) return rc;
  PoolBuf<int> status(2);
  PoolBuf<int32_t> flag(n + 1), pos(n + 1);
  CS_REQUIRE(status.p && flag.p && pos.p, CS_ERR_HIP, "cs_coordmap_stride: scratch allocation failed");
  int32_t h_last[2] = {0, 0};
  int h_status[2] = {0, 0};
  if (n > 0) {
    const unsigned g = (unsigned)ceil_div(n, 256);
    hipError_t e = hipMemsetAsync(status.p, 0, 2 * sizeof(int), s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_insert, dim3(g), dim3(256), 0, s, in->d_coords, n, cell, m->d_keys,
                         m->d_vals, m->capacity - 1, status.p);
      hipLaunchKernelGGL(k_flag_first, dim3(g), dim3(256), 0, s, in->d_coords, n, cell,
                         m->d_keys, m->d_vals, m->capacity - 1, flag.p);
      e = hipGetLastError();
    }
    CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_coordmap_stride: %s", hipGetErrorString(e));
    rc = exclusive_scan_i32(flag.p, pos.p, n, s);
    if (rc) return rc;
    e = download_async(&h_last[0], pos.p + (n - 1), sizeof(int32_t), s);
    if (e == hipSuccess)
      e = download_async(&h_last[1], flag.p + (n - 1), sizeof(int32_t), s);
    if (e == hipSuccess)
      e = download_async(h_status, status.p, sizeof(h_status), s);
    if (e == hipSuccess) e = download_sync(s);
    CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_coordmap_stride: %s", hipGetErrorString(e));
    CS_REQUIRE(!h_status[0], CS_ERR_RANGE,
               "cs_coordmap_stride: cell out of the supported range (|x|,|y|,|z| < 32768, 0 <= batch < 65535)");
  }
  m->n = (int64_t)h_last[0] + h_last[1];
  m->d_coords = (int32_t*)pool_alloc((m->n ? m->n : 1) * 4 * sizeof(int32_t));
  CS_REQUIRE(m->d_coords, CS_ERR_HIP, "cs_coordmap_stride: coordinate allocation failed");
  if (n > 0) {
    hipLaunchKernelGGL(k_emit_strided, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s,
                       in->d_coords, n, cell, flag.p, pos.p, m->d_keys, m->d_vals,
                       m->capacity - 1, m->d_coords);
    const hipError_t e = hipGetLastError();
    // (no synchronisation: flag / pos go back to this thread's stream-ordered cache, whose next user is enqueued
    // behind this kernel)
    CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_coordmap_stride: %s", hipGetErrorString(e));
  }
  *out = m.release();
  return CS_OK;
}

/* All coordinate levels of a batch: out[0] = the map cs_coordmap_create(d_coords, n, tensor_stride) returns, out[l] =
 * cs_coordmap_stride(out[l - 1], 2) -- the same coordinates, row order and tables -- made from the stride-1 rows in one pass
 * with ONE host wait (see k_pyr_insert).  n_batch > 0: rows are announced to be grouped by sample with batch indices
 * < n_batch, and the per-sample segments of every level are made in the same pass (a violated announcement only costs the
 * LDS kernel-map path, never correctness).  Batches of 2^21 rows or more take the chained calls. */
int cs_coordmap_pyramid(const int32_t* d_coords, int64_t n, int tensor_stride, int n_levels, int n_batch, void* stream,
                        cs_coordmap** out) {
  CS_REQUIRE(out && n_levels >= 1 && n_levels <= PYR_MAX_LEVELS, CS_ERR_INVALID, "cs_coordmap_pyramid: bad arguments");
  for (int l = 0; l < n_levels; ++l) out[l] = nullptr;
  CS_REQUIRE(n >= 0 && n < (1LL << 30), CS_ERR_INVALID, "cs_coordmap_pyramid: bad row count %lld", (long long)n);
  CS_REQUIRE(n == 0 || d_coords, CS_ERR_INVALID, "cs_coordmap_pyramid: coords is NULL");
  CS_REQUIRE(tensor_stride >= 1, CS_ERR_INVALID, "cs_coordmap_pyramid: bad tensor stride");
  static const bool chained = getenv("CS_PYRAMID") && getenv("CS_PYRAMID")[0] == '0';
  const bool pow2 = (tensor_stride & (tensor_stride - 1)) == 0;   // cells of every level are tensor_stride << l
  MapOwner m[PYR_MAX_LEVELS];
  if (n == 0 || n >= (1LL << PYR_FIELD) || chained || !pow2) {
    int rc = cs_coordmap_create(d_coords, n, tensor_stride, stream, &m[0].m);
    for (int l = 1; l < n_levels && rc == CS_OK; ++l) rc = cs_coordmap_stride(m[l - 1].m, 2, stream, &m[l].m);
    if (rc != CS_OK) return rc;
    for (int l = 0; l < n_levels; ++l) out[l] = m[l].release();
    return CS_OK;
  }
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  ProfScope prof("kmap", s);
  if (n_batch > kMaxBatch) n_batch = 0;   // (grid.y of the level kernel is n_batch: at most 65535)
  PyrArgs a;
  a.n_levels = n_levels;
  a.n_batch = n_batch;
  constexpr int N_STATUS = 2 + PYR_MAX_LEVELS;
  PoolBuf<int> status(N_STATUS);
  PoolBuf<int32_t> counts(PYR_MAX_LEVELS);
  PoolBuf<unsigned long long> flag(n), pos(n);
  CS_REQUIRE(status.p && counts.p && flag.p && pos.p, CS_ERR_HIP, "cs_coordmap_pyramid: scratch allocation failed");
  a.status = status.p;
  a.counts = counts.p;
  for (int l = 0; l < n_levels; ++l) {
    m[l].m = new cs_coordmap();
    m[l]->tensor_stride = tensor_stride << l;
    // (the coarse levels have at most n rows: tables and coordinate arrays are sized for that)
    const int rc = alloc_table(m[l].m, n, s);
    if (rc != CS_OK) return rc;
    m[l]->d_coords = (int32_t*)pool_alloc((size_t)n * 4 * sizeof(int32_t));
    if (n_batch > 0) m[l]->d_seg = (int32_t*)pool_alloc((size_t)(n_batch + 1) * sizeof(int32_t));
    CS_REQUIRE(m[l]->d_coords && (n_batch <= 0 || m[l]->d_seg), CS_ERR_HIP, "cs_coordmap_pyramid: coordinate allocation failed");
    a.lv[l] = PyrLevel{m[l]->d_keys, m[l]->d_vals, m[l]->capacity - 1, m[l]->d_coords, m[l]->d_seg, tensor_stride << l};
  }
  hipError_t e = hipMemcpyAsync(m[0]->d_coords, d_coords, (size_t)n * 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(status.p, 0, sizeof(int) * N_STATUS, s);
  if (e == hipSuccess) e = hipMemsetAsync(counts.p, 0, sizeof(int32_t) * PYR_MAX_LEVELS, s);
  for (int l = 0; l < n_levels && e == hipSuccess && n_batch > 0; ++l)
    e = hipMemsetAsync(m[l]->d_seg, 0, (size_t)(n_batch + 1) * sizeof(int32_t), s);
  CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_coordmap_pyramid: %s", hipGetErrorString(e));
  const unsigned g = (unsigned)ceil_div(n, 256);
  // level 0's cell is 1 in units of its own stride: its key is the coordinate itself
  PyrArgs a_ins = a;
  a_ins.lv[0].cell = 1;
  hipLaunchKernelGGL(k_pyr_insert, dim3(g), dim3(256), 0, s, m[0]->d_coords, n, a_ins);
  e = hipGetLastError();
  if (e == hipSuccess && n_levels > 1) {
    hipLaunchKernelGGL(k_pyr_flag, dim3(g), dim3(256), 0, s, m[0]->d_coords, n, a, flag.p);
    size_t tmp_bytes = 0;
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, flag.p, pos.p, (int)n, s);
    PoolBuf<char> tmp(tmp_bytes ? tmp_bytes : 1);
    if (e == hipSuccess && !tmp.p) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, flag.p, pos.p, (int)n, s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_pyr_emit, dim3(g), dim3(256), 0, s, m[0]->d_coords, n, a, flag.p, pos.p);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess && n_batch > 0) {
    hipLaunchKernelGGL(k_pyr_segments, dim3(g, (unsigned)n_levels), dim3(256), 0, s, m[0]->d_coords, n, a);
    e = hipGetLastError();
  }
  int h_status[N_STATUS] = {0};
  int32_t h_counts[PYR_MAX_LEVELS] = {0};
  if (e == hipSuccess) e = download_async(h_status, status.p, sizeof(h_status), s);
  if (e == hipSuccess) e = download_async(h_counts, counts.p, sizeof(h_counts), s);
  if (e == hipSuccess) e = download_sync(s);
  CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_coordmap_pyramid: %s", hipGetErrorString(e));
  CS_REQUIRE(!h_status[0], CS_ERR_RANGE,
             "cs_coordmap_pyramid: coordinate out of the supported range (|x|,|y|,|z| < 32768, 0 <= batch < 65535)");
  CS_REQUIRE(!h_status[1], CS_ERR_DUPLICATE,
             "cs_coordmap_pyramid: %d duplicate coordinate rows (quantise the cloud first)", h_status[1]);
  for (int l = 0; l < n_levels; ++l) {
    m[l]->n = l == 0 ? n : (int64_t)h_counts[l];
    if (n_batch > 0 && h_status[2 + l] == 0) {
      m[l]->n_batch = n_batch;
      m[l]->seg_state = 1;
    } else if (n_batch > 0) {       // not grouped by sample: the global-table path serves this map
      pool_free(m[l]->d_seg);
      m[l]->d_seg = nullptr;
      m[l]->seg_state = -1;
    }
    out[l] = m[l].release();
  }
  return CS_OK;
}

int64_t cs_coordmap_size(const cs_coordmap* m) { return m ? m->n : -1; }
int cs_coordmap_tensor_stride(const cs_coordmap* m) { return m ? m->tensor_stride : -1; }
const int32_t* cs_coordmap_coords(const cs_coordmap* m) { return m ? m->d_coords : nullptr; }

void cs_coordmap_free(cs_coordmap* m) {
  if (!m) return;
  pool_free(m->d_coords);
  pool_free(m->d_keys);
  pool_free(m->d_vals);
  pool_free(m->d_seg);
  delete m;
}

}  // extern "C"
