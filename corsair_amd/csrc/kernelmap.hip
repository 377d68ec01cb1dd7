// Kernel maps: the output-stationary neighbour tables of the convolutions, built by probing coordinate maps (coordmap.hip).
//
// Replaces the kernel maps of MinkowskiEngine's coordinate manager (model/resunet.py:49-193).  Data layout in HBM:
//   nbr      int32  [n_out, 27] neighbour table: in-row feeding out-row o through offset k, or -1
//   rowlist  int32  [n_out] output rows in tiling order (Gray rank of the 27-bit neighbour-presence mask)
//   gmask    uint32 [ceil(n_out / 32) rounded up to 8] offsets present in each 32-row group of that order
//   h_cnt    uint64 page-locked slot the pair count lands in behind the build (read on first use)
// Integer work bound by LDS / L2 latency: the builder (k_level_maps) keeps one sample's table in LDS.
#include <hipcub/hipcub.hpp>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "coordmap.h"

namespace cs {

// One thread per (out row, k): probe the in-map.  Offsets: k = (dx+1) + 3(dy+1) + 9(dz+1).
__global__ void k_build_nbr(const int32_t* __restrict__ out_coords, int64_t n_out, int kvol,
                            int step, int sign, const uint64_t* __restrict__ keys,
                            const int32_t* __restrict__ vals, uint64_t mask, int32_t* nbr,
                            unsigned long long* pair_count) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int found = 0;
  if (t < n_out * kvol) {
    int64_t o = t / kvol;
    int k = (int)(t - o * kvol);
    int dx = 0, dy = 0, dz = 0;
    if (kvol == 27) {
      dx = k % 3 - 1;
      dy = (k / 3) % 3 - 1;
      dz = k / 9 - 1;
    }
    int b = out_coords[4 * o + 0];
    int x = out_coords[4 * o + 1] + sign * dx * step;
    int y = out_coords[4 * o + 2] + sign * dy * step;
    int z = out_coords[4 * o + 3] + sign * dz * step;
    int32_t v = -1;
    if (coord_in_range(b, x, y, z)) v = hash_lookup(keys, vals, mask, pack_key(b, x, y, z));
    nbr[t] = v;
    found = v >= 0;
  }
  // wave-level count then one atomic per wave
  unsigned long long m = __ballot(found);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(pair_count, (unsigned long long)__popcll(m));
}

// Page-locked slots for the pair counts of kernel maps (one per live map, recycled on free).
static std::mutex g_slot_mu;
static std::vector<unsigned long long*> g_slot_slabs;
static std::vector<int> g_slot_free;
constexpr int SLOTS_PER_SLAB = 1024;

static unsigned long long* count_slot_acquire(int* slot) {
  std::lock_guard<std::mutex> lk(g_slot_mu);
  if (g_slot_free.empty()) {
    unsigned long long* slab = nullptr;
    if (hipHostMalloc(reinterpret_cast<void**>(&slab), sizeof(unsigned long long) * SLOTS_PER_SLAB, 0) !=
        hipSuccess)
      return nullptr;
    const int first = (int)g_slot_slabs.size() * SLOTS_PER_SLAB;
    g_slot_slabs.push_back(slab);
    for (int i = SLOTS_PER_SLAB - 1; i >= 0; --i) g_slot_free.push_back(first + i);
  }
  *slot = g_slot_free.back();
  g_slot_free.pop_back();
  return g_slot_slabs[*slot / SLOTS_PER_SLAB] + *slot % SLOTS_PER_SLAB;
}

static void count_slot_release(int slot) {
  if (slot < 0) return;
  std::lock_guard<std::mutex> lk(g_slot_mu);
  g_slot_free.push_back(slot);
}

// Maps holding deferred profile units (cs_conv_fwd registers; delivery and cs_kernelmap_free remove).  A map is in the list
// exactly while its prof_flop_per_pair is > 0.  g_prof_maps_mu guards the list AND those two fields of every map, and a
// registered map is only deleted after it left the list under the mutex: whoever holds the mutex may read any listed map.
static std::mutex g_prof_maps_mu;
static std::vector<cs_kernelmap*> g_prof_maps;
struct ProfUnits {
  double units;
  uint64_t epoch;
};

// g_prof_maps_mu held: what km holds becomes work units for `pairs` pairs, and km leaves the list
static ProfUnits prof_take_locked(cs_kernelmap* km, int64_t pairs) {
  const ProfUnits u = {km->prof_flop_per_pair * (double)pairs, km->prof_epoch};
  if (km->prof_flop_per_pair <= 0.0) return u;
  km->prof_flop_per_pair = 0.0;
  for (size_t i = 0; i < g_prof_maps.size(); ++i)
    if (g_prof_maps[i] == km) {
      g_prof_maps[i] = g_prof_maps.back();
      g_prof_maps.pop_back();
      break;
    }
  return u;
}
// cs_kernelmap_free: km leaves the list under the mutex.  The units it holds are delivered if its count has arrived
// (`counted`: its event was waited for) and go with the map otherwise.
static void prof_retire(cs_kernelmap* km, bool counted) {
  ProfUnits u;
  {
    std::lock_guard<std::mutex> lk(g_prof_maps_mu);
    if (km->prof_flop_per_pair <= 0.0) return;
    int64_t pairs = km->num_pairs;
    if (pairs < 0 && counted && km->h_cnt) pairs = (int64_t)*km->h_cnt;
    u = prof_take_locked(km, pairs > 0 ? pairs : 0);
  }
  if (u.units > 0.0) prof_add_units_epoch("conv", u.units, u.epoch);
}

void kernelmap_defer_prof(cs_kernelmap* km, double per_pair) {
  const uint64_t ep = prof_epoch();
  std::lock_guard<std::mutex> lk(g_prof_maps_mu);
  const bool registered = km->prof_flop_per_pair > 0.0;
  if (km->prof_epoch != ep) {      // what it still holds belongs to a region that has been reset away
    km->prof_flop_per_pair = 0.0;
    km->prof_epoch = ep;
  }
  if (!registered) g_prof_maps.push_back(km);
  km->prof_flop_per_pair += per_pair;
}

// Called by a user of the map (never for a map another thread may free): the wait is outside the mutex.
int64_t kernelmap_pairs(const cs_kernelmap* km_c) {
  cs_kernelmap* km = const_cast<cs_kernelmap*>(km_c);  // cached on first use
  if (!km) return -1;
  if (km->num_pairs < 0 && km->cnt_ready && km->h_cnt) {
    if (hipEventSynchronize(km->cnt_ready) != hipSuccess) return -1;
    km->num_pairs = (int64_t)*km->h_cnt;
  }
  if (km->num_pairs >= 0) {   // convolutions profiled before the count had arrived
    std::unique_lock<std::mutex> lk(g_prof_maps_mu);
    const ProfUnits u = prof_take_locked(km, km->num_pairs);
    lk.unlock();
    if (u.units > 0.0) prof_add_units_epoch("conv", u.units, u.epoch);
  }
  return km->num_pairs;
}

// Every registered map delivers, whichever thread owns it.  The mutex is held across the waits for the pair counts, so a
// listed map cannot be freed meanwhile.  That cannot deadlock: a map's cnt_ready is recorded before the map is handed out, so
// its event waits only for GPU work that is already enqueued; the library puts no host callback into a stream; the threads
// that want the mutex meanwhile (cs_conv_fwd while profiling, kernelmap_pairs, cs_kernelmap_free) are held up for the few
// microseconds a count is behind its build.  Only fields that are fixed once the map is built are read here (cnt_ready,
// h_cnt; num_pairs of a map without an event), not the owner's cache of the count.
void kernelmap_flush_prof() {
  std::vector<ProfUnits> got;
  {
    std::lock_guard<std::mutex> lk(g_prof_maps_mu);
    const std::vector<cs_kernelmap*> maps = g_prof_maps;   // (prof_take_locked edits the list)
    for (cs_kernelmap* km : maps) {
      int64_t pairs = -1;   // (stays listed)
      if (!km->cnt_ready || !km->h_cnt) pairs = km->num_pairs;
      else if (hipEventSynchronize(km->cnt_ready) == hipSuccess) pairs = (int64_t)*km->h_cnt;
      if (pairs >= 0) got.push_back(prof_take_locked(km, pairs));
    }
  }
  for (const ProfUnits& u : got)
    if (u.units > 0.0) prof_add_units_epoch("conv", u.units, u.epoch);
}

// Tiling order of the convolution kernels: output rows sorted by the Gray-code RANK of their 27-bit
// neighbour-presence mask (rows with the same mask are adjacent; neighbours in the order differ in few
// offsets).  A 32-row group of k_conv_dma then executes only 1.2 - 1.4x the MFMAs its rows need, because
// it skips every offset none of its rows has (measured on the stress clouds, executed / useful per 32-row
// group at strides 1 / 2 / 4: Gray rank 1.41 / 1.19 / 1.28, plain numeric order 1.48 / 1.20 / 1.29, the
// 12-bit grouping of rounds 1-2 2.05 / 1.59 / 1.52).  The order inside equal keys is the radix sort's
// (stable: row order); every output row is computed independently, results do not depend on the order.
// ---- the tiling order of ALL kernel maps of a batch in one pass (round 4) ---------------------------------------------
// Ten maps of a batch used to mean ten row-key launches, ten device sorts (5 - 20 launches each: hipcub takes a block-sort +
// merge path for the mid-size maps) and ten table launches: 115 launches per stress batch, 60 per chair batch, bound by
// launch latency.  Here the keys of all maps go into ONE array -- key = map index << 27 | Gray rank, so one radix sort
// leaves every map's rows contiguous and ordered -- and one launch writes all sorted tables.  The descriptors travel as a
// kernel argument (no upload).
constexpr int ORDER_MAX_MAPS = 16;
struct OrderMap {
  const int32_t* nbr;
  uint32_t* gmask;
  int32_t* rowlist;
  const unsigned long long* d_cnt;
  unsigned long long* host_cnt;
  int64_t n_out, base, n_groups;
  uint32_t kblk0, tblk0;   // first workgroup of this map in the key / finish launch
  uint32_t tag;            // map index << 27: the sort keeps every map's rows together, in the order of `base`
  int need_keys;           // 1: k_row_keys_all computes this map's keys from its table (maps the level kernel did not build)
};
struct OrderTab {
  int n;
  OrderMap m[ORDER_MAX_MAPS];
};
// Bit j of a row's tiling mask stands for kernel offset KORDER[j]: the centre, the six face neighbours, the twelve edge
// neighbours, the eight corner neighbours (by |d|_1, then by k).  The frequent offsets sit in the low bits, the rare corner
// offsets decide the coarse order of the Gray ranks -- rows that need a rare offset end up in the same 32-row groups.  Against
// the Gray rank of the mask in plain k order the executed / useful matrix work of the convolutions drops 1.190 -> 1.160 on the
// 64-cloud stress batch (stride-1 maps 1.31 -> 1.22), 1.270 -> 1.231 on a 24-cloud batch (tools/exec_ratio_cpu.py).
__device__ const int8_t KORDER[32] = {13, 4, 10, 12, 14, 16, 22, 1, 3, 5, 7, 9, 11, 15, 17, 19, 21, 23, 25, 0, 2, 6, 8, 18, 20, 24, 26, 0, 0, 0, 0, 0};
__device__ __forceinline__ uint32_t unpermute_mask(uint32_t m) {   // tiling mask (bit j = offset KORDER[j]) -> bit k = offset k
  uint32_t out = 0;
#pragma unroll
  for (int j = 0; j < 27; ++j) out |= ((m >> j) & 1u) << KORDER[j];
  return out;
}
__device__ __forceinline__ uint32_t gray_rank(uint32_t m) {   // r with r ^ (r >> 1) == m
  m ^= m >> 1;
  m ^= m >> 2;
  m ^= m >> 4;
  m ^= m >> 8;
  m ^= m >> 16;
  return m;
}
__global__ __launch_bounds__(256) void k_row_keys_all(const OrderTab tab, uint32_t* __restrict__ key,
                                                      int32_t* __restrict__ row) {
  int i = 0;
  while (i + 1 < tab.n && blockIdx.x >= tab.m[i + 1].kblk0) ++i;
  const OrderMap& mp = tab.m[i];
  if (!mp.need_keys) return;
  const int64_t o = (int64_t)(blockIdx.x - mp.kblk0) * 256 + threadIdx.x;
  if (o >= mp.n_out) return;
  uint32_t m = 0;
  for (int j = 0; j < 27; ++j) m |= (mp.nbr[o * 27 + KORDER[j]] >= 0 ? 1u : 0u) << j;
  key[mp.base + o] = mp.tag | gray_rank(m);
  row[mp.base + o] = (int32_t)o;
}
// behind the sort: every map's row list (its slice of the sorted payload), the group masks, and the pair count of the
// build kernels handed to its page-locked slot (a device -> host copy of 8 bytes was one blit-kernel launch per map)
__global__ __launch_bounds__(256) void k_order_finish(const OrderTab tab, const uint32_t* __restrict__ key_sorted,
                                                      const int32_t* __restrict__ row_sorted) {
  int i = 0;
  while (i + 1 < tab.n && blockIdx.x >= tab.m[i + 1].tblk0) ++i;
  const OrderMap& mp = tab.m[i];
  const int64_t e = (int64_t)(blockIdx.x - mp.tblk0) * 256 + threadIdx.x;
  if (e == 0 && mp.host_cnt) __hip_atomic_store(mp.host_cnt, *mp.d_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const int32_t* rl = row_sorted + mp.base;
  const uint32_t* ks = key_sorted + mp.base;
  if (e < mp.n_out) mp.rowlist[e] = rl[e];
  if (e < mp.n_groups) {
    uint32_t m = 0;
    for (int r = 0; r < 32; ++r) {
      const int64_t t = e * 32 + r;
      if (t < mp.n_out) {
        const uint32_t rank = ks[t] & 0x7ffffffu;
        m |= rank ^ (rank >> 1);
      }
    }
    mp.gmask[e] = unpermute_mask(m);
  }
}

// ---- kernel maps built in LDS (k_level_maps, below) ----------------------------------------------------------------------
// Coordinates of a batch are grouped by sample (collate order), and a
// kernel-map probe never leaves its sample, so one workgroup loads the in-map coordinates of ONE sample into an LDS hash
// table (30-bit keys relative to the sample's bounding box, 16-bit local row) and answers the probes of its slice of output
// rows from LDS -- no random global access at all.  Samples with more rows than the table holds or bounding boxes wider
// than 1023 cells are probed in the level's global table by the same workgroup; batches that are not grouped by sample use
// the global kernel (k_build_nbr) for everything.  (The per-map kernels of rounds 1-4, k_build_nbr_lds / _flagged, were
// removed in round 5 after the A/B against k_level_maps: profiles/r5d_kmap_fused_ab.txt, HISTORY.md.)
constexpr int LDS_SLOTS_MAX = 24576;  // 4-B keys + 2-B local rows = 144 KB of the CU's 160 KB LDS (load factor <= 0.625)
// tables for small samples: two more instantiations of k_level_maps, picked by the mean in-rows per sample (launch_level)
constexpr int LDS_SLOTS_SMALL = 2048, LDS_SLOTS_MID = 8192;
// workgroups per level: one per CU and more (a slice re-inserts its sample: 512 workgroups build every table twice as often
// as 256 for the same probes)
constexpr int LEVEL_WGS = 256;
constexpr uint32_t LDS_EMPTY = 0xffffffffu;

// ---- every kernel map that probes ONE coordinate level, in one launch (round 5) ---------------------------------------
// The ten maps of a ResUNet batch probe four tables: level L serves L -> L (submanifold), L -> 2L (strided: output rows of
// level 2L look for level-L rows) and the transposed 2L' -> L' map whose INPUT is level L (output rows of the finer level
// look for level-L rows).  Round 4 launched one kernel per map, every slice of every launch re-inserting its sample into LDS
// (2.2 ms of kernel-map work per batch-64 stress forward, 40 - 48 % of the convolutions' time).  Here a
// workgroup (slice x, sample b) builds the sample's table ONCE and answers the probes of all jobs from it:
//   * the sample's coordinates are read once (16-byte loads, held in registers for the bounding box AND the insert);
//   * a thread owns one (row, offset) with 32 lanes per row (27 used): the 27 results of a row are one contiguous 108-byte
//     store, the row's presence mask is one ballot -- so the tiling key (Gray rank of the mask) and the pair count come out
//     of the builder and nothing has to read the table again (k_row_keys_all re-read 108 B per row);
//   * coordinates of the next four rows of a thread are requested before the first is probed (the probe loop was a chain
//     of dependent global load -> LDS probe -> store per entry, with four waves per SIMD to hide it);
//   * a sample that does not fit the LDS table (too many rows, bounding box wider than 1023 cells) is probed in the level's
//     GLOBAL table by the same workgroup -- no flag array, no second launch that usually does nothing.
constexpr int LEVEL_MAX_JOBS = 4;
struct LevelJob {
  const int32_t* out_coords;   // [n_out,4] rows grouped by sample
  const int32_t* out_seg;      // [n_batch + 1]
  int32_t* nbr;                // [n_out,27]
  uint32_t* key;               // tiling keys / row payload of this map inside the batch's sort arrays (nullptr: not wanted)
  int32_t* row;
  unsigned long long* cnt;     // pair counter
  int step, sign;
  uint32_t tag;                // map index << 27
};
struct LevelArgs {
  int n_jobs;
  LevelJob job[LEVEL_MAX_JOBS];
  const int32_t* in_coords;
  const int32_t* in_seg;
  int unit, ushift;
  const uint64_t* gkeys;       // the level's global table (cs_coordmap): oversized samples
  const int32_t* gvals;
  uint64_t gmask;
  unsigned long long* trace;   // CS_KMAP_TRACE=1: [workgroup][8] phase stamps (100 MHz), else nullptr
};

template <int SLOTS, int NT>
__global__ __launch_bounds__(NT) void k_level_maps(const LevelArgs a) {
  // The table: NB buckets of four 4-byte keys (one ds_read_b128 fetches a bucket) + four 2-byte local rows.  A key goes into
  // the first free slot of its bucket, slots fill in order, a full bucket spills into the next one.  A probe reads ONE
  // bucket and is done unless that bucket is full and does not hold the key (6 % of the probes at the usual load of 1.5
  // keys per bucket) -- so the first reads of several probes can be in flight together: the round-4 kernels chased one
  // linear-probing chain per lane with four waves per SIMD to hide it, and were bound by that latency (trace: 142 us of
  // probes against 22 us of table build per stride-1 level of a stress batch).
  constexpr int NB = SLOTS / 4;
  constexpr int MAX_ROWS = SLOTS / 8 * 5;            // load factor <= 0.625 (2.5 keys per bucket)
  constexpr int RPT = (MAX_ROWS + NT - 1) / NT;      // in-rows a thread holds in registers
  constexpr int ROWS_PER_PASS = NT / 32;             // output rows a workgroup probes at a time
  constexpr int U = 8;                               // probes a lane keeps in flight
  __shared__ __attribute__((aligned(16))) uint32_t keys[SLOTS];
  __shared__ __attribute__((aligned(8))) uint16_t vals[SLOTS];
  __shared__ int bmin[3], bmax[3];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int i0 = a.in_seg[b], i1 = a.in_seg[b + 1];
  const int n_in = i1 - i0;
  // rows of this slice per job; a workgroup without any leaves before the first barrier
  auto slice = [&](int j, int& lo_, int& hi_) {
    const int o0 = a.job[j].out_seg[b], o1 = a.job[j].out_seg[b + 1];
    const int per = (o1 - o0 + (int)gridDim.x - 1) / (int)gridDim.x;
    lo_ = o0 + (int)blockIdx.x * per;
    hi_ = min(o1, lo_ + per);
  };
  bool any = false;
  for (int j = 0; j < a.n_jobs; ++j) {
    int lo_, hi_;
    slice(j, lo_, hi_);
    any = any || lo_ < hi_;
  }
  if (!any) return;
  unsigned long long* tr = a.trace ? a.trace + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 : nullptr;
  if (tr && tid == 0) tr[0] = __builtin_amdgcn_s_memrealtime();
  // cells are counted in units of the tensor stride, a power of two for every level the network makes: shifts and masks.
  // (A stride that is not one goes through the global table below.  With the general `v / unit` kept as the other arm of a
  // select, every probe carried six uniform branches around six 30-instruction integer divisions.)
  const int ushift = a.ushift, unit = a.unit;
  auto udiv = [&](int v) { return v >> ushift; };                    // v >= 0
  auto umult = [&](int v) { return (v & (unit - 1)) == 0; };
  auto bucket_of = [&](uint32_t key) { return __umulhi(key * 2654435761u, (uint32_t)NB); };   // [0, NB)

  bool use_lds = n_in <= MAX_ROWS && ushift >= 0;    // workgroup-uniform
  int4 c[RPT];
  if (use_lds) {
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      const int i = i0 + tid + j * NT;
      c[j] = make_int4(0, 0, 0, 0);
      if (i < i1) c[j] = reinterpret_cast<const int4*>(a.in_coords)[i];
    }
    if (tid < 3) {
      bmin[tid] = 0x7fffffff;
      bmax[tid] = -0x7fffffff;
    }
    for (int i = tid; i < NB; i += NT)
      reinterpret_cast<uint4*>(keys)[i] = make_uint4(LDS_EMPTY, LDS_EMPTY, LDS_EMPTY, LDS_EMPTY);
    __syncthreads();
    // bounding box: per thread (registers), per wave (shuffles), one LDS atomic per wave and axis
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      if (i0 + tid + j * NT < i1) {
        lo[0] = min(lo[0], c[j].y);
        hi[0] = max(hi[0], c[j].y);
        lo[1] = min(lo[1], c[j].z);
        hi[1] = max(hi[1], c[j].z);
        lo[2] = min(lo[2], c[j].w);
        hi[2] = max(hi[2], c[j].w);
      }
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        lo[ax] = min(lo[ax], __shfl_xor(lo[ax], off));
        hi[ax] = max(hi[ax], __shfl_xor(hi[ax], off));
      }
      if ((tid & 63) == 0) {
        atomicMin(&bmin[ax], lo[ax]);
        atomicMax(&bmax[ax], hi[ax]);
      }
    }
    __syncthreads();
  }
  int mx = 0, my = 0, mz = 0, ex = -1, ey = -1, ez = -1;   // an empty sample: no cell is inside the box
  if (use_lds && n_in > 0) {
    mx = bmin[0];
    my = bmin[1];
    mz = bmin[2];
    ex = udiv(bmax[0] - mx);
    ey = udiv(bmax[1] - my);
    ez = udiv(bmax[2] - mz);
    if (ex > 1023 || ey > 1023 || ez > 1023) use_lds = false;   // (uniform: every thread reads the same box)
  }
  if (tr && tid == 0) tr[1] = __builtin_amdgcn_s_memrealtime();
  if (use_lds) {
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      const int i = i0 + tid + j * NT;
      if (i < i1) {
        const uint32_t key = (uint32_t)udiv(c[j].y - mx) | ((uint32_t)udiv(c[j].z - my) << 10) |
                             ((uint32_t)udiv(c[j].w - mz) << 20);
        uint32_t slot = bucket_of(key) * 4u;   // coordinates are unique inside a map: every key claims its own slot
        while (atomicCAS(&keys[slot], LDS_EMPTY, key) != LDS_EMPTY) slot = slot + 1 == SLOTS ? 0 : slot + 1;
        vals[slot] = (uint16_t)(i - i0);
      }
    }
    __syncthreads();
  }
  if (tr && tid == 0) tr[2] = __builtin_amdgcn_s_memrealtime();

  const int kj = tid & 31;                            // lane j of a row handles offset KORDER[j]; lanes 27..31 idle
  const int k = kj < 27 ? (int)KORDER[kj] : 27;       // (the ballot bit of lane j is then bit j of the tiling mask)
  const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
  const int sh = tid & 32;                            // this row's half of the wave ballot
#pragma unroll 1
  for (int j = 0; j < a.n_jobs; ++j) {
    const LevelJob& J = a.job[j];
    const int ox = J.sign * dx * J.step - mx, oy = J.sign * dy * J.step - my, oz = J.sign * dz * J.step - mz;
    const int4* oc = reinterpret_cast<const int4*>(J.out_coords);
    int32_t* const nbr = J.nbr;
    uint32_t* const jkey = J.key;
    int32_t* const jrow = J.row;
    const uint32_t tag = J.tag;
    int found = 0;
    int s0j, s1j;
    slice(j, s0j, s1j);
    // the row's mask is a ballot, its tiling key and row payload come from the lane of offset 0
    auto emit = [&](int o, int32_t v) {
      if (k < 27) nbr[(int64_t)o * 27 + k] = v;
      const uint32_t m = (uint32_t)(__ballot(v >= 0) >> sh) & 0x7ffffffu;
      if (kj == 0) {
        found += __popc(m);
        if (jkey) {
          jkey[o] = tag | gray_rank(m);
          jrow[o] = o;
        }
      }
    };
    if (use_lds) {
      for (int ob = s0j + (tid >> 5); ob < s1j; ob += U * ROWS_PER_PASS) {
        int4 p[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int o = ob + u * ROWS_PER_PASS;
          p[u] = make_int4(0, 0, 0, 0);
          if (o < s1j) p[u] = oc[o];
        }
        uint32_t key[U], bk[U];
        bool live[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int x = p[u].y + ox, y = p[u].z + oy, z = p[u].w + oz;      // relative to the box corner
          const int cx = udiv(max(x, 0)), cy = udiv(max(y, 0)), cz = udiv(max(z, 0));
          live[u] = k < 27 && ob + u * ROWS_PER_PASS < s1j && (x | y | z) >= 0 && umult(x) && umult(y) && umult(z) &&
                    cx <= ex && cy <= ey && cz <= ez;
          key[u] = (uint32_t)cx | ((uint32_t)cy << 10) | ((uint32_t)cz << 20);
          bk[u] = live[u] ? bucket_of(key[u]) : 0u;
        }
        uint4 K[U];
#pragma unroll
        for (int u = 0; u < U; ++u) K[u] = reinterpret_cast<const uint4*>(keys)[bk[u]];   // U reads in flight
        int32_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int sl = K[u].x == key[u] ? 0 : K[u].y == key[u] ? 1 : K[u].z == key[u] ? 2 : K[u].w == key[u] ? 3 : -1;
          uint32_t bb = bk[u];
          if (live[u] && sl < 0 && K[u].w != LDS_EMPTY) {     // full bucket without the key: it may have spilled on
            while (true) {
              bb = bb + 1 == NB ? 0 : bb + 1;
              const uint4 Kn = reinterpret_cast<const uint4*>(keys)[bb];
              sl = Kn.x == key[u] ? 0 : Kn.y == key[u] ? 1 : Kn.z == key[u] ? 2 : Kn.w == key[u] ? 3 : -1;
              if (sl >= 0 || Kn.w == LDS_EMPTY) break;
            }
          }
          v[u] = (live[u] && sl >= 0) ? i0 + (int32_t)vals[bb * 4 + sl] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int o = ob + u * ROWS_PER_PASS;
          if (o < s1j) emit(o, v[u]);
        }
      }
    } else {
      // a sample too large or too wide for the LDS table: the same probes in the level's global table
      for (int o = s0j + (tid >> 5); o < s1j; o += ROWS_PER_PASS) {
        const int4 pp = oc[o];
        int32_t v = -1;
        if (k < 27) {
          const int X = pp.y + ox + mx, Y = pp.z + oy + my, Z = pp.w + oz + mz;
          if (coord_in_range(pp.x, X, Y, Z)) v = hash_lookup(a.gkeys, a.gvals, a.gmask, pack_key(pp.x, X, Y, Z));
        }
        emit(o, v);
      }
    }
    // pair count: wave reduce, one atomic per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) found += __shfl_xor(found, off);
    if ((tid & 63) == 0 && found) atomicAdd(J.cnt, (unsigned long long)found);
    if (tr && tid == 0) tr[3 + j] = __builtin_amdgcn_s_memrealtime();
  }
}

__global__ void k_export_flag(const int32_t* __restrict__ nbr, int64_t n_out, int kvol,
                              int32_t* flag) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n_out * kvol) return;
  int64_t k = t / n_out, o = t - k * n_out;
  flag[t] = nbr[o * kvol + k] >= 0;
}
__global__ void k_export_emit(const int32_t* __restrict__ nbr, int64_t n_out, int kvol,
                              const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                              int64_t cap, int32_t* ok, int32_t* oin, int32_t* oout) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n_out * kvol || !flag[t]) return;
  int64_t k = t / n_out, o = t - k * n_out;
  int64_t p = pos[t];
  if (p >= cap) return;
  ok[p] = (int32_t)k;
  oin[p] = nbr[o * kvol + k];
  oout[p] = (int32_t)o;
}

// (defined here, beside the radix sort: rocprim builds both on the same int32 copy kernel, one instantiation per unit)
int exclusive_scan_i32(const int32_t* d_in, int32_t* d_out, int64_t n, hipStream_t s) {
  size_t tmp_bytes = 0;
  CS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_in, d_out, (int)n, s));
  PoolBuf<char> tmp(tmp_bytes);
  CS_REQUIRE(tmp.p, CS_ERR_HIP, "scan scratch allocation failed");
  CS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, d_in, d_out, (int)n, s));
  return CS_OK;
}

}  // namespace cs

using namespace cs;

// ---- building the kernel maps of a batch -------------------------------------------------------------------------------
// Geometry of one map: which way the probes go.  Plain: out row at p looks for in rows at p + d * step (step = the in
// map's tensor stride); transposed (in = the coarser map): p - d * step with step = the out map's stride.
static int map_geometry(const cs_coordmap* in, const cs_coordmap* out, int kernel_size, int transposed, int* step, int* sign) {
  CS_REQUIRE(in && out, CS_ERR_INVALID, "cs_kernelmap_build: NULL argument");
  CS_REQUIRE(kernel_size == 3 || kernel_size == 1, CS_ERR_UNSUPPORTED,
             "cs_kernelmap_build: kernel_size %d not supported (1 or 3)", kernel_size);
  if (!transposed) {
    CS_REQUIRE(out->tensor_stride == in->tensor_stride || out->tensor_stride == 2 * in->tensor_stride, CS_ERR_INVALID,
               "cs_kernelmap_build: tensor strides %d -> %d not supported", in->tensor_stride, out->tensor_stride);
    *step = in->tensor_stride;
    *sign = +1;
  } else {
    CS_REQUIRE(in->tensor_stride == 2 * out->tensor_stride, CS_ERR_INVALID,
               "cs_kernelmap_build: transposed map needs in stride == 2 * out stride (%d, %d)", in->tensor_stride,
               out->tensor_stride);
    *step = out->tensor_stride;
    *sign = -1;
  }
  return CS_OK;
}

static int ushift_of(int ts) {
  if (ts <= 0 || (ts & (ts - 1)) != 0) return -1;
  int sh = 0;
  while ((1 << sh) < ts) ++sh;
  return sh;
}

struct MapPlan {
  cs_kernelmap* km = nullptr;
  const cs_coordmap* in = nullptr;
  const cs_coordmap* out = nullptr;
  int step = 0, sign = 0;
  unsigned long long* d_cnt = nullptr;   // device pair counter (zeroed before the streams fork)
  bool fused = false;                    // built by k_level_maps (keys come out of the builder)
  bool ordered = false;                  // gets a tiling order (kvol 27, n_out > 0)
  int64_t base = 0;                      // first element of this map in the batch's sort arrays
};

// CS_KMAP_TRACE=1: phase stamps of one k_level_maps launch, averaged over its workgroups (synchronises; diagnostics)
static void level_trace_report(unsigned long long* d_trace, int wgs, int n_jobs, int slots, int nb, int slices,
                               int64_t n_in, hipStream_t s) {
  std::vector<unsigned long long> h((size_t)wgs * 8);
  if (hipStreamSynchronize(s) != hipSuccess) return;
  if (hipMemcpy(h.data(), d_trace, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
  double ph[8] = {0};
  int live = 0;
  unsigned long long t_min = ~0ULL, t_max = 0;
  for (int w = 0; w < wgs; ++w) {
    const unsigned long long* t = &h[(size_t)w * 8];
    if (!t[0]) continue;
    ++live;
    for (int i = 1; i < 3 + n_jobs; ++i) ph[i] += (double)(t[i] - t[i - 1]) * 0.01;   // 100 MHz -> us
    t_min = std::min(t_min, t[0]);
    t_max = std::max(t_max, t[2 + n_jobs]);
  }
  if (!live) return;
  fprintf(stderr, "[kmap trace] level n_in %lld, %d samples x %d slices, %d slots, %d jobs: box+fill %.1f us, insert %.1f us",
          (long long)n_in, nb, slices, slots, n_jobs, ph[1] / live, ph[2] / live);
  for (int j = 0; j < n_jobs; ++j) fprintf(stderr, ", job %d %.1f us", j, ph[3 + j] / live);
  fprintf(stderr, "; %d workgroups, launch span %.1f us\n", live, (double)(t_max - t_min) * 0.01);
}

// all fused maps that probe the table of `in`, on stream s: jobs[0..nj) index into plans
static int launch_level(const cs_coordmap* in, const MapPlan* plans, const int* jobs, int nj, uint32_t* key, int32_t* row,
                        hipStream_t s) {
  const int nb = in->n_batch;
  LevelArgs a;
  a.n_jobs = nj;
  for (int j = 0; j < nj; ++j) {
    const MapPlan& p = plans[jobs[j]];
    a.job[j] = LevelJob{p.out->d_coords, p.out->d_seg, p.km->d_nbr, p.ordered ? key + p.base : nullptr,
                        p.ordered ? row + p.base : nullptr, p.d_cnt, p.step, p.sign, (uint32_t)(jobs[j] % ORDER_MAX_MAPS) << 27};
  }
  a.in_coords = in->d_coords;
  a.in_seg = in->d_seg;
  a.unit = in->tensor_stride;
  a.ushift = ushift_of(in->tensor_stride);
  a.gkeys = in->d_keys;
  a.gvals = in->d_vals;
  a.gmask = in->capacity - 1;
  a.trace = nullptr;
  int slices = LEVEL_WGS / (nb > 0 ? nb : 1);
  slices = std::min(std::max(slices, 1), 8);
  // table size from the mean in-sample size (2.5x headroom; a larger sample is probed in the global table)
  const int64_t need = (in->n / (nb > 0 ? nb : 1)) * 5 / 2;
  const int slots = need <= LDS_SLOTS_SMALL / 8 * 5 ? LDS_SLOTS_SMALL : need <= LDS_SLOTS_MID / 8 * 5 ? LDS_SLOTS_MID : LDS_SLOTS_MAX;
  static const bool trace_on = getenv("CS_KMAP_TRACE") && getenv("CS_KMAP_TRACE")[0] == '1';
  const int wgs = slices * nb;
  if (trace_on) {
    if (hipMalloc(reinterpret_cast<void**>(&a.trace), (size_t)wgs * 64) != hipSuccess) a.trace = nullptr;
    if (a.trace) (void)hipMemsetAsync(a.trace, 0, (size_t)wgs * 64, s);
  }
  const dim3 grid((unsigned)slices, (unsigned)nb);
  if (slots == LDS_SLOTS_SMALL)
    hipLaunchKernelGGL((k_level_maps<LDS_SLOTS_SMALL, 256>), grid, dim3(256), 0, s, a);
  else if (slots == LDS_SLOTS_MID)
    hipLaunchKernelGGL((k_level_maps<LDS_SLOTS_MID, 512>), grid, dim3(512), 0, s, a);
  else
    hipLaunchKernelGGL((k_level_maps<LDS_SLOTS_MAX, 1024>), grid, dim3(1024), 0, s, a);
  CS_LAUNCH_CHECK();
  if (a.trace) {
    level_trace_report(a.trace, wgs, nj, slots, nb, slices, in->n, s);
    (void)hipFree(a.trace);
  }
  return CS_OK;
}

// one map through the GLOBAL table (1x1 "maps", rows not grouped by sample, CS_KMAP_GLOBAL)
static int launch_single(const MapPlan& p, hipStream_t s) {
  cs_kernelmap* km = p.km;
  const int64_t total = km->n_out * km->kvol;
  if (total == 0) return CS_OK;
  hipLaunchKernelGGL(k_build_nbr, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, p.out->d_coords, km->n_out, km->kvol,
                     p.step, p.sign, p.in->d_keys, p.in->d_vals, p.in->capacity - 1, km->d_nbr, p.d_cnt);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// Tiling order of the maps plans[idx[0..m)] (m <= ORDER_MAX_MAPS, all `ordered`) on stream s, which is behind every stream
// that built them: keys of the maps the level kernel did not build, ONE radix sort, one finish launch (row lists, group
// masks, pair counts to the host slots).
static int order_many(const MapPlan* plans, const int* idx, int m, uint32_t* key, int32_t* row, uint32_t* key_sorted,
                      int32_t* row_sorted, int64_t first, int64_t total, hipStream_t s) {
  if (m == 0) return CS_OK;
  OrderTab tab;
  tab.n = m;
  uint64_t kblk = 0, tblk = 0;
  bool any_keys = false;
  for (int j = 0; j < m; ++j) {
    const MapPlan& p = plans[idx[j]];
    cs_kernelmap* km = p.km;
    OrderMap& o = tab.m[j];
    const int64_t n = km->n_out;
    o.n_out = n;
    o.base = p.base - first;
    o.n_groups = ceil_div(ceil_div(n, 32), 8) * 8;
    o.nbr = km->d_nbr;
    km->d_rowlist = (int32_t*)pool_alloc(n * sizeof(int32_t));
    km->d_gmask = (uint32_t*)pool_alloc((size_t)o.n_groups * sizeof(uint32_t));
    CS_REQUIRE(km->d_rowlist && km->d_gmask, CS_ERR_HIP, "cs_kernelmap_build_many: tiling order allocation failed");
    o.rowlist = km->d_rowlist;
    o.gmask = km->d_gmask;
    o.d_cnt = p.d_cnt;
    o.host_cnt = nullptr;
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&o.host_cnt), km->h_cnt, 0) != hipSuccess) o.host_cnt = nullptr;
    CS_REQUIRE(o.host_cnt, CS_ERR_HIP, "cs_kernelmap_build_many: no device view of the pair-count slot");
    o.tag = (uint32_t)(idx[j] % ORDER_MAX_MAPS) << 27;
    o.need_keys = p.fused ? 0 : 1;
    any_keys = any_keys || !p.fused;
    o.kblk0 = (uint32_t)kblk;
    o.tblk0 = (uint32_t)tblk;
    kblk += (uint64_t)ceil_div(n, 256);
    tblk += (uint64_t)std::max<int64_t>(ceil_div(n, 256), 1);
  }
  CS_REQUIRE(total < (1LL << 31) && kblk < (1ULL << 31), CS_ERR_UNSUPPORTED, "cs_kernelmap_build_many: batch too large");
  int map_bits = 0;
  while ((1 << map_bits) < ORDER_MAX_MAPS) ++map_bits;
  size_t tmp_bytes = 0;
  CS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, key + first, key_sorted + first, row + first,
                                                  row_sorted + first, (int)total, 0, 27 + map_bits, s));
  PoolBuf<char> tmp(tmp_bytes ? tmp_bytes : 1);
  CS_REQUIRE(tmp.p, CS_ERR_HIP, "cs_kernelmap_build_many: row order scratch allocation failed");
  if (any_keys) {
    hipLaunchKernelGGL(k_row_keys_all, dim3((unsigned)kblk), dim3(256), 0, s, tab, key + first, row + first);
    CS_LAUNCH_CHECK();
  }
  CS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, key + first, key_sorted + first, row + first,
                                                  row_sorted + first, (int)total, 0, 27 + map_bits, s));
  hipLaunchKernelGGL(k_order_finish, dim3((unsigned)tblk), dim3(256), 0, s, tab, key_sorted + first, row_sorted + first);
  CS_LAUNCH_CHECK();
  for (int j = 0; j < m; ++j) CS_HIP_CHECK(hipEventRecord(plans[idx[j]].km->cnt_ready, s));
  return CS_OK;
}

// ---- the steps of cs_kernelmap_build_many ---------------------------------------------------------------------------------
// What a call builds: the maps (owned until release(): a failed call frees them), their device pair counters and the batch's
// sort arrays.
struct BatchPlan {
  std::vector<MapPlan> maps;
  PoolBuf<unsigned long long> cnts;
  int64_t total_rows = 0;              // rows of all ordered maps
  PoolBuf<uint32_t> key, key_sorted;
  PoolBuf<int32_t> row, row_sorted;
  ~BatchPlan() {
    for (MapPlan& p : maps) cs_kernelmap_free(p.km);   // (nullptr is fine)
  }
  void release(cs_kernelmap** km_out) {
    for (size_t i = 0; i < maps.size(); ++i) km_out[i] = std::exchange(maps[i].km, nullptr);
  }
};

// plan: map objects and count slots, which maps the level kernel builds (`fused`) and which get a tiling order (`ordered`),
// their bases in the sort arrays; the pair counters are zeroed on s (before the streams fork)
static int plan_batch(BatchPlan& b, const int* kernel_size, const int* transposed, bool global_only, hipStream_t s) {
  const int n = (int)b.maps.size();
  CS_REQUIRE(b.cnts.alloc(n), CS_ERR_HIP, "cs_kernelmap_build_many: allocation failed");
  for (int i = 0; i < n; ++i) {
    MapPlan& p = b.maps[i];
    cs_kernelmap* km = new cs_kernelmap();
    p.km = km;
    km->n_out = p.out->n;
    km->n_in = p.in->n;
    km->kvol = kernel_size[i] == 3 ? 27 : 1;
    km->transposed = transposed[i];
    const int64_t total = km->n_out * km->kvol;
    km->d_nbr = (int32_t*)pool_alloc((total ? total : 1) * sizeof(int32_t));
    p.d_cnt = b.cnts.p + i;
    CS_REQUIRE(km->d_nbr, CS_ERR_HIP, "cs_kernelmap_build_many: allocation failed");
    if (total == 0) {
      km->num_pairs = 0;
      continue;
    }
    km->h_cnt = count_slot_acquire(&km->cnt_slot);
    CS_REQUIRE(km->h_cnt && hipEventCreateWithFlags(&km->cnt_ready, hipEventDisableTiming) == hipSuccess, CS_ERR_HIP,
               "cs_kernelmap_build_many: pair-count slot allocation failed");
    p.ordered = km->kvol == 27;
    p.fused = !global_only && km->kvol == 27 && p.in->seg_state == 1 && p.out->seg_state == 1 &&
              p.in->n_batch == p.out->n_batch;
    if (p.ordered) {
      p.base = b.total_rows;
      b.total_rows += km->n_out;
    }
  }
  CS_REQUIRE(b.total_rows < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_kernelmap_build_many: batch too large");
  const size_t rows = (size_t)b.total_rows;
  CS_REQUIRE(b.key.alloc(rows) && b.key_sorted.alloc(rows) && b.row.alloc(rows) && b.row_sorted.alloc(rows), CS_ERR_HIP,
             "cs_kernelmap_build_many: row order scratch allocation failed");
  CS_REQUIRE(hipMemsetAsync(b.cnts.p, 0, sizeof(unsigned long long) * n, s) == hipSuccess, CS_ERR_HIP,
             "cs_kernelmap_build_many: memset failed");
  return CS_OK;
}

// The caller's stream and up to four of the thread's side streams.  fork(): every side stream starts behind the caller's
// stream; join(): the caller's stream continues behind all of them.  A fork that was not joined is joined on scope exit (the
// error paths: the side streams may hold work that reads scratch of the call).
struct StreamFork {
  hipStream_t st[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int ns = 1, lane = 0;
  bool open = false;
  hipEvent_t fork_ev = nullptr, join_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  StreamFork(hipStream_t s, int n_streams) {
    st[0] = s;
    for (int k = 1; k < n_streams; ++k) st[k] = side_stream(k - 1);
    while (ns < n_streams && st[ns]) ++ns;
  }
  StreamFork(const StreamFork&) = delete;
  StreamFork& operator=(const StreamFork&) = delete;
  ~StreamFork() {
    if (open) (void)join();
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    for (hipEvent_t e : join_ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipStream_t next() { return st[lane++ % ns]; }   // round-robin over the streams
  hipError_t fork() {
    if (ns == 1) return hipSuccess;
    hipError_t e = hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(fork_ev, st[0]);
    for (int k = 1; k < ns && e == hipSuccess; ++k) {
      e = hipEventCreateWithFlags(&join_ev[k], hipEventDisableTiming);
      if (e == hipSuccess) e = hipStreamWaitEvent(st[k], fork_ev, 0);
    }
    open = e == hipSuccess;
    return e;
  }
  hipError_t join() {
    hipError_t je = hipSuccess;
    for (int k = 1; k < ns && open; ++k) {
      hipError_t e = hipEventRecord(join_ev[k], st[k]);
      if (e == hipSuccess) e = hipStreamWaitEvent(st[0], join_ev[k], 0);
      if (e != hipSuccess) {
        (void)hipStreamSynchronize(st[k]);   // the join by the host instead
        je = e;
      }
    }
    open = false;
    return je;
  }
};

// blocks freed inside the scope change hands when it is left: the pool's cache is ordered against ONE stream
struct PoolDeferScope {
  PoolDeferScope() { pool_defer_begin(); }
  ~PoolDeferScope() { pool_defer_end(); }
};

// builders: one launch per probed level and chunk of ORDER_MAX_MAPS (fused maps), one per remaining map
static int launch_builders(BatchPlan& b, StreamFork& streams) {
  const int n = (int)b.maps.size();
  const MapPlan* plans = b.maps.data();
  std::vector<char> done(n, 0);
  for (int i = 0; i < n; ++i) {
    if (done[i] || !plans[i].fused) continue;
    int jobs[LEVEL_MAX_JOBS], nj = 0;
    for (int j = i; j < n && nj < LEVEL_MAX_JOBS; ++j)
      if (!done[j] && plans[j].fused && plans[j].in == plans[i].in && (j / ORDER_MAX_MAPS) == (i / ORDER_MAX_MAPS)) {
        jobs[nj++] = j;
        done[j] = 1;
      }
    const int rc = launch_level(plans[i].in, plans, jobs, nj, b.key.p, b.row.p, streams.next());
    if (rc != CS_OK) return rc;
  }
  for (int i = 0; i < n; ++i) {
    if (done[i]) continue;
    const int rc = launch_single(plans[i], streams.next());
    if (rc != CS_OK) return rc;
  }
  return CS_OK;
}

// tiling order of all ordered maps (ONE sort per ORDER_MAX_MAPS maps) and the pair counts of the others, on the caller's
// stream behind the join
static int order_and_count(BatchPlan& b, hipStream_t s) {
  const int n = (int)b.maps.size();
  const MapPlan* plans = b.maps.data();
  for (int c0 = 0; c0 < n; c0 += ORDER_MAX_MAPS) {
    int idx[ORDER_MAX_MAPS], m = 0;
    int64_t first = -1, rows = 0;
    for (int i = c0; i < std::min(n, c0 + ORDER_MAX_MAPS); ++i)
      if (plans[i].ordered) {
        if (first < 0) first = plans[i].base;
        rows += plans[i].km->n_out;
        idx[m++] = i;
      }
    if (!m) continue;
    const int rc = order_many(plans, idx, m, b.key.p, b.row.p, b.key_sorted.p, b.row_sorted.p, first, rows, s);
    if (rc != CS_OK) return rc;
  }
  // maps without a tiling order (1x1 "maps"): the count goes to the host slot by a copy
  for (int i = 0; i < n; ++i) {
    cs_kernelmap* km = plans[i].km;
    if (plans[i].ordered || km->num_pairs == 0) continue;
    hipError_t e = hipMemcpyAsync(km->h_cnt, plans[i].d_cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(km->cnt_ready, s);
    CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_kernelmap_build_many: %s", hipGetErrorString(e));
  }
  return CS_OK;
}

extern "C" {

// The kernel maps of a batch.  Maps are grouped by the coordinate level they PROBE (their `in` map): one k_level_maps launch
// per level serves every map of the group from one LDS table per sample, and the levels run on up to five streams (four by
// default: the caller's and the thread's side streams; every side stream starts behind the caller's stream and the caller's stream
// continues behind all of them; scratch freed meanwhile is handed back to the pool only after that join).  Then ONE radix
// sort gives every map its tiling order.  CS_KMAP_STREAMS=1: everything on the caller's stream; CS_KMAP_GLOBAL=1: the
// global-table kernel for everything.
int cs_kernelmap_build_many(int n, const cs_coordmap* const* in, const cs_coordmap* const* out, const int* kernel_size,
                            const int* transposed, void* stream, cs_kernelmap** km_out) {
  CS_REQUIRE(n >= 0 && (n == 0 || (in && out && kernel_size && transposed && km_out)), CS_ERR_INVALID,
             "cs_kernelmap_build_many: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  for (int i = 0; i < n; ++i) km_out[i] = nullptr;
  if (n == 0) return CS_OK;
  BatchPlan plan;
  plan.maps.resize(n);
  for (int i = 0; i < n; ++i) {
    MapPlan& p = plan.maps[i];
    const int rc = map_geometry(in[i], out[i], kernel_size[i], transposed[i], &p.step, &p.sign);
    if (rc != CS_OK) return rc;
    p.in = in[i];
    p.out = out[i];
  }
  const bool global_only = getenv("CS_KMAP_GLOBAL") != nullptr;
  // per-sample segments of the coordinate maps (lazily, cached on the map): on the caller's stream before the streams fork
  if (!global_only) {
    std::vector<cs_coordmap*> need;
    for (int i = 0; i < n; ++i)
      if (kernel_size[i] == 3) {
        need.push_back(const_cast<cs_coordmap*>(in[i]));
        need.push_back(const_cast<cs_coordmap*>(out[i]));
      }
    const int rc_seg = ensure_segments_many(need.data(), (int)need.size(), s);
    if (rc_seg != CS_OK) return rc_seg;
  }
  // read per call, like every other knob (tests flip it between calls of one process)
  const int n_streams = [] {
    const char* e = getenv("CS_KMAP_STREAMS");
    int v = e ? atoi(e) : 4;   // 2 / 3 / 4 / 5 streams: stress 6016 / 6201 / 6235 / 5608 clouds/s (the runtime maps streams to 4 queues)
    return v < 1 ? 1 : (v > 5 ? 5 : v);
  }();
  // (on every exit, in this order: the streams are joined, deferred blocks change hands, a failed call's maps are freed)
  PoolDeferScope defer;
  StreamFork streams(s, n_streams);
  int rc = plan_batch(plan, kernel_size, transposed, global_only, s);
  if (rc != CS_OK) return rc;
  hipError_t e = streams.fork();
  CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_kernelmap_build_many: %s", hipGetErrorString(e));
  {
    ProfScope prof("kmap", s);
    rc = launch_builders(plan, streams);
    e = streams.join();   // also behind a failed launch
  }
  if (rc != CS_OK) return rc;
  CS_REQUIRE(e == hipSuccess, CS_ERR_HIP, "cs_kernelmap_build_many: joining the streams failed: %s", hipGetErrorString(e));
  {
    ProfScope prof("kmap", s);
    rc = order_and_count(plan, s);
  }
  if (rc != CS_OK) return rc;
  plan.release(km_out);
  return CS_OK;
}

int cs_kernelmap_build(const cs_coordmap* in, const cs_coordmap* out, int kernel_size, int transposed, void* stream,
                       cs_kernelmap** km_out) {
  CS_REQUIRE(km_out, CS_ERR_INVALID, "cs_kernelmap_build: NULL argument");
  *km_out = nullptr;
  const cs_coordmap* ins[1] = {in};
  const cs_coordmap* outs[1] = {out};
  return cs_kernelmap_build_many(1, ins, outs, &kernel_size, &transposed, stream, km_out);
}

int64_t cs_kernelmap_num_pairs(const cs_kernelmap* km) { return cs::kernelmap_pairs(km); }
int64_t cs_kernelmap_rows(const cs_kernelmap* km) { return km ? km->n_out : -1; }
const int32_t* cs_kernelmap_table(const cs_kernelmap* km) { return km ? km->d_nbr : nullptr; }

int64_t cs_kernelmap_export(const cs_kernelmap* km, int32_t* d_k, int32_t* d_in, int32_t* d_out,
                            int64_t capacity, void* stream) {
  CS_REQUIRE(km && d_k && d_in && d_out, CS_ERR_INVALID, "cs_kernelmap_export: NULL argument");
  const int64_t pairs = cs::kernelmap_pairs(km);
  CS_REQUIRE(pairs >= 0 && capacity >= pairs, CS_ERR_INVALID,
             "cs_kernelmap_export: capacity %lld < %lld pairs", (long long)capacity, (long long)pairs);
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const int64_t total = km->n_out * km->kvol;
  if (total == 0) return 0;
  CS_REQUIRE(total < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_kernelmap_export: table too large");
  PoolBuf<int32_t> flag(total), pos(total);
  CS_REQUIRE(flag.p && pos.p, CS_ERR_HIP, "cs_kernelmap_export: scratch allocation failed");
  const unsigned g = (unsigned)ceil_div(total, 256);
  hipLaunchKernelGGL(k_export_flag, dim3(g), dim3(256), 0, s, km->d_nbr, km->n_out, km->kvol,
                     flag.p);
  CS_LAUNCH_CHECK();
  int rc = exclusive_scan_i32(flag.p, pos.p, total, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_export_emit, dim3(g), dim3(256), 0, s, km->d_nbr, km->n_out, km->kvol,
                     flag.p, pos.p, capacity, d_k, d_in, d_out);
  CS_LAUNCH_CHECK();
  CS_HIP_CHECK(download_sync(s));
  return pairs;
}

void cs_kernelmap_free(cs_kernelmap* km) {
  if (!km) return;
  pool_free(km->d_nbr);
  pool_free(km->d_rowlist);
  pool_free(km->d_gmask);
  bool counted = false;
  // (the slot must not be recycled under a pending copy)
  if (km->cnt_ready) counted = hipEventSynchronize(km->cnt_ready) == hipSuccess;
  cs::prof_retire(km, counted);   // before the event goes: kernelmap_flush_prof waits on the events of listed maps
  if (km->cnt_ready) (void)hipEventDestroy(km->cnt_ready);
  count_slot_release(km->cnt_slot);
  delete km;
}

}  // extern "C"
