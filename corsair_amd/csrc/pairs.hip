// Training-batch geometry: batched fixed-radius pair search, PiP / PiN / NiN pair sampling and the f64
// rigid transform of the train-mode augmentation.  Replaces utils/preprocess.py:get_matching_indices (an Open3D
// KD-tree radius query from a Python loop), generate_rand_negative_pairs + _hash and the np.matmul of
// random_rotation, as datasets/CategoryDataset.py:121-151,229-251 use them.
//
// Radius search: the target rows of every problem are sorted by (problem, cell) with cell = floor(t / c), c slightly
// larger than r; an open-addressing table maps a cell to its [begin, end) range of the sorted rows; every source row
// probes the 27 neighbouring cells.  The cell function, the table and the probe are cellgrid.h's (shared with
// normals.hip), with the completeness argument and the clamp to the 16-bit key range; the distance chain rp_d2 is this
// unit's own.
#include <hipcub/hipcub.hpp>

#include <vector>

#include "cellgrid.h"

namespace cs {
namespace {

struct RPProb {
  int64_t s0, ns;    // first global source row, source rows
  int64_t t0, nt;    // first global target row, target rows
  int64_t row0;      // first output row (problem-major)
  int64_t m0;        // first entry of the problem in the sorted target arrays
};

constexpr int kSmallRow = 32;   // rows with at most this many hits are sorted in private memory

__device__ __forceinline__ double rp_d2(double sx, double sy, double sz, double tx, double ty, double tz) {
  const double dx = sx - tx, dy = sy - ty, dz = sz - tz;
  return (dx * dx + dy * dy) + dz * dz;   // -ffp-contract=off: no fma
}

struct RPTable {
  CellTable cells;
  const double* xyz;   // sorted target rows [M,3]
  const int32_t* j;    // local target index of every sorted row
};

// calls f(d2, j) for every target j of problem p with d2 < r2 (in no particular order)
template <typename F>
__device__ __forceinline__ void rp_probe(const RPTable& tb, int p, double sx, double sy, double sz, double cell,
                                         double r2, F&& f) {
  cg_probe<3>(
      tb.cells, tb.xyz, p, sx, sy, sz, cell, r2, [&](const double* t) { return rp_d2(sx, sy, sz, t[0], t[1], t[2]); },
      [&](double d2, int32_t m) { f(d2, tb.j[m]); });
}

__global__ void k_rp_keys(const RPProb* __restrict__ probs, const double* __restrict__ tgt, double cell,
                          uint64_t* keys, int32_t* vals) {
  const int p = blockIdx.y;
  const RPProb P = probs[p];
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= P.nt) return;
  const double* t = tgt + 3 * (P.t0 + j);
  keys[P.m0 + j] = pack_key(p, cg_cell(t[0], cell), cg_cell(t[1], cell), cg_cell(t[2], cell));
  vals[P.m0 + j] = (int32_t)j;
}

__global__ void k_rp_gather(const RPProb* __restrict__ probs, const double* __restrict__ tgt,
                            const uint64_t* __restrict__ keys, const int32_t* __restrict__ j, int64_t m_total,
                            double* xyz) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= m_total) return;
  const int p = (int)(keys[m] >> 48);
  const double* t = tgt + 3 * (probs[p].t0 + j[m]);
  xyz[3 * m] = t[0];
  xyz[3 * m + 1] = t[1];
  xyz[3 * m + 2] = t[2];
}

__global__ void k_cg_table_fill(uint64_t* keys, uint64_t cap) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x)
    keys[i] = kEmptyKey;
}

__device__ __forceinline__ uint64_t cg_insert(uint64_t* keys, uint64_t mask, uint64_t key) {
  uint64_t slot = hash64(key) & mask;
  while (true) {
    const unsigned long long old = atomicCAS((unsigned long long*)&keys[slot], (unsigned long long)kEmptyKey,
                                             (unsigned long long)key);
    if (old == kEmptyKey || old == key) return slot;
    slot = (slot + 1) & mask;
  }
}

// every run of equal keys (one cell of one problem) gets its [begin, end) range
__global__ void k_cg_insert(const uint64_t* __restrict__ skeys, int64_t m_total, uint64_t* keys, int32_t* beg,
                            int32_t* end, uint64_t mask) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= m_total) return;
  const uint64_t k = skeys[m];
  if (m == 0 || skeys[m - 1] != k) beg[cg_insert(keys, mask, k)] = (int32_t)m;
  if (m == m_total - 1 || skeys[m + 1] != k) end[cg_insert(keys, mask, k)] = (int32_t)(m + 1);
}

__global__ void k_rp_count(const RPProb* __restrict__ probs, const double* __restrict__ src, RPTable tb,
                           double cell, double r2, int k_max, int32_t* cnt_full, int64_t* cnt_cap) {
  const int p = blockIdx.y;
  const RPProb P = probs[p];
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= P.ns) return;
  const double* s = src + 3 * (P.s0 + i);
  int n = 0;
  rp_probe(tb, p, s[0], s[1], s[2], cell, r2, [&](double, int32_t) { ++n; });
  cnt_full[P.row0 + i] = n;
  cnt_cap[P.row0 + i] = k_max > 0 && n > k_max ? k_max : n;
}

__device__ __forceinline__ bool rp_less(double da, int32_t ja, double db, int32_t jb) {
  return da < db || (da == db && ja < jb);
}

// each row's hits in ascending (d2, j): the first row_ptr[r+1] - row_ptr[r] of them
__global__ void k_rp_fill(const RPProb* __restrict__ probs, const double* __restrict__ src, RPTable tb, double cell,
                          double r2, const int32_t* __restrict__ cnt_full, const int64_t* __restrict__ row_ptr,
                          int32_t* out) {
  const int p = blockIdx.y;
  const RPProb P = probs[p];
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= P.ns) return;
  const int64_t r = P.row0 + i;
  const int64_t o0 = row_ptr[r];
  const int cap = (int)(row_ptr[r + 1] - o0);
  if (cap == 0) return;
  const double* s = src + 3 * (P.s0 + i);
  const double sx = s[0], sy = s[1], sz = s[2];
  if (cnt_full[r] <= kSmallRow) {
    double d[kSmallRow];
    int32_t jj[kSmallRow];
    int n = 0;
    rp_probe(tb, p, sx, sy, sz, cell, r2, [&](double d2, int32_t j) {   // insertion sort
      int q = n++;
      while (q > 0 && rp_less(d2, j, d[q - 1], jj[q - 1])) {
        d[q] = d[q - 1];
        jj[q] = jj[q - 1];
        --q;
      }
      d[q] = d2;
      jj[q] = j;
    });
    for (int q = 0; q < cap; ++q) out[o0 + q] = jj[q];
    return;
  }
  // long rows (no bound holds: targets quantised in a rotated frame can lie arbitrarily close): the position of a
  // hit is the number of hits before it in (d2, j) order, counted by a second probe -- exact for any length
  rp_probe(tb, p, sx, sy, sz, cell, r2, [&](double d2, int32_t j) {
    int rank = 0;
    rp_probe(tb, p, sx, sy, sz, cell, r2, [&](double e2, int32_t k) { rank += rp_less(e2, k, d2, j); });
    if (rank < cap) out[o0 + rank] = j;
  });
}

// ---- pair sampling ---------------------------------------------------------------------------------------------
struct SPProb {
  int64_t b0, nb;      // base segment (first global row, rows)
  int64_t q0, nq;      // positive segment
  int64_t g0, ng;      // negative segment
  int64_t row0, row1;  // this problem's rows of the PiP CSR
  int64_t slot;
};

// the generator of include/corsair_hip.h (cs_sample_pairs)
__device__ __forceinline__ uint64_t sp_rng(uint64_t seed, uint64_t slot, uint64_t round, uint64_t stream,
                                           uint64_t ctr) {
  return rng_u64(seed, 0, (slot << 40) | (round << 36) | (stream << 32) | ctr);
}
__device__ __forceinline__ int64_t sp_index(uint64_t x, int64_t n) {
  const double u = (double)(x >> 11) * 0x1.0p-53;
  return (int64_t)floor(u * (double)n);
}

constexpr int kSpThreads = 256;

// PiN (blockIdx.y = 0) / NiN (1) of one problem per block: candidates in draw order, the first `sample` survivors
__global__ void __launch_bounds__(kSpThreads) k_sp_negatives(const SPProb* __restrict__ probs, const float* __restrict__ xyz,
                                                             const int64_t* __restrict__ row_ptr, uint64_t seed, int round,
                                                             double r2, float min_dist, int sample, int32_t* pin,
                                                             int32_t* nin, int32_t* counts) {
  using Scan = hipcub::BlockScan<int, kSpThreads>;
  __shared__ typename Scan::TempStorage tmp;
  const int p = blockIdx.x, list = 1 + blockIdx.y;   // generator stream 1 = PiN, 2 = NiN
  const SPProb P = probs[p];
  const int64_t n_draw = row_ptr[P.row1] - row_ptr[P.row0];
  const int64_t n1 = list == 1 ? P.nq : P.ng;
  const int64_t t0 = list == 1 ? P.q0 : P.g0;
  int32_t* out = (list == 1 ? pin : nin) + 2 * (int64_t)p * sample;
  int total = 0;
  for (int64_t c0 = 0; c0 < n_draw && total < sample; c0 += kSpThreads) {
    const int64_t t = c0 + threadIdx.x;
    int keep = 0;
    int64_t i = 0, j = 0;
    if (t < n_draw && n1 > 0) {   // n_draw > 0 implies base rows; an empty negative cloud has no candidates
      i = sp_index(sp_rng(seed, P.slot, round, list, 2 * t), P.nb);
      j = sp_index(sp_rng(seed, P.slot, round, list, 2 * t + 1), n1);
      i = i < P.nb ? i : P.nb - 1;   // floor(u * n) < n already; kept as a bound
      j = j < n1 ? j : n1 - 1;
      const float* a = xyz + 3 * (P.b0 + i);
      const float* b = xyz + 3 * (t0 + j);
      if (list == 1)
        keep = !(rp_d2(a[0], a[1], a[2], b[0], b[1], b[2]) < r2);   // not in PiP: exactly the radius test
      else
        keep = !(i == 0 && j == 0);
      const float fx = a[0] - b[0], fy = a[1] - b[1], fz = a[2] - b[2];
      keep = keep && __fsqrt_rn((fx * fx + fy * fy) + fz * fz) > min_dist;
    }
    int pos, agg;
    Scan(tmp).ExclusiveSum(keep, pos, agg);
    if (keep && total + pos < sample) {
      out[2 * (total + pos)] = (int32_t)i;
      out[2 * (total + pos) + 1] = (int32_t)j;
    }
    total += agg;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[4 * p + 0] = (int32_t)n_draw;
    counts[4 * p + list + 1] = total < sample ? total : sample;
  }
}

// PiP of one problem per block.  Sort key of pair t (its CSR position within the problem) = (high 32 bits of the
// generator, stream 0) << 32 | t, unique; the min(sample, n) smallest keys, ascending (radix select + LDS sort)
__global__ void __launch_bounds__(1024) k_sp_positives(const SPProb* __restrict__ probs, const int64_t* __restrict__ row_ptr,
                                                       const int32_t* __restrict__ tgt_idx, uint64_t seed, int round,
                                                       int sample, int32_t* pip, int32_t* counts) {
  extern __shared__ uint64_t s_keys[];   // [next power of two >= sample]
  __shared__ uint32_t hist[256];
  __shared__ uint64_t s_prefix;
  __shared__ int64_t s_need;
  __shared__ int s_fill;
  const int p = blockIdx.x;
  const SPProb P = probs[p];
  const int64_t g0 = row_ptr[P.row0];
  const int64_t n = row_ptr[P.row1] - g0;
  const int c = n < sample ? (int)n : sample;
  auto key_of = [&](int64_t t) {
    return (sp_rng(seed, P.slot, round, 0, (uint64_t)t) & 0xFFFFFFFF00000000ULL) | (uint64_t)t;
  };
  if (threadIdx.x == 0) {
    s_prefix = 0;
    s_need = c;
    s_fill = 0;
    counts[4 * p + 1] = c;
  }
  __syncthreads();
  if (c == 0) return;
  for (int shift = 56; shift >= 0; shift -= 8) {   // radix select of the c-th smallest key
    for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    const uint64_t hi = shift == 56 ? 0 : ~0ULL << (shift + 8);
    const uint64_t pre = s_prefix;
    for (int64_t t = threadIdx.x; t < n; t += blockDim.x) {
      const uint64_t k = key_of(t);
      if ((k & hi) == (pre & hi)) atomicAdd(&hist[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t need = s_need;
      int b = 0;
      while ((int64_t)hist[b] < need) need -= hist[b++];
      s_need = need;
      s_prefix = pre | ((uint64_t)b << shift);
    }
    __syncthreads();
  }
  const uint64_t thr = s_prefix;
  int np2 = 1;
  while (np2 < c) np2 <<= 1;
  for (int q = threadIdx.x; q < np2; q += blockDim.x) s_keys[q] = ~0ULL;
  __syncthreads();
  for (int64_t t = threadIdx.x; t < n; t += blockDim.x) {
    const uint64_t k = key_of(t);
    if (k <= thr) {   // exactly c keys (they are unique); the sort below fixes their order
      const int q = atomicAdd(&s_fill, 1);
      if (q < np2) s_keys[q] = k;
    }
  }
  __syncthreads();
  for (int size = 2; size <= np2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int q = threadIdx.x; q < np2; q += blockDim.x) {
        const int r = q ^ stride;
        if (r > q) {
          const uint64_t a = s_keys[q], b = s_keys[r];
          if ((a > b) == ((q & size) == 0)) {
            s_keys[q] = b;
            s_keys[r] = a;
          }
        }
      }
      __syncthreads();
    }
  int32_t* out = pip + 2 * (int64_t)p * sample;
  for (int q = threadIdx.x; q < c; q += blockDim.x) {
    const int64_t g = g0 + (int64_t)(s_keys[q] & 0xFFFFFFFFULL);
    int64_t lo = P.row0, hi = P.row1;   // the source row: last r with row_ptr[r] <= g
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (row_ptr[mid] <= g) lo = mid; else hi = mid;
    }
    out[2 * q] = (int32_t)(lo - P.row0);
    out[2 * q + 1] = tgt_idx[g];
  }
}

// ---- f64 rigid transform ---------------------------------------------------------------------------------------
__global__ void k_transform_f64(const float* __restrict__ xyz, const int64_t* __restrict__ desc,
                                const double* __restrict__ T, double* out) {
  const int p = blockIdx.y;
  const int64_t s0 = desc[3 * p], n = desc[3 * p + 1], o0 = desc[3 * p + 2];
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = xyz[3 * (s0 + i)], y = xyz[3 * (s0 + i) + 1], z = xyz[3 * (s0 + i) + 2];
  const double* M = T + 16 * p;
  out[3 * (o0 + i) + 0] = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  out[3 * (o0 + i) + 1] = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  out[3 * (o0 + i) + 2] = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

}  // namespace
}  // namespace cs

struct cs_radius_plan {
  int n_prob = 0;
  int64_t rows = 0, m_total = 0, max_ns = 0;
  double cell = 0.0, r2 = 0.0;
  const double* d_src = nullptr;   // the caller's source rows (kept alive until the fill)
  cs::RPProb* d_probs = nullptr;
  uint64_t* d_tkeys = nullptr;
  int32_t *d_tbeg = nullptr, *d_tend = nullptr;
  uint64_t cap = 0;
  double* d_xyz = nullptr;
  int32_t* d_j = nullptr;
  int32_t* d_cnt_full = nullptr;
};

namespace cs {
namespace {

void plan_release(cs_radius_plan* pl) {
  if (!pl) return;
  void* bufs[] = {pl->d_probs, pl->d_tkeys, pl->d_tbeg, pl->d_tend, pl->d_xyz, pl->d_j, pl->d_cnt_full};
  for (void* b : bufs)
    if (b) pool_free(b);
  delete pl;
}

RPTable plan_table(const cs_radius_plan* pl) {
  return RPTable{CellTable{pl->d_tkeys, pl->d_tbeg, pl->d_tend, pl->cap - 1}, pl->d_xyz, pl->d_j};
}

}  // namespace

// the launchers of cellgrid.h
void cellgrid_table_fill(uint64_t* d_keys, uint64_t cap, hipStream_t s) {
  hipLaunchKernelGGL(k_cg_table_fill, dim3((unsigned)(cap / 256 < 2048 ? cap / 256 : 2048)), dim3(256), 0, s, d_keys, cap);
}
void cellgrid_insert_ranges(const uint64_t* d_skeys, int64_t m_total, uint64_t* d_keys, int32_t* d_beg, int32_t* d_end,
                            uint64_t mask, hipStream_t s) {
  hipLaunchKernelGGL(k_cg_insert, dim3((unsigned)ceil_div(m_total, 256)), dim3(256), 0, s, d_skeys, m_total, d_keys, d_beg,
                     d_end, mask);
}
}  // namespace cs

using namespace cs;

extern "C" {

int cs_radius_pairs(const double* d_src, const int64_t* h_soff, const double* d_tgt, const int64_t* h_toff,
                    const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, double radius, int k_max,
                    int64_t* d_row_ptr, void* stream, cs_radius_plan** plan) {
  CS_REQUIRE(plan && h_soff && h_toff && h_src_seg && h_tgt_seg && d_row_ptr, CS_ERR_INVALID,
             "cs_radius_pairs: NULL argument");
  *plan = nullptr;
  CS_REQUIRE(n_prob >= 1 && n_prob < 65536, CS_ERR_INVALID, "cs_radius_pairs: 1 <= n_prob < 65536");
  CS_REQUIRE(radius > 0.0 && radius < 1e300, CS_ERR_INVALID, "cs_radius_pairs: radius must be positive and finite");
  std::vector<RPProb> hp(n_prob);
  int64_t rows = 0, m_total = 0, max_ns = 0, max_nt = 0;
  for (int p = 0; p < n_prob; ++p) {
    const int64_t ss = h_src_seg[p], ts = h_tgt_seg[p];
    CS_REQUIRE(ss >= 0 && ts >= 0, CS_ERR_INVALID, "cs_radius_pairs: negative segment id");
    RPProb& P = hp[p];
    P.s0 = h_soff[ss];
    P.ns = h_soff[ss + 1] - P.s0;
    P.t0 = h_toff[ts];
    P.nt = h_toff[ts + 1] - P.t0;
    CS_REQUIRE(P.ns >= 0 && P.nt >= 0 && P.s0 >= 0 && P.t0 >= 0, CS_ERR_INVALID, "cs_radius_pairs: bad offsets");
    P.row0 = rows;
    P.m0 = m_total;
    rows += P.ns;
    m_total += P.nt;
    if (P.ns > max_ns) max_ns = P.ns;
    if (P.nt > max_nt) max_nt = P.nt;
  }
  CS_REQUIRE(m_total < (1LL << 31) && rows < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_radius_pairs: too many rows");
  CS_REQUIRE((rows == 0 || d_src) && (m_total == 0 || d_tgt), CS_ERR_INVALID, "cs_radius_pairs: NULL points");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  cs_radius_plan* pl = new cs_radius_plan();
  pl->n_prob = n_prob;
  pl->rows = rows;
  pl->m_total = m_total;
  pl->max_ns = max_ns;
  pl->cell = radius * (1.0 + 1.0 / 1024.0);   // > r by far more than any rounding of floor(x / cell) can move
  pl->r2 = radius * radius;
  pl->d_src = d_src;
  pl->cap = 1024;
  while (pl->cap < (uint64_t)(2 * m_total)) pl->cap <<= 1;
  const int64_t m1 = m_total ? m_total : 1;
  pl->d_probs = (RPProb*)pool_alloc(sizeof(RPProb) * n_prob);
  pl->d_tkeys = (uint64_t*)pool_alloc(sizeof(uint64_t) * pl->cap);
  pl->d_tbeg = (int32_t*)pool_alloc(sizeof(int32_t) * pl->cap);
  pl->d_tend = (int32_t*)pool_alloc(sizeof(int32_t) * pl->cap);
  pl->d_xyz = (double*)pool_alloc(sizeof(double) * 3 * m1);
  pl->d_j = (int32_t*)pool_alloc(sizeof(int32_t) * m1);
  pl->d_cnt_full = (int32_t*)pool_alloc(sizeof(int32_t) * (rows ? rows : 1));
  PoolBuf<uint64_t> keys(m1), skeys(m1);
  PoolBuf<int32_t> vals(m1);
  PoolBuf<int64_t> cnt(rows + 1);
  if (!(pl->d_probs && pl->d_tkeys && pl->d_tbeg && pl->d_tend && pl->d_xyz && pl->d_j && pl->d_cnt_full && keys.p &&
        skeys.p && vals.p && cnt.p)) {
    plan_release(pl);
    set_error("cs_radius_pairs: scratch allocation failed");
    return CS_ERR_HIP;
  }
  hipError_t e = hipMemcpyAsync(pl->d_probs, hp.data(), sizeof(RPProb) * n_prob, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(cnt.p, 0, sizeof(int64_t) * (rows + 1), s);
  if (e == hipSuccess) {
    cellgrid_table_fill(pl->d_tkeys, pl->cap, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess && m_total > 0) {
    hipLaunchKernelGGL(k_rp_keys, dim3((unsigned)ceil_div(max_nt, 256), (unsigned)n_prob), dim3(256), 0, s,
                       pl->d_probs, d_tgt, pl->cell, keys.p, vals.p);
    size_t tmp_bytes = 0;
    e = hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.p, skeys.p, vals.p, pl->d_j, (int)m_total, 0, 64, s);
    PoolBuf<char> tmp(tmp_bytes);
    if (e == hipSuccess && !tmp.p) e = hipErrorOutOfMemory;
    if (e == hipSuccess)
      e = hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.p, skeys.p, vals.p, pl->d_j, (int)m_total, 0, 64, s);
    if (e == hipSuccess) {
      const unsigned g = (unsigned)ceil_div(m_total, 256);
      hipLaunchKernelGGL(k_rp_gather, dim3(g), dim3(256), 0, s, pl->d_probs, d_tgt, skeys.p, pl->d_j, m_total,
                         pl->d_xyz);
      cellgrid_insert_ranges(skeys.p, m_total, pl->d_tkeys, pl->d_tbeg, pl->d_tend, pl->cap - 1, s);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess && rows > 0) {
    hipLaunchKernelGGL(k_rp_count, dim3((unsigned)ceil_div(max_ns, 256), (unsigned)n_prob), dim3(256), 0, s,
                       pl->d_probs, d_src, plan_table(pl), pl->cell, pl->r2, k_max, pl->d_cnt_full, cnt.p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    size_t tmp_bytes = 0;
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt.p, d_row_ptr, (int)(rows + 1), s);
    PoolBuf<char> tmp(tmp_bytes);
    if (e == hipSuccess && !tmp.p) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, cnt.p, d_row_ptr, (int)(rows + 1), s);
  }
  if (e != hipSuccess) {
    plan_release(pl);
    set_error("cs_radius_pairs: %s", hipGetErrorString(e));
    return CS_ERR_HIP;
  }
  *plan = pl;
  return CS_OK;
}

int cs_radius_pairs_fill(const cs_radius_plan* plan, const int64_t* d_row_ptr, int32_t* d_tgt_idx, void* stream) {
  CS_REQUIRE(plan && d_row_ptr, CS_ERR_INVALID, "cs_radius_pairs_fill: NULL argument");
  if (plan->rows == 0) return CS_OK;
  CS_REQUIRE(d_tgt_idx, CS_ERR_INVALID, "cs_radius_pairs_fill: NULL output");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  hipLaunchKernelGGL(k_rp_fill, dim3((unsigned)ceil_div(plan->max_ns, 64), (unsigned)plan->n_prob), dim3(64), 0, s,
                     plan->d_probs, plan->d_src, plan_table(plan), plan->cell, plan->r2, plan->d_cnt_full, d_row_ptr,
                     d_tgt_idx);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

void cs_radius_plan_free(cs_radius_plan* plan) { plan_release(plan); }

int cs_sample_pairs(const float* d_xyz, const int64_t* h_off, const int32_t* h_base_seg, const int32_t* h_pos_seg,
                    const int32_t* h_neg_seg, const int32_t* h_slot, int n_prob, const int64_t* h_row_base,
                    const int64_t* d_row_ptr, const int32_t* d_tgt_idx, int lists, uint64_t seed, int round,
                    double radius, int sample, int32_t* d_pip, int32_t* d_pin, int32_t* d_nin, int32_t* d_counts,
                    void* stream) {
  CS_REQUIRE(d_xyz && h_off && h_base_seg && h_pos_seg && h_neg_seg && h_slot && h_row_base && d_row_ptr && d_counts,
             CS_ERR_INVALID, "cs_sample_pairs: NULL argument");
  CS_REQUIRE(n_prob >= 1 && n_prob < 65536, CS_ERR_INVALID, "cs_sample_pairs: 1 <= n_prob < 65536");
  CS_REQUIRE(sample >= 1 && sample <= 4096, CS_ERR_UNSUPPORTED, "cs_sample_pairs: 1 <= sample <= 4096");
  CS_REQUIRE(round >= 0 && round < 16, CS_ERR_UNSUPPORTED, "cs_sample_pairs: 0 <= round < 16");
  CS_REQUIRE(lists >= 1 && lists <= 3, CS_ERR_INVALID, "cs_sample_pairs: lists is a mask of 1 (PiP) and 2 (PiN, NiN)");
  CS_REQUIRE(!(lists & 1) || (d_tgt_idx && d_pip), CS_ERR_INVALID, "cs_sample_pairs: PiP needs the filled CSR");
  CS_REQUIRE(!(lists & 2) || (d_pin && d_nin), CS_ERR_INVALID, "cs_sample_pairs: NULL PiN / NiN output");
  std::vector<SPProb> hp(n_prob);
  for (int p = 0; p < n_prob; ++p) {
    SPProb& P = hp[p];
    CS_REQUIRE(h_slot[p] >= 0 && h_slot[p] < (1 << 24), CS_ERR_UNSUPPORTED, "cs_sample_pairs: slot out of range");
    CS_REQUIRE(h_base_seg[p] >= 0 && h_pos_seg[p] >= 0 && h_neg_seg[p] >= 0, CS_ERR_INVALID,
               "cs_sample_pairs: negative segment id");
    P.b0 = h_off[h_base_seg[p]];
    P.nb = h_off[h_base_seg[p] + 1] - P.b0;
    P.q0 = h_off[h_pos_seg[p]];
    P.nq = h_off[h_pos_seg[p] + 1] - P.q0;
    P.g0 = h_off[h_neg_seg[p]];
    P.ng = h_off[h_neg_seg[p] + 1] - P.g0;
    P.row0 = h_row_base[p];
    P.row1 = h_row_base[p + 1];
    P.slot = h_slot[p];
    CS_REQUIRE(P.row1 - P.row0 == P.nb, CS_ERR_INVALID, "cs_sample_pairs: CSR rows of a problem != its base rows");
    CS_REQUIRE(P.nb < (1LL << 31) && P.nq < (1LL << 31) && P.ng < (1LL << 31), CS_ERR_UNSUPPORTED,
               "cs_sample_pairs: segment too large");
  }
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<SPProb> dp(n_prob);
  CS_REQUIRE(dp.p, CS_ERR_HIP, "cs_sample_pairs: scratch allocation failed");
  CS_HIP_CHECK(hipMemcpyAsync(dp.p, hp.data(), sizeof(SPProb) * n_prob, hipMemcpyHostToDevice, s));
  if (lists & 2) {
    hipLaunchKernelGGL(k_sp_negatives, dim3((unsigned)n_prob, 2), dim3(kSpThreads), 0, s, dp.p, d_xyz, d_row_ptr,
                       seed, round, radius * radius, 0.1f, sample, d_pin, d_nin, d_counts);
    CS_LAUNCH_CHECK();
  }
  if (lists & 1) {
    int np2 = 1;
    while (np2 < sample) np2 <<= 1;
    hipLaunchKernelGGL(k_sp_positives, dim3((unsigned)n_prob), dim3(1024), sizeof(uint64_t) * np2, s, dp.p, d_row_ptr,
                       d_tgt_idx, seed, round, sample, d_pip, d_counts);
    CS_LAUNCH_CHECK();
  }
  return CS_OK;
}

int cs_transform_f64(const float* d_xyz, const int64_t* h_off, const int32_t* h_seg, int n_prob, const double* d_T,
                     double* d_out, void* stream) {
  CS_REQUIRE(h_off && h_seg && d_T && d_out && d_xyz, CS_ERR_INVALID, "cs_transform_f64: NULL argument");
  CS_REQUIRE(n_prob >= 1 && n_prob < 65536, CS_ERR_INVALID, "cs_transform_f64: 1 <= n_prob < 65536");
  std::vector<int64_t> desc(3 * (size_t)n_prob);
  int64_t o = 0, max_n = 0;
  for (int p = 0; p < n_prob; ++p) {
    CS_REQUIRE(h_seg[p] >= 0, CS_ERR_INVALID, "cs_transform_f64: negative segment id");
    const int64_t s0 = h_off[h_seg[p]], n = h_off[h_seg[p] + 1] - s0;
    CS_REQUIRE(s0 >= 0 && n >= 0, CS_ERR_INVALID, "cs_transform_f64: bad offsets");
    desc[3 * p] = s0;
    desc[3 * p + 1] = n;
    desc[3 * p + 2] = o;
    o += n;
    if (n > max_n) max_n = n;
  }
  if (max_n == 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<int64_t> dd(desc.size());
  CS_REQUIRE(dd.p, CS_ERR_HIP, "cs_transform_f64: scratch allocation failed");
  CS_HIP_CHECK(hipMemcpyAsync(dd.p, desc.data(), sizeof(int64_t) * desc.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_transform_f64, dim3((unsigned)ceil_div(max_n, 256), (unsigned)n_prob), dim3(256), 0, s, d_xyz,
                     dd.p, d_T, d_out);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
