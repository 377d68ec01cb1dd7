// Descriptor retrieval, exact in f64 so that the returned indices equal those of the reference's SciPy routine:
//   cs_l2_topk / cs_l2_topk_sq / cs_l2_topk_catalog <- scipy cdist + argsort   (utils/retrieval.py:139-177)
// The canonical distance is one f64 fma chain over the feature dimension in ascending order, sum_c (q_c - x_c)^2;
// ties go to the smaller catalog row.  Every returned index / distance is that of the canonical chain:
//   * nq * nx >= 2^24, d = 64 / 128 / 256 / 512, k <= 10, nx >= 64 (default at these sizes): k_topk_f16 shortlists by
//     |x|^2 - 2 q.x on the f16 matrix cores, k_topk_rescore evaluates the shortlist with the canonical chain and ranks
//     it, k_tkf_verify checks it against the shortlist threshold; the queries that fail go through the f64 shortlist.
//     A cs_topk_catalog keeps the catalog's f16 image and norms across calls.
//   * nq * nx >= 2^24, other shapes with k <= 10: k_topk_mfma shortlists on the f64 matrix pipe, k_topk_rescore ranks.
//   * everything else: k_dist_matrix + k_row_topk, the exact slab path -- what the tests hold the other two against.
// CS_TOPK_MFMA forces a path whatever the size ("0" slab, "1" / "64" f64 shortlist, "16" f16 shortlist where the shape
// allows); CS_TOPK_XCD=0 turns off the dealing of the f16 shortlist's work items over the XCDs.
// Non-finite rows (include/corsair_hip.h): a catalog row at NaN or +inf distance is never a neighbour, on any path -- the
// shortlists never admit it (`dist < bd[..]` is false, fminf drops a NaN), the slab path leaves it a placeholder when it
// loads the distance (k_row_topk), and a list that runs out of rows ends in (-1, +inf).  The f16 verification hands a
// query or a catalog outside its range (|q|^2 >= 1e8, max |x|^2 >= 4e8, not finite; a NaN row does not enter the
// maximum) to the f64 shortlist.
// k_row_norms lives here, behind row_norms() (nn_common.h).
#include <algorithm>


#include "nn_common.h"

namespace cs {

// ------------------------------------------------------------------------------------------
// descriptor distance matrix + row top-k
// ------------------------------------------------------------------------------------------
constexpr int DM_QT = 16;   // queries per block
constexpr int DM_CT = 64;   // catalog rows per block
constexpr int DM_DC = 64;   // feature chunk staged in LDS

// D2[q, x] = sum_c (q_c - x_c)^2 in f64, c ascending.  thread = (catalog row j, query group g of 4).
__global__ __launch_bounds__(256) void k_dist_matrix(const float* __restrict__ Q, int64_t nq,
                                                     const float* __restrict__ X, int64_t nx,
                                                     int d, int64_t x_begin, int64_t x_count,
                                                     double* __restrict__ D2) {
  __shared__ float q_lds[DM_QT * DM_DC];
  __shared__ float x_lds[DM_DC * (DM_CT + 1)];
  const int tid = threadIdx.x;
  const int j = tid & 63;
  const int g = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.y * DM_QT;
  const int64_t xl0 = (int64_t)blockIdx.x * DM_CT;  // local to the slab
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < d; c0 += DM_DC) {
    const int dc = min(DM_DC, d - c0);
    __syncthreads();
    for (int i = tid; i < DM_QT * DM_DC; i += 256) {
      int r = i / DM_DC, c = i - r * DM_DC;
      float v = 0.f;
      if (q0 + r < nq && c < dc) v = Q[(q0 + r) * d + c0 + c];
      q_lds[i] = v;
    }
    for (int i = tid; i < DM_CT * DM_DC; i += 256) {
      int r = i / DM_DC, c = i - r * DM_DC;
      float v = 0.f;
      if (xl0 + r < x_count && c < dc) v = X[(x_begin + xl0 + r) * d + c0 + c];
      x_lds[c * (DM_CT + 1) + r] = v;
    }
    __syncthreads();
    for (int c = 0; c < dc; ++c) {
      double xv = (double)x_lds[c * (DM_CT + 1) + j];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        double diff = (double)q_lds[(g * 4 + u) * DM_DC + c] - xv;
        acc[u] = fma(diff, diff, acc[u]);
      }
    }
  }
  if (xl0 + j < x_count) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int64_t qi = q0 + g * 4 + u;
      if (qi < nq) D2[qi * x_count + xl0 + j] = acc[u];
    }
  }
}

constexpr int TK_CAP = 2048;  // LDS sort capacity (entries)

__device__ __forceinline__ bool key_less(unsigned long long da, int ia, unsigned long long db,
                                         int ib) {
  return da < db || (da == db && ia < ib);
}

// Bitonic sort of the n (a power of two) keys (sd[i], si[i]) in LDS, ascending by key_less, by the 256 threads of the
// workgroup.  The keys are visible to the workgroup before the call (a barrier) and sorted for all of it after.
__device__ __forceinline__ void bitonic_sort_keys(unsigned long long* sd, int* si, int n, int tid) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < n / 2; t += 256) {
        const int lo = (t / stride) * stride * 2 + (t % stride);
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const unsigned long long dl = sd[lo], dh = sd[hi];
        const int il = si[lo], ih = si[hi];
        const bool swap = up ? key_less(dh, ih, dl, il) : key_less(dl, il, dh, ih);
        if (swap) {
          sd[lo] = dh;
          si[lo] = ih;
          sd[hi] = dl;
          si[hi] = il;
        }
      }
      __syncthreads();
    }
  }
}

// One block per query: merge the carried top-k with a slab of squared distances by a bitonic sort
// of (distance bits, index) in LDS.  carry_* hold k entries per query (distance = +inf when unset).
__global__ __launch_bounds__(256) void k_row_topk(const double* __restrict__ D2, int64_t x_count,
                                                  int64_t x_begin, int k,
                                                  unsigned long long* carry_d, int* carry_i) {
  __shared__ unsigned long long sd[TK_CAP];
  __shared__ int si[TK_CAP];
  const int tid = threadIdx.x;
  const int64_t qi = blockIdx.x;
  const unsigned long long INF_BITS = 0x7ff0000000000000ULL;
  for (int64_t base = 0; base < x_count; base += TK_CAP - k) {
    const int cnt = (int)min((int64_t)(TK_CAP - k), x_count - base);
    __syncthreads();
    for (int i = tid; i < TK_CAP; i += 256) {
      unsigned long long dv = INF_BITS;
      int iv = 0x7fffffff;
      if (i < k) {
        dv = carry_d[qi * k + i];
        iv = carry_i[qi * k + i];
      } else if (i - k < cnt) {
        // a NaN or +inf distance is never a neighbour: the row stays a placeholder, as on the shortlist paths (whose
        // `dist < bd[..]` tests are false for it) -- with its real index an infinite row sorted before the placeholders
        const double d2 = D2[qi * x_count + base + (i - k)];
        if (d2 < INFINITY) {
          dv = (unsigned long long)__double_as_longlong(d2);
          iv = (int)(x_begin + base + (i - k));
        }
      }
      sd[i] = dv;
      si[i] = iv;
    }
    __syncthreads();
    bitonic_sort_keys(sd, si, TK_CAP, tid);
    for (int i = tid; i < k; i += 256) {
      carry_d[qi * k + i] = sd[i];
      carry_i[qi * k + i] = si[i];
    }
  }
}

__global__ void k_topk_init(unsigned long long* carry_d, int* carry_i, int64_t n) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t < n) {
    carry_d[t] = 0x7ff0000000000000ULL;
    carry_i[t] = 0x7fffffff;
  }
}
// squared: write the squared distances the ranking was made on (cs_l2_topk_sq: shard merges compare exactly
// what the kernels compared; two different squares can share one rounded square root)
// (an explicit argument of every internal top-k function: no side channel between the entry points)
__global__ void k_topk_finish(const unsigned long long* carry_d, const int* carry_i, int64_t n,
                              int64_t* idx, double* dist, int squared) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t < n) {
    int i = carry_i[t];
    idx[t] = i == 0x7fffffff ? -1 : (int64_t)i;
    const double d2 = __longlong_as_double((long long)carry_d[t]);
    if (dist) dist[t] = squared ? d2 : sqrt(d2);
  }
}

// ------------------------------------------------------------------------------------------
// Large-scale descriptor top-k (BASELINE config C5: 10^6 x 10^6 x 256-d, top-10) on the f64 matrix
// pipe.  d^2 = |q|^2 + |x|^2 - 2 q.x with the dot products on v_mfma_f64_16x16x4_f64 (absolute error
// ~1e-15 for unit descriptors) is used ONLY to shortlist: every lane keeps the TKM_KK best rows of
// the catalog rows it sees for its query; the shortlist (k + margin per lane) is then re-scored with
// the canonical chain sum_c (q_c - x_c)^2 and ranked by (distance, index), so the returned ids and
// distances are those of the exact kernel unless more than `margin` catalog rows tie with the k-th
// neighbour to within ~2e-15 -- the same caveat cdist itself has.
// ------------------------------------------------------------------------------------------
constexpr int TKM_QT = 64;     // queries per block (16 per wave)
constexpr int TKM_XT = 64;     // catalog rows per tile
constexpr int TKM_DC = 64;     // feature chunk in LDS
constexpr int TKM_PITCH = TKM_DC + 2;  // doubles; 2*(pitch) = 4 mod 64 banks: conflict-free b64 reads
constexpr int TKM_KK = 12;     // shortlist per lane (k <= TKM_KK - 2)

__global__ void k_row_norms(const float* __restrict__ X, int64_t n, int d, double* __restrict__ out) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int c = 0; c < d; ++c) {
    const double v = (double)X[i * d + c];
    s = fma(v, v, s);
  }
  out[i] = s;
}

// grid: x = query tile, y = catalog split.  cand_*: [nq][nsplit*4][TKM_KK]
__global__ __launch_bounds__(256) void k_topk_mfma(const float* __restrict__ Q, int64_t nq,
                                                   const float* __restrict__ X, int64_t nx, int d,
                                                   const double* __restrict__ qn,
                                                   const double* __restrict__ xn, int nsplit,
                                                   double* __restrict__ cand_d,
                                                   int* __restrict__ cand_i) {
  __shared__ double q_lds[TKM_QT * TKM_PITCH];
  __shared__ double x_lds[TKM_XT * TKM_PITCH];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 15;   // query within the wave's 16, and catalog row within an MFMA tile (A side)
  const int kq = lane >> 4;    // k slot of the operands, and row group of the results
  const int64_t q0 = (int64_t)blockIdx.x * TKM_QT;
  const int64_t per = ((nx + nsplit - 1) / nsplit + TKM_XT - 1) / TKM_XT * TKM_XT;
  const int64_t xb = (int64_t)blockIdx.y * per;
  const int64_t xe = min(nx, xb + per);
  const int64_t my_q = q0 + wave * 16 + col;
  const double my_qn = my_q < nq ? qn[my_q] : 0.0;

  double bd[TKM_KK];
  int bi[TKM_KK];
#pragma unroll
  for (int j = 0; j < TKM_KK; ++j) {
    bd[j] = INFINITY;
    bi[j] = 0x7fffffff;
  }

  for (int64_t x0 = xb; x0 < xe; x0 += TKM_XT) {
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < d; c0 += TKM_DC) {
      const int dc = min(TKM_DC, d - c0);
      __syncthreads();
      for (int i = tid; i < TKM_QT * TKM_DC; i += 256) {
        const int r = i / TKM_DC, c = i - r * TKM_DC;
        double v = 0.0;
        if (q0 + r < nq && c < dc) v = (double)Q[(q0 + r) * d + c0 + c];
        q_lds[r * TKM_PITCH + c] = v;
      }
      for (int i = tid; i < TKM_XT * TKM_DC; i += 256) {
        const int r = i / TKM_DC, c = i - r * TKM_DC;
        double v = 0.0;
        if (x0 + r < xe && c < dc) v = (double)X[(x0 + r) * d + c0 + c];
        x_lds[r * TKM_PITCH + c] = v;
      }
      __syncthreads();
      const double* qp = q_lds + (wave * 16 + col) * TKM_PITCH + kq;
      const double* xp = x_lds + col * TKM_PITCH + kq;
#pragma unroll 4
      for (int k4 = 0; k4 < TKM_DC; k4 += 4) {
        const double b = qp[k4];                       // B[k][query]
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double a = xp[t * 16 * TKM_PITCH + k4];  // A[catalog row][k]
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
        }
      }
    }
    // results: acc[t][r] = dot(catalog row x0 + 16 t + kq + 4 r, query my_q)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = x0 + 16 * t + kq + 4 * r;
        double dist = INFINITY;
        if (row < xe) dist = fma(-2.0, acc[t][r], my_qn + xn[row]);
        if (dist < bd[TKM_KK - 1]) {
          // (knf_insert's loop in f64, on purpose: with knf_insert generic over the value type this kernel grew from 3256 to 5511 instructions)
          double cd = dist;
          int ci = (int)row;
          bool carry = false;
#pragma unroll
          for (int s2 = 0; s2 < TKM_KK; ++s2) {
            if (carry || cd < bd[s2]) {
              carry = true;
              const double td = bd[s2];
              const int ti = bi[s2];
              bd[s2] = cd;
              bi[s2] = ci;
              cd = td;
              ci = ti;
            }
          }
        }
      }
    }
  }
  if (my_q < nq) {
    const int64_t base = (my_q * (nsplit * 4) + blockIdx.y * 4 + kq) * TKM_KK;
#pragma unroll
    for (int j = 0; j < TKM_KK; ++j) {
      cand_d[base + j] = bd[j];
      cand_i[base + j] = bi[j];
    }
  }
}

// Re-score the shortlist of one query with the canonical chain and keep the k best (dist, idx).
// One workgroup per query, one THREAD per candidate (the f64 chain of a candidate is sequential in the feature index:
// that order is the parity contract), 256 candidates at a time.  Round 5: the candidates' rows come through LDS in
// chunks of TKR_CH features -- 32 consecutive lanes copy one row's 128-byte piece, so a wave's load touches two cache
// lines, and every thread then walks ITS row in LDS (pitch TKR_CH + 1: conflict-free) -- and the ranking sorts the next
// power of two above the candidate count.  Before, every thread read its own row from global memory (64 cache lines per
// wave-load, 256 loads per thread) and the bitonic network always ran over TKM_MERGE_CAP = 1 024 slots: 2.97 ms per
// 10 240 x 144 candidates of 256-d, as much as a fifth of the shortlist kernel it follows.
constexpr int TKM_MERGE_CAP = 1024;
constexpr int TKR_CH = 32;
__global__ __launch_bounds__(256) void k_topk_rescore(const float* __restrict__ Q,
                                                      const float* __restrict__ X, int d,
                                                      const int* __restrict__ cand_i, int ncand,
                                                      int k, unsigned long long* carry_d,
                                                      int* carry_i) {
  __shared__ unsigned long long sd[TKM_MERGE_CAP];
  __shared__ int si[TKM_MERGE_CAP];
  __shared__ float rows[256][TKR_CH + 1];
  __shared__ float qs[TKR_CH];
  __shared__ int srow[256];
  const int tid = threadIdx.x;
  const int64_t qi = blockIdx.x;
  const unsigned long long INF_BITS = 0x7ff0000000000000ULL;
  int P = 2;
  while (P < ncand || P < k) P <<= 1;
  if (P > TKM_MERGE_CAP) P = TKM_MERGE_CAP;   // (the callers keep ncand <= TKM_MERGE_CAP)
  for (int gb = 0; gb < P; gb += 256) {
    const int i = gb + tid;
    const int row = i < ncand ? cand_i[qi * ncand + i] : 0x7fffffff;
    __syncthreads();   // the previous group has finished reading rows / srow
    srow[tid] = row;
    double acc = 0.0;
    const int n_rows = min(256, ncand - gb);   // candidates of this group (block-uniform, may be <= 0)
    for (int c0 = 0; c0 < d && n_rows > 0; c0 += TKR_CH) {
      const int cl = min(TKR_CH, d - c0);
      __syncthreads();   // srow visible; the previous chunk has been consumed
      {
        // thread (r0, c) copies column c of the rows r0, r0 + 8, ...: all of its loads are issued before the first one is
        // waited for (unconditional, clamped addresses -- a load under a condition is waited for at once)
        static_assert(TKR_CH == 32, "one 32-lane half-wave per row piece");
        const int c = tid & 31, r0 = tid >> 5;
        const int cc = c0 + (c < cl ? c : 0);
        float v[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          const int rr = srow[r0 + 8 * j];
          v[j] = X[(int64_t)(rr != 0x7fffffff ? rr : 0) * d + cc];
        }
#pragma unroll
        for (int j = 0; j < 32; ++j) rows[r0 + 8 * j][c] = v[j];
      }
      if (tid < cl) qs[tid] = Q[qi * d + c0 + tid];
      __syncthreads();
      if (row != 0x7fffffff) {
        for (int c = 0; c < cl; ++c) {
          const double diff = (double)qs[c] - (double)rows[tid][c];
          acc = fma(diff, diff, acc);
        }
      }
    }
    if (i < TKM_MERGE_CAP) {
      // (a shortlisted row has a finite ranking value, hence finite elements; the test keeps the rule "NaN / +inf is
      // never a neighbour" in this kernel's own terms)
      const bool have = row != 0x7fffffff && acc < INFINITY;
      sd[i] = have ? (unsigned long long)__double_as_longlong(acc) : INF_BITS;
      si[i] = have ? row : 0x7fffffff;
    }
  }
  __syncthreads();
  bitonic_sort_keys(sd, si, P, tid);
  for (int i = tid; i < k; i += 256) {
    carry_d[qi * k + i] = sd[i];
    carry_i[qi * k + i] = si[i];
  }
}


// ------------------------------------------------------------------------------------------
// The same shortlist on the f16 matrix cores (d = 64 / 128 / 256 / 512, k <= 10): 16x the f64 matrix rate.
// s~ = |x|^2 - 2 q.x with x = x_hi + x_lo and v = -2 q = v_hi + v_lo split into f16 (the lo * lo
// products are dropped): 3 v_mfma_f32_32x32x16_f16 per 16 features of a 32 x 32 (catalog x query) tile,
// accumulator preloaded with |x|^2.  Queries live in registers (32 per wave, 8 waves per workgroup:
// 256 queries reuse every staged catalog row), the catalog streams through LDS as a padded f16 image
// (row = [hi(16) | lo(16)] per 16 features + 16 B: odd 16-B slot pitch, conflict-free ds_read_b128),
// 64 rows per stage, copied by LDS-DMA one stage ahead.  A lane keeps the TKF_KK best rows of its half
// of the tile rows.  Exactness: the shortlist is re-scored with the canonical f64 chain (k_topk_rescore)
// and VERIFIED -- every row outside the shortlist has s~ >= tau (the smallest of the lanes' TKF_KK-th
// values), hence exact s >= tau - eps with eps = (3 d + 4) 2^-22 (|q|^2 + max |x|^2) bounding the f16
// pipeline error (split residuals 3 * 2^-21 |q||x|, 3 d + 1 f32 accumulations of partial sums
// <= |x|^2 + 2 |q||x|) plus an ABSOLUTE term 2^-24 sqrt(d) (2|q| + max|x|) for elements whose hi or lo part
// is an f16 subnormal (spacing 2^-24 whatever the magnitude: descriptors with norms << 1);
// queries whose exact k-th value is not below that go through the f64 path.
// d = 512 (TERMS = 2): the 32 queries of a wave would need 256 VGPRs for hi + lo operands, so only v_hi is
// kept in registers (128 VGPRs) and the x_hi v_lo term is dropped as well -- 2 MFMAs per 16 features, and
// eps grows by its bound 1.001 * 2^-10 |q| max|x| (about 1e-3 for unit descriptors, against a gap of ~0.1
// between the k-th neighbour and the shortlist threshold on the C5 data); 32-row stages (2 x 64.5 KiB of LDS).
// ------------------------------------------------------------------------------------------
constexpr int TKF_ROWS = 64;   // catalog rows per LDS stage (2 MFMA row tiles); the image is padded to whole 64s
constexpr int TKF_QT = 256;    // queries per workgroup (8 waves x 32)
constexpr int TKF_KK = 12;     // shortlist per lane (two lanes per query and catalog split)
constexpr int TKF_AHEAD = 2;   // MFMA steps by which the LDS reads of the A fragments run ahead

// f16 image of n rows (+ zero rows up to n_pad): per 16 features [hi(16) | lo(16)] of scale * X
__global__ void k_tkf_pack(const float* __restrict__ X, int64_t n, int64_t n_pad, int d, float scale,
                           _Float16* __restrict__ img, int pitch_h) {
  const int dch = d / 16;
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n_pad * dch) return;
  const int64_t row = t / dch;
  const int c = (int)(t - row * dch);
  union {
    _Float16 h[32];
    uint4 v[4];
  } u;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const double v = row < n ? (double)scale * (double)X[row * d + c * 16 + j] : 0.0;
    const _Float16 hi = (_Float16)v;
    u.h[j] = hi;
    u.h[16 + j] = (_Float16)(v - (double)hi);
  }
  uint4* dst = reinterpret_cast<uint4*>(img + row * pitch_h + c * 32);
#pragma unroll
  for (int j = 0; j < 4; ++j) dst[j] = u.v[j];
  if (c == 0 && pitch_h > dch * 32) {  // the 16-B pad of a catalog row (never read by the MFMA fragments; keep it defined)
    uint4* pad = reinterpret_cast<uint4*>(img + row * pitch_h + dch * 32);
    *pad = make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ void k_max_bits(const double* __restrict__ v, int64_t n, unsigned* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  knf_seg_max(i < n ? __double2float_ru(v[i]) : 0.f, out);
}

// work item = (catalog split, query tile of TKF_QT); 512 threads; dynamic LDS: 2 stages + 2 x TKF_ROWS floats.
// cand_i: [nq][nsplit * 2][TKF_KK], tau: [nq][nsplit * 2]
template <int DCH, int TERMS, int ROWS>
__global__ __launch_bounds__(512) void k_topk_f16(const _Float16* __restrict__ qimg, int64_t nq,
                                                  const _Float16* __restrict__ ximg, int64_t nx,
                                                  const double* __restrict__ xn, int nsplit, int qtiles, int xcd_deal,
                                                  int* __restrict__ cand_i, float* __restrict__ tau) {
  // 1-D grid of 8 * ceil(qtiles * nsplit / 8) workgroups.  The hardware deals workgroup b to XCD b % 8: the work items
  // (catalog split, query tile) -- query tile fastest -- are cut into 8 contiguous runs, one per XCD, so that the
  // workgroups that share an XCD's 4-MiB L2 stream the SAME catalog split at about the same pace (each split's image
  // is then read from HBM / Infinity Cache about once per XCD that works on it instead of once per workgroup: at
  // 10 240 x 10^6 x 256-d, 40 query tiles x 6 splits, a workgroup needs 10.6 B per cycle at the full matrix rate, 6 TB/s
  // over the chip).  xcd_deal = 0 (CS_TOPK_XCD=0): item = workgroup id, the mapping of rounds 2-4.
  const int n_items = qtiles * nsplit;
  const int per_xcd = (n_items + 7) / 8;
  const int item = xcd_deal ? (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  if (item >= n_items) return;
  const int split = item / qtiles;
  const int qtile = item - split * qtiles;
  constexpr int PITCH_B = DCH * 64 + 16;              // bytes per image row
  constexpr int STAGE_BYTES = ROWS * PITCH_B;         // whole KiB for DCH = 4, 8, 16; 64.5 KiB for DCH = 32
  constexpr int STAGE_PIECES = (STAGE_BYTES + 1023) / 1024;   // 1-KiB LDS-DMA instructions (the last may be partial)
  constexpr int STAGE_PITCH = STAGE_PIECES * 1024;
  constexpr int NT = ROWS / 32;                       // MFMA row tiles per stage
  static_assert(STAGE_BYTES % 16 == 0 && ROWS % 32 == 0 && TKF_ROWS % ROWS == 0, "stage shape");
  extern __shared__ __attribute__((aligned(1024))) char lds[];
  float* tn_s = reinterpret_cast<float*>(lds + 2 * STAGE_PITCH);  // [2][ROWS]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int col = lane & 31;
  const int64_t my_q = (int64_t)qtile * TKF_QT + wave * 32 + col;
  const int64_t per = ((nx + nsplit - 1) / nsplit + TKF_ROWS - 1) / TKF_ROWS * TKF_ROWS;
  const int64_t xb = (int64_t)split * per;
  const int64_t xe = min(nx, xb + per);
  // B operands of the wave's 32 queries: lane supplies k = 8 half .. +8 of every 16-feature chunk
  f16x8 qh[DCH], ql[TERMS == 3 ? DCH : 1];
  {
    const _Float16* qrow = qimg + (my_q < nq ? my_q : 0) * (int64_t)(DCH * 32) + 8 * half;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      qh[c] = *reinterpret_cast<const f16x8*>(qrow + c * 32);
      if (TERMS == 3) ql[c] = *reinterpret_cast<const f16x8*>(qrow + c * 32 + 16);
    }
  }
  float bd[TKF_KK];
  int bi[TKF_KK];
#pragma unroll
  for (int j = 0; j < TKF_KK; ++j) {
    bd[j] = INFINITY;
    bi[j] = 0x7fffffff;
  }
  const char* gimg = reinterpret_cast<const char*>(ximg) + lane * 16;
  // A stage = the catalog image (LDS-DMA, written as inline asm: behind the builtin form hipcc waits vmcnt(0)
  // in front of the first ds_read that follows, i.e. for the stage it has just issued "one ahead" -- lds_dma16,
  // common.h) + the |x|^2 of its rows (a plain load, issued BEFORE the DMAs and stored to LDS AFTER the current
  // stage is computed: hipcc's wait for it is then the only wait in the loop body and the DMAs have landed by then).
  const unsigned lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(lds));
  auto issue_dma = [&](int b, int64_t base) {
    const char* gp = gimg + base * PITCH_B;
#pragma unroll
    for (int i = 0; i < (STAGE_PIECES + 7) / 8; ++i) {
      const int piece = wave + 8 * i;  // wave-uniform
      // (the last piece of a 64.5-KiB stage is half a KiB: the upper lanes sit it out)
      if (piece < STAGE_PIECES && piece * 1024 + lane * 16 < STAGE_BYTES)
        lds_dma16(gp + piece * 1024, lds_base + b * STAGE_PITCH + piece * 1024);
    }
  };
  auto load_norm = [&](int64_t base) {   // unconditional (clamped) load: a load under a condition is waited for at once
    int64_t r = base + (tid % ROWS);
    if (r > xe - 1) r = xe - 1;
    return (float)xn[r < xb ? xb : r];
  };
  auto store_norm = [&](int b, int64_t base, float v) {
    if (tid < ROWS) tn_s[b * ROWS + tid] = base + tid < xe ? v : INFINITY;
  };
  if (xb < xe) {
    const float v0 = load_norm(xb);
    issue_dma(0, xb);
    store_norm(0, xb, v0);
  }
  int buf = 0;
  for (int64_t base = xb; base < xe; base += ROWS) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool more = base + ROWS < xe;
    const float v_next = load_norm(base + ROWS);
    if (more) issue_dma(buf ^ 1, base + ROWS);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      // accumulator input: |x|^2 of the 16 rows this lane owns: (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const float4 v = *reinterpret_cast<const float4*>(&tn_s[buf * ROWS + t * 32 + 8 * q4 + 4 * half]);
        acc[t][4 * q4 + 0] = v.x; acc[t][4 * q4 + 1] = v.y; acc[t][4 * q4 + 2] = v.z; acc[t][4 * q4 + 3] = v.w;
      }
    }
    const char* st = lds + buf * STAGE_PITCH + col * PITCH_B + half * 16;
    // The A fragments of step i + TKF_AHEAD are requested BEFORE the MFMAs of step i are issued (a ring of register
    // pairs): left to itself hipcc asks for a step's two ds_read_b128 right in front of its MFMAs and waits for them
    // at once -- the whole LDS latency once per 3 MFMAs, with two waves per SIMD the matrix pipe sat at 0.37.
    constexpr int NSTEP = DCH * NT;
    f16x8 rah[TKF_AHEAD + 1], ral[TKF_AHEAD + 1];
    auto fetch = [&](int i) {
      const int c = i / NT, t = i % NT;
      rah[i % (TKF_AHEAD + 1)] = *reinterpret_cast<const f16x8*>(st + t * 32 * PITCH_B + c * 64);
      ral[i % (TKF_AHEAD + 1)] = *reinterpret_cast<const f16x8*>(st + t * 32 * PITCH_B + c * 64 + 32);
    };
#pragma unroll
    for (int i = 0; i < TKF_AHEAD; ++i) fetch(i);
#pragma unroll
    for (int i = 0; i < NSTEP; ++i) {
      if (i + TKF_AHEAD < NSTEP) fetch(i + TKF_AHEAD);
      __builtin_amdgcn_sched_barrier(0);   // keep the request in front of this step's MFMAs
      const int c = i / NT, t = i % NT;
      const f16x8 ah = rah[i % (TKF_AHEAD + 1)], al = ral[i % (TKF_AHEAD + 1)];
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qh[c], acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qh[c], acc[t], 0, 0, 0);
      if (TERMS == 3) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ql[c], acc[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // One test per 32 x 32 tile (v_min3 tree over the lane's 16 results against its KK-th best) instead of one per result:
    // late in the scan a wave finds a candidate in about one tile of four.  The insertion itself is branch-free
    // (one v_med3 per slot for the sorted values, two selects for the rows): written as the usual compare-and-carry loop
    // hipcc copied the whole list at every slot, ~1 000 cycles per event with 2.6 events per wave and stage -- together
    // with the 32 compare-and-branch sequences more than the stage's MFMAs.
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float m = acc[t][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) m = fminf(m, acc[t][r]);
      if (m < bd[TKF_KK - 1]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[t][r];
          if (v < bd[TKF_KK - 1]) {
            const int ci = (int)(base + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half);
            bool lt_cur = true;   // v < bd[KK - 1]
#pragma unroll
            for (int j = TKF_KK - 1; j >= 1; --j) {
              const bool lt_prev = v < bd[j - 1];
              bi[j] = lt_prev ? bi[j - 1] : (lt_cur ? ci : bi[j]);
              bd[j] = __builtin_amdgcn_fmed3f(bd[j - 1], v, bd[j]);
              lt_cur = lt_prev;
            }
            bi[0] = lt_cur ? ci : bi[0];
            bd[0] = fminf(bd[0], v);
          }
        }
      }
    }
    if (more) store_norm(buf ^ 1, base + ROWS, v_next);
    buf ^= 1;
  }
  if (my_q < nq) {
    const int64_t slot = my_q * (nsplit * 2) + split * 2 + half;
#pragma unroll
    for (int j = 0; j < TKF_KK; ++j) cand_i[slot * TKF_KK + j] = bi[j];
    tau[slot] = bd[TKF_KK - 1];
  }
}

template <int DCH, int TERMS, int ROWS>
static int launch_topk_f16(int qtiles, hipStream_t s, const _Float16* qimg, int64_t nq, const _Float16* ximg,
                           int64_t nx, const double* xn, int nsplit, int xcd_deal, int* cand_i, float* tau) {
  constexpr int LDS_BYTES = 2 * ((ROWS * (DCH * 64 + 16) + 1023) / 1024 * 1024) + 2 * ROWS * (int)sizeof(float);
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_topk_f16<DCH, TERMS, ROWS>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  CS_REQUIRE(attr == hipSuccess, CS_ERR_HIP, "cs_l2_topk: cannot reserve %d bytes of LDS", LDS_BYTES);
  const int n_items = qtiles * nsplit;
  const dim3 grid((unsigned)(xcd_deal ? 8 * ((n_items + 7) / 8) : n_items));
  hipLaunchKernelGGL((k_topk_f16<DCH, TERMS, ROWS>), grid, dim3(512), LDS_BYTES, s, qimg, nq, ximg, nx, xn, nsplit,
                     qtiles, xcd_deal, cand_i, tau);
  return CS_OK;
}

// One thread per query: is the re-scored k-th value provably below everything outside the shortlist?
// flagged queries (compact list + count) go through the f64 path.
__global__ void k_tkf_verify(const unsigned long long* __restrict__ carry_d, int k, int64_t nq,
                             const float* __restrict__ tau, int nlane, const double* __restrict__ qn,
                             const unsigned* __restrict__ xmax_bits, int d, int terms,
                             int* __restrict__ flagged, int* __restrict__ n_flagged) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (q >= nq) return;
  float t = INFINITY;
  for (int j = 0; j < nlane; ++j) t = fminf(t, tau[q * nlane + j]);
  const double dk = __longlong_as_double((long long)carry_d[q * k + k - 1]);   // exact k-th squared distance
  const double xm = (double)__uint_as_float(*xmax_bits);   // max |x|^2 (rounded up)
  double eps = (double)(3 * d + 4) * 2.384185791015625e-07 * (qn[q] + xm)                    // relative: 2^-22
               + 5.9604644775390625e-08 * sqrt((double)d) * (2.0 * sqrt(qn[q]) + sqrt(xm));  // absolute: 2^-24
  if (terms < 3) eps += 1.001 * 9.765625e-04 * sqrt(qn[q]) * sqrt(xm);                      // dropped x_hi v_lo: 2^-10 |q||x|
  // f16 range: |x| and |-2 q| below 2e4 keep every hi part (and every product sum) finite; anything larger
  // (or not finite) cannot be trusted and takes the f64 path
  const bool in_range = __uint_as_float(*xmax_bits) < 4.0e8f && qn[q] < 1.0e8;
  const bool ok = in_range && dk - qn[q] < (double)t - eps;   // false for NaN / missing candidates
  if (!ok) flagged[atomicAdd(n_flagged, 1)] = (int)q;
}

__global__ void k_gather_rows(const float* __restrict__ X, int d, const int* __restrict__ rows, int64_t n,
                              float* __restrict__ out) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * d) return;
  const int64_t r = t / d;
  out[t] = X[(int64_t)rows[r] * d + (t - r * d)];
}

__global__ void k_scatter_topk(const int64_t* __restrict__ idx, const double* __restrict__ dist, int k,
                               const int* __restrict__ rows, int64_t n, int64_t* __restrict__ out_idx,
                               double* __restrict__ out_dist) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * k) return;
  const int64_t r = t / k;
  const int64_t o = (int64_t)rows[r] * k + (t - r * k);
  out_idx[o] = idx[t];
  if (out_dist) out_dist[o] = dist[t];
}

}  // namespace cs

using namespace cs;

void cs::row_norms(const float* d_x, int64_t n, int d, double* d_out, hipStream_t s) {
  hipLaunchKernelGGL(k_row_norms, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, d_x, n, d, d_out);
}

// The environment switches of cs_l2_topk / cs_l2_topk_sq / cs_l2_topk_catalog.
struct TopkOptions {
  // CS_TOPK_MFMA: "0" exact slab path, "1" / "64" f64 matrix pipe, "16" f16 matrix cores (where the shape allows),
  // unset: f16 where the shape allows, else f64, for nq * nx >= 2^24
  bool forced, force16, force64;
  bool xcd_deal;  // CS_TOPK_XCD=0: work items of the f16 shortlist in launch order instead of dealt over the XCDs
};
static TopkOptions read_options() {
  const char* force = getenv("CS_TOPK_MFMA");
  TopkOptions o;
  o.forced = force != nullptr;
  o.force16 = force && force[0] == '1' && force[1] == '6';
  o.force64 = force && (force[0] == '1' || force[0] == '6');
  o.xcd_deal = !env_first_is("CS_TOPK_XCD", '0');
  return o;
}

// f64 matrix-pipe shortlist + canonical re-score (k <= TKM_KK - 2)
static int topk_f64_shortlist(const float* d_q, int64_t nq, const float* d_x, int64_t nx, int d, int k,
                              int64_t* d_idx, double* d_dist, hipStream_t s, int squared) {
  int nsplit = (int)(2048 / ceil_div(nq, TKM_QT));
  if (nsplit < 1) nsplit = 1;
  if (nsplit > 64) nsplit = 64;
  while (nsplit > 1 && (nx / nsplit < 4 * TKM_XT || nsplit * 4 * TKM_KK > TKM_MERGE_CAP)) --nsplit;
  const int ncand = nsplit * 4 * TKM_KK;
  PoolBuf<double> qn(nq), xn(nx), cand_d((size_t)nq * ncand);
  PoolBuf<int> cand_i((size_t)nq * ncand);
  PoolBuf<unsigned long long> cd((size_t)nq * k);
  PoolBuf<int> ci((size_t)nq * k);
  CS_REQUIRE(qn.p && xn.p && cand_d.p && cand_i.p && cd.p && ci.p, CS_ERR_HIP,
             "cs_l2_topk: scratch allocation failed");
  row_norms(d_q, nq, d, qn.p, s);
  row_norms(d_x, nx, d, xn.p, s);
  hipLaunchKernelGGL(k_topk_mfma, dim3((unsigned)ceil_div(nq, TKM_QT), (unsigned)nsplit), dim3(256), 0,
                     s, d_q, nq, d_x, nx, d, qn.p, xn.p, nsplit, cand_d.p, cand_i.p);
  hipLaunchKernelGGL(k_topk_rescore, dim3((unsigned)nq), dim3(256), 0, s, d_q, d_x, d, cand_i.p, ncand,
                     k, cd.p, ci.p);
  hipLaunchKernelGGL(k_topk_finish, dim3((unsigned)ceil_div(nq * k, 256)), dim3(256), 0, s, cd.p,
                     ci.p, nq * k, d_idx, d_dist, squared);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// {queries through the f16 shortlist, of those recomputed by the f64 path}
static std::atomic<unsigned long long> g_topk_stats[2];

// What topk_f16_shortlist makes of the catalog before it looks at a query: the padded f16 hi / lo image, the f64 row
// norms and the bit pattern of their maximum.  A cs_topk_catalog keeps them across calls.
struct TkfCatalog {
  _Float16* ximg = nullptr;
  double* xn = nullptr;
  unsigned* xmax = nullptr;
};
static int tkf_pitch(int d) { return (d / 16) * 32 + 8; }   // halfs per catalog image row (16 B of padding)
static int64_t tkf_rows_padded(int64_t nx) { return ceil_div(nx, TKF_ROWS) * TKF_ROWS; }
static bool tkf_shape(int d, int64_t nx) { return (d == 64 || d == 128 || d == 256 || d == 512) && nx >= TKF_ROWS; }
static int tkf_prepare_catalog(const float* d_x, int64_t nx, int d, const TkfCatalog& cat, hipStream_t s) {
  const int dch = d / 16;
  const int64_t n_pad = tkf_rows_padded(nx);
  CS_HIP_CHECK(hipMemsetAsync(cat.xmax, 0, sizeof(unsigned), s));
  row_norms(d_x, nx, d, cat.xn, s);
  hipLaunchKernelGGL(k_max_bits, dim3((unsigned)ceil_div(nx, 256)), dim3(256), 0, s, cat.xn, nx, cat.xmax);
  hipLaunchKernelGGL(k_tkf_pack, dim3((unsigned)ceil_div(n_pad * dch, 256)), dim3(256), 0, s, d_x, nx, n_pad, d, 1.0f,
                     cat.ximg, tkf_pitch(d));
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// Workgroup slots of one round of k_topk_f16.  d >= 256 leaves room for ONE workgroup per CU (2 x 65 KiB of LDS
// stages): 256 slots, filled without a partial second round (every split adds 24 candidates per query to the exact
// re-score: 10 240 x 10^6 x 256-d went from 30 to 22.5 ms with 6 splits instead of 13); the smaller images fit two
// per CU.
static int tkf_wg_slots(int d) { return d >= 256 ? 256 : 512; }

// f16 matrix-core shortlist (d = 64 / 128 / 256 / 512, k <= 10), canonical re-score, verification, f64 path for
// the queries that fail it.  Waits for the stream once (the number of such queries).  `prepared`: the catalog image
// of a handle, made for exactly (d_x, nx, d); nullptr: the catalog is prepared for this call only.
static int topk_f16_shortlist(const float* d_q, int64_t nq, const float* d_x, int64_t nx, int d, int k,
                              int64_t* d_idx, double* d_dist, hipStream_t s, int squared, bool xcd_deal,
                              const TkfCatalog* prepared) {
  const int dch = d / 16;
  const int64_t qtiles = ceil_div(nq, TKF_QT);
  // catalog splits: one full round of workgroups
  int nsplit = (int)(tkf_wg_slots(d) / qtiles);   // (rounded DOWN: one workgroup more than slots costs a whole second round)
  if (nsplit < 2) nsplit = 2;   // (10^6 x 10^6: two half-catalog rounds measured 8 % faster than one full one)
  if (nsplit > 32) nsplit = 32;
  while (nsplit > 1 && nx / nsplit < 8 * TKF_ROWS) --nsplit;
  if (nsplit < 1) nsplit = 1;
  const int nlane = nsplit * 2;
  const int ncand = nlane * TKF_KK;  // <= 768 <= TKM_MERGE_CAP
  PoolBuf<_Float16> qimg((size_t)nq * dch * 32), ximg_own;
  PoolBuf<double> qn(nq), xn_own;
  PoolBuf<unsigned> xmax_own;
  PoolBuf<int> cand_i((size_t)nq * ncand), ci((size_t)nq * k), flagged((size_t)nq + 1);
  PoolBuf<float> tau((size_t)nq * nlane);
  PoolBuf<unsigned long long> cd((size_t)nq * k);
  TkfCatalog cat;
  if (prepared) {
    cat = *prepared;
  } else {
    CS_REQUIRE(ximg_own.alloc((size_t)tkf_rows_padded(nx) * tkf_pitch(d)) && xn_own.alloc((size_t)nx) && xmax_own.alloc(1),
               CS_ERR_HIP, "cs_l2_topk: scratch allocation failed");
    cat = {ximg_own.p, xn_own.p, xmax_own.p};
    const int rc0 = tkf_prepare_catalog(d_x, nx, d, cat, s);
    if (rc0) return rc0;
  }
  CS_REQUIRE(qimg.p && qn.p && cand_i.p && ci.p && flagged.p && tau.p && cd.p,
             CS_ERR_HIP, "cs_l2_topk: scratch allocation failed");
  int* const n_flagged = flagged.p + nq;
  CS_HIP_CHECK(hipMemsetAsync(n_flagged, 0, sizeof(int), s));
  row_norms(d_q, nq, d, qn.p, s);
  hipLaunchKernelGGL(k_tkf_pack, dim3((unsigned)ceil_div(nq * dch, 256)), dim3(256), 0, s, d_q, nq, nq, d,
                     -2.0f, qimg.p, dch * 32);
  const int terms = dch == 32 ? 2 : 3;
  int rc = dch == 32   ? launch_topk_f16<32, 2, 32>((int)qtiles, s, qimg.p, nq, cat.ximg, nx, cat.xn, nsplit, xcd_deal, cand_i.p, tau.p)
           : dch == 16 ? launch_topk_f16<16, 3, 64>((int)qtiles, s, qimg.p, nq, cat.ximg, nx, cat.xn, nsplit, xcd_deal, cand_i.p, tau.p)
           : dch == 8  ? launch_topk_f16<8, 3, 64>((int)qtiles, s, qimg.p, nq, cat.ximg, nx, cat.xn, nsplit, xcd_deal, cand_i.p, tau.p)
                       : launch_topk_f16<4, 3, 64>((int)qtiles, s, qimg.p, nq, cat.ximg, nx, cat.xn, nsplit, xcd_deal, cand_i.p, tau.p);
  if (rc) return rc;
  hipLaunchKernelGGL(k_topk_rescore, dim3((unsigned)nq), dim3(256), 0, s, d_q, d_x, d, cand_i.p, ncand, k,
                     cd.p, ci.p);
  hipLaunchKernelGGL(k_tkf_verify, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, s, cd.p, k, nq, tau.p,
                     nlane, qn.p, cat.xmax, d, terms, flagged.p, n_flagged);
  hipLaunchKernelGGL(k_topk_finish, dim3((unsigned)ceil_div(nq * k, 256)), dim3(256), 0, s, cd.p, ci.p,
                     nq * k, d_idx, d_dist, squared);
  CS_LAUNCH_CHECK();
  int h_flagged = 0;
  CS_HIP_CHECK(download_async(&h_flagged, n_flagged, sizeof(int), s));
  CS_HIP_CHECK(download_sync(s));
  g_topk_stats[0] += (unsigned long long)nq;
  g_topk_stats[1] += (unsigned long long)h_flagged;
  if (h_flagged > 0) {
    const int64_t nf = h_flagged;
    PoolBuf<float> qf((size_t)nf * d);
    PoolBuf<int64_t> fi((size_t)nf * k);
    PoolBuf<double> fd((size_t)nf * k);
    CS_REQUIRE(qf.p && fi.p && fd.p, CS_ERR_HIP, "cs_l2_topk: scratch allocation failed");
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)ceil_div(nf * d, 256)), dim3(256), 0, s, d_q, d, flagged.p,
                       nf, qf.p);
    rc = topk_f64_shortlist(qf.p, nf, d_x, nx, d, k, fi.p, fd.p, s, squared);
    if (rc) return rc;
    hipLaunchKernelGGL(k_scatter_topk, dim3((unsigned)ceil_div(nf * k, 256)), dim3(256), 0, s, fi.p, fd.p, k,
                       flagged.p, nf, d_idx, d_dist);
    CS_LAUNCH_CHECK();
  }
  return CS_OK;
}

// Exact slab path: f64 distance matrix of a slab of catalog rows (k_dist_matrix), row top-k carried from slab to
// slab (k_row_topk).  Any d, k <= 1024.
static int topk_exact(const float* d_q, int64_t nq, const float* d_x, int64_t nx, int d, int k, int64_t* d_idx,
                      double* d_dist, hipStream_t s, int squared) {
  // slab of catalog rows so that the f64 distance slab stays <= 1 GiB
  int64_t slab = (1LL << 27) / (nq > 0 ? nq : 1);
  if (slab < DM_CT) slab = DM_CT;
  if (slab > nx) slab = nx;
  PoolBuf<double> D2((size_t)nq * slab);
  PoolBuf<unsigned long long> cd((size_t)nq * k);
  PoolBuf<int> ci((size_t)nq * k);
  CS_REQUIRE(D2.p && cd.p && ci.p, CS_ERR_HIP, "cs_l2_topk: scratch allocation failed");
  hipLaunchKernelGGL(k_topk_init, dim3((unsigned)ceil_div(nq * k, 256)), dim3(256), 0, s, cd.p,
                     ci.p, nq * k);
  for (int64_t xb = 0; xb < nx; xb += slab) {
    int64_t xc = nx - xb < slab ? nx - xb : slab;
    dim3 grid((unsigned)ceil_div(xc, DM_CT), (unsigned)ceil_div(nq, DM_QT));
    hipLaunchKernelGGL(k_dist_matrix, grid, dim3(256), 0, s, d_q, nq, d_x, nx, d, xb, xc, D2.p);
    hipLaunchKernelGGL(k_row_topk, dim3((unsigned)nq), dim3(256), 0, s, D2.p, xc, xb, k, cd.p,
                       ci.p);
  }
  hipLaunchKernelGGL(k_topk_finish, dim3((unsigned)ceil_div(nq * k, 256)), dim3(256), 0, s, cd.p,
                     ci.p, nq * k, d_idx, d_dist, squared);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// Argument checks and path choice of the three entry points.  Scratch of every path goes back to this thread's
// stream-ordered cache when the call returns; outputs are valid in stream order.
static int l2_topk_impl(const float* d_q, int64_t nq, const float* d_x, int64_t nx, int d, int k, int64_t* d_idx,
                        double* d_dist, void* stream, const TkfCatalog* prepared, int squared) {
  CS_REQUIRE(d_q && d_x && d_idx, CS_ERR_INVALID, "cs_l2_topk: NULL argument");
  CS_REQUIRE(d >= 1 && k >= 1 && k <= 1024 && k <= nx, CS_ERR_INVALID,
             "cs_l2_topk: need 1 <= k <= min(1024, nx) (k %d, nx %lld)", k, (long long)nx);
  CS_REQUIRE(nx < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_l2_topk: catalog too large");
  if (nq == 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  ProfScope prof("topk", s, 2.0 * (double)nq * (double)nx * (double)d);
  // large problems with a short list: shortlist on the matrix cores, exact re-score
  const TopkOptions opt = read_options();
  const bool big = (double)nq * (double)nx >= 16777216.0;
  const bool want16 = opt.forced ? opt.force16 : big;
  const bool want64 = opt.forced ? opt.force64 : big;
  if (want16 && tkf_shape(d, nx) && k <= TKF_KK - 2)
    return topk_f16_shortlist(d_q, nq, d_x, nx, d, k, d_idx, d_dist, s, squared, opt.xcd_deal, prepared);
  if (want64 && k <= TKM_KK - 2) return topk_f64_shortlist(d_q, nq, d_x, nx, d, k, d_idx, d_dist, s, squared);
  return topk_exact(d_q, nq, d_x, nx, d, k, d_idx, d_dist, s, squared);
}

// ---- catalog handle -------------------------------------------------------------------------------------------
// The catalog of a retrieval run is fixed (evaluation.py:264-283 embeds the CAD library once and ranks every scan
// against it); what the f16 path makes of it -- image, norms, their maximum: 4.2 ms per call at 10^6 x 256 -- is made
// once here and reused by every cs_l2_topk_catalog call.  Shapes the f16 path does not take keep only the pointer.
struct cs_topk_catalog {
  const float* d_x = nullptr;
  int64_t nx = 0;
  int d = 0;
  TkfCatalog f16;               // all three set, or none
  hipEvent_t ready = nullptr;   // recorded behind the kernels that make them
};

extern "C" {

void cs_topk_catalog_free(cs_topk_catalog* c) {
  if (!c) return;
  pool_free(c->f16.ximg);
  pool_free(c->f16.xn);
  pool_free(c->f16.xmax);
  if (c->ready) (void)hipEventDestroy(c->ready);
  delete c;
}

int cs_topk_catalog_create(const float* d_x, int64_t nx, int d, void* stream, cs_topk_catalog** out) {
  CS_REQUIRE(d_x && out, CS_ERR_INVALID, "cs_topk_catalog_create: NULL argument");
  *out = nullptr;
  CS_REQUIRE(d >= 1 && nx >= 1 && nx < (1LL << 31), CS_ERR_INVALID, "cs_topk_catalog_create: bad shape (%lld x %d)",
             (long long)nx, d);
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  cs_topk_catalog* c = new cs_topk_catalog();
  c->d_x = d_x;
  c->nx = nx;
  c->d = d;
  if (tkf_shape(d, nx)) {
    TkfCatalog& f = c->f16;
    f.ximg = (_Float16*)pool_alloc((size_t)tkf_rows_padded(nx) * tkf_pitch(d) * sizeof(_Float16));
    f.xn = (double*)pool_alloc((size_t)nx * sizeof(double));
    f.xmax = (unsigned*)pool_alloc(sizeof(unsigned));
    const bool have = f.ximg && f.xn && f.xmax;
    int rc = have ? tkf_prepare_catalog(d_x, nx, d, f, s) : CS_ERR_HIP;
    if (!have) set_error("cs_topk_catalog_create: allocation failed");
    if (rc == CS_OK && (hipEventCreateWithFlags(&c->ready, hipEventDisableTiming) != hipSuccess ||
                        hipEventRecord(c->ready, s) != hipSuccess)) {
      set_error("cs_topk_catalog_create: could not record the ready event");
      rc = CS_ERR_HIP;
    }
    if (rc) {
      cs_topk_catalog_free(c);
      return rc;
    }
  }
  *out = c;
  return CS_OK;
}

int cs_l2_topk_catalog(const float* d_q, int64_t nq, const cs_topk_catalog* cat, int k, int64_t* d_idx, double* d_dist,
                       int squared, void* stream) {
  CS_REQUIRE(cat, CS_ERR_INVALID, "cs_l2_topk_catalog: NULL catalog");
  // what the handle holds was made on the creating call's stream: every user waits for it in stream order
  if (cat->ready) CS_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, cat->ready, 0));
  return l2_topk_impl(d_q, nq, cat->d_x, cat->nx, cat->d, k, d_idx, d_dist, stream, cat->f16.ximg ? &cat->f16 : nullptr,
                      squared ? 1 : 0);
}

void cs_l2_topk_stats(uint64_t out[2], int reset) { read_stats(g_topk_stats, out, reset); }

int cs_l2_topk_sq(const float* d_q, int64_t nq, const float* d_x, int64_t nx, int d, int k, int64_t* d_idx,
                  double* d_dist2, void* stream) {
  return l2_topk_impl(d_q, nq, d_x, nx, d, k, d_idx, d_dist2, stream, nullptr, 1);
}

int cs_l2_topk(const float* d_q, int64_t nq, const float* d_x, int64_t nx, int d, int k,
               int64_t* d_idx, double* d_dist, void* stream) {
  return l2_topk_impl(d_q, nq, d_x, nx, d, k, d_idx, d_dist, stream, nullptr, 0);
}

}  // extern "C"
