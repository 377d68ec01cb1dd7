// Sparse convolution backward: the weight gradient (cs_conv_wgrad).
//
//   dW[k, ci, co] = sum_{o : T[o][k] >= 0} x[T[o][k], ci] * g[o, co]
//
// T is the kernel map's output-stationary table [n_out, kvol]; the same formula holds for stride-1, strided and
// transposed maps as built (the map already says which input row every (output row, offset) pair reads).  The data
// gradient needs no kernel of its own: it is cs_conv_fwd on the reverse map (corsair_amd/backend.py, conv_dgrad).
//
// Kernel design (gfx950):
//   * the map's output rows, in the tiling order of the forward kernel (d_rowlist: rows sorted by neighbour-presence
//     mask), are cut into fixed chunks of CH rows; CH depends only on (n_out, kvol, cin, cout), so the chunking -- and
//     with it every summation order below -- is the same on every call.
//   * chunk masks: bit k of a chunk's mask = some row of the chunk has offset k.  Maps with a tiling order carry the
//     offsets present in every 32-row group (d_gmask): k_wgrad_masks_groups ORs a chunk's groups, and the MFMA kernel
//     also skips the 32-row groups without offset k.  Other maps (kernel size 1): k_wgrad_masks scans the table.
//     Skipped offsets and groups would only add zeros.
//   * k_wgrad_mfma<NT> (cin, cout multiples of 32): one workgroup per (chunk, offset k, 4 tiles); a wave owns one tile of
//     32 input channels x 32 NT output channels and walks the chunk's rows in order, two rows per
//     v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation).  Lane l of the A operand is x[pair l>>5][ci l&31],
//     lane l of the B operand g[pair l>>5][co l&31]: both are plain 128-byte row loads of gathered rows (no transpose).
//     The row indices of 32 rows are read once per wave (one lane per row) and broadcast with ds_bpermute.
//   * k_wgrad_valu (any other shape: cin = 1 of the stem convolution, cout = 16 of `final`): one workgroup per
//     (chunk, k); the chunk's (out row, in row) pairs are staged in LDS, a thread owns one (ci, co) element and runs a
//     sequential fma chain over the chunk's rows.
//   * per-(chunk, k) partial sums land in stream-ordered scratch; k_wgrad_reduce adds them per element in ascending
//     chunk order.  No float atomics anywhere: the result is bit-identical run to run and independent of timing.
#include "common.h"

namespace cs {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int WGRAD_MIN_ROWS = 128;                   // smallest chunk (64 MFMA steps per wave)
constexpr int WGRAD_VALU_MAX_ROWS = 4096;             // LDS index staging of the VALU kernel
constexpr int64_t WGRAD_PARTIAL_BUDGET = 16LL << 20;  // partial floats aimed for (64 MB of scratch)

// bit k of cmask[chunk] = some row of the chunk has a neighbour at offset k (nbr == NULL: the 1x1 identity map)
__global__ __launch_bounds__(256) void k_wgrad_masks(const int32_t* __restrict__ nbr, const int32_t* __restrict__ rowlist,
                                                     int kvol, int64_t n_out, int chunk_rows,
                                                     uint32_t* __restrict__ cmask) {
  __shared__ unsigned mask_lds;
  if (threadIdx.x == 0) mask_lds = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * chunk_rows;
  const int64_t r1 = r0 + chunk_rows < n_out ? r0 + chunk_rows : n_out;
  const int64_t total = (r1 - r0) * kvol;
  unsigned m = 0;
  for (int64_t i = threadIdx.x; i < total; i += blockDim.x) {
    const int64_t r = r0 + i / kvol;
    const int k = (int)(i % kvol);
    const int64_t o = rowlist ? rowlist[r] : r;
    if (!nbr || nbr[o * kvol + k] >= 0) m |= 1u << k;
  }
  if (m) atomicOr(&mask_lds, m);
  __syncthreads();
  if (threadIdx.x == 0) cmask[blockIdx.x] = mask_lds;
}

// the same from the per-32-row-group masks of the tiling order (chunk_rows is a multiple of 32)
__global__ void k_wgrad_masks_groups(const uint32_t* __restrict__ gmask, int64_t n_out, int chunk_rows, int64_t n_chunks,
                                     uint32_t* __restrict__ cmask) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= n_chunks) return;
  const int64_t r1 = c * chunk_rows + chunk_rows < n_out ? c * chunk_rows + chunk_rows : n_out;
  const int64_t g0 = c * (chunk_rows / 32), g1 = (r1 + 31) / 32;
  unsigned m = 0;
  for (int64_t g = g0; g < g1; ++g) m |= gmask[g];
  cmask[c] = m;
}

template <int NT>
__global__ __launch_bounds__(256) void k_wgrad_mfma(const int32_t* __restrict__ nbr, const int32_t* __restrict__ rowlist,
                                                    int kvol, int64_t n_out, const float* __restrict__ x, int ld_in,
                                                    int cin, const float* __restrict__ g, int ld_g, int cout,
                                                    int chunk_rows, const uint32_t* __restrict__ cmask,
                                                    const uint32_t* __restrict__ gmask, float* __restrict__ partial) {
  const int chunk = blockIdx.x, k = blockIdx.y;
  if (!((cmask[chunk] >> k) & 1u)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int co_tiles = cout / (32 * NT);
  const int tile = blockIdx.z * 4 + wave;
  if (tile >= (cin / 32) * co_tiles) return;
  const int ci0 = (tile / co_tiles) * 32, co0 = (tile % co_tiles) * 32 * NT;
  const int64_t r0 = (int64_t)chunk * chunk_rows;
  const int64_t r1 = r0 + chunk_rows < n_out ? r0 + chunk_rows : n_out;
  const int half = lane >> 5, col = lane & 31;

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

  // the next 32-row group at or after r with a neighbour at offset k (r1 when none): rows start at r0, a multiple of 32
  auto live_group = [&](int64_t r) {
    if (gmask)
      while (r < r1 && !((gmask[r >> 5] >> k) & 1u)) r += 32;
    return r < r1 ? r : r1;
  };
  // (output row, input row) of row r + (lane & 31); -1 past the end or where the row has no neighbour at k
  auto pair_of = [&](int64_t r, int32_t& o, int32_t& src) {
    const int64_t rr = r + col;
    o = -1;
    src = -1;
    if (rr < r1) {
      o = rowlist ? rowlist[rr] : (int32_t)rr;
      src = nbr ? nbr[(int64_t)o * kvol + k] : o;
    }
  };
  int32_t o_cur, s_cur;
  int64_t r = live_group(r0);
  pair_of(r, o_cur, s_cur);
  while (r < r1) {
    const int64_t r_nxt = live_group(r + 32);
    int32_t o_nxt = -1, s_nxt = -1;
    if (r_nxt < r1) pair_of(r_nxt, o_nxt, s_nxt);   // indices of the next live 32 rows in flight during this step
    float a[16], b[16][NT];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int src_lane = 2 * s + half;
      const int32_t src = __shfl(s_cur, src_lane);
      const int32_t o = __shfl(o_cur, src_lane);
      const bool live = src >= 0;
      a[s] = live ? x[(int64_t)src * ld_in + ci0 + col] : 0.0f;
#pragma unroll
      for (int t = 0; t < NT; ++t) b[s][t] = live ? g[(int64_t)o * ld_g + co0 + 32 * t + col] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s][t], acc[t], 0, 0, 0);
    o_cur = o_nxt;
    s_cur = s_nxt;
    r = r_nxt;
  }

  // C/D layout: col = lane & 31 (output channel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (input channel)
  float* dst = partial + ((int64_t)chunk * kvol + k) * cin * cout;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ci = ci0 + (i & 3) + 8 * (i >> 2) + 4 * half;
      dst[(int64_t)ci * cout + co0 + 32 * t + col] = acc[t][i];
    }
}

__global__ __launch_bounds__(256) void k_wgrad_valu(const int32_t* __restrict__ nbr, const int32_t* __restrict__ rowlist,
                                                    int kvol, int64_t n_out, const float* __restrict__ x, int ld_in,
                                                    int cin, const float* __restrict__ g, int ld_g, int cout,
                                                    int chunk_rows, const uint32_t* __restrict__ cmask,
                                                    float* __restrict__ partial) {
  __shared__ int32_t o_lds[WGRAD_VALU_MAX_ROWS];
  __shared__ int32_t s_lds[WGRAD_VALU_MAX_ROWS];
  const int chunk = blockIdx.x, k = blockIdx.y;
  if (!((cmask[chunk] >> k) & 1u)) return;
  const int64_t r0 = (int64_t)chunk * chunk_rows;
  const int rows = (int)((r0 + chunk_rows < n_out ? r0 + chunk_rows : n_out) - r0);
  for (int i = threadIdx.x; i < rows; i += blockDim.x) {
    const int32_t o = rowlist ? rowlist[r0 + i] : (int32_t)(r0 + i);
    o_lds[i] = o;
    s_lds[i] = nbr ? nbr[(int64_t)o * kvol + k] : o;
  }
  __syncthreads();
  float* dst = partial + ((int64_t)chunk * kvol + k) * cin * cout;
  for (int e = threadIdx.x; e < cin * cout; e += blockDim.x) {
    const int ci = e / cout, co = e - ci * cout;
    float acc = 0.0f;
    for (int i = 0; i < rows; ++i) {
      const int32_t src = s_lds[i];
      if (src >= 0) acc = __fmaf_rn(x[(int64_t)src * ld_in + ci], g[(int64_t)o_lds[i] * ld_g + co], acc);
    }
    dst[e] = acc;
  }
}

// dW[k, ci, co] = sum over chunks in ascending order of the chunks' partials (chunks without offset k are skipped)
__global__ void k_wgrad_reduce(const float* __restrict__ partial, const uint32_t* __restrict__ cmask, int64_t n_chunks,
                               int kvol, int64_t per_k, float* __restrict__ dw) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= per_k * kvol) return;
  const int k = (int)(t / per_k);
  float acc = 0.0f;
  // eight chunks' loads in flight, then their adds in ascending chunk order (the order is that of the plain loop)
  for (int64_t c0 = 0; c0 < n_chunks; c0 += 8) {
    float v[8];
    bool on[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t c = c0 + j;
      on[j] = c < n_chunks && ((cmask[c] >> k) & 1u);
      v[j] = on[j] ? partial[c * kvol * per_k + t] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (on[j]) acc += v[j];
  }
  dw[t] = acc;
}

}  // namespace cs

using namespace cs;

extern "C" {

int cs_conv_wgrad(const cs_kernelmap* km, int64_t n_in, int64_t n_out, const float* d_in, int ld_in, int cin,
                  const float* d_gout, int ld_gout, int cout, float* d_dw, void* stream) {
  CS_REQUIRE(cin >= 1 && cout >= 1 && ld_in >= cin && ld_gout >= cout && n_in >= 0 && n_out >= 0, CS_ERR_INVALID,
             "cs_conv_wgrad: bad channel / leading dimension (cin %d ld_in %d cout %d ld_gout %d)", cin, ld_in, cout,
             ld_gout);
  CS_REQUIRE(d_dw, CS_ERR_INVALID, "cs_conv_wgrad: NULL weight gradient");
  CS_REQUIRE(n_in < (1LL << 31) && n_out < (1LL << 31), CS_ERR_INVALID, "cs_conv_wgrad: too many rows");
  int kvol = 1;
  const int32_t* nbr = nullptr;
  const int32_t* rowlist = nullptr;
  if (km) {
    CS_REQUIRE(km->n_out == n_out && km->n_in == n_in, CS_ERR_INVALID,
               "cs_conv_wgrad: kernel map is for %lld -> %lld rows, tensors have %lld -> %lld", (long long)km->n_in,
               (long long)km->n_out, (long long)n_in, (long long)n_out);
    CS_REQUIRE(km->kvol >= 1 && km->kvol <= 32, CS_ERR_UNSUPPORTED, "cs_conv_wgrad: kernel volume %d", km->kvol);
    kvol = km->kvol;
    nbr = km->d_nbr;
    rowlist = km->d_rowlist;
  } else {
    CS_REQUIRE(n_in == n_out, CS_ERR_INVALID, "cs_conv_wgrad: 1x1 conv needs n_in == n_out");
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t per_k = (int64_t)cin * cout;
  if (n_out == 0) return hipMemsetAsync(d_dw, 0, (size_t)kvol * per_k * 4, s) == hipSuccess ? CS_OK : CS_ERR_HIP;
  CS_REQUIRE(d_in && d_gout, CS_ERR_INVALID, "cs_conv_wgrad: NULL tensor");

  const bool mfma = cin % 32 == 0 && cout % 32 == 0;
  // chunking: a function of the shapes only (never of timing), so the summation order is fixed
  int64_t chunks = ceil_div(n_out, WGRAD_MIN_ROWS);
  const int64_t cap = WGRAD_PARTIAL_BUDGET / (kvol * per_k);
  chunks = chunks < cap ? chunks : (cap > 1 ? cap : 1);
  int64_t chunk_rows = ceil_div(ceil_div(n_out, chunks), 32) * 32;
  if (!mfma && chunk_rows > WGRAD_VALU_MAX_ROWS) chunk_rows = WGRAD_VALU_MAX_ROWS;
  CS_REQUIRE(chunk_rows < (1LL << 31), CS_ERR_INVALID, "cs_conv_wgrad: too many rows");
  const int64_t n_chunks = ceil_div(n_out, chunk_rows);
  CS_REQUIRE(n_chunks < 65536, CS_ERR_UNSUPPORTED, "cs_conv_wgrad: %lld row chunks", (long long)n_chunks);

  pool_use_stream(s);
  PoolBuf<uint32_t> cmask((size_t)n_chunks);
  PoolBuf<float> partial((size_t)(n_chunks * kvol * per_k));
  CS_REQUIRE(cmask.p && partial.p, CS_ERR_HIP, "cs_conv_wgrad: scratch allocation failed");
  // per-32-row-group masks of the tiling order (maps of kernel size 3); they index rows of d_rowlist
  const uint32_t* gmask = (km && km->d_rowlist && km->d_gmask) ? km->d_gmask : nullptr;
  if (gmask)
    hipLaunchKernelGGL(k_wgrad_masks_groups, dim3((unsigned)ceil_div(n_chunks, 256)), dim3(256), 0, s, gmask, n_out,
                       (int)chunk_rows, n_chunks, cmask.p);
  else
    hipLaunchKernelGGL(k_wgrad_masks, dim3((unsigned)n_chunks), dim3(256), 0, s, nbr, rowlist, kvol, n_out,
                       (int)chunk_rows, cmask.p);
  if (mfma) {
    const int nt = cout % 64 == 0 ? 2 : 1;
    const int64_t tiles = (int64_t)(cin / 32) * (cout / (32 * nt));
    const dim3 grid((unsigned)n_chunks, (unsigned)kvol, (unsigned)ceil_div(tiles, 4));
    if (nt == 2)
      hipLaunchKernelGGL(k_wgrad_mfma<2>, grid, dim3(256), 0, s, nbr, rowlist, kvol, n_out, d_in, ld_in, cin, d_gout,
                         ld_gout, cout, (int)chunk_rows, cmask.p, gmask, partial.p);
    else
      hipLaunchKernelGGL(k_wgrad_mfma<1>, grid, dim3(256), 0, s, nbr, rowlist, kvol, n_out, d_in, ld_in, cin, d_gout,
                         ld_gout, cout, (int)chunk_rows, cmask.p, gmask, partial.p);
  } else {
    hipLaunchKernelGGL(k_wgrad_valu, dim3((unsigned)n_chunks, (unsigned)kvol), dim3(256), 0, s, nbr, rowlist, kvol,
                       n_out, d_in, ld_in, cin, d_gout, ld_gout, cout, (int)chunk_rows, cmask.p, partial.p);
  }
  const int64_t total = kvol * per_k;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, partial.p, cmask.p,
                     n_chunks, kvol, per_k, d_dw);
  CS_LAUNCH_CHECK();
  return CS_OK;  // no synchronisation: the scratch returns to this thread's stream-ordered cache
}

}  // extern "C"
