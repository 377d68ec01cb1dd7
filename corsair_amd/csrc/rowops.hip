// The small dense row operators of the ResUNet: affine/ReLU/residual, row L2 normalise, per-sample max and
// instance normalisation.  None of them is a convolution; k_affine_act shares the convolutions' epilogue.
//
// Summation orders are fixed and restated by the CPU oracle: every result is bit-identical to it.
#include "conv_epilogue.h"

namespace cs {

__global__ void k_affine_act(int64_t n, int c, const float* __restrict__ in, int ld_in,
                             const float* __restrict__ scale, const float* __restrict__ shift,
                             const float* __restrict__ residual, int ld_res, int relu,
                             float* __restrict__ out, int ld_out) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; t < n * c; t += stride) {
    int64_t r = t / c;
    int col = (int)(t - r * c);
    const float* res_row = residual ? residual + r * ld_res : nullptr;
    out[r * ld_out + col] = epilogue(in[r * ld_in + col], col, scale, shift, res_row, relu);
  }
}

// one wave per row; sequential-per-lane partial sums then a fixed xor-tree -> deterministic
__global__ void k_row_l2norm(int64_t n, int c, const float* __restrict__ in, int ld_in, float eps,
                             float* __restrict__ out, int ld_out) {
  int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* x = in + row * ld_in;
  float s = 0.0f;
  for (int i = lane; i < c; i += 64) s = __fmaf_rn(x[i], x[i], s);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  float nrm = sqrtf(s);
  nrm = fmaxf(nrm, eps);
  for (int i = lane; i < c; i += 64) out[row * ld_out + i] = x[i] / nrm;
}

// c <= 16 (the 16-channel voxel features): 16 lanes per row, four rows per wave.  The same butterfly as above from
// offset 8 down -- the offsets 32 and 16 of the one-wave-per-row kernel only ever add the exact zeros of the lanes
// beyond c -- so the same sums, bit for bit, with a quarter of the waves and whole 64-B rows per load.
__global__ void k_row_l2norm16(int64_t n, int c, const float* __restrict__ in, int ld_in, float eps,
                               float* __restrict__ out, int ld_out) {
  const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t row = g >> 4;
  const int ch = (int)(g & 15);
  const bool live = row < n && ch < c;
  const float x = live ? in[row * ld_in + ch] : 0.0f;
  float s = __fmaf_rn(x, x, 0.0f);
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  float nrm = sqrtf(s);
  nrm = fmaxf(nrm, eps);
  if (live) out[row * ld_out + ch] = x / nrm;
}

__device__ __forceinline__ unsigned f2ord(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__global__ void k_segmax_init(unsigned* buf, int64_t n) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t < n) buf[t] = f2ord(-INFINITY);
}
// One atomic per RUN of rows of one sample (not one per row): a thread owns one column of a block
// of SEGMAX_ROWS consecutive rows, keeps the running maximum while the batch index stays the same and flushes it when
// it changes (rows grouped by sample, the usual case: 32 x fewer atomics; any other order is still correct).
constexpr int SEGMAX_ROWS = 32;
__global__ void k_segmax_runs(int64_t n, int c, const float* __restrict__ in, int ld_in,
                              const int32_t* __restrict__ batch, int batch_ld, int n_batch, unsigned* obuf) {
  const int col = blockIdx.y * blockDim.x + threadIdx.x;
  if (col >= c) return;
  const int64_t r0 = (int64_t)blockIdx.x * SEGMAX_ROWS;
  const int64_t r1 = r0 + SEGMAX_ROWS < n ? r0 + SEGMAX_ROWS : n;
  int cur = -1;
  unsigned best = 0;
  for (int64_t r = r0; r < r1; ++r) {
    const int b = batch[r * batch_ld];
    if (b != cur) {
      if (cur >= 0 && cur < n_batch) atomicMax(&obuf[(int64_t)cur * c + col], best);
      cur = b;
      best = 0;   // f2ord maps every float above 0: the first value of the run replaces it
    }
    const unsigned v = f2ord(in[r * ld_in + col]);
    best = v > best ? v : best;
  }
  if (cur >= 0 && cur < n_batch && r1 > r0) atomicMax(&obuf[(int64_t)cur * c + col], best);
}
__global__ void k_segmax_fin(unsigned* buf, int64_t n) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t < n) reinterpret_cast<float*>(buf)[t] = ord2f(buf[t]);
}

// ------------------------------------------------------------------------------------------------
// Instance normalisation (MinkowskiInstanceNorm of the IN network variants, model/common.py:23-24):
// per sample and channel  out = (x - mean) / sqrt(var + eps) * weight + bias  with the biased variance.
// Fixed summation order (the oracle restates it): a sample's rows in chunks of INORM_CHUNK consecutive
// rows, f64 sequential sum inside a chunk, chunk sums added in chunk order.  mean and var are rounded to
// f32, 1/sqrt in f64 rounded to f32, the affine part in f32 without contraction.
// Rows must be grouped by sample (seg[b] .. seg[b+1], the collate order).
// ------------------------------------------------------------------------------------------------
constexpr int INORM_CHUNK = 256;
constexpr int INORM_SLICES = 64;

__device__ __forceinline__ int64_t inorm_slot(const int32_t* seg, int b) { return (int64_t)(seg[b] / INORM_CHUNK) + b; }

// grid (INORM_SLICES, n_batch, channel groups of 256); thread = channel.  PASS 0: sum of x; PASS 1: sum of
// (x - mean)^2 with the f32 mean of PASS 0.
template <int PASS>
__global__ __launch_bounds__(256) void k_inorm_partial(const float* __restrict__ x, int ld, int c,
                                                       const int32_t* __restrict__ seg,
                                                       const float* __restrict__ mean,
                                                       double* __restrict__ partial) {
  const int b = blockIdx.y;
  const int ch = blockIdx.z * 256 + threadIdx.x;
  if (ch >= c) return;
  const int r0 = seg[b], r1 = seg[b + 1];
  const int chunks = (r1 - r0 + INORM_CHUNK - 1) / INORM_CHUNK;
  const float m = PASS ? mean[(int64_t)b * c + ch] : 0.f;
  for (int k = blockIdx.x; k < chunks; k += gridDim.x) {
    const int a = r0 + k * INORM_CHUNK, e = min(r1, a + INORM_CHUNK);
    double acc = 0.0;
    for (int r = a; r < e; ++r) {
      const float v = x[(int64_t)r * ld + ch];
      if (PASS) {
        const float d = v - m;
        acc += (double)d * (double)d;
      } else {
        acc += (double)v;
      }
    }
    partial[(inorm_slot(seg, b) + k) * c + ch] = acc;
  }
}

// one thread per (sample, channel): chunk sums in order.  PASS 0 -> mean; PASS 1 -> 1 / sqrt(var + eps)
template <int PASS>
__global__ void k_inorm_stat(const double* __restrict__ partial, int c, int n_batch,
                             const int32_t* __restrict__ seg, float eps, float* __restrict__ stat) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= (int64_t)n_batch * c) return;
  const int b = (int)(t / c), ch = (int)(t - (int64_t)b * c);
  const int len = seg[b + 1] - seg[b];
  const int chunks = (len + INORM_CHUNK - 1) / INORM_CHUNK;
  double acc = 0.0;
  for (int k = 0; k < chunks; ++k) acc += partial[(inorm_slot(seg, b) + k) * c + ch];
  if (len == 0) {
    stat[t] = 0.f;
    return;
  }
  const float v = (float)(acc / (double)len);
  stat[t] = PASS ? (float)(1.0 / sqrt((double)v + (double)eps)) : v;
}

__global__ void k_inorm_apply(const float* __restrict__ x, int ld_in, int c, int n_batch,
                              const int32_t* __restrict__ seg, const float* __restrict__ mean,
                              const float* __restrict__ inv_std, const float* __restrict__ weight,
                              const float* __restrict__ bias, float* __restrict__ out, int ld_out) {
  const int b = blockIdx.y;
  const int r0 = seg[b], r1 = seg[b + 1];
  const int64_t total = (int64_t)(r1 - r0) * c;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int r = r0 + (int)(t / c), ch = (int)(t % c);
    const float d = x[(int64_t)r * ld_in + ch] - mean[(int64_t)b * c + ch];
    float v = d * inv_std[(int64_t)b * c + ch];
    if (weight) v = v * weight[ch];
    if (bias) v = v + bias[ch];
    out[(int64_t)r * ld_out + ch] = v;
  }
}

}  // namespace cs

using namespace cs;

extern "C" {

int cs_affine_act(int64_t n, int c, const float* d_in, int ld_in, const float* d_scale,
                  const float* d_shift, const float* d_residual, int ld_res, int relu,
                  float* d_out, int ld_out, void* stream) {
  CS_REQUIRE(d_in && d_out && c >= 1 && ld_in >= c && ld_out >= c, CS_ERR_INVALID,
             "cs_affine_act: bad argument");
  CS_REQUIRE(!d_scale || d_shift, CS_ERR_INVALID, "cs_affine_act: scale without shift");
  if (n == 0) return CS_OK;
  int64_t total = n * c;
  unsigned g = (unsigned)(ceil_div(total, 256) < 4096 ? ceil_div(total, 256) : 4096);
  hipLaunchKernelGGL(k_affine_act, dim3(g), dim3(256), 0, (hipStream_t)stream, n, c, d_in, ld_in,
                     d_scale, d_shift, d_residual, ld_res, relu, d_out, ld_out);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

int cs_row_l2_normalize(int64_t n, int c, const float* d_in, int ld_in, float eps, float* d_out,
                        int ld_out, void* stream) {
  CS_REQUIRE(d_in && d_out && c >= 1 && ld_in >= c && ld_out >= c, CS_ERR_INVALID,
             "cs_row_l2_normalize: bad argument");
  if (n == 0) return CS_OK;
  if (c <= 16)
    hipLaunchKernelGGL(k_row_l2norm16, dim3((unsigned)ceil_div(n * 16, 256)), dim3(256), 0, (hipStream_t)stream, n, c, d_in,
                       ld_in, eps, d_out, ld_out);
  else
    hipLaunchKernelGGL(k_row_l2norm, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0,
                       (hipStream_t)stream, n, c, d_in, ld_in, eps, d_out, ld_out);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

int cs_segmented_max(int64_t n, int c, const float* d_in, int ld_in, const int32_t* d_batch,
                     int batch_ld, int n_batch, float* d_out, void* stream) {
  CS_REQUIRE(d_in && d_batch && d_out && c >= 1 && n_batch >= 0 && batch_ld >= 1,
             CS_ERR_INVALID, "cs_segmented_max: bad argument");
  hipStream_t s = (hipStream_t)stream;
  int64_t on = (int64_t)n_batch * c;
  if (on == 0) return CS_OK;
  unsigned* obuf = reinterpret_cast<unsigned*>(d_out);
  hipLaunchKernelGGL(k_segmax_init, dim3((unsigned)ceil_div(on, 256)), dim3(256), 0, s, obuf, on);
  if (n > 0)
    hipLaunchKernelGGL(k_segmax_runs, dim3((unsigned)ceil_div(n, SEGMAX_ROWS), (unsigned)ceil_div(c, 256)), dim3(256), 0, s,
                       n, c, d_in, ld_in, d_batch, batch_ld, n_batch, obuf);
  hipLaunchKernelGGL(k_segmax_fin, dim3((unsigned)ceil_div(on, 256)), dim3(256), 0, s, obuf, on);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

int cs_instance_norm(int64_t n, int c, const float* d_in, int ld_in, const int32_t* d_seg, int n_batch,
                     const float* d_weight, const float* d_bias, float eps, float* d_out, int ld_out,
                     void* stream) {
  CS_REQUIRE(d_in && d_out && d_seg && c >= 1 && ld_in >= c && ld_out >= c && n_batch >= 0 && n >= 0 &&
                 n < (1LL << 31) && eps >= 0.f,
             CS_ERR_INVALID, "cs_instance_norm: bad argument");
  if (n == 0 || n_batch == 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const int64_t slots = n / INORM_CHUNK + n_batch + 1;
  PoolBuf<double> partial((size_t)slots * c);
  PoolBuf<float> mean((size_t)n_batch * c), inv_std((size_t)n_batch * c);
  CS_REQUIRE(partial.p && mean.p && inv_std.p, CS_ERR_HIP, "cs_instance_norm: scratch allocation failed");
  const dim3 pg(INORM_SLICES, (unsigned)n_batch, (unsigned)ceil_div(c, 256));
  const unsigned sg = (unsigned)ceil_div((int64_t)n_batch * c, 256);
  hipLaunchKernelGGL(k_inorm_partial<0>, pg, dim3(256), 0, s, d_in, ld_in, c, d_seg, (const float*)nullptr,
                     partial.p);
  hipLaunchKernelGGL(k_inorm_stat<0>, dim3(sg), dim3(256), 0, s, partial.p, c, n_batch, d_seg, eps, mean.p);
  hipLaunchKernelGGL(k_inorm_partial<1>, pg, dim3(256), 0, s, d_in, ld_in, c, d_seg, mean.p, partial.p);
  hipLaunchKernelGGL(k_inorm_stat<1>, dim3(sg), dim3(256), 0, s, partial.p, c, n_batch, d_seg, eps, inv_std.p);
  hipLaunchKernelGGL(k_inorm_apply, dim3(64, (unsigned)n_batch), dim3(256), 0, s, d_in, ld_in, c, n_batch,
                     d_seg, mean.p, inv_std.p, d_weight, d_bias, d_out, ld_out);
  CS_LAUNCH_CHECK();
  return CS_OK;  // no synchronisation: the scratch returns to this thread's stream-ordered cache
}

}  // extern "C"
