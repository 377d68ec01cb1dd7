// Metric-learning loss on feature pairs: the FCGF-form contrastive loss the PiP / PiN / NiN lists of a
// training batch were mined for, value and feature gradients, reproducible to the bit.
//
// Both sums are 64-bit INTEGER sums of fixed-point values, so neither depends on the order of the pairs, on the launch
// shape or on the run: the value is a block reduction plus one integer atomic per block, the gradient one integer
// atomic (global_atomic_add_x2) per pair side and column.  At C = 16 the 16 lanes of a pair add to one 128-B row
// segment of accumulators.  The arithmetic is the list in include/corsair_hip.h, restated in tests/pair_loss_ref.py.
#include "common.h"

namespace cs {
namespace {

constexpr int kMaxTerms = CS_PAIR_LOSS_MAX_TERMS;
constexpr int kMaxMats = 2 * kMaxTerms;
constexpr int kLanes = 16;   // lanes of one pair in the backward: lane l owns columns l, l + 16, ...

// Value: l_p <= 2^8 (rows of norm <= 8: d <= 16, h <= 16), at most 2^22 pairs: S_t <= 2^8 * 2^32 * 2^22 = 2^62.
constexpr double kValScale = 0x1.0p32;
constexpr double kValMax = 0x1.0p40;    // l_p * 2^32 is clamped here, so the bound holds for ANY input
// Gradient: |e_k| <= 2 h r_t <= 32 w / P, so a row's accumulator stays below 32 * 1024 * 2^44 = 2^59 in magnitude even
// if every pair of a term hits it (and below 2^62 with all 8 terms on it).
constexpr double kGradScale = 0x1.0p44;
constexpr double kGradMax = 0x1.0p59;   // clamp of one contribution (in range by the bound above; keeps the cast defined)

struct LossTerm {
  const float* A;
  const float* B;
  const int32_t* pairs;
  int64_t P;
  int64_t* accA;   // backward: [rows of A, C] accumulators of A's matrix
  int64_t* accB;
  int ldA, ldB;
  int push;        // 0 PULL, 1 PUSH
  float m;
  float r;         // (float)((double)w / P)
  double w;
};
struct LossArgs {
  LossTerm t[kMaxTerms];
  int n, C;
};
struct GradMat {
  const int64_t* acc;
  float* out;
  int64_t rows;
  int ld;
};
struct GradArgs {
  GradMat m[kMaxMats];
  int n, C;
};

// d of pair (a, b): s = s + diff * diff for k ascending (product rounded, then the sum: no contraction), sqrt rounded
__device__ __forceinline__ float pl_dist(const float* __restrict__ a, const float* __restrict__ b, int C) {
  float s = 0.f;
  for (int k = 0; k < C; ++k) {
    const float diff = a[k] - b[k];
    s = s + diff * diff;
  }
  return __fsqrt_rn(s);
}
__device__ __forceinline__ float pl_hinge(float d, float m, int push) {
  return fmaxf(push ? m - d : d - m, 0.f);   // fmaxf(NaN, 0) = 0: a non-finite row contributes nothing
}

__global__ void __launch_bounds__(256) k_pl_fwd(LossArgs a, unsigned long long* S) {
  __shared__ unsigned long long part[4];
  const LossTerm& T = a.t[blockIdx.y];
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (blockIdx.x * (int64_t)blockDim.x >= T.P) return;   // whole block beyond this term's list
  unsigned long long v = 0;
  if (p < T.P) {
    const float d = pl_dist(T.A + (int64_t)T.pairs[2 * p] * T.ldA, T.B + (int64_t)T.pairs[2 * p + 1] * T.ldB, a.C);
    const float h = pl_hinge(d, T.m, T.push);
    const float l = h * h;
    const double x = fmin(fmax((double)l * kValScale, 0.0), kValMax);
    v = (unsigned long long)x;   // truncates
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&S[blockIdx.y], (part[0] + part[1]) + (part[2] + part[3]));
}

__global__ void k_pl_value(LossArgs a, const unsigned long long* __restrict__ S, double* term_loss, float* total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sum = 0.0;
  for (int t = 0; t < a.n; ++t) {
    const double L = a.t[t].P > 0 ? a.t[t].w * (double)S[t] * 0x1.0p-32 / (double)a.t[t].P : 0.0;
    term_loss[t] = L;
    sum = sum + L;
  }
  *total = (float)sum;
}

__global__ void __launch_bounds__(256) k_pl_bwd(LossArgs a) {
  const LossTerm& T = a.t[blockIdx.y];
  const int64_t p = blockIdx.x * (int64_t)(256 / kLanes) + threadIdx.x / kLanes;
  if (p >= T.P) return;
  const int lane = threadIdx.x % kLanes;
  const int64_t i = T.pairs[2 * p], j = T.pairs[2 * p + 1];
  const float* ra = T.A + i * T.ldA;
  const float* rb = T.B + j * T.ldB;
  const float d = pl_dist(ra, rb, a.C);   // every lane of the pair: the same bits
  const float h = pl_hinge(d, T.m, T.push);
  if (!(h > 0.f) || !(d > 0.f)) return;
  const float c = (h + h) * T.r;
  for (int k = lane; k < a.C; k += kLanes) {
    const float diff = ra[k] - rb[k];
    const float u = __fdiv_rn(diff, d);
    float e = c * u;
    if (T.push) e = -e;
    const double x = fmin(fmax((double)e * kGradScale, -kGradMax), kGradMax);
    const long long q = (long long)x;   // truncates toward zero, so the B side is exactly -q
    atomicAdd((unsigned long long*)&T.accA[i * a.C + k], (unsigned long long)q);
    atomicAdd((unsigned long long*)&T.accB[j * a.C + k], (unsigned long long)(-q));
  }
}

__global__ void __launch_bounds__(256) k_pl_grad(GradArgs a, const float* __restrict__ g_up) {
  const GradMat& M = a.m[blockIdx.y];
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= M.rows * a.C) return;
  const int64_t i = e / a.C;
  const int k = (int)(e - i * a.C);
  M.out[i * M.ld + k] = (float)((double)M.acc[e] * 0x1.0p-44) * g_up[0];
}

int fill_args(const char* who, int n_mat, const float* const* d_mat, const int64_t* h_rows, const int32_t* h_ld, int C,
              int n_term, const int32_t* h_a, const int32_t* h_b, const int32_t* h_kind, const float* h_margin,
              const double* h_weight, const int32_t* const* d_pairs, const int64_t* h_npairs, LossArgs* out,
              int64_t* max_p) {
  CS_REQUIRE(d_mat && h_rows && h_ld && h_a && h_b && h_kind && h_margin && h_weight && d_pairs && h_npairs,
             CS_ERR_INVALID, "%s: NULL argument", who);
  CS_REQUIRE(n_term >= 1 && n_term <= kMaxTerms, CS_ERR_INVALID, "%s: 1 <= terms <= %d", who, kMaxTerms);
  CS_REQUIRE(n_mat >= 1 && n_mat <= kMaxMats, CS_ERR_INVALID, "%s: 1 <= matrices <= %d", who, kMaxMats);
  CS_REQUIRE(C >= 1 && C <= 256, CS_ERR_UNSUPPORTED, "%s: 1 <= C <= 256", who);
  for (int m = 0; m < n_mat; ++m) {
    CS_REQUIRE(h_rows[m] >= 0 && h_rows[m] < (1LL << 31), CS_ERR_INVALID, "%s: rows of matrix %d out of range", who, m);
    CS_REQUIRE(h_ld[m] >= C, CS_ERR_INVALID, "%s: leading dimension of matrix %d is below C", who, m);
    CS_REQUIRE(d_mat[m] || h_rows[m] == 0, CS_ERR_INVALID, "%s: matrix %d is NULL", who, m);
  }
  out->n = n_term;
  out->C = C;
  *max_p = 0;
  for (int t = 0; t < n_term; ++t) {
    CS_REQUIRE(h_a[t] >= 0 && h_a[t] < n_mat && h_b[t] >= 0 && h_b[t] < n_mat, CS_ERR_INVALID,
               "%s: term %d names a matrix that is not there", who, t);
    CS_REQUIRE(h_kind[t] == CS_PAIR_PULL || h_kind[t] == CS_PAIR_PUSH, CS_ERR_INVALID, "%s: term %d: unknown kind", who, t);
    CS_REQUIRE(h_npairs[t] >= 0 && h_npairs[t] <= (1LL << 22), CS_ERR_UNSUPPORTED, "%s: term %d: at most 2^22 pairs", who, t);
    CS_REQUIRE(h_margin[t] >= 0.f && h_margin[t] <= 16.f, CS_ERR_INVALID, "%s: term %d: margin outside [0, 16]", who, t);
    CS_REQUIRE(h_weight[t] >= 0.0 && h_weight[t] <= 1024.0, CS_ERR_INVALID, "%s: term %d: weight outside [0, 1024]", who, t);
    CS_REQUIRE(h_npairs[t] == 0 || d_pairs[t], CS_ERR_INVALID, "%s: term %d: NULL pair list", who, t);
    CS_REQUIRE(h_npairs[t] == 0 || (h_rows[h_a[t]] > 0 && h_rows[h_b[t]] > 0), CS_ERR_INVALID,
               "%s: term %d has pairs on an empty matrix", who, t);
    LossTerm& T = out->t[t];
    T.A = d_mat[h_a[t]];
    T.B = d_mat[h_b[t]];
    T.ldA = h_ld[h_a[t]];
    T.ldB = h_ld[h_b[t]];
    T.pairs = d_pairs[t];
    T.P = h_npairs[t];
    T.accA = T.accB = nullptr;
    T.push = h_kind[t] == CS_PAIR_PUSH;
    T.m = h_margin[t];
    T.w = h_weight[t];
    T.r = T.P > 0 ? (float)(h_weight[t] / (double)T.P) : 0.f;
    if (T.P > *max_p) *max_p = T.P;
  }
  return CS_OK;
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_pair_loss_fwd(int n_mat, const float* const* d_mat, const int64_t* h_rows, const int32_t* h_ld, int C,
                     int n_term, const int32_t* h_a, const int32_t* h_b, const int32_t* h_kind, const float* h_margin,
                     const double* h_weight, const int32_t* const* d_pairs, const int64_t* h_npairs,
                     double* d_term_loss, float* d_total, void* stream) {
  LossArgs args;
  int64_t max_p = 0;
  const int rc = fill_args("cs_pair_loss_fwd", n_mat, d_mat, h_rows, h_ld, C, n_term, h_a, h_b, h_kind, h_margin,
                           h_weight, d_pairs, h_npairs, &args, &max_p);
  if (rc != CS_OK) return rc;
  CS_REQUIRE(d_term_loss && d_total, CS_ERR_INVALID, "cs_pair_loss_fwd: NULL output");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<unsigned long long> S(kMaxTerms);
  CS_REQUIRE(S.p, CS_ERR_HIP, "cs_pair_loss_fwd: scratch allocation failed");
  ProfScope prof("loss", s);
  CS_HIP_CHECK(hipMemsetAsync(S.p, 0, sizeof(unsigned long long) * kMaxTerms, s));
  if (max_p > 0) {
    hipLaunchKernelGGL(k_pl_fwd, dim3((unsigned)ceil_div(max_p, 256), (unsigned)n_term), dim3(256), 0, s, args, S.p);
    CS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pl_value, dim3(1), dim3(64), 0, s, args, S.p, d_term_loss, d_total);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

int cs_pair_loss_bwd(int n_mat, const float* const* d_mat, const int64_t* h_rows, const int32_t* h_ld, int C,
                     int n_term, const int32_t* h_a, const int32_t* h_b, const int32_t* h_kind, const float* h_margin,
                     const double* h_weight, const int32_t* const* d_pairs, const int64_t* h_npairs,
                     const float* d_grad_up, float* const* d_grad, const int32_t* h_ld_grad, void* stream) {
  LossArgs args;
  int64_t max_p = 0;
  const int rc = fill_args("cs_pair_loss_bwd", n_mat, d_mat, h_rows, h_ld, C, n_term, h_a, h_b, h_kind, h_margin,
                           h_weight, d_pairs, h_npairs, &args, &max_p);
  if (rc != CS_OK) return rc;
  CS_REQUIRE(d_grad_up && d_grad && h_ld_grad, CS_ERR_INVALID, "cs_pair_loss_bwd: NULL argument");
  int64_t first[kMaxMats + 1] = {0}, max_elems = 0;
  for (int m = 0; m < n_mat; ++m) {
    CS_REQUIRE(h_ld_grad[m] >= C, CS_ERR_INVALID, "cs_pair_loss_bwd: leading dimension of gradient %d is below C", m);
    CS_REQUIRE(d_grad[m] || h_rows[m] == 0, CS_ERR_INVALID, "cs_pair_loss_bwd: gradient %d is NULL", m);
    first[m + 1] = first[m] + h_rows[m] * C;
    if (h_rows[m] * C > max_elems) max_elems = h_rows[m] * C;
  }
  if (max_elems == 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<int64_t> acc((size_t)first[n_mat]);   // zeroed below: one accumulator per gradient element
  CS_REQUIRE(acc.p, CS_ERR_HIP, "cs_pair_loss_bwd: scratch allocation failed");
  GradArgs ga;
  ga.n = n_mat;
  ga.C = C;
  for (int m = 0; m < n_mat; ++m) ga.m[m] = GradMat{acc.p + first[m], d_grad[m], h_rows[m], h_ld_grad[m]};
  for (int t = 0; t < n_term; ++t) {
    args.t[t].accA = acc.p + first[h_a[t]];
    args.t[t].accB = acc.p + first[h_b[t]];
  }
  ProfScope prof("loss", s);
  CS_HIP_CHECK(hipMemsetAsync(acc.p, 0, sizeof(int64_t) * (size_t)first[n_mat], s));
  if (max_p > 0) {
    hipLaunchKernelGGL(k_pl_bwd, dim3((unsigned)ceil_div(max_p, 256 / kLanes), (unsigned)n_term), dim3(256), 0, s,
                       args);
    CS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pl_grad, dim3((unsigned)ceil_div(max_elems, 256), (unsigned)n_mat), dim3(256), 0, s, ga,
                     d_grad_up);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
