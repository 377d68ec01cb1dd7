// RANSAC hypotheses (see ransac.hip for the round they belong to): k_ransac_pack, the packed copies of the correspondences,
// and k_ransac_hyp, one lane per hypothesis -- sample ransac_n pairs, closed-form rigid fit (horn.h), R|t as f64 and, in a
// prefiltered round, the hypothesis' prefilter row (pf_emit_row, ransac.h).  The only RANSAC unit that includes horn.h and
// exact_div.h: the register budget of k_ransac_hyp (comment above it) depends on this file, those two and pf_emit_row alone.
#include "ransac.h"
#include "exact_div.h"
#include "horn.h"

namespace cs {

// rng_u64, rng_index: common.h

// structure-of-arrays copy of the correspondences: pk[c * total + i], c = sx,sy,sz,qx,qy,qz
// + pair32[i] = (sx, sy, sz, qx | qy, qz, 0, 0): one aligned 32-B sector per pair for the random
// sampling of k_ransac_hyp (two 12-B rows of the caller's arrays would touch two to four lines)
__global__ void k_ransac_pack(const float* __restrict__ src, const float* __restrict__ tgt,
                              int64_t n, float* __restrict__ pk, float4* __restrict__ pair32) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  pair32[2 * i + 0] = make_float4(src[3 * i + 0], src[3 * i + 1], src[3 * i + 2], tgt[3 * i + 0]);
  pair32[2 * i + 1] = make_float4(tgt[3 * i + 1], tgt[3 * i + 2], 0.f, 0.f);
  pk[0 * n + i] = src[3 * i + 0];
  pk[1 * n + i] = src[3 * i + 1];
  pk[2 * n + i] = src[3 * i + 2];
  pk[3 * n + i] = tgt[3 * i + 0];
  pk[4 * n + i] = tgt[3 * i + 1];
  pk[5 * n + i] = tgt[3 * i + 2];
}

// centroids = sums / ransac_n, six quotients with one divisor: exact_div.h's multiply-and-correct sequence, which returns the
// IEEE quotient (proof and conditions there), when the host found the divisor admissible (inv_n != 0) and all six sums are in
// the proven range; otherwise (a sum that is 0, subnormal or not finite) the six divisions as before
__device__ __forceinline__ void centroid_div(double (&cs_)[3], double (&ct_)[3], double dn, double inv_n) {
  bool fast = inv_n != 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) fast = fast && exact_div_ok(cs_[a]) && exact_div_ok(ct_[a]);
  if (fast) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      cs_[a] = exact_div(cs_[a], dn, inv_n);
      ct_[a] = exact_div(ct_[a], dn, inv_n);
    }
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      cs_[a] = cs_[a] / dn;
      ct_[a] = ct_[a] / dn;
    }
  }
}

// Five waves per SIMD: the attribute holds the register allocator to that budget for BOTH instantiations -- <10> takes 96
// registers and <0> 94, neither uses scratch (without it <10> takes 107 and runs at four waves).  The budget is not free: a
// change in this file, in horn.h, in exact_div.h or in pf_emit_row (ransac.h) that needs more registers would spill instead of
// failing, so check the compiler's resource report (-Rpass-analysis=kernel-resource-usage: VGPRs <= 96, ScratchSize 0) after
// touching any of them.  The other RANSAC units cannot affect this kernel.
// hyp layout: [prob][12][bmax] (structure of arrays), element 4a+b = R[a][b], 4a+3 = t[a]
// RN = ransac_n when it is known at compile time (10: the reference's value; the loops are unrolled and the sampled
// pairs stay in registers between the centroid and the covariance pass), 0 = read it from the argument and read the
// pairs again; inv_n = exact_div_recip(ransac_n)
template <int RN>
__attribute__((amdgpu_waves_per_eu(5, 5)))
__global__ __launch_bounds__(256) void k_ransac_hyp(const RansacProb* probs,
                                                    const float4* __restrict__ pair32, int it0,
                                                    int bcount, int bmax, int ransac_n, double inv_n,
                                                    uint64_t seed,
                                                    const int32_t* __restrict__ xcd_prob, const XcdTab xcd_tab,
                                                    int slots, int tiles, int force_jacobi,
                                                    double* __restrict__ hyp,
                                                    // prefilter rows of the chunk (A16 != nullptr): pf_emit_row
                                                    const unsigned* __restrict__ pf_stat, const double* __restrict__ pf_sums,
                                                    double thr2, double tcap, _Float16* __restrict__ A16,
                                                    float* __restrict__ c_h, int32_t* __restrict__ cnt_zero) {
  // 1-D grid dealt round-robin to the XCDs: XCD x samples only the problems xcd_prob[x][.], whose
  // correspondences then stay in that XCD's L2 (the sampling is a random gather of 24-B rows)
  const int xcd = blockIdx.x & 7;
  const int item = blockIdx.x >> 3;
  const int slot = item / tiles;
  const int p = xcd_problem(xcd_prob, xcd_tab, xcd * slots + slot);
  if (p < 0) return;
  const int h = (item - slot * tiles) * blockDim.x + threadIdx.x;
  if (h >= bcount) return;
  // the prefilter behind this kernel adds the partial counts of its pair-range splits with atomics: cleared here
  if (cnt_zero) cnt_zero[(int64_t)p * bmax + h] = 0;
  const RansacProb pr = prob_view(probs, p);
  const int itr = it0 + h;
  if (pr.done || itr >= pr.est_k) return;
  const uint32_t m = (uint32_t)pr.m;
  double cs_[3] = {0, 0, 0}, ct_[3] = {0, 0, 0};
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  if (RN > 0) {
    // the ten samples stay in registers between the two passes AS THE f32 VALUES THEY WERE LOADED AS (60 registers)
    float pa[RN > 0 ? RN : 1][6];
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int64_t i = pr.off + rng_index(seed, (uint64_t)itr, (uint64_t)j, m);
      const float4 a = pair32[2 * i], b = pair32[2 * i + 1];  // one 32-B sector
      pa[j][0] = a.x; pa[j][1] = a.y; pa[j][2] = a.z; pa[j][3] = a.w; pa[j][4] = b.x; pa[j][5] = b.y;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        cs_[c] += (double)pa[j][c];
        ct_[c] += (double)pa[j][3 + c];
      }
    }
    centroid_div(cs_, ct_, (double)RN, inv_n);
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      // opaque copies, so that the values are converted to f64 AGAIN here: the compiler otherwise keeps the sixty f64
      // conversions of the first pass alive (120 registers; the kernel then held 164 and ran at three waves per SIMD).
      // Reading the sectors a second time instead was measured slower than the parent (113 vs 105 us per launch).
#pragma unroll
      for (int c = 0; c < 6; ++c) asm volatile("" : "+v"(pa[j][c]));
      const double ds[3] = {(double)pa[j][0] - cs_[0], (double)pa[j][1] - cs_[1], (double)pa[j][2] - cs_[2]};
      const double dt[3] = {(double)pa[j][3] - ct_[0], (double)pa[j][4] - ct_[1], (double)pa[j][5] - ct_[2]};
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) S[x][y] = fma(ds[x], dt[y], S[x][y]);
    }
  } else {
    for (int j = 0; j < ransac_n; ++j) {
      const int64_t i = pr.off + rng_index(seed, (uint64_t)itr, (uint64_t)j, m);
      const float4 a = pair32[2 * i], b = pair32[2 * i + 1];  // one 32-B sector
      cs_[0] += (double)a.x;
      cs_[1] += (double)a.y;
      cs_[2] += (double)a.z;
      ct_[0] += (double)a.w;
      ct_[1] += (double)b.x;
      ct_[2] += (double)b.y;
    }
    centroid_div(cs_, ct_, (double)ransac_n, inv_n);
    for (int j = 0; j < ransac_n; ++j) {
      const int64_t i = pr.off + rng_index(seed, (uint64_t)itr, (uint64_t)j, m);
      const float4 a = pair32[2 * i], b = pair32[2 * i + 1];
      const double ds[3] = {(double)a.x - cs_[0], (double)a.y - cs_[1], (double)a.z - cs_[2]};
      const double dt[3] = {(double)a.w - ct_[0], (double)b.x - ct_[1], (double)b.y - ct_[2]};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) S[a][b] = fma(ds[a], dt[b], S[a][b]);
    }
  }
  double N[4][4], V[4][4];
  N[0][0] = S[0][0] + S[1][1] + S[2][2];
  N[0][1] = S[1][2] - S[2][1];
  N[0][2] = S[2][0] - S[0][2];
  N[0][3] = S[0][1] - S[1][0];
  N[1][1] = S[0][0] - S[1][1] - S[2][2];
  N[1][2] = S[0][1] + S[1][0];
  N[1][3] = S[2][0] + S[0][2];
  N[2][2] = -S[0][0] + S[1][1] - S[2][2];
  N[2][3] = S[1][2] + S[2][1];
  N[3][3] = -S[0][0] - S[1][1] + S[2][2];
  N[1][0] = N[0][1];
  N[2][0] = N[0][2];
  N[3][0] = N[0][3];
  N[2][1] = N[1][2];
  N[3][1] = N[1][3];
  N[3][2] = N[2][3];
  double qv[4];
  if (force_jacobi || !horn_qcp(S, N, qv)) {
    // rare (ill-separated largest eigenvalue): the lanes that need it run the Jacobi solver
    jacobi4(N, V);
    // eigenvector of the largest eigenvalue (ties -> lowest index), selected without dynamic indexing
    double best = N[0][0];
    qv[0] = V[0][0]; qv[1] = V[1][0]; qv[2] = V[2][0]; qv[3] = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
      if (N[c][c] > best) {
        best = N[c][c];
        qv[0] = V[0][c];
        qv[1] = V[1][c];
        qv[2] = V[2][c];
        qv[3] = V[3][c];
      }
    }
  }
  double qw = qv[0], qx = qv[1], qy = qv[2], qz = qv[3];
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw = qw / qn;
  qx = qx / qn;
  qy = qy / qn;
  qz = qz / qn;
  double R[3][3];
  R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  R[0][1] = 2.0 * (qx * qy - qw * qz);
  R[0][2] = 2.0 * (qx * qz + qw * qy);
  R[1][0] = 2.0 * (qx * qy + qw * qz);
  R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
  R[1][2] = 2.0 * (qy * qz - qw * qx);
  R[2][0] = 2.0 * (qx * qz - qw * qy);
  R[2][1] = 2.0 * (qy * qz + qw * qx);
  R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
  double* o = hyp + ((int64_t)p * 12) * bmax + h;
  double tv[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t = ct_[a] - (R[a][0] * cs_[0] + R[a][1] * cs_[1] + R[a][2] * cs_[2]);
    tv[a] = t;
    o[(int64_t)(4 * a + 0) * bmax] = R[a][0];
    o[(int64_t)(4 * a + 1) * bmax] = R[a][1];
    o[(int64_t)(4 * a + 2) * bmax] = R[a][2];
    o[(int64_t)(4 * a + 3) * bmax] = t;
  }
  if (A16) pf_emit_row(pr, p, h, bmax, R, tv, pf_stat, pf_sums, thr2, tcap, A16, c_h);
}

void ransac_launch_pack(const RansacIn& in, const float* src, const float* tgt, hipStream_t s) {
  hipLaunchKernelGGL(k_ransac_pack, dim3((unsigned)ceil_div(in.tot1, 256)), dim3(256), 0, s, src, tgt, in.tot1, in.pk,
                     in.pair32);
}

void ransac_launch_hyp(const RansacIn& in, const Front& f, int ransac_n, uint64_t seed, int force_jacobi, double* hyp,
                       const unsigned* pf_stat, const double* pf_sums, double thr2, double tcap, _Float16* A16, float* c_h,
                       int32_t* cnt_zero, hipStream_t s) {
  const int htiles = (f.b + 255) / 256;
  const auto kernel = ransac_n == 10 ? k_ransac_hyp<10> : k_ransac_hyp<0>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(8 * f.pslots * htiles)), dim3(256), 0, s, in.probs, in.pair32, f.it0, f.b, BMAX,
                     ransac_n, exact_div_recip((double)ransac_n), seed, f.xcd_prob, f.xtab, f.pslots, htiles, force_jacobi, hyp,
                     pf_stat, pf_sums, thr2, tcap, A16, c_h, cnt_zero);
}
}  // namespace cs
