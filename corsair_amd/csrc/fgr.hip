// Fast Global Registration on a fixed correspondence list: cs_fgr_batch, the second correspondence estimator
// beside cs_ransac_batch.  The specification is the comment of the entry in include/corsair_hip.h; tests/fgr_ref.py restates
// it bit for bit.  One launch, k_fgr: ONE persistent workgroup of FGR_BLOCK lanes per problem goes through
//   frame      the exact f32 bounding boxes of both sides (midpoints cs, ct) and the radius g of the normalised frame
//   table      (q^, p^) of all m pairs, f64, one 48-byte row per pair in global scratch: the divisions are made once
//   tuple test trials in chunks of FGR_BLOCK x 4 (four consecutive trials per lane, three row gathers each), an ordered
//              compaction of the passing ones (wave prefix by shuffles, the wave totals through LDS) until max_tuple are
//              kept; their rows are copied to the problem's working list.  With the test off the table IS the list
//   line process  iteration_number rounds: lanes stride over the working list and pose, weigh and sum 16 fixed-point terms
//              per pair; wave shuffle, the waves through LDS, lane 0 solves the 6x6 system (icp_update.h) and hands the
//              new T and mu back through LDS
//   result     the de-normalised transform, inliers and rmse of it over all pairs of the problem.
// Nothing waits on the host and there is no float atomic (no atomic at all: a problem lives in one workgroup).
//
// Fixed-point sums.  At the start |q^|, |p^| <= 1 (g is the largest distance from the midpoints).  T^ = (R^, t^) with R^ a
// product of exactly normalised Cayley rotations, so |q| = |R^ q^ + t^| <= 1 + |t^|.  A translation that serves the list
// keeps some posed pair near its target: |t^| <= 2 + |e|, and the budget below is |q| <= 4 (|t^| <= 3), beyond which no
// pair of the list lies within 1 of its target and the estimate is meaningless anyway.  With 0 < w <= 1, |e| <= |q| + 1 <= 5
// and n working pairs, n <= 2^eN:
//   sum w              w <= 1                       scale 2^(61 - eN)
//   sum w q_c          |q_c| <= 4 = 2^2             scale 2^(61 - eN - 2)
//   sum (w q_a) q_b    |q_a q_b| <= 16 = 2^4        scale 2^(61 - eN - 4)
//   sum w e_c          |e_c| <= 5 < 2^3             scale 2^(61 - eN - 3)
//   sum w (q x e)_c    |q x e| <= 20 < 2^5          scale 2^(61 - eN - 5)
// Rounding to nearest is monotone, so a rounded product of bounded factors obeys the bound of the exact one up to the
// representable bound itself; every scaled term is at most 2^(61 - eN) and every sum at most 2^61 in magnitude, a factor of
// two inside the 2^62 that the restatement asserts.  Every scaled term is clamped to +-2^(61 - eN) before the conversion
// (NaN becomes the lower clamp), so the sums are defined and the same in every run for ANY T^, also one outside the
// budget; such sums carry no meaning and the pivot rule or the finiteness test of T^ ends the problem.  The smallest
// scale, 2^(61 - 31 - 5), still resolves 2^-25 per term at 2^31 pairs; a 3000-pair working list has 2^-44.
// The exponents lie in [25, 61]: normal f64 powers of two, exact scaling.
//
// Budget (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): k_fgr 223 VGPRs, no AGPRs, no scratch,
// 1776 bytes of LDS, 512 lanes = 8 waves: two waves per SIMD, one workgroup per CU, which is all a batch of 100 - 300 problems
// on 256 CUs can use anyway.  512 lanes rather than 256 halve the trials and the pairs per lane; 1024 would need 128 VGPRs.
#include <math.h>

#include <algorithm>
#include <vector>

#include "icp_update.h"
#include "nn_common.h"

namespace cs {
namespace {

constexpr int FGR_BLOCK = 512;              // lanes of the workgroup of a problem
constexpr int FGR_NW = FGR_BLOCK / 64;      // its waves
constexpr int FGR_TPL = 4;                  // trials per lane and chunk
constexpr int FGR_NSUM = 16;                // sum w, w q (3), (w q_a) q_b (6 upper), w e (3), w q x e (3)
constexpr int FGR_MIN_PAIRS = 10;           // [O3D-knowledge] Open3D answers with the identity below ten pairs
constexpr int FGR_SUM_BITS = 61;
constexpr int FGR_MAX_TUPLE_CAP = 65536;    // 3 * 65536 working pairs = 9 MiB of scratch per problem

struct FgrProb {
  int64_t off;    // first pair of the problem
  int64_t t0;     // first row of its table of normalised pairs
  int64_t w0;     // first row of its working list (tuple test on)
  int32_t m;      // pairs
};
struct FgrParams {
  double thr2;            // max_corr * max_corr
  int thr_ex;             // thr2 = f * 2^thr_ex, 0.5 <= f < 1
  double mu_floor, division_factor, tuple_scale;
  int iteration_number, tuple_test, max_tuple;
  uint64_t seed;
};

__device__ __forceinline__ long long fgr_fix(double v, double scale, double clamp) {
  const double x = fmin(fmax(v * scale, -clamp), clamp);   // (NaN becomes -clamp)
  return (long long)x;                                     // truncates toward zero
}

// one row of the table: (q^, p^) of a pair, 48 bytes, 16-byte aligned
struct FgrRow {
  double2 a, b, c;   // (q^x, q^y), (q^z, p^x), (p^y, p^z)
};

__device__ __forceinline__ double fgr_len(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ __launch_bounds__(FGR_BLOCK) void k_fgr(const FgrProb* __restrict__ probs, const float* __restrict__ src,
                                             const float* __restrict__ tgt, FgrParams prm, FgrRow* table, FgrRow* wlist,
                                             float* __restrict__ T32, double* __restrict__ T64,
                                             int32_t* __restrict__ inliers, double* __restrict__ rmse,
                                             int32_t* __restrict__ iters_out, int32_t* __restrict__ ntuple) {
  __shared__ float box_s[FGR_NW][12];
  __shared__ double g_s[FGR_NW];
  __shared__ int nan_s[FGR_NW];
  __shared__ int wtot[FGR_NW];
  __shared__ unsigned long long part[FGR_NW][FGR_NSUM];
  __shared__ double T_s[12];
  __shared__ double mu_s;
  __shared__ int stop_s;
  __shared__ unsigned long long ev_s[FGR_NW][2];
  const FgrProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = pr.m;
  const float* __restrict__ S = src + pr.off * 3;
  const float* __restrict__ Q = tgt + pr.off * 3;

  // ---- frame: the exact f32 boxes of both sides --------------------------------------------------------------------
  float mn[6], mx[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    mn[c] = INFINITY;
    mx[c] = -INFINITY;
  }
  for (int i = tid; i < m; i += FGR_BLOCK) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = S[3 * (int64_t)i + c], b = Q[3 * (int64_t)i + c];
      mn[c] = fminf(mn[c], a);
      mx[c] = fmaxf(mx[c], a);
      mn[3 + c] = fminf(mn[3 + c], b);
      mx[3 + c] = fmaxf(mx[3 + c], b);
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      mn[c] = fminf(mn[c], __shfl_xor(mn[c], off));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off));
    }
    if (lane == 0) {
      box_s[wave][c] = mn[c];
      box_s[wave][6 + c] = mx[c];
    }
  }
  __syncthreads();
  double cen[2][3];   // cs, ct
  bool bad = m == 0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    float lo = box_s[0][c], hi = box_s[0][6 + c];
#pragma unroll
    for (int w = 1; w < FGR_NW; ++w) {
      lo = fminf(lo, box_s[w][c]);
      hi = fmaxf(hi, box_s[w][6 + c]);
    }
    cen[c / 3][c % 3] = 0.5 * ((double)lo + (double)hi);
    bad = bad || !(isfinite(lo) && isfinite(hi));
  }
  // g^2 = the largest squared distance of a row from its side's midpoint; a NaN distance spoils the frame
  double d2max = 0.0;
  int has_nan = 0;
  if (!bad) {   // (block-uniform: every lane read the same twelve numbers)
    for (int i = tid; i < m; i += FGR_BLOCK) {
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const float* r = (side ? Q : S) + 3 * (int64_t)i;
        const double dx = (double)r[0] - cen[side][0], dy = (double)r[1] - cen[side][1], dz = (double)r[2] - cen[side][2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 != d2) has_nan = 1;
        d2max = fmax(d2max, d2);
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) d2max = fmax(d2max, __shfl_xor(d2max, off));
  has_nan = __any(has_nan);
  if (lane == 0) {
    g_s[wave] = d2max;
    nan_s[wave] = has_nan;
  }
  __syncthreads();
  double g2 = g_s[0];
  int any_nan = nan_s[0];
#pragma unroll
  for (int w = 1; w < FGR_NW; ++w) {
    g2 = fmax(g2, g_s[w]);
    any_nan |= nan_s[w];
  }
  const double g = sqrt(g2);
  bad = bad || any_nan || !(g > 0.0) || !isfinite(g);

  // ---- table of normalised pairs, working list -------------------------------------------------------------------------
  FgrRow* N = table + pr.t0;
  FgrRow* Wc = wlist + pr.w0;     // 3 max_tuple rows (tuple test on)
  int kept = 0;
  if (!bad) {
    for (int i = tid; i < m; i += FGR_BLOCK) {
      const float* a = S + 3 * (int64_t)i;
      const float* b = Q + 3 * (int64_t)i;
      FgrRow r;
      r.a = make_double2(((double)a[0] - cen[0][0]) / g, ((double)a[1] - cen[0][1]) / g);
      r.b = make_double2(((double)a[2] - cen[0][2]) / g, ((double)b[0] - cen[1][0]) / g);
      r.c = make_double2(((double)b[1] - cen[1][1]) / g, ((double)b[2] - cen[1][2]) / g);
      N[i] = r;
    }
    __syncthreads();   // the rows are read by other lanes from here on (block-uniform branch)
    if (prm.tuple_test) {
      const int64_t n_trial = 100 * (int64_t)m;
      const double ts = prm.tuple_scale;
      for (int64_t base = 0; base < n_trial && kept < prm.max_tuple; base += FGR_BLOCK * FGR_TPL) {
        unsigned mask = 0;
#pragma unroll
        for (int k = 0; k < FGR_TPL; ++k) {
          const int64_t t = base + tid * FGR_TPL + k;
          if (t < n_trial) {
            FgrRow r[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) r[j] = N[rng_index(prm.seed, (uint64_t)t, (uint64_t)j, (uint32_t)m)];
            bool pass = true;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              const FgrRow &u = r[j], &v = r[j == 2 ? 0 : j + 1];
              const double ls = fgr_len(u.a.x, u.a.y, u.b.x, v.a.x, v.a.y, v.b.x);
              const double lt = fgr_len(u.b.y, u.c.x, u.c.y, v.b.y, v.c.x, v.c.y);
              pass = pass && (ls * ts < lt) && (lt * ts < ls);
            }
            if (pass) mask |= 1u << k;
          }
        }
        // ordered compaction: lanes hold consecutive trials, so trial order = (wave, lane, k)
        const int cnt = __popc(mask);
        int inc = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int v = __shfl_up(inc, off);
          if (lane >= off) inc += v;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int rank = kept + inc - cnt, total = 0;
#pragma unroll
        for (int w = 0; w < FGR_NW; ++w) {
          if (w < wave) rank += wtot[w];
          total += wtot[w];
        }
#pragma unroll 1
        for (int k = 0; k < FGR_TPL; ++k) {
          if (!((mask >> k) & 1u)) continue;
          if (rank < prm.max_tuple) {
            const int64_t t = base + tid * FGR_TPL + k;
#pragma unroll 1
            for (int j = 0; j < 3; ++j)   // row 3 rank + j < 3 max_tuple
              Wc[3 * (int64_t)rank + j] = N[rng_index(prm.seed, (uint64_t)t, (uint64_t)j, (uint32_t)m)];
          }
          ++rank;
        }
        kept = min(kept + total, prm.max_tuple);   // block-uniform
        __syncthreads();                           // wtot is rewritten by the next chunk
      }
    }
  }
  const FgrRow* W = prm.tuple_test ? Wc : N;
  const int n_work = bad ? 0 : (prm.tuple_test ? 3 * kept : m);
  const bool solve = !bad && n_work >= FGR_MIN_PAIRS;

  // ---- line process ------------------------------------------------------------------------------------------------
  const int eN = n_work <= 1 ? 0 : 32 - __clz(n_work - 1);   // n_work <= 2^eN
  const double clamp = ldexp(1.0, FGR_SUM_BITS - eN);
  const double sc_w = clamp, sc_q = ldexp(1.0, FGR_SUM_BITS - eN - 2), sc_qq = ldexp(1.0, FGR_SUM_BITS - eN - 4),
               sc_e = ldexp(1.0, FGR_SUM_BITS - eN - 3), sc_x = ldexp(1.0, FGR_SUM_BITS - eN - 5);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) T_s[i] = (i % 5 == 0) ? 1.0 : 0.0;
    mu_s = 1.0;
    stop_s = solve ? 0 : 1;
  }
  __syncthreads();   // (also: the working list written above is visible to the whole workgroup)
  int n_upd = 0;     // lane 0's count of applied updates
  for (int itr = 0; itr < prm.iteration_number; ++itr) {
    if (stop_s) break;   // block-uniform: written before the barrier that ended the previous round
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = T_s[i];
    const double mu = mu_s;
    long long acc[FGR_NSUM];
#pragma unroll
    for (int k = 0; k < FGR_NSUM; ++k) acc[k] = 0;
    for (int slot = tid; slot < n_work; slot += FGR_BLOCK) {
      const FgrRow row = W[slot];
      const double qh[3] = {row.a.x, row.a.y, row.b.x}, ph[3] = {row.b.y, row.c.x, row.c.y};
      double q[3], e[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        q[c] = ((T[4 * c] * qh[0] + T[4 * c + 1] * qh[1]) + T[4 * c + 2] * qh[2]) + T[4 * c + 3];
        e[c] = q[c] - ph[c];
      }
      const double r2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
      const double w0 = mu / (r2 + mu);
      const double w = w0 * w0;
      const double wqv[3] = {w * q[0], w * q[1], w * q[2]};
      const double x[3] = {q[1] * e[2] - q[2] * e[1], q[2] * e[0] - q[0] * e[2], q[0] * e[1] - q[1] * e[0]};
      acc[0] += fgr_fix(w, sc_w, clamp);
      int at = 4;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        acc[1 + a] += fgr_fix(wqv[a], sc_q, clamp);
#pragma unroll
        for (int b = a; b < 3; ++b) acc[at++] += fgr_fix(wqv[a] * q[b], sc_qq, clamp);
        acc[10 + a] += fgr_fix(w * e[a], sc_e, clamp);
        acc[13 + a] += fgr_fix(w * x[a], sc_x, clamp);
      }
    }
#pragma unroll
    for (int k = 0; k < FGR_NSUM; ++k) {
      unsigned long long s = (unsigned long long)acc[k];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off);
      if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (tid == 0) {
      double s[FGR_NSUM];
#pragma unroll
      for (int k = 0; k < FGR_NSUM; ++k) {
        unsigned long long u = part[0][k];
#pragma unroll
        for (int w = 1; w < FGR_NW; ++w) u += part[w][k];
        const long long v = (long long)u;
        const double inv = k == 0 ? 1.0 / sc_w : k < 4 ? 1.0 / sc_q : k < 10 ? 1.0 / sc_qq : k < 13 ? 1.0 / sc_e : 1.0 / sc_x;
        s[k] = (double)v * inv;
      }
      // r = q + omega x q + t - p^: J = [-[q]x | I], A = sum w J^T J, b = sum w J^T e, A x = -b
      const double sw = s[0], qx = s[1], qy = s[2], qz = s[3];
      const double xx = s[4], xy = s[5], xz = s[6], yy = s[7], yz = s[8], zz = s[9];
      double A[6][6], bv[6], xv[6];
      A[0][0] = yy + zz; A[0][1] = -xy;     A[0][2] = -xz;
      A[1][1] = xx + zz; A[1][2] = -yz;     A[2][2] = xx + yy;
      A[0][3] = 0.0;     A[0][4] = -qz;     A[0][5] = qy;
      A[1][3] = qz;      A[1][4] = 0.0;     A[1][5] = -qx;
      A[2][3] = -qy;     A[2][4] = qx;      A[2][5] = 0.0;
      A[3][3] = sw;      A[3][4] = 0.0;     A[3][5] = 0.0;
      A[4][4] = sw;      A[4][5] = 0.0;     A[5][5] = sw;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) A[i][j] = A[j][i];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        bv[c] = s[13 + c];
        bv[3 + c] = s[10 + c];
      }
      bool ok = icp_chol_solve<6>(A, bv, xv);
      double Tn[12];
      if (ok) {
        double R[3][3];
        const double t[3] = {xv[3], xv[4], xv[5]};
        icp_quat_rotation(1.0, 0.5 * xv[0], 0.5 * xv[1], 0.5 * xv[2], R);
        icp_compose(R, t, T, Tn);
#pragma unroll
        for (int i = 0; i < 12; ++i) ok = ok && isfinite(Tn[i]);
      }
      if (ok) {
#pragma unroll
        for (int i = 0; i < 12; ++i) T_s[i] = Tn[i];
        ++n_upd;
        if (itr % 4 == 0 && mu > prm.mu_floor) mu_s = mu / prm.division_factor;
      } else {
        stop_s = 1;
      }
    }
    __syncthreads();
  }

  // ---- result ------------------------------------------------------------------------------------------------------
  __syncthreads();
  if (tid == 0) {
    double Tf[12];
    if (solve) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) Tf[4 * a + b] = T_s[4 * a + b];
        const double rc = (T_s[4 * a] * cen[0][0] + T_s[4 * a + 1] * cen[0][1]) + T_s[4 * a + 2] * cen[0][2];
        Tf[4 * a + 3] = (g * T_s[4 * a + 3] + cen[1][a]) - rc;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) Tf[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) T_s[i] = Tf[i];
  }
  __syncthreads();
  double R[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) R[i] = T_s[i];
  // inliers and squared error as cs_ransac_batch evaluates a hypothesis: residual2_f64's chain (ransac.h), strict threshold
  const int eM = m <= 1 ? 0 : 32 - __clz(m - 1);
  const double err_scale = ldexp(1.0, FGR_SUM_BITS - eM - prm.thr_ex);   // terms d2 * scale < 2^(61 - eM)
  unsigned long long cnt = 0, err = 0;
  for (int i = tid; i < m; i += FGR_BLOCK) {
    const float* a = S + 3 * (int64_t)i;
    const float* b = Q + 3 * (int64_t)i;
    const double sx = a[0], sy = a[1], sz = a[2];
    const double dx = fma(R[2], sz, fma(R[1], sy, fma(R[0], sx, R[3]))) - (double)b[0];
    const double dy = fma(R[6], sz, fma(R[5], sy, fma(R[4], sx, R[7]))) - (double)b[1];
    const double dz = fma(R[10], sz, fma(R[9], sy, fma(R[8], sx, R[11]))) - (double)b[2];
    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
    if (d2 < prm.thr2) {
      ++cnt;
      err += (unsigned long long)(d2 * err_scale);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    cnt += __shfl_down(cnt, off);
    err += __shfl_down(err, off);
  }
  if (lane == 0) {
    ev_s[wave][0] = cnt;
    ev_s[wave][1] = err;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long n = 0, se = 0;
#pragma unroll
    for (int w = 0; w < FGR_NW; ++w) {
      n += ev_s[w][0];
      se += ev_s[w][1];
    }
    const int64_t o = (int64_t)blockIdx.x * 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const double v = i < 12 ? R[i] : (i == 15 ? 1.0 : 0.0);
      T32[o + i] = (float)v;
      if (T64) T64[o + i] = v;
    }
    inliers[blockIdx.x] = (int32_t)n;
    rmse[blockIdx.x] = n > 0 ? sqrt(((double)se / err_scale) / (double)n) : 0.0;
    iters_out[blockIdx.x] = n_upd;
    ntuple[blockIdx.x] = prm.tuple_test ? kept : -1;
  }
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_fgr_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, int n_prob, double max_corr,
                 double mu_floor, double division_factor, int iteration_number, int tuple_test, double tuple_scale,
                 int max_tuple, uint64_t seed, float* d_T, double* d_T64, int32_t* d_inliers, double* d_rmse,
                 int32_t* d_iters, int32_t* d_ntuple, void* stream) {
  const char* name = "cs_fgr_batch";
  CS_REQUIRE(h_off, CS_ERR_INVALID, "%s: NULL offset table", name);
  CS_REQUIRE(n_prob >= 0, CS_ERR_INVALID, "%s: negative problem count", name);
  CS_REQUIRE(std::isfinite(max_corr) && max_corr > 0.0, CS_ERR_INVALID, "%s: max_corr must be positive and finite", name);
  CS_REQUIRE(std::isfinite(mu_floor) && mu_floor > 0.0, CS_ERR_INVALID, "%s: mu_floor must be positive and finite", name);
  CS_REQUIRE(division_factor > 1.0, CS_ERR_INVALID, "%s: division_factor must exceed 1", name);   // (NaN fails)
  CS_REQUIRE(tuple_scale > 0.0 && tuple_scale < 1.0, CS_ERR_INVALID, "%s: tuple_scale outside (0, 1)", name);
  CS_REQUIRE(max_tuple >= 1, CS_ERR_INVALID, "%s: max_tuple must be at least 1", name);
  CS_REQUIRE(iteration_number >= 0 && iteration_number <= 1000, CS_ERR_UNSUPPORTED,
             "%s: iteration_number outside [0, 1000]", name);
  CS_REQUIRE(max_tuple <= FGR_MAX_TUPLE_CAP, CS_ERR_UNSUPPORTED, "%s: max_tuple above %d", name, FGR_MAX_TUPLE_CAP);
  if (n_prob == 0) return CS_OK;
  CS_REQUIRE(d_T && d_inliers && d_rmse && d_iters && d_ntuple, CS_ERR_INVALID, "%s: NULL output", name);
  std::vector<FgrProb> probs(n_prob);
  int64_t slots = 0;
  double units = 0.0;
  for (int p = 0; p < n_prob; ++p) {
    const int64_t m = h_off[p + 1] - h_off[p];
    CS_REQUIRE(m >= 0 && h_off[p] >= 0, CS_ERR_INVALID, "%s: bad segment %d", name, p);
    CS_REQUIRE(m < (1LL << 31), CS_ERR_UNSUPPORTED, "%s: problem %d has 2^31 pairs or more", name, p);
    FgrProb& pr = probs[p];
    pr.off = h_off[p];
    pr.t0 = h_off[p] - h_off[0];
    pr.w0 = slots;
    pr.m = (int32_t)m;
    const int64_t cap = m == 0 ? 0 : (tuple_test ? 3 * (int64_t)max_tuple : m);   // rows of its working list
    if (tuple_test) slots += cap;
    units += 64.0 * (double)cap * (double)iteration_number;   // about 64 f64 operations per working pair and round
  }
  CS_REQUIRE(h_off[n_prob] == h_off[0] || (d_src && d_tgt), CS_ERR_INVALID, "%s: NULL pair array", name);
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<FgrProb> dprob;
  PoolBuf<FgrRow> table((size_t)(h_off[n_prob] - h_off[0]));   // the normalised pairs of every problem
  PoolBuf<FgrRow> wlist((size_t)slots);                        // the working lists the tuple test fills
  CS_REQUIRE(table.p && wlist.p, CS_ERR_HIP, "%s: scratch allocation failed", name);
  const int rc = upload(dprob, probs, s);
  if (rc) return rc;
  FgrParams prm;
  prm.thr2 = max_corr * max_corr;
  prm.thr_ex = 1024;
  if (std::isfinite(prm.thr2)) (void)frexp(prm.thr2, &prm.thr_ex);
  prm.thr_ex = std::max(prm.thr_ex, -900);   // keeps the error scale 2^(61 - eM - thr_ex) a normal f64 power of two
  prm.mu_floor = mu_floor;
  prm.division_factor = division_factor;
  prm.tuple_scale = tuple_scale;
  prm.iteration_number = iteration_number;
  prm.tuple_test = tuple_test ? 1 : 0;
  prm.max_tuple = max_tuple;
  prm.seed = seed;
  ProfScope prof("fgr", s, units);
  hipLaunchKernelGGL(k_fgr, dim3((unsigned)n_prob), dim3(FGR_BLOCK), 0, s, dprob.p, d_src, d_tgt, prm, table.p, wlist.p, d_T, d_T64,
                     d_inliers, d_rmse, d_iters, d_ntuple);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
