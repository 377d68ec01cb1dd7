// Batched ICP: point-to-point (cs_icp_batch), point-to-plane (cs_icp_plane_batch),
// point-to-plane with a robust kernel (cs_icp_plane_robust_batch), both estimations with an isotropic scale
// (cs_icp_scale_batch) and plane-to-plane, Generalized ICP (cs_icp_gicp_batch).  The specifications are the comments of the
// five entries in include/corsair_hip.h; tests/icp_ref.py, tests/icp_plane_ref.py, tests/icp_robust_ref.py,
// tests/icp_scale_ref.py and tests/gicp_ref.py restate them bit for bit.  The estimation is a compile-time parameter
// EST (0 = point, 1 = plane, 2 = plane with a per-pair weight, 3 = point + scale, 4 = plane + scale, 5 = plane-to-plane) of
// the sums at the end of the association kernels and of the update; pose chain, association, evaluation, loop and stop rule
// are one code.  The rigid instantiations are what they were before the others existed: kernel = L2 runs EST = 1, nothing of
// EST = 3 / 4 is launched unless cs_icp_scale_batch is called and nothing of EST = 5 unless cs_icp_gicp_batch is.
//
// One call = one target preparation + (max_iter + 1) rounds, all enqueued without a host wait:
//   k_icp_frame    per problem: the bounding box of its target segment (exact min / max), the origin and the
//                  power-of-two scales of its fixed-point sums
//   chamfer_pack16 the f16 hi / lo image, |S t|^2 and the float4 rows of every target, once per call
//   round r:       k_icp_f16 (+ k_icp_exact for the workgroups it flags) or k_icp_exact alone -- association of the posed
//                  ORIGINAL sources under the current T, 17 (point), 29 (plane), 30 (weighted plane), 18 (point + scale),
//                  37 (plane + scale) or 30 (GICP) order-free 64-bit integer sums per problem; k_icp_step -- one lane per problem:
//                  fitness / rmse of that association, the stop rule, Horn's fit (point) or the 6x6 / 7x7 normal equations
//                  by Cholesky (plane) from the sums, T <- U T.
// A problem that has stopped raises its device flag; its workgroups leave on it in every later round.
#include <math.h>

#include <algorithm>

#include "horn.h"
#include "icp_update.h"
#include "nn_common.h"

namespace cs {
namespace {

constexpr int ICP_ST = 4 * 32 * CHF_NG;   // sources per workgroup (both association kernels)
constexpr int ICP_TT = 512;               // target rows per LDS stage of the exact kernel
constexpr int ICP_NSUM = 17;              // count, sum p' (3), sum q' (3), sum p' q'^T (9), sum d^2
constexpr int ICP_NSUM_PLANE = 29;        // count, sum J_i J_j (i <= j, 21), sum J_i r (6), sum d^2
constexpr int ICP_NSUM_ROBUST = 30;       // the 29 plane sums (27 of them weighted) + sum w
constexpr int ICP_NSUM_POINT_S = 18;      // the 17 point sums + sum p'.p'
constexpr int ICP_NSUM_PLANE_S = 37;      // count, sum J_i J_j (i <= j, 28), sum J_i r (7), sum d^2
constexpr int ICP_NSUM_GICP = 30;         // count, sum (J^T W J)_ij (i <= j, 21), sum (J^T W e)_i (6), sum d^2, sum e.We
constexpr int ICP_POINT = 0, ICP_PLANE = 1, ICP_ROBUST = 2, ICP_POINT_S = 3, ICP_PLANE_S = 4, ICP_GICP = 5;
// the estimations with a target normal array, the plane frame and the 6x6 / 7x7 normal equations: GICP's 30 sums have the
// plane layout (count, 21 matrix entries, 6 right-hand sides, d^2) with one more sum behind it
template <int EST>
constexpr bool icp_is_plane() {
  return EST == ICP_PLANE || EST == ICP_ROBUST || EST == ICP_PLANE_S || EST == ICP_GICP;
}
template <int EST>
constexpr bool icp_has_scale() {
  return EST == ICP_POINT_S || EST == ICP_PLANE_S;
}
template <int EST>
constexpr int icp_nsum() {
  return EST == ICP_ROBUST    ? ICP_NSUM_ROBUST
         : EST == ICP_GICP    ? ICP_NSUM_GICP
         : EST == ICP_PLANE   ? ICP_NSUM_PLANE
         : EST == ICP_POINT_S ? ICP_NSUM_POINT_S
         : EST == ICP_PLANE_S ? ICP_NSUM_PLANE_S
                              : ICP_NSUM;
}
// columns of the plane Jacobian: (a, n) and, with a scale, p'.n
template <int EST>
constexpr int icp_nj() {
  return EST == ICP_PLANE_S ? 7 : 6;
}
// sum d^2 is the 17th of both point layouts and the one after the J_i r sums of every plane layout (the 29th / 37th)
template <int EST>
constexpr int icp_d2_at() {
  return icp_is_plane<EST>() ? icp_nj<EST>() * (icp_nj<EST>() + 1) / 2 + icp_nj<EST>() + 1 : ICP_NSUM - 1;
}
// a rotational column of the plane Jacobian (bounded by 2 M) as opposed to a translational one (bounded by 1)
__host__ __device__ constexpr bool icp_rot_col(int i) { return i < 3 || i == 6; }

// Fixed-point sums.  A kept pair has |p - q|^2 < max_dist^2 and q inside the bounding box of the target segment, so
// relative to the box's midpoint o every coordinate obeys |q'_c| <= h_c and |p'_c| <= h_c + max_dist, h = the box's
// half-extent.  With M = max_c h_c + max_dist < 2^eM (eM from frexp, clamped to [ICP_EM_MIN, ICP_EM_MAX]) and
// n_src <= 2^eN:
//   linear terms    |p'_c|, |q'_c|          < 2^eM      scale 2^s1, s1 = 61 - eN - eM      -> each < 2^(61 - eN)
//   quadratic terms |p'_a q'_b|, d^2        < 2^(2 eM)  scale 2^s2, s2 = 61 - eN - 2 eM    -> each < 2^(61 - eN)
// and a sum of at most 2^eN of them stays below 2^61 in magnitude: a factor of two inside 2^62, which also covers the
// rounding of p, of the subtraction of o and of the product (each relative 2^-53).  Every scaled term is clamped to
// +-2^(61 - eN) before the conversion, so the bound holds for ANY input (a box that is not finite, an absurd max_dist):
// those sums then carry no meaning, but they are defined and the same in every run.
// eM in [-100, 400] and eN in [0, 31] keep both scales and their inverses normal f64 powers of two (s1 in [-370, 161],
// s2 in [-770, 261]), so scaling is exact.
//
// Point-to-plane (EST = 1).  Per kept pair n = the widened normal row of the matched target, e = p - q, r = e . n,
// a = p' x n, J = (a, n).  With |p'_c| <= M < 2^eM as above, |n_c| <= 1 (a unit normal cast to f32) and |e| < max_dist <= M:
//   |a_c| = |p'_b n_c - p'_c n_b| <= 2 M,  |r| <= |e| |n| < max_dist  -- each up to a few roundings of relative 2^-53
//   (and of 2^-24 in |n| for a normal normalised in f32), for which every class below gets ONE extra bit:
//   rot x rot     |a_i a_j| <= 4 M^2        < 2^(2 eM + 2)   scale 2^(61 - eN - 2 eM - 3)
//   rot x trans   |a_i n_j| <= 2 M          < 2^(eM + 1)     scale 2^(61 - eN - eM - 2)
//   trans x trans |n_i n_j| <= 1                             scale 2^(61 - eN - 1)
//   rot x r       |a_i r|   <  2 M max_dist < 2^(2 eM + 1)   scale 2^(61 - eN - 2 eM - 2)
//   trans x r     |n_i r|   <  max_dist     < 2^eM           scale 2^(61 - eN - eM - 1)
// so every scaled term is below 2^(61 - eN) and every sum below 2^61, as for the point sums; d^2 keeps the scale 2^s2.
// The clamp makes that hold for ANY normals a caller passes (length 10^3, NaN): such sums are defined, not meaningful.
// The exponents stay inside [-773, 260]: normal f64 powers of two, exact scaling.
//
// Weighted plane sums (EST = 2).  Each of the 27 rounded products is multiplied by the pair's weight w before it is scaled.
// 0 <= w <= 1 for every kernel below (a NaN weight is replaced by 0) and rounding to nearest is monotone, so
// |fl(x w)| <= |x|: no weighted term is larger than the unweighted term bounded above.  The 30th sum adds I(w 2^(61 - eN)),
// at most 2^eN terms of at most 2^(61 - eN).  Nothing leaves 2^61; count and d^2 are not weighted.
//
// Point + scale (EST = 3).  The 18th sum is p'.p' = fma(p'_z, p'_z, fma(p'_y, p'_y, p'_x p'_x)) <= 3 M^2 < 2^(2 eM + 2):
// scale 2^(61 - eN - 2 eM - 2), two bits below s2, so each term stays below 2^(61 - eN) (exponent inside [-772, 259]).
//
// Plane + scale (EST = 4).  The seventh column J_6 = p'.n has |J_6| <= |p'| |n| <= sqrt(3) M < 2 M: bounded like a
// rotational column a_c, so J_6 J_6 and a_i J_6 join the class rot x rot, n_i J_6 the class rot x trans and J_6 r the class
// rot x r; their bounds are those above and no new scale is needed.
//
// Plane-to-plane, GICP (EST = 5).  Per kept pair W = Mc^-1 is symmetric with eigenvalues in [1/2, 1/(2 eps)], so
// |W_ij| <= |W|_2 <= 1/(2 eps) <= 2^eW (eW in [-1, 9] for eps in [2^-10, 1]).  With |p'_c| <= M, |p'| <= sqrt(3) M, and
// |e| < max_dist <= M:
//   trans x trans |W_ij|                  <= 2^eW
//   rot x trans   |K_ij| = |(p' x w_j)_i| <= |p'| |w_j| <= sqrt(3) M 2^eW            < 2^(eM + 1 + eW)
//   rot x rot     |(p' x k_i)_j|          <= |p'| |[p']x W|_2 <= 3 M^2 2^eW          < 2^(2 eM + 2 + eW)
//   trans x e     |u_i| <= |W e|          <  2^eW max_dist                           < 2^(eM + eW)
//   rot x e       |(p' x u)_i|            <  sqrt(3) M 2^eW max_dist                 < 2^(2 eM + 1 + eW)
//   e . u         <= |e|^2 / (2 eps)                                                  < 2^(2 eM + eW)
// (w_j a column of W, k_i a row of K; the 3 x 3 contractions are inside the norm bounds, sqrt(3) < 2 and 3 < 4 are the bits
// they need).  These are the plane classes times 2^eW, so the five plane scales carry -eW and e . u shares the scale of
// rot x e, one bit above its bound; with the ONE extra bit per class for the roundings (the adjugate inverse has a relative
// error of a few 2^-53 / eps <= 2^-40) every scaled term is below 2^(61 - eN) and every sum below 2^61 for normals of any
// length, since the covariances are built from normalised directions.  The clamp keeps the sums defined for any input.
// The exponents stay inside [-782, 261]: normal f64 powers of two, exact scaling.
constexpr int ICP_EM_MIN = -100;
constexpr int ICP_EM_MAX = 400;
constexpr int ICP_SUM_BITS = 61;

struct IcpProb {
  int64_t s0, t0;   // first source / target row (global)
  int64_t c0;       // first entry of the problem in d_corr
  int32_t sn, tn;
};
struct IcpWork {
  int64_t s0;       // first source row of this workgroup (global)
  int64_t c0;       // its first entry in d_corr
  int32_t sn;       // source rows (<= ICP_ST)
  int32_t prob;
};
struct IcpFrame {
  double o[3];      // origin: midpoint of the target segment's bounding box
  double sc1, sc2;  // 2^s1, 2^s2
  double inv1, inv2;
  double clamp;     // 2^(61 - eN)
  double sc_pp, inv_pp;   // 2^(s2 - 2) and its inverse: the sum of p'.p' (EST = 3)
};
struct IcpPlaneFrame {   // 2^s and 2^-s of the five product classes of the plane sums
  double sc_rr, inv_rr, sc_rt, inv_rt, sc_tt, inv_tt, sc_rd, inv_rd, sc_td, inv_td;
};
struct IcpLoss {     // the robust kernel of EST = 2 (CS_ICP_KERNEL_*), unused otherwise
  int kind;
  double k;          // kernel_scale
};
struct IcpCriteria {
  double thr2;      // max_dist * max_dist
  double rel_fitness, rel_rmse;
  double scale_min, scale_max;   // the interval of the accumulated scale (EST = 3, 4)
};

// eW: the exponent the plane scales give up to GICP's weight matrix (0 for every other estimation)
__global__ __launch_bounds__(256) void k_icp_frame(const IcpProb* __restrict__ probs, const float* __restrict__ tgt,
                                                   double max_dist, IcpFrame* __restrict__ frame,
                                                   IcpPlaneFrame* __restrict__ pframe, int eW) {
  __shared__ float red[2][3][4];
  const IcpProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t j = tid; j < pr.tn; j += 256) {
    const float* t = tgt + (pr.t0 + j) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mn[c] = fminf(mn[c], t[c]);
      mx[c] = fmaxf(mx[c], t[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      mn[c] = fminf(mn[c], __shfl_xor(mn[c], off));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off));
    }
    if ((tid & 63) == 0) {
      red[0][c][tid >> 6] = mn[c];
      red[1][c][tid >> 6] = mx[c];
    }
  }
  __syncthreads();
  if (tid != 0) return;
  IcpFrame f;
  double hmax = 0.0;
  bool finite = pr.tn > 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double lo = (double)fminf(fminf(red[0][c][0], red[0][c][1]), fminf(red[0][c][2], red[0][c][3]));
    const double hi = (double)fmaxf(fmaxf(red[1][c][0], red[1][c][1]), fmaxf(red[1][c][2], red[1][c][3]));
    f.o[c] = 0.5 * (lo + hi);
    const double h = 0.5 * (hi - lo);
    hmax = fmax(hmax, h);
    finite = finite && isfinite(f.o[c]) && isfinite(h);
  }
  if (!finite) {
    f.o[0] = f.o[1] = f.o[2] = 0.0;
    hmax = 0.0;
  }
  const double M = hmax + max_dist;
  int eM = 0;
  (void)frexp(M, &eM);                       // M = m 2^eM, 0.5 <= m < 1: M < 2^eM
  if (!isfinite(M)) eM = ICP_EM_MAX;
  eM = min(max(eM, ICP_EM_MIN), ICP_EM_MAX);
  const int eN = pr.sn <= 1 ? 0 : 32 - __clz(pr.sn - 1);   // n_src <= 2^eN
  const int s1 = ICP_SUM_BITS - eN - eM, s2 = ICP_SUM_BITS - eN - 2 * eM;
  f.sc1 = ldexp(1.0, s1);
  f.inv1 = ldexp(1.0, -s1);
  f.sc2 = ldexp(1.0, s2);
  f.inv2 = ldexp(1.0, -s2);
  f.clamp = ldexp(1.0, ICP_SUM_BITS - eN);
  f.sc_pp = ldexp(1.0, s2 - 2);
  f.inv_pp = ldexp(1.0, -(s2 - 2));
  frame[blockIdx.x] = f;
  if (pframe) {
    const int b = ICP_SUM_BITS - eN - eW;
    IcpPlaneFrame g;
    g.sc_rr = ldexp(1.0, b - 2 * eM - 3);
    g.inv_rr = ldexp(1.0, -(b - 2 * eM - 3));
    g.sc_rt = ldexp(1.0, b - eM - 2);
    g.inv_rt = ldexp(1.0, -(b - eM - 2));
    g.sc_tt = ldexp(1.0, b - 1);
    g.inv_tt = ldexp(1.0, -(b - 1));
    g.sc_rd = ldexp(1.0, b - 2 * eM - 2);
    g.inv_rd = ldexp(1.0, -(b - 2 * eM - 2));
    g.sc_td = ldexp(1.0, b - eM - 1);
    g.inv_td = ldexp(1.0, -(b - eM - 1));
    pframe[blockIdx.x] = g;
  }
}

__device__ __forceinline__ long long icp_fix(double v, double scale, double clamp) {
  const double x = fmin(fmax(v * scale, -clamp), clamp);   // (NaN becomes -clamp: never reached by a kept pair)
  return (long long)x;                                     // truncates toward zero
}

// The weight of a kept pair from its point-to-plane residual r: [O3D-knowledge] Open3D's HuberLoss, CauchyLoss and
// TukeyLoss::Weight.  One IEEE operation each; the branch is uniform over the launch.
__device__ __forceinline__ double icp_weight(const IcpLoss& ls, double r) {
  const double a = fabs(r), k = ls.k;
  double w;
  if (ls.kind == CS_ICP_KERNEL_HUBER) {
    w = a <= k ? 1.0 : k / a;
  } else if (ls.kind == CS_ICP_KERNEL_CAUCHY) {
    const double q = r / k;
    w = 1.0 / (1.0 + q * q);
  } else if (ls.kind == CS_ICP_KERNEL_TUKEY) {
    if (!(a < k)) {
      w = 0.0;
    } else {
      const double q = r / k;
      const double e = 1.0 - q * q;
      w = e * e;
    }
  } else {
    w = 1.0;
  }
  return w == w ? w : 0.0;
}

// GICP: the gain g of the covariance C = I - g n n^T, g = (1 - eps) / (n . n), of a normal n.  A normal with a non-finite
// component, or with n . n zero or not finite, is replaced by 0 with g = 0: C = I.
__device__ __forceinline__ double icp_gicp_gain(double (&n)[3], double ome) {
  const double nn = fma(n[2], n[2], fma(n[1], n[1], n[0] * n[0]));
  if (!(isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]) && isfinite(nn) && nn > 0.0)) {
    n[0] = n[1] = n[2] = 0.0;
    return 0.0;
  }
  return ome / nn;
}

// p x v, the fma shape of the plane Jacobian's a = p' x n
__device__ __forceinline__ void icp_cross(const double (&p)[3], double v0, double v1, double v2, double (&out)[3]) {
  out[0] = fma(p[1], v2, -(p[2] * v1));
  out[1] = fma(p[2], v0, -(p[0] * v2));
  out[2] = fma(p[0], v1, -(p[1] * v0));
}

// The sums of one workgroup (17 point, 29 plane, 30 weighted plane, 18 point + scale, 37 plane + scale, 30 GICP): thread =
// one source (kept or not), wave shuffle, LDS across the four waves, then ONE 64-bit integer atomic per sum.  Integer
// addition: the same total in any order.  nrow: the normal row of the matched target (plane estimations, kept pairs only);
// srow, Tp, ome: the source's own normal row, the round's T and 1 - eps (GICP, kept pairs only).
template <int EST>
__device__ __forceinline__ void icp_block_sums(bool kept, double px, double py, double pz, float qx, float qy, float qz,
                                               double d2, const IcpFrame& fr, const IcpPlaneFrame* __restrict__ pfr,
                                               const float* __restrict__ nrow, const IcpLoss& loss,
                                               unsigned long long* __restrict__ sums,
                                               unsigned long long (*part)[icp_nsum<EST>()],
                                               const float* __restrict__ srow = nullptr,
                                               const double* __restrict__ Tp = nullptr, double ome = 0.0) {
  constexpr int NS = icp_nsum<EST>();
  const int tid = threadIdx.x;
  long long v[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) v[k] = 0;
  if constexpr (EST == ICP_GICP) {
    if (kept) {
      const IcpPlaneFrame g = *pfr;
      const double p[3] = {px - fr.o[0], py - fr.o[1], pz - fr.o[2]};
      const double e[3] = {px - (double)qx, py - (double)qy, pz - (double)qz};
      double nt[3] = {(double)nrow[0], (double)nrow[1], (double)nrow[2]};
      // m = A n_s, A the upper 3 x 3 block of T: icp_pose's chain without the translation
      const double sx = srow[0], sy = srow[1], sz = srow[2];
      double m[3] = {fma(Tp[0], sx, fma(Tp[1], sy, Tp[2] * sz)), fma(Tp[4], sx, fma(Tp[5], sy, Tp[6] * sz)),
                     fma(Tp[8], sx, fma(Tp[9], sy, Tp[10] * sz))};
      const double gt = icp_gicp_gain(nt, ome), gs = icp_gicp_gain(m, ome);
      const double at[3] = {gt * nt[0], gt * nt[1], gt * nt[2]}, as[3] = {gs * m[0], gs * m[1], gs * m[2]};
      // Mc = 2 I - g_t n_t n_t^T - g_s m m^T (symmetric, the six entries i <= j)
      const double M00 = fma(-as[0], m[0], fma(-at[0], nt[0], 2.0)), M01 = fma(-as[0], m[1], -(at[0] * nt[1])),
                   M02 = fma(-as[0], m[2], -(at[0] * nt[2])), M11 = fma(-as[1], m[1], fma(-at[1], nt[1], 2.0)),
                   M12 = fma(-as[1], m[2], -(at[1] * nt[2])), M22 = fma(-as[2], m[2], fma(-at[2], nt[2], 2.0));
      // W = adj(Mc) / det(Mc): cofactors, the determinant along the first row, ONE division
      const double c00 = fma(M11, M22, -(M12 * M12)), c01 = fma(M02, M12, -(M01 * M22)),
                   c02 = fma(M01, M12, -(M02 * M11)), c11 = fma(M00, M22, -(M02 * M02)),
                   c12 = fma(M01, M02, -(M00 * M12)), c22 = fma(M00, M11, -(M01 * M01));
      const double det = fma(M02, c02, fma(M01, c01, M00 * c00));
      const double id = 1.0 / det;
      double W[3][3];
      W[0][0] = c00 * id;
      W[0][1] = W[1][0] = c01 * id;
      W[0][2] = W[2][0] = c02 * id;
      W[1][1] = c11 * id;
      W[1][2] = W[2][1] = c12 * id;
      W[2][2] = c22 * id;
      double u[3], K[3][3], RR[3][3], bu[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) u[i] = fma(W[i][2], e[2], fma(W[i][1], e[1], W[i][0] * e[0]));
#pragma unroll
      for (int j = 0; j < 3; ++j) {   // column j of K = p' x column j of W
        double col[3];
        icp_cross(p, W[0][j], W[1][j], W[2][j], col);
        K[0][j] = col[0];
        K[1][j] = col[1];
        K[2][j] = col[2];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) icp_cross(p, K[i][0], K[i][1], K[i][2], RR[i]);   // row i = p' x row i of K
      icp_cross(p, u[0], u[1], u[2], bu);
      v[0] = 1;
      int at_ = 1;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
          const double val = j < 3 ? RR[i][j] : (i < 3 ? K[i][j - 3] : W[i - 3][j - 3]);
          const double sc = j < 3 ? g.sc_rr : (i < 3 ? g.sc_rt : g.sc_tt);
          v[at_++] = icp_fix(val, sc, fr.clamp);
        }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        v[22 + i] = icp_fix(bu[i], g.sc_rd, fr.clamp);
        v[25 + i] = icp_fix(u[i], g.sc_td, fr.clamp);
      }
      v[28] = icp_fix(d2, fr.sc2, fr.clamp);
      v[29] = icp_fix(fma(e[2], u[2], fma(e[1], u[1], e[0] * u[0])), g.sc_rd, fr.clamp);
    }
  } else if constexpr (icp_is_plane<EST>()) {
    constexpr int NJ = icp_nj<EST>(), NJJ = NJ * (NJ + 1) / 2;
    if (kept) {
      const IcpPlaneFrame g = *pfr;
      const double p[3] = {px - fr.o[0], py - fr.o[1], pz - fr.o[2]};
      const double n[3] = {(double)nrow[0], (double)nrow[1], (double)nrow[2]};
      const double e[3] = {px - (double)qx, py - (double)qy, pz - (double)qz};
      const double r = fma(e[2], n[2], fma(e[1], n[1], e[0] * n[0]));
      double J[NJ] = {fma(p[1], n[2], -(p[2] * n[1])), fma(p[2], n[0], -(p[0] * n[2])),
                      fma(p[0], n[1], -(p[1] * n[0])), n[0], n[1], n[2]};
      if constexpr (NJ == 7) J[6] = fma(p[2], n[2], fma(p[1], n[1], p[0] * n[0]));
      double w = 1.0;
      if constexpr (EST == ICP_ROBUST) w = icp_weight(loss, r);
      v[0] = 1;
      int at = 1;
#pragma unroll
      for (int i = 0; i < NJ; ++i)
#pragma unroll
        for (int j = i; j < NJ; ++j) {
          double prod = J[i] * J[j];   // rounded product (no contraction)
          if constexpr (EST == ICP_ROBUST) prod = prod * w;
          const bool ri = icp_rot_col(i), rj = icp_rot_col(j);
          const double sc = ri && rj ? g.sc_rr : (ri || rj ? g.sc_rt : g.sc_tt);
          v[at++] = icp_fix(prod, sc, fr.clamp);
        }
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        double prod = J[i] * r;
        if constexpr (EST == ICP_ROBUST) prod = prod * w;
        v[1 + NJJ + i] = icp_fix(prod, icp_rot_col(i) ? g.sc_rd : g.sc_td, fr.clamp);
      }
      v[1 + NJJ + NJ] = icp_fix(d2, fr.sc2, fr.clamp);
      if constexpr (EST == ICP_ROBUST) v[29] = icp_fix(w, fr.clamp, fr.clamp);
    }
  } else if (kept) {
    const double p[3] = {px - fr.o[0], py - fr.o[1], pz - fr.o[2]};
    const double q[3] = {(double)qx - fr.o[0], (double)qy - fr.o[1], (double)qz - fr.o[2]};
    v[0] = 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[1 + c] = icp_fix(p[c], fr.sc1, fr.clamp);
      v[4 + c] = icp_fix(q[c], fr.sc1, fr.clamp);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const double prod = p[a] * q[b];   // rounded product (no contraction)
        v[7 + 3 * a + b] = icp_fix(prod, fr.sc2, fr.clamp);
      }
    v[16] = icp_fix(d2, fr.sc2, fr.clamp);
    if constexpr (EST == ICP_POINT_S) v[17] = icp_fix(fma(p[2], p[2], fma(p[1], p[1], p[0] * p[0])), fr.sc_pp, fr.clamp);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    unsigned long long s = (unsigned long long)v[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off);
    if ((tid & 63) == 0) part[tid >> 6][k] = s;
  }
  __syncthreads();
  if (tid < NS) {
    const unsigned long long s = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    if (s) atomicAdd(&sums[tid], s);
  }
}

__device__ __forceinline__ void icp_pose(const double* __restrict__ Tp, const float* __restrict__ sp, double& px,
                                         double& py, double& pz) {
  const double x = sp[0], y = sp[1], z = sp[2];
  px = fma(Tp[0], x, fma(Tp[1], y, fma(Tp[2], z, Tp[3])));
  py = fma(Tp[4], x, fma(Tp[5], y, fma(Tp[6], z, Tp[7])));
  pz = fma(Tp[8], x, fma(Tp[9], y, fma(Tp[10], z, Tp[11])));
}

// Exhaustive association, one source per thread: the canonical chain over every target row in ascending order with a
// strict comparison, i.e. the minimum by (distance, row).  The whole path under CS_ICP_F16=0, and the recomputation of
// the workgroups k_icp_f16 flags.
template <int EST>
__global__ __launch_bounds__(256) void k_icp_exact(const IcpWork* __restrict__ work, const IcpProb* __restrict__ probs,
                                                   const float* __restrict__ src, const float* __restrict__ tgt,
                                                   const float* __restrict__ tnrm, const double* __restrict__ T,
                                                   const IcpFrame* __restrict__ frame,
                                                   const IcpPlaneFrame* __restrict__ pframe,
                                                   const int32_t* __restrict__ done, double thr2,
                                                   IcpLoss loss, unsigned long long* __restrict__ sums,
                                                   int32_t* __restrict__ corr,
                                                   const int32_t* __restrict__ only_flagged,
                                                   const float* __restrict__ snrm, double ome) {
  __shared__ float t_lds[ICP_TT * 3];
  __shared__ unsigned long long part[4][icp_nsum<EST>()];
  if (only_flagged && !only_flagged[blockIdx.x]) return;
  const IcpWork wk = work[blockIdx.x];
  if (done[wk.prob]) return;
  const IcpProb pr = probs[wk.prob];
  const int tid = threadIdx.x;
  const bool active = tid < wk.sn;
  double px = 0, py = 0, pz = 0;
  if (active) icp_pose(T + (int64_t)wk.prob * 16, src + (wk.s0 + tid) * 3, px, py, pz);
  double best = INFINITY;
  int bidx = -1;
  for (int tbase = 0; tbase < pr.tn; tbase += ICP_TT) {
    const int tcount = min(ICP_TT, pr.tn - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * 3; i += 256) t_lds[i] = tgt[(pr.t0 + tbase) * 3 + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) {
      const double dx = px - (double)t_lds[3 * j + 0];
      const double dy = py - (double)t_lds[3 * j + 1];
      const double dz = pz - (double)t_lds[3 * j + 2];
      const double d = fma(dz, dz, fma(dy, dy, dx * dx));
      if (d < best) {
        best = d;
        bidx = tbase + j;
      }
    }
  }
  const bool kept = active && bidx >= 0 && best < thr2;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (kept) {
    const float* tp = tgt + (pr.t0 + bidx) * 3;
    qx = tp[0];
    qy = tp[1];
    qz = tp[2];
  }
  if (corr && active) corr[wk.c0 + tid] = kept ? bidx : -1;
  icp_block_sums<EST>(kept, px, py, pz, qx, qy, qz, best, frame[wk.prob], icp_is_plane<EST>() ? pframe + wk.prob : nullptr,
                      icp_is_plane<EST>() && kept ? tnrm + (pr.t0 + bidx) * 3 : nullptr, loss,
                      sums + (int64_t)wk.prob * icp_nsum<EST>(), part,
                      EST == ICP_GICP && kept ? snrm + (wk.s0 + tid) * 3 : nullptr, T + (int64_t)wk.prob * 16, ome);
}

// The association on the f16 matrix cores: k_chamfer_f16's ranking (same image, same operand layout, same error budget;
// chamfer.hip and DESIGN 3 / 12) keeping (distance, row) of the evaluated rows and vouching STRICTLY: the result stands only
// when it lies below the smallest unevaluated tile minimum minus the error budget, so a row that was not evaluated can
// neither beat nor tie it.  A workgroup with a source that fails the test, or with coordinates outside the f16 range,
// adds nothing and raises its flag; k_icp_exact recomputes it.
template <int EST>
__global__ __launch_bounds__(256) void k_icp_f16(const IcpWork* __restrict__ work, const IcpProb* __restrict__ probs,
                                                 const float* __restrict__ src, const float4* __restrict__ t4f,
                                                 const _Float16* __restrict__ img, const float* __restrict__ tn32,
                                                 const float* __restrict__ tnrm, const double* __restrict__ T,
                                                 const IcpFrame* __restrict__ frame,
                                                 const IcpPlaneFrame* __restrict__ pframe,
                                                 const int32_t* __restrict__ done, double thr2,
                                                 IcpLoss loss, unsigned long long* __restrict__ sums,
                                                 int32_t* __restrict__ corr, int32_t* __restrict__ flag,
                                                 unsigned long long* __restrict__ stats,
                                                 const float* __restrict__ snrm, double ome) {
  __shared__ __attribute__((aligned(16))) _Float16 a_s[2][CHF_ROWS * CHF_PITCH];
  __shared__ __attribute__((aligned(16))) float tn_s[2][CHF_ROWS];
  __shared__ unsigned long long part[4][icp_nsum<EST>()];
  __shared__ float wmax[4];
  __shared__ int wg_bad;
  const IcpWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  if (done[wk.prob]) {
    if (tid == 0) flag[blockIdx.x] = 0;
    return;
  }
  const IcpProb pr = probs[wk.prob];
  const int tn = pr.tn;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int half = lane >> 5;
  const int col = lane & 31;
  const double* Tp = T + (int64_t)wk.prob * 16;
  if (tid == 0) wg_bad = 0;
  double px[CHF_NG], py[CHF_NG], pz[CHF_NG];
  f16x8 bop[CHF_NG];
  float b1[CHF_NG], b2[CHF_NG], b3[CHF_NG];
  int t1[CHF_NG], t2[CHF_NG];
  bool in_range = true;
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    icp_pose(Tp, src + (wk.s0 + (sloc < wk.sn ? sloc : 0)) * 3, px[g], py[g], pz[g]);
    const float pf[3] = {(float)px[g] * CHF_SCALE, (float)py[g] * CHF_SCALE, (float)pz[g] * CHF_SCALE};
    _Float16 hi[3], lo[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      knf_split(-2.0f * pf[c], &hi[c], &lo[c]);
      in_range = in_range && fabsf(pf[c]) < 60.0f * CHF_SCALE;   // (NaN fails too)
    }
    // B rows k: 0..2 = -2 ph (x th), 3..5 = -2 ph (x tl), 6..8 = -2 pl (x th), 9..15 = 0; this lane holds k = 8 half .. + 7
    const _Float16 z0 = (_Float16)0.0f;
    if (half == 0)
      bop[g] = f16x8{hi[0], hi[1], hi[2], hi[0], hi[1], hi[2], lo[0], lo[1]};
    else
      bop[g] = f16x8{lo[2], z0, z0, z0, z0, z0, z0, z0};
    b1[g] = b2[g] = b3[g] = INFINITY;
    t1[g] = t2[g] = -1;
  }
  // register-staged double buffer of the 12-KiB image stages, as in k_chamfer_f16
  const uint4* gimg = reinterpret_cast<const uint4*>(img + pr.t0 * CHF_PITCH);
  constexpr int U4_PER_STAGE = CHF_ROWS * CHF_PITCH * 2 / 16;
  static_assert(U4_PER_STAGE == 3 * 256, "three 16-byte pieces per thread");
  uint4 st0, st1, st2;
  float stn;
  float tmax2 = 0.0f;
  auto load_stage = [&](int base) {
    const uint4* g = gimg + (int64_t)base * (CHF_PITCH * 2 / 16) + tid;
    st0 = g[0];
    st1 = g[256];
    st2 = g[512];
    const int r = base + tid;
    stn = r < tn ? tn32[pr.t0 + r] : INFINITY;   // rows past the segment (another problem's rows) never win
    if (r < tn) tmax2 = fmaxf(tmax2, stn);
  };
  auto store_stage = [&](int b) {
    uint4* d = reinterpret_cast<uint4*>(a_s[b]) + tid;
    d[0] = st0;
    d[256] = st1;
    d[512] = st2;
    tn_s[b][tid] = stn;
  };
  if (tn > 0) {
    load_stage(0);
    store_stage(0);
  }
  int buf = 0;
  for (int base = 0; base < tn; base += CHF_ROWS) {
    __syncthreads();
    const bool more = base + CHF_ROWS < tn;
    if (more) load_stage(base + CHF_ROWS);
#pragma unroll 1
    for (int t = 0; t < CHF_ROWS / 32; ++t) {
      if (base + 32 * t >= tn) break;   // whole tile past the range (block-uniform)
      const f16x8 a = *reinterpret_cast<const f16x8*>(a_s[buf] + (t * 32 + col) * CHF_PITCH + 8 * half);
      f32x16 c16;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const float4 v = *reinterpret_cast<const float4*>(&tn_s[buf][t * 32 + 8 * q4 + 4 * half]);
        c16[4 * q4 + 0] = v.x; c16[4 * q4 + 1] = v.y; c16[4 * q4 + 2] = v.z; c16[4 * q4 + 3] = v.w;
      }
      const int tile = base / 32 + t;
#pragma unroll
      for (int g = 0; g < CHF_NG; ++g) {
        const f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop[g], c16, 0, 0, 0);
        float m = fminf(fminf(d[0], d[1]), d[2]);
        m = fminf(fminf(m, d[3]), d[4]);
        m = fminf(fminf(m, d[5]), d[6]);
        m = fminf(fminf(m, d[7]), d[8]);
        m = fminf(fminf(m, d[9]), d[10]);
        m = fminf(fminf(m, d[11]), d[12]);
        m = fminf(fminf(m, d[13]), d[14]);
        m = fminf(m, d[15]);
        const float o1 = b1[g], o2 = b2[g];
        const bool lt1 = m < o1, lt2 = m < o2;
        b1[g] = fminf(o1, m);
        b2[g] = __builtin_amdgcn_fmed3f(o1, o2, m);
        b3[g] = __builtin_amdgcn_fmed3f(o2, b3[g], m);
        t2[g] = lt1 ? t1[g] : (lt2 ? tile : t2[g]);
        t1[g] = lt1 ? tile : t1[g];
      }
    }
    if (more) store_stage(buf ^ 1);
    buf ^= 1;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) tmax2 = fmaxf(tmax2, __shfl_xor(tmax2, off));
  if (lane == 0) wmax[wave] = tmax2;
  __syncthreads();
  const double tmax = sqrt((double)fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))) / (double)CHF_SCALE;
  bool bad = !in_range || !(tmax < 60.0);
  const float4* trow = t4f + pr.t0;
  // canonical distances of this lane's 16 rows of a tile, ascending rows, strict <: the smallest by (distance, row)
  auto eval_tile = [&](int g, int tile, double& e, int& er) {
    e = INFINITY;
    er = 0x7fffffff;
    if (tile >= 0) {
      float4 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = tile * 32 + 4 * half + (i & 3) + 8 * (i >> 2);
        v[i] = trow[row < tn ? row : 0];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = tile * 32 + 4 * half + (i & 3) + 8 * (i >> 2);
        const double dx = px[g] - (double)v[i].x, dy = py[g] - (double)v[i].y, dz = pz[g] - (double)v[i].z;
        const double d = fma(dz, dz, fma(dy, dy, dx * dx));
        if (row < tn && d < e) {
          e = d;
          er = row;
        }
      }
    }
  };
  // (distance, row) minimum of the two lanes of a source
  auto pair_min = [&](double& e, int& er) {
    const double oe = __shfl_xor(e, 32);
    const int orow = __shfl_xor(er, 32);
    if (oe < e || (oe == e && orow < er)) {
      e = oe;
      er = orow;
    }
  };
  double my_e = INFINITY;
  int my_row = 0x7fffffff;
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    // error budget: the derivation in k_chamfer_f16 (the ranking value and its operands are the same)
    const double pn2 = fma(pz[g], pz[g], fma(py[g], py[g], px[g] * px[g]));
    const double S = (double)CHF_SCALE, PT = S * (sqrt(pn2) + tmax);
    const double eps = 0x1.0p-19 * PT * PT + 0x1.0p-10 * PT;
    double e;
    int er;
    eval_tile(g, t1[g], e, er);
    pair_min(e, er);
    float rest = fminf(b2[g], __shfl_xor(b2[g], 32));     // smallest unevaluated tile minimum of the source
    bool ok = rest == INFINITY || (e - pn2) * S * S < (double)rest - eps;
    if (__any(!ok)) {
      double e2 = INFINITY;
      int er2 = 0x7fffffff;
      if (!ok) eval_tile(g, t2[g], e2, er2);
      pair_min(e2, er2);
      if (!ok) {
        if (e2 < e || (e2 == e && er2 < er)) {
          e = e2;
          er = er2;
        }
        rest = fminf(b3[g], __shfl_xor(b3[g], 32));
        ok = rest == INFINITY || (e - pn2) * S * S < (double)rest - eps;
      }
    }
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    if (sloc < wk.sn && !ok) bad = true;
    if (g == half) {       // both lanes of a source hold its result: lane `half` carries the source of group `half`
      my_e = e;
      my_row = er;
    }
  }
  static_assert(CHF_NG == 2, "one source per thread in the sums: group g is carried by the lanes of half g");
  if (__any(bad) && lane == 0) atomicOr(&wg_bad, 1);
  __syncthreads();
  const int wbad = wg_bad;
  if (tid == 0) {
    flag[blockIdx.x] = wbad;
    if (stats) {
      atomicAdd(&stats[0], 1ULL);
      if (wbad) atomicAdd(&stats[1], 1ULL);
    }
  }
  if (wbad) return;   // block-uniform
  const double mpx = half ? px[1] : px[0], mpy = half ? py[1] : py[0], mpz = half ? pz[1] : pz[0];
  const bool active = tid < wk.sn;   // sloc of (wave, g = half, col) = tid
  const bool kept = active && my_row != 0x7fffffff && my_e < thr2;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (kept) q = trow[my_row];
  if (corr && active) corr[wk.c0 + tid] = kept ? my_row : -1;
  icp_block_sums<EST>(kept, mpx, mpy, mpz, q.x, q.y, q.z, my_e, frame[wk.prob],
                      icp_is_plane<EST>() ? pframe + wk.prob : nullptr,
                      icp_is_plane<EST>() && kept ? tnrm + (pr.t0 + my_row) * 3 : nullptr, loss,
                      sums + (int64_t)wk.prob * icp_nsum<EST>(), part,
                      EST == ICP_GICP && kept ? snrm + (wk.s0 + tid) * 3 : nullptr, Tp, ome);
}

__device__ __forceinline__ bool icp_all_finite(const double* v, int n) {
  bool f = true;
  for (int i = 0; i < n; ++i) f = f && isfinite(v[i]);
  return f;
}

// The scale step of EST = 3, 4: the problem stops (false) when s_u is not a finite positive number or the accumulated scale
// s_u * scale would leave [scale_min, scale_max] (a NaN fails both comparisons).
__device__ __forceinline__ bool icp_scale_ok(double su, double scale, const IcpCriteria& crit, double& scale_new) {
  scale_new = su * scale;
  return isfinite(su) && su > 0.0 && scale_new >= crit.scale_min && scale_new <= crit.scale_max;
}

// The point-to-point update from the 17 sums: Horn's fit about the means.  SCALE: Umeyama's scale from the 18th sum on top
// of it, U = [s_u R | q_mean - s_u R p_mean]; false = the problem stops on the scale rules.
template <bool SCALE>
__device__ __forceinline__ bool icp_update_point(const unsigned long long* __restrict__ S, double dn, const IcpFrame& fr,
                                                 const double* __restrict__ Tp, double (&Tn)[12], double scale,
                                                 const IcpCriteria& crit, double& scale_new) {
  double sp[3], sq[3], mp[3], mq[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sp[c] = (double)(long long)S[1 + c] * fr.inv1;
    sq[c] = (double)(long long)S[4 + c] * fr.inv1;
    mp[c] = sp[c] / dn;
    mq[c] = sq[c] / dn;
  }
  // cross-covariance about the means, source index first (the RANSAC's S): sum p'_a q'_b - (sum p'_a) mean q'_b
  double Sm[3][3], N[4][4], V[4][4];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Sm[a][b] = fma(-sp[a], mq[b], (double)(long long)S[7 + 3 * a + b] * fr.inv2);
  N[0][0] = Sm[0][0] + Sm[1][1] + Sm[2][2];
  N[0][1] = Sm[1][2] - Sm[2][1];
  N[0][2] = Sm[2][0] - Sm[0][2];
  N[0][3] = Sm[0][1] - Sm[1][0];
  N[1][1] = Sm[0][0] - Sm[1][1] - Sm[2][2];
  N[1][2] = Sm[0][1] + Sm[1][0];
  N[1][3] = Sm[2][0] + Sm[0][2];
  N[2][2] = -Sm[0][0] + Sm[1][1] - Sm[2][2];
  N[2][3] = Sm[1][2] + Sm[2][1];
  N[3][3] = -Sm[0][0] - Sm[1][1] + Sm[2][2];
  N[1][0] = N[0][1];
  N[2][0] = N[0][2];
  N[3][0] = N[0][3];
  N[2][1] = N[1][2];
  N[3][1] = N[1][3];
  N[3][2] = N[2][3];
  double qv[4];
  if (!horn_qcp(Sm, N, qv)) {
    jacobi4(N, V);
    // eigenvector of the largest eigenvalue (ties -> lowest index), as the RANSAC selects it
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
  double R[3][3];
  icp_quat_rotation(qv[0], qv[1], qv[2], qv[3], R);
  // t = q_mean - R p_mean on the unprimed means; T <- U T
  double pm[3], qm[3], t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pm[c] = mp[c] + fr.o[c];
    qm[c] = mq[c] + fr.o[c];
  }
  if constexpr (SCALE) {
    // s_u = sum_ab R_ab S_ab / (sum p'.p' - sum_a (sum p'_a) mean p'_a): the variance of the posed sources about their mean
    double den = (double)(long long)S[17] * fr.inv_pp;
#pragma unroll
    for (int a = 0; a < 3; ++a) den = fma(-sp[a], mp[a], den);
    double num = R[0][0] * Sm[0][0];
#pragma unroll
    for (int k = 1; k < 9; ++k) num = fma(R[k / 3][k % 3], Sm[k / 3][k % 3], num);
    if (!(isfinite(den) && den > 0.0)) return false;
    const double su = num / den;
    if (!icp_scale_ok(su, scale, crit, scale_new)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[a] = fma(-su, fma(R[a][2], pm[2], fma(R[a][1], pm[1], R[a][0] * pm[0])), qm[a]);
#pragma unroll
      for (int b = 0; b < 3; ++b) R[a][b] = su * R[a][b];
    }
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = qm[a] - fma(R[a][2], pm[2], fma(R[a][1], pm[1], R[a][0] * pm[0]));
  }
  icp_compose(R, t, Tp, Tn);
  return true;
}

// The point-to-plane update from the 29 sums (the weighted layout has the same entries in the same places): A x = -b by an
// unpivoted Cholesky, x = (alpha, t') about the origin o, the rotation of the quaternion (1, alpha / 2).  false: a pivot is
// not finite or too small -- the problem stops.  NJ = 7 (plane + scale): the 37 sums, a seventh unknown sigma,
// s_u = 1 + sigma, U = [s_u R | t' + o - s_u R o]; false also when the scale rules stop the problem.
template <int NJ>
__device__ __forceinline__ bool icp_update_plane(const unsigned long long* __restrict__ S, const IcpFrame& fr,
                                                 const IcpPlaneFrame& g, const double* __restrict__ Tp, double (&Tn)[12],
                                                 double scale, const IcpCriteria& crit, double& scale_new) {
  constexpr int NJJ = NJ * (NJ + 1) / 2;
  double A[NJ][NJ], bv[NJ], xv[NJ];
  {
    int at = 1;
#pragma unroll
    for (int i = 0; i < NJ; ++i)
#pragma unroll
      for (int j = i; j < NJ; ++j) {
        const bool ri = icp_rot_col(i), rj = icp_rot_col(j);
        const double inv = ri && rj ? g.inv_rr : (ri || rj ? g.inv_rt : g.inv_tt);
        A[i][j] = (double)(long long)S[at++] * inv;
        A[j][i] = A[i][j];
      }
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i) bv[i] = (double)(long long)S[1 + NJJ + i] * (icp_rot_col(i) ? g.inv_rd : g.inv_td);
  if (!icp_chol_solve<NJ>(A, bv, xv)) return false;
  double R[3][3], t[3];
  icp_quat_rotation(1.0, 0.5 * xv[0], 0.5 * xv[1], 0.5 * xv[2], R);
  if constexpr (NJ == 7) {
    // p <- s_u R (p - o) + t' + o:  t = t' + o - s_u R o
    const double su = 1.0 + xv[6];
    if (!icp_scale_ok(su, scale, crit, scale_new)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[a] = fma(-su, fma(R[a][2], fr.o[2], fma(R[a][1], fr.o[1], R[a][0] * fr.o[0])), xv[3 + a] + fr.o[a]);
#pragma unroll
      for (int b = 0; b < 3; ++b) R[a][b] = su * R[a][b];
    }
  } else {
    // p <- R (p - o) + t' + o:  t = t' + o - R o
#pragma unroll
    for (int a = 0; a < 3; ++a)
      t[a] = (xv[3 + a] + fr.o[a]) - fma(R[a][2], fr.o[2], fma(R[a][1], fr.o[1], R[a][0] * fr.o[0]));
  }
  icp_compose(R, t, Tp, Tn);
  return true;
}

// One lane per problem: the evaluation of the association just made, the stop rule, the update.  last = the round after
// the max_iter-th update (or the only one when max_iter = 0): nothing is fitted, the f32 copy of T is written.
template <int EST>
__global__ void k_icp_step(const IcpProb* __restrict__ probs, int n_prob, const IcpFrame* __restrict__ frame,
                           const IcpPlaneFrame* __restrict__ pframe, IcpCriteria crit, int round, int last,
                           unsigned long long* __restrict__ sums, int32_t* __restrict__ done, double* __restrict__ T,
                           float* __restrict__ T32, double* __restrict__ fitness, double* __restrict__ rmse,
                           double* __restrict__ wfitness, double* __restrict__ scale, int32_t* __restrict__ iters,
                           int32_t* __restrict__ ncorr, double* __restrict__ mrmse) {
  constexpr int NS = icp_nsum<EST>();
  constexpr int MIN_CORR = icp_is_plane<EST>() ? icp_nj<EST>() : 3;   // one pair per unknown of the plane system
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  double* Tp = T + (int64_t)p * 16;
  if (!done[p]) {
    const IcpProb pr = probs[p];
    const IcpFrame fr = frame[p];
    unsigned long long* S = sums + (int64_t)p * NS;
    const long long n = (long long)S[0];
    const double dn = (double)n;
    const double fit = pr.sn > 0 ? dn / (double)pr.sn : 0.0;
    const double sd2 = (double)(long long)S[icp_d2_at<EST>()] * fr.inv2;
    const double rm = n > 0 ? sqrt(sd2 / dn) : 0.0;
    const double pfit = fitness[p], prm = rmse[p];
    fitness[p] = fit;
    rmse[p] = rm;
    ncorr[p] = (int32_t)n;
    if (wfitness) {   // sum w = S_w 2^-(61 - eN); every weight is 1 without a kernel, and the share is the fitness
      if constexpr (EST == ICP_ROBUST)
        wfitness[p] = pr.sn > 0 ? ((double)(long long)S[NS - 1] * (1.0 / fr.clamp)) / (double)pr.sn : 0.0;
      else
        wfitness[p] = fit;
    }
    if constexpr (EST == ICP_GICP) {   // the Mahalanobis rmse of this association: sum e.We shares the scale of rot x e
      if (mrmse) {
        const double sm = (double)(long long)S[NS - 1] * pframe[p].inv_rd;
        mrmse[p] = n > 0 && sm > 0.0 ? sqrt(sm / dn) : 0.0;
      }
    }
    bool stop = last != 0;
    if (round > 0 && fabs(fit - pfit) < crit.rel_fitness && fabs(rm - prm) < crit.rel_rmse) stop = true;
    if (n < MIN_CORR || !isfinite(fit) || !isfinite(rm)) stop = true;
    if (!stop) {
      double Tn[12];
      bool solved = true;
      double sc_old = 1.0, sc_new = 1.0;   // the accumulated scale before and after this update (EST = 3, 4)
      if constexpr (icp_has_scale<EST>()) sc_old = scale[p];
      if constexpr (icp_is_plane<EST>())
        solved = icp_update_plane<icp_nj<EST>()>(S, fr, pframe[p], Tp, Tn, sc_old, crit, sc_new);
      else
        solved = icp_update_point<EST == ICP_POINT_S>(S, dn, fr, Tp, Tn, sc_old, crit, sc_new);
      if (solved && icp_all_finite(Tn, 12)) {
#pragma unroll
        for (int i = 0; i < 12; ++i) Tp[i] = Tn[i];
        if constexpr (icp_has_scale<EST>()) scale[p] = sc_new;
        iters[p] = iters[p] + 1;
#pragma unroll
        for (int k = 0; k < NS; ++k) S[k] = 0;
      } else {
        stop = true;
      }
    }
    if (stop) done[p] = 1;
  }
  if (last && T32) {
    for (int i = 0; i < 16; ++i) T32[(int64_t)p * 16 + i] = (float)Tp[i];
  }
}

__global__ void k_icp_init(const float* __restrict__ T0, int n_prob, double* __restrict__ T, double* __restrict__ fitness,
                           double* __restrict__ rmse, double* __restrict__ wfitness, double* __restrict__ scale,
                           int32_t* __restrict__ iters, int32_t* __restrict__ ncorr, int32_t* __restrict__ done) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  for (int i = 0; i < 16; ++i) T[(int64_t)p * 16 + i] = (double)T0[(int64_t)p * 16 + i];
  fitness[p] = 0.0;
  rmse[p] = 0.0;
  if (wfitness) wfitness[p] = 0.0;
  if (scale) scale[p] = 1.0;
  iters[p] = 0;
  ncorr[p] = 0;
  done[p] = 0;
}

std::atomic<unsigned long long> g_icp_stats[2];

// Every entry: d_tnrm is the normal array of the plane estimations (EST = 1, 2), loss the kernel of EST = 2, d_wfitness the
// optional weighted inlier share of cs_icp_plane_robust_batch (NULL for the other entries), scale_min / scale_max / d_scale
// the interval and the output of cs_icp_scale_batch (EST = 3, 4), d_snrm / epsilon / d_mrmse the source normals, the
// covariance floor and the optional Mahalanobis rmse of cs_icp_gicp_batch (EST = 5).
template <int EST>
int icp_run(const char* name, const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tnrm,
            const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, const float* d_T0,
            double max_dist, int max_iter, double relative_fitness, double relative_rmse, double* d_T, float* d_T32,
            double* d_fitness, double* d_rmse, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream,
            IcpLoss loss = IcpLoss{CS_ICP_KERNEL_L2, 0.0}, double* d_wfitness = nullptr, double scale_min = 1.0,
            double scale_max = 1.0, double* d_scale = nullptr, const float* d_snrm = nullptr, double epsilon = 1.0,
            double* d_mrmse = nullptr) {
  constexpr int NS = icp_nsum<EST>();
  CS_REQUIRE(h_soff && h_toff && h_src_seg && h_tgt_seg, CS_ERR_INVALID, "%s: NULL table", name);
  CS_REQUIRE(n_prob >= 0, CS_ERR_INVALID, "%s: negative problem count", name);
  CS_REQUIRE(max_dist > 0.0 && std::isfinite(max_dist), CS_ERR_INVALID, "%s: max_dist must be positive and finite", name);
  CS_REQUIRE(max_iter >= 0 && max_iter <= 1000, CS_ERR_UNSUPPORTED, "%s: max_iter outside [0, 1000]", name);
  CS_REQUIRE(!std::isnan(relative_fitness) && !std::isnan(relative_rmse), CS_ERR_INVALID,
             "%s: a convergence threshold is NaN", name);
  if (n_prob == 0) return CS_OK;
  CS_REQUIRE(d_T0 && d_T && d_fitness && d_rmse && d_iters && d_ncorr, CS_ERR_INVALID, "%s: NULL argument", name);
  CS_REQUIRE(!icp_has_scale<EST>() || d_scale, CS_ERR_INVALID, "%s: NULL scale output", name);
  std::vector<IcpProb> probs(n_prob);
  std::vector<IcpWork> work;
  int64_t nt_rows = 0, n_corr_rows = 0;
  double flop = 0.0;
  for (int p = 0; p < n_prob; ++p) {
    const int ss = h_src_seg[p], ts = h_tgt_seg[p];
    CS_REQUIRE(ss >= 0 && ts >= 0, CS_ERR_INVALID, "%s: negative segment id in problem %d", name, p);
    const int64_t sn = h_soff[ss + 1] - h_soff[ss], tn = h_toff[ts + 1] - h_toff[ts];
    CS_REQUIRE(sn >= 0 && tn >= 0, CS_ERR_INVALID, "%s: bad segment in problem %d", name, p);
    CS_REQUIRE(sn < (1LL << 31) && tn < (1LL << 31), CS_ERR_UNSUPPORTED,
               "%s: a segment of problem %d has 2^31 rows or more", name, p);
    IcpProb& pr = probs[p];
    pr.s0 = h_soff[ss];
    pr.t0 = h_toff[ts];
    pr.c0 = n_corr_rows;
    pr.sn = (int32_t)sn;
    pr.tn = (int32_t)tn;
    if (tn > 0) nt_rows = std::max<int64_t>(nt_rows, h_toff[ts + 1]);
    for (int64_t q = 0; q < sn; q += ICP_ST) {
      IcpWork w;
      w.s0 = pr.s0 + q;
      w.c0 = pr.c0 + q;
      w.sn = (int32_t)std::min<int64_t>(sn - q, ICP_ST);
      w.prob = p;
      work.push_back(w);
    }
    n_corr_rows += sn;
    flop += 8.0 * (double)sn * (double)tn;
  }
  CS_REQUIRE(work.empty() || d_src, CS_ERR_INVALID, "%s: NULL source array", name);
  CS_REQUIRE(nt_rows == 0 || d_tgt, CS_ERR_INVALID, "%s: NULL target array", name);
  CS_REQUIRE(!icp_is_plane<EST>() || nt_rows == 0 || d_tnrm, CS_ERR_INVALID, "%s: NULL target normal array", name);
  CS_REQUIRE(EST != ICP_GICP || work.empty() || d_snrm, CS_ERR_INVALID, "%s: NULL source normal array", name);
  // GICP: 1 - eps, and eW = the smallest integer with 1 / (2 eps) <= 2^eW, i.e. 1 <= eps * 2^(eW + 1) (exact); in [-1, 9]
  const double ome = 1.0 - epsilon;
  int eW = 0;
  if (EST == ICP_GICP)
    for (eW = -1; std::ldexp(epsilon, eW + 1) < 1.0; ++eW) {
    }
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const bool use_f16 = !env_first_is("CS_ICP_F16", '0');
  const bool want_stats = use_f16 && env_first_is("CS_ICP_STATS", '1');
  const unsigned n_work = (unsigned)work.size();
  PoolBuf<IcpProb> dprob;
  PoolBuf<IcpWork> dwork;
  PoolBuf<IcpFrame> frame((size_t)n_prob);
  PoolBuf<IcpPlaneFrame> pframe;
  PoolBuf<unsigned long long> sums((size_t)n_prob * NS + 2);   // + the two statistics counters
  PoolBuf<int32_t> done((size_t)n_prob);
  CS_REQUIRE(frame.p && sums.p && done.p, CS_ERR_HIP, "%s: scratch allocation failed", name);
  if (icp_is_plane<EST>()) CS_REQUIRE(pframe.alloc((size_t)n_prob), CS_ERR_HIP, "%s: scratch allocation failed", name);
  int rc = upload(dprob, probs, s);
  if (!rc) rc = upload(dwork, work, s);
  if (rc) return rc;
  unsigned long long* dstats = sums.p + (size_t)n_prob * NS;
  ProfScope prof("icp", s, flop * (double)(max_iter + 1));
  CS_HIP_CHECK(hipMemsetAsync(sums.p, 0, sizeof(unsigned long long) * ((size_t)n_prob * NS + 2), s));
  const dim3 pgrid((unsigned)ceil_div(n_prob, 64));
  hipLaunchKernelGGL(k_icp_init, pgrid, dim3(64), 0, s, d_T0, n_prob, d_T, d_fitness, d_rmse, d_wfitness,
                     icp_has_scale<EST>() ? d_scale : (double*)nullptr, d_iters, d_ncorr, done.p);
  hipLaunchKernelGGL(k_icp_frame, dim3((unsigned)n_prob), dim3(256), 0, s, dprob.p, d_tgt, max_dist, frame.p, pframe.p, eW);
  if (EST == ICP_GICP && d_mrmse) CS_HIP_CHECK(hipMemsetAsync(d_mrmse, 0, sizeof(double) * (size_t)n_prob, s));
  // the targets do not move: one image for every round
  PoolBuf<_Float16> img16;
  PoolBuf<float> tn16;
  PoolBuf<float4> t4f;
  PoolBuf<int32_t> wflag;
  if (use_f16 && n_work) {
    const int64_t n_pad = nt_rows + CHF_ROWS;   // the last stage of the last segment reads past its end
    img16.alloc((size_t)n_pad * CHF_PITCH);
    tn16.alloc((size_t)n_pad);
    t4f.alloc((size_t)(nt_rows ? nt_rows : 1));
    wflag.alloc(n_work);
    CS_REQUIRE(img16.p && tn16.p && t4f.p && wflag.p, CS_ERR_HIP, "%s: scratch allocation failed", name);
    chamfer_pack16(d_tgt, nt_rows, n_pad, img16.p, tn16.p, t4f.p, s);
  }
  CS_LAUNCH_CHECK();
  IcpCriteria crit;
  crit.thr2 = max_dist * max_dist;
  crit.rel_fitness = relative_fitness;
  crit.rel_rmse = relative_rmse;
  crit.scale_min = scale_min;
  crit.scale_max = scale_max;
  for (int round = 0; round <= max_iter; ++round) {
    if (n_work) {
      if (use_f16) {
        hipLaunchKernelGGL(k_icp_f16<EST>, dim3(n_work), dim3(256), 0, s, dwork.p, dprob.p, d_src, t4f.p, img16.p, tn16.p,
                           d_tnrm, (const double*)d_T, frame.p, pframe.p, done.p, crit.thr2, loss, sums.p, d_corr, wflag.p,
                           want_stats ? dstats : (unsigned long long*)nullptr, d_snrm, ome);
        hipLaunchKernelGGL(k_icp_exact<EST>, dim3(n_work), dim3(256), 0, s, dwork.p, dprob.p, d_src, d_tgt, d_tnrm,
                           (const double*)d_T, frame.p, pframe.p, done.p, crit.thr2, loss, sums.p, d_corr,
                           (const int32_t*)wflag.p, d_snrm, ome);
      } else {
        hipLaunchKernelGGL(k_icp_exact<EST>, dim3(n_work), dim3(256), 0, s, dwork.p, dprob.p, d_src, d_tgt, d_tnrm,
                           (const double*)d_T, frame.p, pframe.p, done.p, crit.thr2, loss, sums.p, d_corr,
                           (const int32_t*)nullptr, d_snrm, ome);
      }
    }
    hipLaunchKernelGGL(k_icp_step<EST>, pgrid, dim3(64), 0, s, dprob.p, n_prob, frame.p, pframe.p, crit, round,
                       round == max_iter ? 1 : 0, sums.p, done.p, d_T, d_T32, d_fitness, d_rmse, d_wfitness, d_scale,
                       d_iters, d_ncorr, d_mrmse);
  }
  CS_LAUNCH_CHECK();
  if (want_stats) {
    unsigned long long h[2] = {0, 0};
    CS_HIP_CHECK(download_async(h, dstats, sizeof(h), s));
    CS_HIP_CHECK(download_sync(s));
    g_icp_stats[0] += h[0];
    g_icp_stats[1] += h[1];
  }
  return CS_OK;
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

void cs_icp_stats(uint64_t out[2], int reset) { read_stats(g_icp_stats, out, reset); }

int cs_icp_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const int64_t* h_toff,
                 const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, const float* d_T0, double max_dist,
                 int max_iter, double relative_fitness, double relative_rmse, double* d_T, float* d_T32,
                 double* d_fitness, double* d_rmse, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream) {
  return icp_run<ICP_POINT>("cs_icp_batch", d_src, h_soff, d_tgt, nullptr, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T0,
                            max_dist, max_iter, relative_fitness, relative_rmse, d_T, d_T32, d_fitness, d_rmse, d_iters,
                            d_ncorr, d_corr, stream);
}

int cs_icp_plane_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                       const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                       const float* d_T0, double max_dist, int max_iter, double relative_fitness, double relative_rmse,
                       double* d_T, float* d_T32, double* d_fitness, double* d_rmse, int32_t* d_iters, int32_t* d_ncorr,
                       int32_t* d_corr, void* stream) {
  return icp_run<ICP_PLANE>("cs_icp_plane_batch", d_src, h_soff, d_tgt, d_tgt_normal, h_toff, h_src_seg, h_tgt_seg, n_prob,
                            d_T0, max_dist, max_iter, relative_fitness, relative_rmse, d_T, d_T32, d_fitness, d_rmse,
                            d_iters, d_ncorr, d_corr, stream);
}

int cs_icp_plane_robust_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                              const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                              const float* d_T0, double max_dist, int max_iter, double relative_fitness,
                              double relative_rmse, int kernel, double kernel_scale, double* d_T, float* d_T32,
                              double* d_fitness, double* d_rmse, double* d_wfitness, int32_t* d_iters, int32_t* d_ncorr,
                              int32_t* d_corr, void* stream) {
  const char* name = "cs_icp_plane_robust_batch";
  CS_REQUIRE(kernel >= CS_ICP_KERNEL_L2 && kernel <= CS_ICP_KERNEL_TUKEY, CS_ERR_INVALID, "%s: unknown kernel %d", name,
             kernel);
  if (kernel == CS_ICP_KERNEL_L2)   // every weight is 1: cs_icp_plane_batch's instantiation, the scale is ignored
    return icp_run<ICP_PLANE>(name, d_src, h_soff, d_tgt, d_tgt_normal, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T0, max_dist,
                              max_iter, relative_fitness, relative_rmse, d_T, d_T32, d_fitness, d_rmse, d_iters, d_ncorr,
                              d_corr, stream, IcpLoss{CS_ICP_KERNEL_L2, 0.0}, d_wfitness);
  CS_REQUIRE(std::isfinite(kernel_scale) && kernel_scale > 0.0, CS_ERR_INVALID,
             "%s: kernel_scale must be positive and finite", name);
  return icp_run<ICP_ROBUST>(name, d_src, h_soff, d_tgt, d_tgt_normal, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T0, max_dist,
                             max_iter, relative_fitness, relative_rmse, d_T, d_T32, d_fitness, d_rmse, d_iters, d_ncorr,
                             d_corr, stream, IcpLoss{kernel, kernel_scale}, d_wfitness);
}

int cs_icp_scale_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                       const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                       const float* d_T0, double max_dist, int max_iter, double relative_fitness, double relative_rmse,
                       double scale_min, double scale_max, double* d_T, float* d_T32, double* d_fitness, double* d_rmse,
                       double* d_scale, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream) {
  const char* name = "cs_icp_scale_batch";
  CS_REQUIRE(std::isfinite(scale_min) && std::isfinite(scale_max), CS_ERR_INVALID, "%s: a scale bound is not finite", name);
  CS_REQUIRE(scale_min > 0.0 && scale_min <= 1.0 && scale_max >= 1.0, CS_ERR_INVALID,
             "%s: the scale interval must satisfy 0 < scale_min <= 1 <= scale_max", name);
  const IcpLoss l2{CS_ICP_KERNEL_L2, 0.0};
  if (d_tgt_normal)
    return icp_run<ICP_PLANE_S>(name, d_src, h_soff, d_tgt, d_tgt_normal, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T0,
                                max_dist, max_iter, relative_fitness, relative_rmse, d_T, d_T32, d_fitness, d_rmse, d_iters,
                                d_ncorr, d_corr, stream, l2, nullptr, scale_min, scale_max, d_scale);
  return icp_run<ICP_POINT_S>(name, d_src, h_soff, d_tgt, nullptr, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T0, max_dist,
                              max_iter, relative_fitness, relative_rmse, d_T, d_T32, d_fitness, d_rmse, d_iters, d_ncorr,
                              d_corr, stream, l2, nullptr, scale_min, scale_max, d_scale);
}

int cs_icp_gicp_batch(const float* d_src, const float* d_src_normal, const int64_t* h_soff, const float* d_tgt,
                      const float* d_tgt_normal, const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg,
                      int n_prob, const float* d_T0, double max_dist, int max_iter, double relative_fitness,
                      double relative_rmse, double epsilon, double* d_T, float* d_T32, double* d_fitness, double* d_rmse,
                      double* d_mrmse, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream) {
  const char* name = "cs_icp_gicp_batch";
  CS_REQUIRE(std::isfinite(epsilon) && epsilon >= 0x1.0p-10 && epsilon <= 1.0, CS_ERR_INVALID,
             "%s: epsilon must lie in [2^-10, 1]", name);
  return icp_run<ICP_GICP>(name, d_src, h_soff, d_tgt, d_tgt_normal, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T0, max_dist,
                           max_iter, relative_fitness, relative_rmse, d_T, d_T32, d_fitness, d_rmse, d_iters, d_ncorr, d_corr,
                           stream, IcpLoss{CS_ICP_KERNEL_L2, 0.0}, nullptr, 1.0, 1.0, nullptr, d_src_normal, epsilon, d_mrmse);
}

}  // extern "C"
