// The specification of the ICP sums: why every sum fits 64 bits, then icp_block_sums --
// the terms of one kept pair for each estimation and the block reduction -- which both association kernels (icp_assoc.hip)
// end with, and the pose chain they begin with.
#pragma once
#include <math.h>

#include "icp.h"

namespace cs {

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
// The three estimation bodies and the reduction stay ONE function body on purpose: each of them moved into a function of its
// own (force-inlined or not) compiles to the same instructions in the same order, but with other register numbers in every
// instantiation of both association kernels, and the rule of these units is that a kernel's code changes only when its
// arithmetic does.
template <int EST>
__device__ __forceinline__ void icp_block_sums(bool kept, double px, double py, double pz, float qx, float qy, float qz,
                                               double d2, const IcpFrame& fr, const IcpPlaneFrame* __restrict__ pfr,
                                               const float* __restrict__ nrow, const IcpLoss& loss,
                                               unsigned long long* __restrict__ sums,
                                               unsigned long long (*part)[icp_nsum(EST)],
                                               const float* __restrict__ srow, const double* __restrict__ Tp,
                                               double ome) {
  constexpr int NS = icp_nsum(EST);
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
  } else if constexpr (icp_is_plane(EST)) {
    constexpr int NJ = icp_nj(EST), NJJ = NJ * (NJ + 1) / 2;
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

// p = T (s, 1): the pose chain of a source row, one fma chain per coordinate
__device__ __forceinline__ void icp_pose(const double* __restrict__ Tp, const float* __restrict__ sp, double& px,
                                         double& py, double& pz) {
  const double x = sp[0], y = sp[1], z = sp[2];
  px = fma(Tp[0], x, fma(Tp[1], y, fma(Tp[2], z, Tp[3])));
  py = fma(Tp[4], x, fma(Tp[5], y, fma(Tp[6], z, Tp[7])));
  pz = fma(Tp[8], x, fma(Tp[9], y, fma(Tp[10], z, Tp[11])));
}

}  // namespace cs
