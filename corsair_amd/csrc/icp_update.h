// The small-pose update shared by the plane ICP (icp_step.hip) and Fast Global Registration (fgr.hip): the rotation of a
// quaternion normalised by division, the chain T <- U T, and the unpivoted Cholesky solve of the normal equations with its
// pivot rule.  One lane per problem runs these; every operation is ONE IEEE f64 operation unless an fma is written.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace cs {

// R of the quaternion (w, x, y, z), normalised by division: cs_ransac_batch's formula.
__device__ __forceinline__ void icp_quat_rotation(double qw, double qx, double qy, double qz, double (&R)[3][3]) {
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw = qw / qn;
  qx = qx / qn;
  qy = qy / qn;
  qz = qz / qn;
  R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  R[0][1] = 2.0 * (qx * qy - qw * qz);
  R[0][2] = 2.0 * (qx * qz + qw * qy);
  R[1][0] = 2.0 * (qx * qy + qw * qz);
  R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
  R[1][2] = 2.0 * (qy * qz - qw * qx);
  R[2][0] = 2.0 * (qx * qz - qw * qy);
  R[2][1] = 2.0 * (qy * qz + qw * qx);
  R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
}

// Tn = U T, U = (R, t): the first three rows of the 4x4.
__device__ __forceinline__ void icp_compose(const double (&R)[3][3], const double (&t)[3], const double* __restrict__ Tp,
                                            double (&Tn)[12]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) Tn[4 * a + b] = fma(R[a][0], Tp[b], fma(R[a][1], Tp[4 + b], R[a][2] * Tp[8 + b]));
    Tn[4 * a + 3] = fma(R[a][0], Tp[3], fma(R[a][1], Tp[7], fma(R[a][2], Tp[11], t[a])));
  }
}

// A pivot of the Cholesky factorisation must exceed this fraction of its own original diagonal entry.  pivot_j / A_jj is
// the share of column j of the Jacobian that the columns before it do not explain; the fixed-point sums carry each A_jj to
// 2^-44 relative or better (scale 2^(61 - eN - ...) against at most 2^eN terms of that magnitude bound), so a share below
// 2^-30 is four decimal orders above the noise of the sums and far below any geometry that constrains the pose.
// cs_icp_gicp_batch's sums give up eW <= 9 bits to the weight matrix; its header comment and DESIGN 19 re-derive the margin
// (relative noise of a translational A_jj at most 2^-(59 - eN - eW); a pivot share at least epsilon times the geometry's).
constexpr double ICP_PIVOT_MIN = 0x1.0p-30;

// A x = -b for the symmetric NJ x NJ matrix A by an unpivoted Cholesky (the operation sequence is the header comment of
// cs_icp_plane_batch).  false: a pivot is not finite or too small; xv is then not written.
template <int NJ>
__device__ __forceinline__ bool icp_chol_solve(const double (&A)[NJ][NJ], const double (&bv)[NJ], double (&xv)[NJ]) {
  double L[NJ][NJ], yv[NJ];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = fma(-L[j][k], L[j][k], d);
    if (!(isfinite(d) && d > ICP_PIVOT_MIN * A[j][j])) ok = false;
    const double ljj = sqrt(d);
    L[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < NJ; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
      L[i][j] = v / ljj;
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    double v = -bv[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = fma(-L[i][k], yv[k], v);
    yv[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    double v = yv[i];
#pragma unroll
    for (int k = i + 1; k < NJ; ++k) v = fma(-L[k][i], xv[k], v);
    xv[i] = v / L[i][i];
  }
  return true;
}

}  // namespace cs
