// The rigid-fit eigen-solvers shared by the RANSAC's hypothesis kernel (ransac_hyp.hip) and the ICP's update (icp_step.hip): the
// largest eigenpair of Horn's 4x4 matrix from its characteristic polynomial (horn_qcp), with the cyclic Jacobi solver
// (jacobi4) as the fallback of the lanes it does not accept.  oracle/corsair_oracle.c (oc_horn_qcp / oc_jacobi4) and
// tests/icp_ref.py restate both operation sequences.  jacobi3 is jacobi4's 3x3 sibling for the scatter matrices of
// normals.hip (restated in tests/normals_ref.py).
#pragma once
#include "common.h"

namespace cs {

// Cyclic Jacobi on a symmetric 4x4, eigenvectors in v (columns).  Fixed 5 sweeps: Horn matrices of
// 10-point samples have a relative off-diagonal of at most 2.5e-12 after 5 (round-off after 6), five
// orders below the f32 rounding of the hypothesis that is stored.  Rotation from h = (aqq - app) / 2 and
// g = apq as t = sgn(h) g / (|h| + sqrt(h^2 + g^2)) -- the textbook sgn(theta) / (|theta| + sqrt(theta^2 + 1))
// with theta = h / g, without that division (one f64 divide less per rotation; h = 0 gives t = +1).
__device__ __forceinline__ void jacobi4(double a[4][4], double v[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 5; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q];
        if (apq != 0.0) {
          const double h = 0.5 * (a[q][q] - a[p][p]);
          const double den = fabs(h) + sqrt(h * h + apq * apq);
          const double sg = (h == 0.0 || ((h > 0.0) == (apq > 0.0))) ? 1.0 : -1.0;
          const double t = den > 0.0 ? sg * fabs(apq) / den : sg;
          const double c = 1.0 / sqrt(t * t + 1.0);
          const double s = t * c;
          a[p][p] = a[p][p] - t * apq;
          a[q][q] = a[q][q] + t * apq;
          a[p][q] = 0.0;
          a[q][p] = 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (r != p && r != q) {
              const double arp = a[r][p], arq = a[r][q];
              const double nrp = c * arp - s * arq;
              const double nrq = s * arp + c * arq;
              a[r][p] = nrp;
              a[p][r] = nrp;
              a[r][q] = nrq;
              a[q][r] = nrq;
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double vrp = v[r][p], vrq = v[r][q];
            v[r][p] = c * vrp - s * vrq;
            v[r][q] = s * vrp + c * vrq;
          }
        }
      }
    }
  }
}

// Cyclic Jacobi on a symmetric 3x3 (the scatter matrix of cs_estimate_normals, normals.hip), eigenvectors in v (columns):
// jacobi4's rotation, pairs (0,1), (0,2), (1,2) per sweep.  Fixed 5 sweeps: over 1 320 scatter matrices of 3, 8, 16 and 32
// neighbours on box, sphere and cylinder samples the off-diagonal Frobenius norm relative to the diagonal's is at most
// 2.4e-7 after 3 sweeps and 1.4e-28 after 4 (the convergence is cubic), twelve orders below the f64 rounding of the
// eigenvector; the 5th is the spare one, and a 6th to 8th change no bit of any of these normals
// (tests/test_normals_cpu.py pins both statements on the restatement tests/normals_ref.py).
template <int P, int Q>
__device__ __forceinline__ void jacobi3_rotate(double (&a)[3][3], double (&v)[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = a[P][Q];
  if (apq != 0.0) {
    const double h = 0.5 * (a[Q][Q] - a[P][P]);
    const double den = fabs(h) + sqrt(h * h + apq * apq);
    const double sg = (h == 0.0 || ((h > 0.0) == (apq > 0.0))) ? 1.0 : -1.0;
    const double t = den > 0.0 ? sg * fabs(apq) / den : sg;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = 0.0;
    a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    const double nrp = c * arp - s * arq;
    const double nrq = s * arp + c * arq;
    a[R][P] = nrp;
    a[P][R] = nrp;
    a[R][Q] = nrq;
    a[Q][R] = nrq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double vip = v[i][P], viq = v[i][Q];
      v[i][P] = c * vip - s * viq;
      v[i][Q] = s * vip + c * viq;
    }
  }
}
__device__ __forceinline__ void jacobi3(double (&a)[3][3], double (&v)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) v[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 5; ++sweep) {
    jacobi3_rotate<0, 1>(a, v);
    jacobi3_rotate<0, 2>(a, v);
    jacobi3_rotate<1, 2>(a, v);
  }
}

// Largest eigenpair of the Horn matrix from its characteristic polynomial (round 4; oracle/corsair_oracle.c
// oc_horn_qcp is the same operation sequence, so the hypotheses stay bit-identical).  N is symmetric and
// traceless: P(l) = l^4 + c2 l^2 + c1 l + c0, c2 = -2 |S|_F^2, c1 = -8 det S, c0 = det N.  All roots are real,
// so Halley's iteration from the upper bound sqrt(3) |S|_F descends monotonically onto the largest one with
// cubic order (3-6 steps, one f64 divide each); the eigenvector is the row of adj(N - l I) with the largest
// diagonal entry.  Against the 5-sweep Jacobi (30 rotations x 2 IEEE sqrt + 2 IEEE divides, ~3 000 f64
// instructions) this is ~400.  Accepted only when the iteration converged and P'(l) >= 0.02 l^3 (the largest
// eigenvalue is well separated); the caller falls back to jacobi4 otherwise (3 in 10^5 samples on the bench).
__device__ __forceinline__ bool horn_qcp(const double (&S)[3][3], const double (&N)[4][4], double (&q)[4]) {
  double f2 = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) f2 = fma(S[a][b], S[a][b], f2);
  const double c2 = -2.0 * f2;
  const double detS = S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) -
                      S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0]) +
                      S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0]);
  const double c1 = -8.0 * detS;
  const double u5 = N[0][2] * N[1][3] - N[0][3] * N[1][2];
  const double w0 = N[2][0] * N[3][1] - N[2][1] * N[3][0];
  double c0;
  {
    const double u0 = N[0][0] * N[1][1] - N[0][1] * N[1][0];
    const double u1 = N[0][0] * N[1][2] - N[0][2] * N[1][0];
    const double u2 = N[0][0] * N[1][3] - N[0][3] * N[1][0];
    const double u3 = N[0][1] * N[1][2] - N[0][2] * N[1][1];
    const double u4 = N[0][1] * N[1][3] - N[0][3] * N[1][1];
    const double w1 = N[2][0] * N[3][2] - N[2][2] * N[3][0];
    const double w2 = N[2][0] * N[3][3] - N[2][3] * N[3][0];
    const double w3 = N[2][1] * N[3][2] - N[2][2] * N[3][1];
    const double w4 = N[2][1] * N[3][3] - N[2][3] * N[3][1];
    const double w5 = N[2][2] * N[3][3] - N[2][3] * N[3][2];
    c0 = u0 * w5 - u1 * w4 + u2 * w3 + u3 * w2 - u4 * w1 + u5 * w0;
  }
  double lam = sqrt(3.0 * f2);
  bool conv = false;
  for (int it = 0; it < 8 && !conv; ++it) {
    const double l2 = lam * lam;
    const double P = fma(fma(l2 + c2, lam, c1), lam, c0);
    const double dP = fma(fma(4.0, l2, 2.0 * c2), lam, c1);
    const double ddP = fma(12.0, l2, 2.0 * c2);
    const double d = (2.0 * P * dP) / fma(2.0 * dP, dP, -(P * ddP));
    lam = lam - d;
    conv = fabs(d) <= 1e-6 * lam;  // false for NaN
  }
  {
    const double l2 = lam * lam;
    const double dP = fma(fma(4.0, l2, 2.0 * c2), lam, c1);
    if (!(conv && dP >= 0.02 * (l2 * lam))) return false;
  }
  const double m00 = N[0][0] - lam, m11 = N[1][1] - lam, m22 = N[2][2] - lam, m33 = N[3][3] - lam;
  const double m01 = N[0][1], m02 = N[0][2], m03 = N[0][3], m12 = N[1][2], m13 = N[1][3], m23 = N[2][3];
  const double u0 = m00 * m11 - m01 * m01;
  const double u1 = m00 * m12 - m02 * m01;
  const double u2 = m00 * m13 - m03 * m01;
  const double u3 = m01 * m12 - m02 * m11;
  const double u4 = m01 * m13 - m03 * m11;
  const double w1 = m02 * m23 - m22 * m03;
  const double w2 = m02 * m33 - m23 * m03;
  const double w3 = m12 * m23 - m22 * m13;
  const double w4 = m12 * m33 - m23 * m13;
  const double w5 = m22 * m33 - m23 * m23;
  const double a00 = m11 * w5 - m12 * w4 + m13 * w3;
  const double a01 = -m01 * w5 + m02 * w4 - m03 * w3;
  const double a02 = m13 * u5 - m23 * u4 + m33 * u3;
  const double a03 = -m12 * u5 + m22 * u4 - m23 * u3;
  const double a11 = m00 * w5 - m02 * w2 + m03 * w1;
  const double a12 = -m03 * u5 + m23 * u2 - m33 * u1;
  const double a13 = m02 * u5 - m22 * u2 + m23 * u1;
  const double a22 = m03 * u4 - m13 * u2 + m33 * u0;
  const double a23 = -m02 * u4 + m12 * u2 - m23 * u0;
  const double a33 = m02 * u3 - m12 * u1 + m22 * u0;
  (void)w0;
  // row of the largest |diagonal| (first one on ties), selected without dynamic indexing
  double best = fabs(a00);
  q[0] = a00; q[1] = a01; q[2] = a02; q[3] = a03;
  if (fabs(a11) > best) { best = fabs(a11); q[0] = a01; q[1] = a11; q[2] = a12; q[3] = a13; }
  if (fabs(a22) > best) { best = fabs(a22); q[0] = a02; q[1] = a12; q[2] = a22; q[3] = a23; }
  if (fabs(a33) > best) { best = fabs(a33); q[0] = a03; q[1] = a13; q[2] = a23; q[3] = a33; }
  return best > 0.0;
}

}  // namespace cs
