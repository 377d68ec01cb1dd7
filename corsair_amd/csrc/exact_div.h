// x / n for a small integer n without the f64 division expansion: one multiplication by the correctly rounded reciprocal and
// one fma-based correction (Markstein's division step: P. Markstein, "Computation of elementary functions on the IBM RISC
// System/6000 processor", IBM J. Res. Dev. 34(1), 1990; with the divisor known in advance: Brisebarre, Muller, Raina,
// "Accelerating correctly rounded floating-point division when the divisor is known in advance", IEEE TC 53(8), 2004).
// Shared by k_ransac_hyp (ransac_hyp.hip) and the CPU sweep tools/div_sweep.cpp, which compares it with `/`.
//
// Claim: for an integer 1 <= n <= 64, r = RN(1 / n) and a double x with 2^-900 <= |x| < 2^901,
//   q0 = RN(x r),  e = RN(x - q0 n) (one fma),  q = RN(q0 + e r) (one fma)      gives      q = RN(x / n).
// Proof (Q = x / n, u = 2^-53; nothing below leaves the normal range for such x):
//   * r = (1 + d) / n and q0 = Q (1 + d)(1 + d'), |d|, |d'| <= u, so |x - q0 n| <= |x| (2u + u^2).
//   * q0 n and x are multiples of ulp(q0) (n is an integer; x is a multiple of ulp(x), and ulp(x) >= ulp(q0): for n >= 2
//     because |q0| <= |x| (1 + 2u) / 2, for n = 1 because r = 1 exactly and q0 = x), so
//     x - q0 n = k ulp(q0) with |k| < 2^9: representable, the fma returns e = x - q0 n EXACTLY, and Q = q0 + e / n.
//   * the last fma rounds q0 + e r = Q + (e / n) d, off Q by at most |Q| (2u + u^2) u < |Q| 2^-104.
//   * Q is never a midpoint of two doubles, and not within |Q| 2^-62 of one: for a midpoint mu, a multiple of g / 2 with
//     g the spacing of the doubles in Q's binade (g / 4 at the lower edge of the binade), x - n mu is a multiple of g / 4
//     (x is a multiple of ulp(x) >= g), and it is not 0 because n mu needs 54 significant bits; so
//     |Q - mu| >= g / (4 n) >= g / 256 > |Q| 2^-62.
//   Hence Q and the value the last fma rounds lie strictly between the same two midpoints (or Q is a double and the
//   perturbation is below a quarter of the spacing): q = RN(Q).                                                      []
// Enforced in code: exact_div_ok() admits only finite x with 2^-900 <= |x| < 2^901 (zeros, subnormals, infinities and NaN
// take the plain division), exact_div_recip() returns 0 -- "always divide" -- unless n is an integer in [1, 64].
// tools/div_sweep.cpp runs > 10^9 operands (random, and the adversarial ones: significands of all ones or one off, powers of
// two, signed zeros, the smallest sums of f32 values, n = 3 .. 64) through both: 0 mismatches.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CS_XDIV_FN __host__ __device__ inline
#else
#include <math.h>
#define CS_XDIV_FN static inline
#endif

namespace cs {

// the reciprocal to hand to exact_div(), or 0 when the sequence is not proven for this divisor (the caller divides)
CS_XDIV_FN double exact_div_recip(double n) {
  return (n >= 1.0 && n <= 64.0 && n == (double)(int)n) ? 1.0 / n : 0.0;
}

// 2^-900 <= |x| < 2^901 (biased exponent in [123, 1923]); false for 0, subnormals, infinities and NaN
CS_XDIV_FN bool exact_div_ok(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof(b));
  return (uint32_t)((b >> 52) & 0x7ffu) - 123u <= 1800u;
}

// RN(x / n) for exact_div_ok(x) and r = exact_div_recip(n) != 0
CS_XDIV_FN double exact_div(double x, double n, double r) {
  const double q0 = x * r;
  const double e = fma(-q0, n, x);
  return fma(e, r, q0);
}

}  // namespace cs
