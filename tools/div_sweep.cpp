// CPU sweep for corsair_amd/csrc/exact_div.h: the multiply-and-correct sequence k_ransac_hyp uses for centroid = sum / ransac_n
// against the IEEE division, bit for bit.
//   c++ -O2 -ffp-contract=off -pthread -I corsair_amd/csrc tools/div_sweep.cpp -o div_sweep && ./div_sweep [operands] [threads]
// (a second build with -fsanitize=address,undefined checks the program itself).  Default: 1.2e9 (x, n) pairs.  Every x goes
// through the guarded form the kernel runs -- exact_div() where exact_div_ok(x), `/` elsewhere -- and, inside the proven range,
// through the bare sequence.  Operands:
//   random      53-bit significands with exponents over the range sums of <= 64 f32 values can take (2^-149 .. 2^135), and
//               actual sums of ten f32 coordinates in [-2, 2) (the kernel's own operands)
//   adversarial per n = 3 .. 64 and EVERY binary exponent (subnormals to the largest): significands of all ones, one off, zero
//               (powers of two), one; quotients next to rounding midpoints: x = RN(n (Q + ulp / 2)) and its neighbours for random Q;
//               exact multiples n k and their neighbours; +-0, the smallest f32-derived sums k 2^-149, infinities, NaN
// Prints the number of comparisons and of mismatches; exit status 1 on any mismatch.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "exact_div.h"

namespace {

uint64_t bits(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}
double from_bits(uint64_t b) {
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}
bool same(double a, double b) { return bits(a) == bits(b) || (a != a && b != b); }

struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
};

struct Tally {
  uint64_t n = 0, bad = 0;
  double first_x = 0.0, first_n = 0.0;
};

// what k_ransac_hyp's centroid_div computes for one operand
double guarded(double x, double n, double r) { return (r != 0.0 && cs::exact_div_ok(x)) ? cs::exact_div(x, n, r) : x / n; }

void check(double x, double n, double r, Tally* t) {
  volatile double want = x / n;   // (volatile: the quotient is the run-time division, never a folded constant)
  bool ok = same(guarded(x, n, r), want);
  if (r != 0.0 && cs::exact_div_ok(x)) ok = ok && same(cs::exact_div(x, n, r), want);
  ++t->n;
  if (!ok) {
    if (!t->bad) t->first_x = x, t->first_n = n;
    ++t->bad;
  }
}

void adversarial(Tally* t) {
  Rng rng{12345};
  for (int n = 3; n <= 64; ++n) {
    const double dn = (double)n, r = cs::exact_div_recip(dn);
    if (r == 0.0) ++t->bad;   // every ransac_n the library accepts must be admissible
    for (uint64_t e = 0; e <= 2046; ++e)
      for (uint64_t sig : {0xfffffffffffffull, 0xffffffffffffeull, 0x0ull, 0x1ull, 0x8000000000000ull, 0x7ffffffffffffull})
        for (uint64_t sign : {0ull, 1ull}) check(from_bits(sign << 63 | e << 52 | sig), dn, r, t);
    for (int k = 0; k <= 64; ++k) {   // zeros and the smallest sums of f32 values
      check(ldexp((double)k, -149), dn, r, t);
      check(-ldexp((double)k, -149), dn, r, t);
      check(ldexp((double)k, -126), dn, r, t);
    }
    check(-0.0, dn, r, t);
    check(INFINITY, dn, r, t);
    check(-INFINITY, dn, r, t);
    check(NAN, dn, r, t);
    for (int i = 0; i < 200000; ++i) {
      // Q + half an ulp has 54 bits; x = RN(n (Q + ulp / 2)) puts x / n as close to a midpoint as a double can
      const uint64_t q = (rng.next() >> 12) | (1ull << 52);            // 53-bit significand
      const int ex = (int)(rng.next() % 280) - 150;
      const long double mid = ((long double)q + 0.5L) * (long double)n;   // exact in 64-bit significands
      const double x0 = ldexp((double)mid, ex);
      for (double x : {x0, nextafter(x0, INFINITY), nextafter(x0, -INFINITY)}) check(x, dn, r, t);
      const double m0 = ldexp((double)q * dn, ex);                      // (nearly) exact multiples and their neighbours
      for (double x : {m0, nextafter(m0, INFINITY), nextafter(m0, -INFINITY)}) check(-x, dn, r, t);
    }
  }
  // divisors the sequence is not proven for: the reciprocal is refused
  for (double d : {0.0, 0.5, 2.5, 65.0, 1e300, -3.0, (double)NAN, (double)INFINITY})
    if (cs::exact_div_recip(d) != 0.0) ++t->bad;
}

void random_part(uint64_t count, uint64_t seed, Tally* t) {
  Rng rng{seed};
  const double r10 = cs::exact_div_recip(10.0);
  int nrot = 3;
  for (uint64_t i = 0; i < count; i += 4) {
    double x;
    const uint64_t a = rng.next();
    if ((a & 7) == 0) {   // a sum of ten f32 coordinates, as the kernel forms it
      x = 0.0;
      for (int j = 0; j < 10; ++j) x += (double)(float)((double)(int64_t)(rng.next() >> 11) * 0x1p-51 - 2.0);
    } else {
      const uint64_t ex = 1023 - 149 + rng.next() % 285;   // 2^-149 .. 2^135
      x = from_bits((a & 0x8000000000000000ull) | ex << 52 | (rng.next() >> 12));
    }
    check(x, 10.0, r10, t);   // the reference's ransac_n, and three more divisors in rotation
    for (int j = 0; j < 3; ++j) {
      nrot = nrot == 64 ? 3 : nrot + 1;
      check(x, (double)nrot, cs::exact_div_recip((double)nrot), t);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1200000000ull;
  int threads = argc > 2 ? atoi(argv[2]) : 8;
  if (threads < 1) threads = 1;
  std::vector<Tally> tally(threads + 1);
  std::vector<std::thread> pool;
  for (int i = 0; i < threads; ++i)
    pool.emplace_back(random_part, count / threads, 0x1234u + 977u * (uint64_t)i, &tally[i]);
  adversarial(&tally[threads]);
  for (auto& th : pool) th.join();
  Tally sum;
  for (const Tally& t : tally) {
    if (t.bad && !sum.bad) sum.first_x = t.first_x, sum.first_n = t.first_n;
    sum.n += t.n;
    sum.bad += t.bad;
  }
  printf("div_sweep: %llu comparisons (%llu adversarial), %llu mismatches\n", (unsigned long long)sum.n,
         (unsigned long long)tally[threads].n, (unsigned long long)sum.bad);
  if (sum.bad) printf("first mismatch: x = %a, n = %g\n", sum.first_x, sum.first_n);
  return sum.bad ? 1 : 0;
}
