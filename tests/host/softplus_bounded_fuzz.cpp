// softplus_bounded_fuzz.cpp -- TEST INFRASTRUCTURE: softplus_bounded of csrc/amwg_math.h (the certified logistic pass's log(1 + e^x): exp_bounded, a quotient
// without the general division's exponent juggling, a polynomial) against softplus in __float128 (libquadmath) on the host, over the arguments
// tests/host/softplus_fuzz.cpp walks restricted to |x| <= 690 -- random arguments, arguments whose exp() lands next to the thresholds of fdlibm's log1p, the edges
// of the reference's straight line (-20, 36), the cut at 64 and the ends of the range.  Prints the largest ABSOLUTE error, to be compared with
// kSoftplusBoundedAbs (the derived bound must hold with room: exit status 1 if it does not), and the largest one for |x| <= 1.
//   softplus_bounded_fuzz [cases] [pairs.bin]      pairs.bin: every argument with the host's value, 2 doubles each (tests/test_gpu_logit_tail.py: the device
//   build must give the same bits)
// g++ -std=c++17 -O2 -ffp-contract=off -I bayes.js_amd/csrc tests/host/softplus_bounded_fuzz.cpp -lquadmath
#include <quadmath.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "amwg_math.h"

using namespace amwg;

static long seen = 0, bad_regs = 0;
static double worst = 0.0, worst_at = 0.0, worst_small = 0.0;
static FILE *pairs = nullptr;
static void check(double x) {
  if (!(std::fabs(x) <= 690.0)) return;
  const double got = softplus_bounded(x), got_r = softplus_bounded(x, softplus_regs());
  if (memcmp(&got, &got_r, 8) != 0) ++bad_regs;
  const __float128 q = (__float128)x, want = (q > 0 ? q : 0) + log1pq(expq(q > 0 ? -q : q));
  const double err = (double)fabsq((__float128)got - want);
  ++seen;
  if (!(err <= worst)) { worst = err; worst_at = x; }      // (a NaN error would stick)
  if (std::fabs(x) <= 1.0 && !(err <= worst_small)) worst_small = err;
  if (pairs) { const double rec[2] = {x, got}; fwrite(rec, 8, 2, pairs); }
}

int main(int argc, char **argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 1000000;
  if (argc > 2) pairs = fopen(argv[2], "wb");
  std::mt19937_64 rng(777);
  auto bits = [](uint64_t u) { double v; memcpy(&v, &u, 8); return v; };
  std::uniform_real_distribution<double> U(-8.0, 8.0), V(-22.0, 38.0), W(-690.0, 690.0);
  for (long c = 0; c < cases; ++c) {
    check(U(rng));
    check(V(rng));
    if (c % 4 == 0) check(W(rng));
    const uint64_t e = 1023 - 60 + rng() % 67;          // 2^-60 .. 2^6
    check(bits(((rng() & 1) << 63) | (e << 52) | (rng() & 0x000fffffffffffffull)));
  }
  // exp(x) next to sqrt(2) - 1, 2^-29, 2^53 and a few plain values
  const uint32_t vw[] = {0x3FDA827Au, 0x3e200000u, 0x43400000u, 0x3ff00000u, 0x3fe00000u, 0x40000000u};
  for (uint32_t h : vw)
    for (int d = -3; d <= 3; ++d)
      for (long c = 0; c < cases / 20 + 8; ++c) {
        uint32_t lo = (uint32_t)rng();
        if (c == 0) lo = 0;
        if (c == 1) lo = 0xffffffffu;
        const double x = std::log(bits(((uint64_t)(h + d) << 32) | lo));
        check(x); check(std::nextafter(x, 1e300)); check(std::nextafter(x, -1e300));
      }
  // 1 + exp(x) = m 2^k with m next to sqrt(2) and next to 1 / 2, k = 0 .. 52
  const uint32_t mw[] = {0x3ff6a09eu, 0x3ff00000u, 0x3ffffffdu, 0x3ff00004u, 0x3ff80000u};
  for (uint32_t h : mw)
    for (int d = -3; d <= 3; ++d)
      for (long c = 0; c < cases / 10 + 8; ++c) {
        const double m = bits(((uint64_t)(h + d) << 32) | (uint32_t)rng());
        const int k = (int)(rng() % 53);
        const double t = std::ldexp(m, k) - 1.0;
        if (!(t > 0)) continue;
        const double x = std::log(t);
        check(x); check(std::nextafter(x, 1e300)); check(std::nextafter(x, -1e300));
      }
  // the edges: the reference's straight line, this function's cut at 64 and its range, exp_bounded's reduction points, binade ends below 690
  const double ed[] = {-20.0, 36.0, -20.10126823623841, 36.7368005696771, 30.0, 0.0, -0.0, 1.0, -1.0, 64.0, -64.0, 690.0, -690.0, 512.0, -512.0, 256.0, 689.9,
                       1e-300, -1e-300, 5e-324, 0.34657359027997264, -0.34657359027997264, 1.0397207708399179, -1.0397207708399179, -0.8813735870195429,
                       0.8813735870195429, 0.6931471805599453, -0.6931471805599453};
  for (double x : ed)
    for (int s = -40; s <= 40; ++s) {
      double y = x;
      for (int j = 0; j < (s < 0 ? -s : s); ++j) y = std::nextafter(y, s < 0 ? -1e300 : 1e300);
      check(y);
    }
  if (pairs) fclose(pairs);
  printf("arguments=%ld max_abs_error=%.6e at x=%a (|x| <= 1: %.6e) kSoftplusBoundedAbs=%a regs_vs_literals_mismatches=%ld\n", seen, worst, worst_at, worst_small,
         kSoftplusBoundedAbs, bad_regs);
  if (seen < 1000) { printf("coverage too thin\n"); return 2; }
  return (worst <= kSoftplusBoundedAbs && bad_regs == 0) ? 0 : 1;
}
