// twoval_fuzz.cpp -- TEST INFRASTRUCTURE: the exact fast-forward of two-valued sequential sums (csrc/amwg_twoval.h, the same
// source the kernels compile) against the plain fp64 loop, on the host, over random and adversarial cases: independent and
// STRUCTURED data (runs, runs around 32-bit word boundaries, alternating, one value only, one value but for a few places), random
// and PLANTED starts and addends (far above the addends, just below a power of two, half an ulp on a stalled sum, a landing
// exactly on a power of two, a product n * d of 2^64).  It prints what it reached: a census of the binade visits along the plain
// sum, by the header's definitions (tests/test_translate.py asserts the counts; tests/twoval_cases.py has the full census).
//   g++ -std=c++17 -O2 -ffp-contract=off -I bayes.js_amd/csrc tests/host/twoval_fuzz.cpp -o twoval_fuzz && ./twoval_fuzz [cases]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "amwg_twoval.h"

using namespace amwg;

static std::vector<uint32_t> tables(const std::vector<uint8_t> &x) {   // same recipe as amwg_create.hip two_valued_tables
  const int N = (int)x.size();
  const size_t W = two_valued_words(N);
  std::vector<uint32_t> tab(6 * W, 0u);
  for (int i = 0; i < N; ++i) if (x[i]) tab[(size_t)i >> 5] |= 1u << (i & 31);
  for (size_t k = 1; k < W; ++k) tab[W + k] = tab[W + k - 1] + (uint32_t)__builtin_popcount(tab[k - 1]);
  for (int sym = 1; sym >= 0; --sym) {
    uint32_t *om = tab.data() + (sym ? 2 : 4) * W, *po = om + W;
    int run = 0;
    for (int i = 0; i < N; ++i) { const int v = x[i] ? 1 : 0; if (v == sym) { if (run & 1) om[(size_t)i >> 5] |= 1u << (i & 31); run = 0; } else ++run; }
    for (size_t k = 1; k < W; ++k) po[k] = po[k - 1] + (uint32_t)__builtin_popcount(om[k - 1]);
  }
  return tab;
}

// visits (maximal runs of observations added to a sum of one exponent, where the header may fast-forward: acc < 0, finite, exponent >= the larger addend's
// + 1) by class: no tie and some increment != 0 | no tie, both increments 0 | both addends tie | one ties, the other's increment even | ... odd | of those,
// visits of 64 observations or more | a tying addend of exactly half an ulp (q = 0) | visits entered ON a power of two (or the final sum is one)
struct Census { long tie_free = 0, stalled = 0, mode1 = 0, mode2 = 0, mode3 = 0, mode3_ge64 = 0, half_ulp_tie = 0, landing = 0; };
static uint64_t bits_of(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

// the plain loop, which is the reference, with the census taken along it
static double plain_sum_with_census(double acc0, double l1, double l0, const std::vector<uint8_t> &x, Census *cen) {
  const int N = (int)x.size();
  const uint64_t kMant = 0x000fffffffffffffull, kHidden = 0x0010000000000000ull;
  const uint64_t b[2] = {bits_of(-l0), bits_of(-l1)};
  const int ec[2] = {(int)(b[0] >> 52), (int)(b[1] >> 52)};
  const bool ok = l1 < 0 && l0 < 0 && ec[0] > 0 && ec[0] < 0x7ff && ec[1] > 0 && ec[1] < 0x7ff;
  const int emax = ec[0] > ec[1] ? ec[0] : ec[1];
  auto exponent = [&](double a) { const int e = (int)(bits_of(-a) >> 52); return (ok && e >= emax + 1 && e < 0x7ff) ? e : 0; };
  double acc = acc0;
  int i = 0;
  while (i < N) {
    const int e = exponent(acc), i0 = i;
    const bool on_power = (bits_of(acc) & kMant) == 0;
    while (i < N && exponent(acc) == e) { acc = acc + (x[i] ? l1 : l0); ++i; }
    if (e == 0) continue;
    if (on_power && i0 > 0) ++cen->landing;
    bool tie[2] = {false, false};
    uint64_t q[2] = {0, 0}, d[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
      const int s = e - ec[k];
      if (s >= 54) continue;
      const uint64_t m = (b[k] & kMant) | kHidden, r = m & ((1ull << s) - 1ull), h = 1ull << (s - 1);
      q[k] = m >> s; tie[k] = r == h; d[k] = q[k] + (r > h ? 1u : 0u);
    }
    if ((tie[0] && q[0] == 0) || (tie[1] && q[1] == 0)) ++cen->half_ulp_tie;
    if (tie[0] && tie[1]) ++cen->mode1;
    else if (tie[0] || tie[1]) {
      const uint64_t dn = tie[1] ? d[0] : d[1];
      if ((dn & 1ull) == 0) ++cen->mode2; else { ++cen->mode3; if (i - i0 >= 64) ++cen->mode3_ge64; }
    } else if (d[0] == 0 && d[1] == 0) ++cen->stalled;
    else ++cen->tie_free;
  }
  if (N > 0 && exponent(acc) != 0 && (bits_of(acc) & kMant) == 0 && bits_of(acc) != bits_of(acc0)) ++cen->landing;
  return acc;
}

int main(int argc, char **argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 20000;
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  long bad = 0, ties_forced = 0, structured = 0, planted = 0;
  Census cen;
  for (long c = 0; c < cases; ++c) {
    int N = (c % 7 == 0) ? (int)(rng() % 20000) : (int)(rng() % 700);
    if (c % 113 == 0) N = 8192;
    const double p_one = (c % 5 == 0) ? 0.02 : (c % 5 == 1 ? 0.97 : U(rng));
    std::vector<uint8_t> x((size_t)N);
    for (auto &v : x) v = U(rng) < p_one;
    // structured data: run parities and word boundaries are what mode 3 (one tie, the other increment odd) depends on
    const int shape = (int)(c % 11);
    if (shape >= 5) ++structured;
    if (shape == 5) { int i = 0; uint8_t v = rng() & 1; while (i < N) { int len = 1 + (int)(rng() % 130); if (len % 32 == 0) ++len; for (; len > 0 && i < N; --len) x[i++] = v; v ^= 1; } }
    if (shape == 6) { int i = 0; uint8_t v = rng() & 1; while (i < N) { int len = 32 * (1 + (int)(rng() % 3)) + (int)(rng() % 3) - 1; for (; len > 0 && i < N; --len) x[i++] = v; v ^= 1; } }
    if (shape == 7) { const uint8_t v = rng() & 1; for (int i = 0; i < N; ++i) x[i] = (uint8_t)((i & 1) ^ v); }
    if (shape == 8) { const int period = 3 + (int)(rng() % 4); const uint8_t v = rng() & 1; for (int i = 0; i < N; ++i) x[i] = (i % period == 0) ? v : (uint8_t)(v ^ 1); }
    if (shape == 9 || c % 113 == 0) { const uint8_t v = c % 113 == 0 ? 1 : (uint8_t)(rng() & 1); for (auto &y : x) y = v; }
    if (shape == 10) { const uint8_t v = rng() & 1; for (auto &y : x) y = v; const int at[4] = {0, 31, 32, N - 1}; for (int a : at) if (a >= 0 && a < N) x[a] = v ^ 1; }
    const std::vector<uint32_t> tab = tables(x);
    const size_t W = two_valued_words(N);
    const BitData B{tab.data(), tab.data() + W, tab.data() + 2 * W, tab.data() + 3 * W, tab.data() + 4 * W, tab.data() + 5 * W, N};
    double l1 = -std::exp(U(rng) * 15 - 12), l0 = -std::exp(U(rng) * 15 - 12);
    // significands ending in z zero bits tie in the binade 2^(z+1) above the addend
    auto trail = [&](double v, int z, bool setbit) { uint64_t u; memcpy(&u, &v, 8); u = (u >> z) << z; if (setbit) u |= 1ull << z; memcpy(&v, &u, 8); return v; };
    if (c % 3 != 0) { l1 = trail(l1, (int)(rng() % 32), rng() & 1); l0 = trail(l0, (int)(rng() % 32), rng() & 1); ++ties_forced; }
    if (c % 97 == 0) l1 = -1.0;
    if (c % 89 == 0) l0 = -0.5;
    if (c % 1013 == 0) l1 = -INFINITY;
    if (c % 1019 == 0) l0 = NAN;
    if (c % 1021 == 0) l1 = 0.25;
    double acc0 = (c % 2) ? -std::exp(U(rng) * 30 - 5) : (U(rng) - 0.5) * 6;
    if (c % 211 == 0) acc0 = 0.0;
    // planted starts
    if (c % 101 == 0) { acc0 = -std::ldexp(1.0, 40 + (int)(c % 45)); ++planted; }                                     // far above the addends: a stall
    if (c % 103 == 0) { acc0 = -std::nextafter(std::ldexp(1.0, (int)(rng() % 24) - 4), 0.0); ++planted; }             // just below a power of two
    if (c % 107 == 0) {                                                                                              // half an ulp (q = 0) on a sum that otherwise stalls
      const double scale = std::ldexp(1.0, (int)(rng() % 40) - 10);
      acc0 = -(std::ldexp(1.0, 53) + 2.0 * (double)(rng() % 8)) * scale;
      const double t = -1.0 * scale, o = ((rng() % 3) ? -0.25 : -1.0) * scale;
      if (rng() & 1) { l1 = t; l0 = o; } else { l1 = o; l0 = t; }
      ++planted;
    }
    if (c % 109 == 0) {                                                                                              // a landing exactly on 2^54: ulp 2, increments 1 .. 3
      const double pairs[4][2] = {{-2, -4}, {-4, -2}, {-6, -2}, {-2, -2}};
      l1 = pairs[c % 4][0]; l0 = pairs[c % 4][1];
      const int p = N ? (int)(rng() % (uint64_t)(N + 1)) : 0;
      double G = 0;
      for (int i = 0; i < p; ++i) G += x[i] ? -l1 : -l0;
      acc0 = -(std::ldexp(1.0, 54) - G);
      ++planted;
    }
    if (c % 113 == 0) { acc0 = -2.0 - 0.25 * (double)(rng() % 4); l1 = -1.0; l0 = -0.3; ++planted; }                    // 8 192 ones: n * d = 8 192 * 2^51 = 2^64
    const double got = two_valued_sum(acc0, l1, l0, B);
    const double want = plain_sum_with_census(acc0, l1, l0, x, &cen);
    if (memcmp(&got, &want, 8) != 0 && !(got != got && want != want)) {
      if (bad < 5) printf("MISMATCH case %ld N=%d acc0=%a l1=%a l0=%a got=%a want=%a\n", c, N, acc0, l1, l0, got, want);
      ++bad;
    }
  }
  printf("visits: tie_free=%ld stalled=%ld mode1=%ld mode2=%ld mode3=%ld mode3_ge64=%ld half_ulp_tie=%ld landing=%ld\n", cen.tie_free, cen.stalled, cen.mode1, cen.mode2,
         cen.mode3, cen.mode3_ge64, cen.half_ulp_tie, cen.landing);
  printf("cases=%ld structured_data=%ld planted_starts=%ld forced_trailing_zero_addends=%ld mismatches=%ld\n", cases, structured, planted, ties_forced, bad);
  return bad ? 1 : 0;
}
