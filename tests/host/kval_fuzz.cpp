// kval_fuzz.cpp -- TEST INFRASTRUCTURE: the exact fast-forward of K-valued sequential sums (csrc/amwg_kval.h, the same source the
// kernels compile) against the plain fp64 loop, on the host, over random and adversarial cases (addends with trailing zero bits tie
// in reachable binades; powers of two; -inf / NaN / positive addends; sums that start positive; sums that start far above every addend).
// It also says what it REACHED: a census follows the plain sum and classifies every visit of a binade the header may fast-forward (acc < 0, finite, exponent >=
// the largest addend's + 1) by the definitions of the header's comment -- the counters are the harness's own, nothing is read from the code under test.
//   g++ -std=c++17 -O2 -ffp-contract=off -I bayes.js_amd/csrc tests/host/kval_fuzz.cpp -o kval_fuzz && ./kval_fuzz [cases]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "amwg_kval.h"

using namespace amwg;

struct Tables { std::vector<uint32_t> tab; std::vector<uint8_t> idx; };
static Tables tables(const std::vector<uint8_t> &v, int K) {      // same recipe as translate.js kValuedTables
  const int N = (int)v.size();
  const size_t W = k_valued_words(N);
  Tables t;
  t.tab.assign((size_t)2 * K * W, 0u);
  t.idx = v;
  for (int i = 0; i < N; ++i) t.tab[((size_t)i >> 5) * (2 * K) + K + v[i]] |= 1u << (i & 31);
  for (size_t w = 1; w < W; ++w)
    for (int k = 0; k < K; ++k) t.tab[w * (2 * K) + k] = t.tab[(w - 1) * (2 * K) + k] + (uint32_t)__builtin_popcount(t.tab[(w - 1) * (2 * K) + K + k]);
  return t;
}

// visits by class: no tie and some d != 0 (bisection) | one tying addend, the block walk moved at least one block | of those, the binade was then left (inside a
// block: the walk breaks, the rest goes term by term) | one tying addend, left before the end of the block it was entered in | two or more tying addends (term by
// term) | no tie, every d = 0 (stalled) | some but not all d = 0
struct Census { long tie_free = 0, one_tie_walked = 0, one_tie_walked_left = 0, one_tie_short = 0, several_ties = 0, stalled = 0, partial_zero = 0; };
static uint64_t bits_of(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

template <int K>
static void census(const double (&cs)[K], double acc0, const std::vector<uint8_t> &v, Census *cen) {
  const int N = (int)v.size();
  int ek[K], emax = 0;
  uint64_t mk[K];
  for (int k = 0; k < K; ++k) {
    const uint64_t b = bits_of(-cs[k]);
    ek[k] = (int)(b >> 52);
    mk[k] = (b & 0x000fffffffffffffull) | 0x0010000000000000ull;
    if (!(cs[k] < 0 && ek[k] > 0 && ek[k] < 0x7ff)) return;      // summed term by term: no visits
    emax = ek[k] > emax ? ek[k] : emax;
  }
  auto exponent = [&](double a) { const int e = (int)(bits_of(-a) >> 52); return (e >= emax + 1 && e < 0x7ff) ? e : 0; };
  double acc = acc0;
  int i = 0;
  while (i < N) {
    const int e = exponent(acc), i0 = i;
    double at_block_end = acc;      // the sum after the last observation of the block the visit was entered in (or after the last observation of all)
    const int block_end = ((i0 >> 5) + 1) * 32 < N ? ((i0 >> 5) + 1) * 32 : N;
    while (i < N && exponent(acc) == e) { acc = acc + cs[v[i]]; ++i; if (i == block_end) at_block_end = acc; }
    if (e == 0) continue;
    int n_tie = 0, zeros = 0;
    for (int k = 0; k < K; ++k) {
      const int s = e - ek[k];
      uint64_t d = 0;
      if (s < 54) {
        const uint64_t r = mk[k] & ((1ull << s) - 1ull), h = 1ull << (s - 1);
        n_tie += r == h;
        d = (mk[k] >> s) + (r > h ? 1u : 0u);
      }
      zeros += d == 0;
    }
    if (zeros != 0 && zeros != K) ++cen->partial_zero;
    if (n_tie >= 2) ++cen->several_ties;
    else if (n_tie == 1) {
      const bool moved = i >= block_end && exponent(at_block_end) == e;      // the whole rest of the entry block stayed inside the binade
      if (!moved) ++cen->one_tie_short;
      else { ++cen->one_tie_walked; if (exponent(acc) != e) ++cen->one_tie_walked_left; }
    } else if (zeros == K) ++cen->stalled;
    else ++cen->tie_free;
  }
}

template <int K>
static long run(long cases, uint64_t seed, long *forced, Census *cen) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  long bad = 0;
  for (long c = 0; c < cases; ++c) {
    const int N = (c % 7 == 0) ? (int)(rng() % 30000) : (int)(rng() % 900);
    std::vector<double> w(K);
    double tot = 0;
    for (auto &x : w) { x = (c % 4 == 0) ? U(rng) * U(rng) * U(rng) : U(rng); tot += x; }
    std::vector<uint8_t> v((size_t)N);
    for (auto &x : v) { double u = U(rng) * tot; int k = 0; while (k < K - 1 && u > w[k]) { u -= w[k]; ++k; } x = (uint8_t)k; }
    const Tables t = tables(v, K);
    const KValData B{t.tab.data(), t.idx.data(), N};
    double cs[K];
    auto trail = [&](double x, int z, bool setbit) { uint64_t u; memcpy(&u, &x, 8); u = (u >> z) << z; if (setbit) u |= 1ull << z; memcpy(&x, &u, 8); return x; };
    for (int k = 0; k < K; ++k) {
      cs[k] = -std::exp(U(rng) * 15 - 12);
      if (c % 3 != 0) { cs[k] = trail(cs[k], (int)(rng() % 40), rng() & 1); }
    }
    if (c % 3 != 0) ++*forced;
    if (c % 97 == 0) cs[0] = -1.0;
    if (c % 89 == 0) cs[K - 1] = -0.5;
    if (c % 1013 == 0) cs[0] = -INFINITY;
    if (c % 1019 == 0) cs[K - 1] = NAN;
    if (c % 1021 == 0) cs[0] = 0.25;
    if (c % 53 == 0) for (int k = 1; k < K; ++k) cs[k] = cs[0] * (double)(k + 1);      // (a log-linear family: exact multiples tie together)
    double acc0 = (c % 2) ? -std::exp(U(rng) * 30 - 5) : (U(rng) - 0.5) * 6;
    if (c % 211 == 0) acc0 = 0.0;
    if (c % 101 == 0) acc0 = -std::ldexp(1.0, 40 + (int)(c % 45));      // far above the addends: some or all of them are below half an ulp
    census<K>(cs, acc0, v, cen);
    const double got = k_valued_sum<K>(acc0, cs, B);
    double want = acc0;
    for (int i = 0; i < N; ++i) want = want + cs[v[i]];
    if (memcmp(&got, &want, 8) != 0 && !(got != got && want != want)) {
      if (bad < 5) printf("MISMATCH K=%d case %ld N=%d acc0=%a got=%a want=%a\n", K, c, N, acc0, got, want);
      ++bad;
    }
  }
  return bad;
}

int main(int argc, char **argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 6000;
  long forced = 0, bad = 0;
  Census cen;
  bad += run<1>(cases / 4, 1, &forced, &cen);
  bad += run<2>(cases, 2, &forced, &cen);
  bad += run<3>(cases, 3, &forced, &cen);
  bad += run<5>(cases, 5, &forced, &cen);
  bad += run<8>(cases, 8, &forced, &cen);
  bad += run<16>(cases / 2, 16, &forced, &cen);
  printf("visits: tie_free=%ld one_tie_walked=%ld one_tie_walked_left=%ld one_tie_short=%ld several_ties=%ld stalled=%ld partial_zero=%ld\n", cen.tie_free,
         cen.one_tie_walked, cen.one_tie_walked_left, cen.one_tie_short, cen.several_ties, cen.stalled, cen.partial_zero);
  printf("cases_per_K=%ld forced_trailing_zero_addends=%ld mismatches=%ld\n", cases, forced, bad);
  return bad ? 1 : 0;
}
