// pair_stream.cpp -- TEST INFRASTRUCTURE (host): the pair draw of the one-lane stream (csrc/amwg_philox.h stream_next_pair, what CoopStream<1>::next_pair of
// csrc/amwg_kernel.h calls) on a host restatement of that stream -- one block held as the two uniforms it yields, `pos` of them consumed, refilled by the draw that
// finds pos == 2 -- against ChainStream::next(), the sequential definition of the stream.  From each of the three positions a pair draw can meet (0, 1, 2), for
// every pattern of pair and single draws of length 1 .. 6, repeated until argv[1] uniforms are consumed: every value and, after every draw, the consumed count
// equal the sequential stream's, and the refills are as many as single draws alone would have made.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "amwg_philox.h"
using namespace amwg;

struct OneLaneStream {      // CoopStream<1>, restated
  uint32_t k0, k1, c2, c3;
  uint64_t b0;
  uint32_t pos;
  double u0, u1;
  long fills;
  void fill() {
    const Philox4 w = philox4x32_10((uint32_t)b0, (uint32_t)(b0 >> 32), c2, c3, k0, k1);
    u0 = u53(w.w0, w.w1); u1 = u53(w.w2, w.w3);
    ++fills;
  }
  void init(uint64_t seed, uint64_t chain, uint64_t consumed) {
    k0 = (uint32_t)seed; k1 = (uint32_t)(seed >> 32);
    c2 = (uint32_t)chain; c3 = (uint32_t)(chain >> 32);
    b0 = consumed >> 1;
    pos = (uint32_t)(consumed & 1u);
    fills = 0;
    fill();
  }
  uint64_t consumed() const { return 2 * b0 + (uint64_t)pos; }
  double next() {
    if (pos >= 2u) { b0 += 1; pos = 0u; fill(); }
    const double mine = (pos & 1u) ? u1 : u0;
    ++pos;
    return mine;
  }
  void next_pair(double &a, double &b) { stream_next_pair(*this, a, b); }
};

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0; }

int main(int argc, char **argv) {
  const long n_uniforms = argc > 1 ? atol(argv[1]) : 10000;
  // (the block number crosses 2^31 early.  argv[2], [3], [4]: another first uniform, seed and chain id -- tests/test_pair_stream.py starts on either side of the
  // carry of the block number into its high word, uniform 2^33, under several keys; argv[5] (a uniform's index): prints ChainStream's value there, for a check
  // against the numpy twin)
  const uint64_t base = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0xFFFFFFFEull;
  const uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 0) : 0x9E3779B97F4A7C15ull, chain = argc > 4 ? strtoull(argv[4], nullptr, 0) : (1ull << 32) + 12345u;
  if (argc > 5) {
    ChainStream at;
    at.init(seed, chain, strtoull(argv[5], nullptr, 0));
    const double u = at.next();
    uint64_t bits;
    memcpy(&bits, &u, 8);
    printf("uniform=%016llx\n", (unsigned long long)bits);
  }
  long bad = 0, patterns = 0, draws = 0;
  auto fail = [&](const char *what, int start, int len, unsigned bits, uint64_t at) {
    if (bad++ < 10) printf("FAIL start=%d pattern(len=%d,bits=%u) at uniform %llu: %s\n", start, len, bits, (unsigned long long)at, what);
  };
  for (int start = 0; start < 3; ++start) {
    for (int len = 1; len <= 6; ++len) {
      for (unsigned bits = 0; bits < (1u << len); ++bits) {      // bit i of the pattern: draw i is a pair (1) or a single (0)
        ++patterns;
        OneLaneStream s, singles;
        ChainStream ref;
        const uint64_t first = base + (start == 1 ? 1u : 0u);
        s.init(seed, chain, first); singles.init(seed, chain, first); ref.init(seed, chain, first);
        if (start == 2) { for (int i = 0; i < 2; ++i) { const double w = ref.next(); if (!same(s.next(), w) || !same(singles.next(), w)) fail("a single draw", start, len, bits, ref.n); } }
        if (s.pos != (uint32_t)start) fail("the starting position", start, len, bits, ref.n);
        const uint64_t begin = ref.n;
        for (int i = 0; ref.n - begin < (uint64_t)n_uniforms; i = (i + 1) % len) {
          if ((bits >> i) & 1u) {
            double a, b;
            s.next_pair(a, b);
            const double wa = ref.next(), wb = ref.next();
            const double sa = singles.next(), sb = singles.next();
            if (!same(a, wa) || !same(b, wb) || !same(sa, wa) || !same(sb, wb)) fail("a pair's values", start, len, bits, ref.n);
            draws += 2;
          } else {
            const double w = ref.next();
            if (!same(s.next(), w) || !same(singles.next(), w)) fail("a single draw", start, len, bits, ref.n);
            draws += 1;
          }
          if (s.consumed() != ref.n || singles.consumed() != ref.n) fail("the consumed count", start, len, bits, ref.n);
          if (s.pos > 2u) fail("a position outside 0 .. 2", start, len, bits, ref.n);
        }
        if (s.fills != singles.fills) fail("not the refills that single draws make", start, len, bits, ref.n);
      }
    }
  }
  printf("patterns=%ld draws=%ld failures=%ld\n", patterns, draws, bad);
  return bad ? 1 : 0;
}
