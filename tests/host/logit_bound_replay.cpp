// logit_bound_replay.cpp -- TEST INFRASTRUCTURE (host only): the derivation behind the certified logistic tail (csrc/amwg_gtail.h glm_tail_approx<LogitLink> and its eps),
// replayed in QUAD precision, in the manner of bound_replay.cpp.
//
// The derivation says: the reference's expression E (fp64: the head, then one running sum over the terms y eta - log1p_exp_v8(eta)) and the pass's value A (fp64:
// per-lane sums of eta y by fused steps and of softplus_bounded(eta), butterflies, their difference) both approximate one REAL number R -- formed from the same fp64
// eta_i, which are the reference's own on both sides -- within |E - R| <= bE and |A - R| <= bA, and the bound handed to the stepper is eps >= 2 (bE + bA).  Here E
// and A are computed in fp64 with those operations and orders, R in __float128, and the three inequalities are checked with the constants AS WRITTEN in the comment
// of amwg_gtail.h: random states and adversarial ones (eta next to 0, +-36, +-690; y in {0, 1}, all zero, all one, real weights of both signs; n in {64, 65, 517, 1e4}).
// Prints the worst ratios; exit 1 if a half exceeds 1, |A - E| / eps exceeds 0.5 (the bar tests/test_gpu_bound_audit.py sets), or the pieces exceed eps.
//   g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -I bayes.js_amd/csrc tests/host/logit_bound_replay.cpp -lquadmath
#include <quadmath.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "amwg_math.h"      // softplus_bounded, log1p_exp_v8, log_v8: the kernel's own sources compiled for the host

using namespace amwg;
typedef __float128 quad;
static const double U = 0x1p-53;
static double worst_E = 0, worst_A = 0, worst_eps = 0;
static long n_cases = 0, n_skipped = 0, n_pieces_over = 0, n_violations = 0;
static std::string worst_name;

static double absq(quad v) { return (double)(v < 0 ? -v : v); }
static quad softplusq(quad x) { return (x > 0 ? x : 0) + log1pq(expq(x > 0 ? -x : x)); }

// the closure: lp = sum_k ld.norm(b[k], 0, 10);  for i: eta = b0 + b1 x1[i] + b2 x2[i];  lp += y[i] eta - log1p(exp(eta))
static void logit_case(const char *name, const std::vector<double> &x1, const std::vector<double> &x2, const std::vector<double> &y, const double (&b)[4]) {
  const int n = (int)y.size();
  const double c0 = -0.5 * log_v8(2 * 3.141592653589793) - log_v8(10.0), den0 = 200.0;
  std::vector<double> eta(n);
  for (int i = 0; i < n; ++i) eta[i] = (b[0] + (b[1] * x1[i])) + (b[2] * x2[i]);      // (the closure's own statements: the same bits on both sides)
  // the head: four additions; their values, magnitudes and count
  double head[4], Hm = 0, Hc = 4;
  for (int k = 0; k < 4; ++k) { head[k] = c0 - (b[k] * b[k]) / den0; Hm += std::fabs(head[k]); }
  // E: one running sum, the head as the closure states it, then the terms in the order of i
  double E = 0;
  for (int k = 0; k < 4; ++k) E += head[k];
  for (int i = 0; i < n; ++i) E += y[i] * eta[i] - log1p_exp_v8(eta[i]);
  // R: the real number both approximate
  quad R = 0;
  for (int k = 0; k < 4; ++k) R += (quad)head[k];
  for (int i = 0; i < n; ++i) R += (quad)y[i] * (quad)eta[i] - softplusq((quad)eta[i]);
  // A: the head in the lanes' order (lane k of the chain's 16 holds term k; a butterfly over 16), the wavefront's pass (lane l holds observations l, l + 64, ...),
  // butterflies over 64 of the differences and of the softplus sums
  double hp[16] = {0};
  for (int k = 0; k < 4; ++k) hp[k] = head[k];
  for (int off = 1; off < 16; off <<= 1) { double w[16]; for (int l = 0; l < 16; ++l) w[l] = hp[l] + hp[l ^ off]; std::copy(w, w + 16, hp); }
  const double P = hp[0];
  const SoftplusRegs K = softplus_regs();
  double t1[64], t2[64], H = 0;
  for (int l = 0; l < 64; ++l) {
    t1[l] = t2[l] = 0;
    for (int i = l; i < n; i += 64) {
      H = std::fmax(H, std::fabs(eta[i]));
      t1[l] = std::fma(eta[i], y[i], t1[l]);
      t2[l] += softplus_bounded(eta[i], K);
    }
  }
  double e1[64], e2[64];
  for (int l = 0; l < 64; ++l) { e1[l] = t1[l] - t2[l]; e2[l] = t2[l]; }
  for (int off = 1; off < 64; off <<= 1) { double w[64], z[64]; for (int l = 0; l < 64; ++l) { w[l] = e1[l] + e1[l ^ off]; z[l] = e2[l] + e2[l ^ off]; } std::copy(w, w + 64, e1); std::copy(z, z + 64, e2); }
  const double L = e2[0], A = P + e1[0];
  double Y = 0;
  for (int i = 0; i < n; ++i) Y += std::fabs(y[i]);
  Y *= 1 + n * 0x1p-52;      // (the translator's Y: pushed up)
  const double W = Hm + H * Y + L + (double)n;
  const double eps = (H <= 690.0) ? (W * ((double)n + (double)(n / 32) + 2.0 * Hc + 200.0) * U + (double)n * kSoftplusBoundedAbs) * 1.25 : INFINITY;
  // amwg_gtail.h, the pieces: E -- the reference's softplus 2 u (n + L), the product u H Y, the subtraction u (H Y + L), the running sum of Hc + n additions;
  // A -- softplus_bounded n kAbs, the head in the lanes' order Hc u Hm, the lanes' sums and butterflies (n / 64 + 7) u (H Y + L), the difference and the closing sum 2 u W
  const double bE = U * (2 * ((double)n + L) + H * Y + (H * Y + L) + (Hc + n) * W);
  const double bA = (double)n * kSoftplusBoundedAbs + U * (Hc * Hm + (n / 64.0 + 7.0) * (H * Y + L) + 2 * W);
  if (!(eps < INFINITY) || !(std::fabs(E) < INFINITY)) { ++n_skipped; return; }      // (a non-finite bound: the stepper evaluates the expression)
  ++n_cases;
  const double rE = absq((quad)E - R) / bE, rA = absq((quad)A - R) / bA, re = std::fabs(A - E) / eps;
  if (rE > worst_E) worst_E = rE;
  if (rA > worst_A) worst_A = rA;
  if (re > worst_eps) { worst_eps = re; worst_name = name; }
  if (rE > 1 || rA > 1 || re > 0.5) { ++n_violations; printf("VIOLATION %s n=%d: |E-R|/bE %.3g  |A-R|/bA %.3g  |A-E|/eps %.3g\n", name, n, rE, rA, re); }
  if (bE + bA > eps) { ++n_pieces_over; if (n_pieces_over <= 5) printf("PIECES %s n=%d: bE + bA = %.3g > eps = %.3g\n", name, n, bE + bA, eps); }
}

int main(int argc, char **argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 20;
  std::mt19937_64 g(20261016);
  std::normal_distribution<double> N01(0.0, 1.0);
  std::uniform_real_distribution<double> U01(0.0, 1.0);
  for (int rep = 0; rep < reps; ++rep)
    for (int n : {64, 65, 517, 10000}) {
      std::vector<double> x1(n), x2(n), y01(n), y0(n, 0.0), y1(n, 1.0), w(n);
      for (int i = 0; i < n; ++i) {
        x1[i] = i == 0 ? 2.0 : i == 1 ? -2.0 : 4 * U01(g) - 2;
        x2[i] = 2 * U01(g) - 1;
        y01[i] = U01(g) < 1 / (1 + std::exp(-(0.3 + 0.9 * x1[i] - 0.6 * x2[i]))) ? 1.0 : 0.0;
        w[i] = i % 37 == 5 ? -0.75 * U01(g) : 3 * U01(g);
      }
      const double posterior[4] = {0.3 + 0.1 * N01(g), 0.9 + 0.1 * N01(g), -0.6 + 0.1 * N01(g), N01(g)};
      const double zero[4] = {1e-9 * N01(g), 1e-9 * N01(g), 1e-9 * N01(g), 0.0};      // eta next to 0
      const double wide[4] = {3 * N01(g), 5 * N01(g), 5 * N01(g), 0.0};
      const double at36[4] = {1e-3 * N01(g), 18.0 + 1e-3 * N01(g), 1e-3 * N01(g), 0.0};      // eta in [-36, 36]: the ends of the reference's straight line
      const double below20[4] = {-30.0 + N01(g), 3.0, 0.0, 0.0};                              // eta in [-36, -24]
      const double above36[4] = {60.0 + N01(g), 10.0, 1.0, 0.0};                              // eta in [40, 80]
      const double at690[4] = {0.0, 344.9 + 0.09 * U01(g), 0.0, 0.0};                         // max |eta| within 0.4 of the cut-off
      const double beyond[4] = {0.0, 345.5, 0.0, 0.0};                                       // beyond it: no finite bound (skipped)
      const double one_sided[4] = {600.0 + 50 * U01(g), 10.0, 5.0, 0.0};                      // every eta large and positive
      for (const auto *y : {&y01, &y0, &y1, &w}) {
        const char *tag = y == &y01 ? "y01" : y == &y0 ? "y_all_zero" : y == &y1 ? "y_all_one" : "weights";
        logit_case((std::string("posterior_") + tag).c_str(), x1, x2, *y, posterior);
        logit_case((std::string("eta_near_0_") + tag).c_str(), x1, x2, *y, zero);
        logit_case((std::string("wide_") + tag).c_str(), x1, x2, *y, wide);
        logit_case((std::string("eta_to_36_") + tag).c_str(), x1, x2, *y, at36);
        logit_case((std::string("eta_below_minus_20_") + tag).c_str(), x1, x2, *y, below20);
        logit_case((std::string("eta_above_36_") + tag).c_str(), x1, x2, *y, above36);
        logit_case((std::string("eta_at_690_") + tag).c_str(), x1, x2, *y, at690);
        logit_case((std::string("eta_beyond_690_") + tag).c_str(), x1, x2, *y, beyond);
        logit_case((std::string("eta_one_sided_") + tag).c_str(), x1, x2, *y, one_sided);
      }
    }
  printf("cases=%ld skipped_nonfinite=%ld worst |E-R|/bE=%.4g worst |A-R|/bA=%.4g worst |A-E|/eps=%.4g (%s) pieces_over_eps=%ld violations=%ld\n", n_cases, n_skipped, worst_E,
         worst_A, worst_eps, worst_name.c_str(), n_pieces_over, n_violations);
  if (n_cases < 100 || n_skipped < 1) { printf("coverage too thin\n"); return 2; }
  return (n_violations == 0 && n_pieces_over == 0 && worst_eps <= 0.5) ? 0 : 1;
}
