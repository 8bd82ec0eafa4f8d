// amwg_cdf.h -- the two distribution functions behind the posterior predictive calibration call (amwg_last_sample_dataset_predictive; amwg_predictive.hip): erfc
// over the whole line, hence the Normal CDF, and the Poisson CDF as the pair (P(Y <= y), P(Y <= y - 1)).  Hand-written fp64 in the project's own exp_v8 / log_v8
// (amwg_math.h); no call into a device or host math library, and the same operations on the device and on the host, so tests/test_cdf_host.py checks on a CPU what
// the kernels run.  Every operation rounds once; the only fused ones are the explicit fma of the split square.  Not a source of the step kernels (tools/build_id.py).
//
// ERFC.  For x >= 0 (erfc(-x) = 2 - erfc(x)), five polynomial pieces, Chebyshev fits to below 2^-57 of the function (tools/cdf_coefficients.py prints them):
//   [0, 1/2)   1 - x A(x^2 - 1/8)                                      (erfc >= 0.47 there: the subtraction costs no accuracy)
//   [1/2, 3/2) exp(-x^2) B(x - 1)        [3/2, 3)  exp(-x^2) C(x - 9/4)
//   [3, 6)     exp(-x^2) D(w - 5/72) / x    [6, 28]  exp(-x^2) E(w - 1/64) / x,  w = 1 / x^2
// THE SPLIT SQUARE: h = x * x rounded and l = fma(x, x, -h) exactly its error; exp(-x^2) = exp(-h) (1 - l), |l| <= 2^-44: the tail keeps RELATIVE accuracy, where
// exp(-(x * x)) alone would lose log2(x^2) bits.  Beyond h = 600 the exponential is taken as exp(-h / 2)^2 with the last product last, so a subnormal result is
// rounded once.  x > 28 is taken at 28 and gives 0 (erfc(27.3) < 2^-1075); erfc(-inf) = 2, erfc(+inf) = 0, erfc(NaN) = NaN.  A lane takes one piece; a
// wavefront whose lanes differ pays for the pieces its lanes take.
// BOUND (measured against mpmath at 50 digits over the grid of tests/test_cdf_host.py, stated as 4 x the largest seen, rounded up to a power of two; tests/README.predictive.md):
//   |erfc(x) - exact| <= kErfcRel * exact  wherever exact >= 2^-1022, and <= 2^-1074 (one subnormal step) below.
//
// THE POISSON PAIR, from an integer y >= 0, lfact = log(y!), lam > 0 and lg = log(lam):
//   p = exp(fma(y, lg, -lam) - lfact), the mass at y -- formed in the exponent, so it stays accurate where exp(-lam) underflows;
//   y <= lam: the lower sums.  P(Y <= y - 1) = p (y / lam) (1 + (y - 1) / lam (1 + ...)), summed term by term toward 0, the terms falling, with an EARLY STOP once a
//             term is below 2^-56 of the sum; P(Y <= y) = that + p.
//   y >  lam: the upper sums, the complement: Q = P(Y > y) = p lam / (y + 1) (1 + lam / (y + 2) (1 + ...)) with the same stop; P(Y <= y) = 1 - Q and
//             P(Y <= y - 1) = 1 - (Q + p).  Neither F nor 1 - F is formed by cancellation on either side.
//   The loop runs about 9 sqrt(lam) times at the mode, less in the tails; it is capped at kPoisMaxTerms, and a pair that would need more (lam beyond about 5e7 near
//   its mode) is NaN.  A y that is negative, not an integer or not finite gives NaN; lam = 0 is the point mass at 0; lam = +inf or NaN gives NaN.
// BOUND (the same procedure): with exact pair (F, Fm) and tail t = min(exact, 1 - exact):  |value - exact| <= kPoisRel * t + 2^-53  (the last term: 1 - Q rounded).
//   The relative part is the exponent's: |y lg| + lam + lfact reach 3e6 on the grid, and one rounding of that is 2^-53 * 3e6 in p.
#pragma once
#include "amwg_ld.h"      // kInf
#include "amwg_math.h"

namespace amwg {

constexpr double kErfcRel = 0x1p-49;      // see BOUND above
constexpr double kPoisRel = 0x1p-29;
constexpr int kPoisMaxTerms = 1 << 16;

namespace cdf {
constexpr double kA[9] = {0x1.8b4b60851826bp-20, -0x1.c0bb73b49d962p-17, 0x1.c5c56ebdde4c3p-14, -0x1.934038e557f46p-11, 0x1.35219bf052861p-8, -0x1.8f7e682ca9335p-6, 0x1.a6db683de1274p-4, -0x1.658407f4c04bbp-2, 0x1.15446b34ed348p+0};
constexpr double kB[18] = {-0x1.504357b3d162cp-25, 0x1.2805d34f13fa4p-23, -0x1.cd9df537d6bd2p-22, 0x1.80f28d1204b75p-20, -0x1.39cb26d313b35p-18, 0x1.ef1520bdad316p-17, -0x1.7ab1b42ac1c6cp-15, 0x1.184fa62a30f35p-13, -0x1.908223a54dd6cp-12, 0x1.135263365ae98p-10, -0x1.6af2654dad28ep-9, 0x1.c8cb958b893d1p-8, -0x1.10fcf1b559836p-6, 0x1.33cad0ef5f604p-5, -0x1.44837f8906fccp-4, 0x1.3c27283c32cbdp-3, -0x1.17c4e3f17c050p-2, 0x1.b5d8780f956b2p-2};
constexpr double kC[19] = {0x1.19e1eafb43781p-35, -0x1.362b843e7d01fp-33, 0x1.2050b175e0025p-31, -0x1.305200e6da12dp-29, 0x1.3e50ecaa2c69ep-27, -0x1.431b217113ea0p-25, 0x1.40e6fa019803cp-23, -0x1.37b8fd25062dfp-21, 0x1.27af449b8807cp-19, -0x1.117a68baebe32p-17, 0x1.ec773cc09580ep-16, -0x1.aed7ebbfe0f1fp-14, 0x1.6d7743d3bc27ep-12, -0x1.2bd251bb39fc9p-10, 0x1.da595561f7c95p-9, -0x1.6883f9919a0c6p-7, 0x1.0615670e25a7bp-5, -0x1.6a70d2bb37411p-4, 0x1.d94446d627932p-3};
constexpr double kD[15] = {0x1.8e010942912f2p+20, -0x1.2d7ace6d1cf9ap+18, 0x1.86f0a7c6c6346p+15, -0x1.454010404080fp+13, 0x1.1f04f0a2f77c5p+11, -0x1.076395350faccp+9, 0x1.0109870261f66p+7, -0x1.0dc963dde15b4p+5, 0x1.34ca11cc22e73p+3, -0x1.8905c2cc1c33fp+1, 0x1.1e292cfb5c13ap+0, -0x1.f26cb8076889cp-2, 0x1.1887f5c6e42e3p-2, -0x1.e15092db1fbdap-3, 0x1.17bb8026aa336p-1};
constexpr double kE[11] = {0x1.526ca7d3c5cdbp+16, -0x1.4d0d563def4fep+13, 0x1.83ec76a443deap+10, -0x1.01bbb9959a9d6p+8, 0x1.8167a339e7c4dp+5, -0x1.4c792e728dc20p+3, 0x1.56029b468e30bp+1, -0x1.b8ecfc309816ap-1, 0x1.837f3c28b63d2p-2, -0x1.14108e58a9bbbp-2, 0x1.1ea8c4009b459p-1};

template <int N> AMWG_HD double horner(const double (&c)[N], double t) {
  double p = c[0];
#pragma unroll
  for (int k = 1; k < N; ++k) p = p * t + c[k];
  return p;
}
}  // namespace cdf

AMWG_HD double erfc_amwg(double x) {
  if (x != x) return x + x;
  const double big = __builtin_fabs(x);
  const double a = big < 28.0 ? big : 28.0;
  double r;
  if (a < 0.5) {
    r = 1.0 - a * cdf::horner(cdf::kA, a * a - 0.125);
  } else {
    double g;      // erfc(a) exp(a^2)
    if (a < 1.5) g = cdf::horner(cdf::kB, a - 1.0);
    else if (a < 3.0) g = cdf::horner(cdf::kC, a - 2.25);
    else {
      const double inv = 1.0 / a, w = inv * inv;
      g = inv * (a < 6.0 ? cdf::horner(cdf::kD, w - 5.0 / 72.0) : cdf::horner(cdf::kE, w - 1.0 / 64.0));
    }
    const double h = a * a, l = __builtin_fma(a, a, -h);
    g = g - g * l;
    if (h < 600.0) r = exp_v8(-h) * g;
    else { const double e = exp_v8(-0.5 * h); r = (e * g) * e; }
  }
  return x < 0.0 ? 2.0 - r : r;
}

// the Normal CDF at z = (x - mean) / sd: 0.5 erfc(-z sqrt(1/2))
AMWG_HD double normal_cdf(double z) { return 0.5 * erfc_amwg(-z * 0.70710678118654752440); }

// F = P(Y <= y), Fm = P(Y <= y - 1); Q = P(Y > y), the complement of F, formed without cancellation (the kernels do not read it: the bound is stated in it)
AMWG_HD void poisson_cdf_pair(double y, double lfact, double lam, double lg, double &F, double &Fm, double &Q) {
  const double nan = __builtin_nan("");
  F = Fm = Q = nan;
  if (!(y >= 0.0 && y < 0x1p53 && y == __builtin_floor(y)) || !(lam >= 0.0 && lam < kInf)) return;
  if (lam == 0.0) { F = 1.0; Fm = y > 0.0 ? 1.0 : 0.0; Q = 0.0; return; }
  const double p = exp_v8(__builtin_fma(y, lg, -lam) - lfact);
  const bool lower = y <= lam;
  // the terms relative to p: lower side k / lam for k = y, y - 1, ... 1; upper side lam / k for k = y + 1, y + 2, ...
  const double inv = 1.0 / lam;
  double k = lower ? y : y + 1.0, term = 1.0, sum = 0.0;
  int n = 0;
  for (; n < kPoisMaxTerms; ++n) {
    if (lower && k < 1.0) break;
    term = term * (lower ? k * inv : lam / k);
    sum = sum + term;
    if (term < sum * 0x1p-56) break;
    k = lower ? k - 1.0 : k + 1.0;
  }
  if (n == kPoisMaxTerms) return;
  const double side = p * sum;      // lower: P(Y <= y - 1); upper: P(Y > y)
  if (lower) { Fm = side; F = side + p; Q = 1.0 - F; }
  else { Q = side; F = 1.0 - side; Fm = 1.0 - (side + p); }
}

}  // namespace amwg
