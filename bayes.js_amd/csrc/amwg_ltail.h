// amwg_ltail.h -- CERTIFIED LOGISTIC TAIL of a translated closure (bayes.js_amd/translate.js logitTailPlan; amwg_kernel.h "certified decisions").
//
// A closure whose last statement is
//     for (i = 0; i < N; i++) { <statements forming eta from the state and row i of the data>;  lp += y[i] * eta - Math.log1p(Math.exp(eta)); }
// -- a logistic regression (y in {0, 1}) or any weighted variant of it, whatever the linear predictor looks like.  The reference's term is
// y eta - log1p_v8(exp_v8(eta)): fdlibm's exp, then its log1p with two quotients (amwg_math.h log1p_exp_v8, ~75 operations).  As real numbers
//     log_post = head + sum eta_i y_i - sum softplus(eta_i),   softplus(x) = log(1 + e^x),
// and that is what the pass below forms, in the manner of amwg_ptail.h (whose ScalarState / wave_uniform it shares):
//   * eta_i by the closure's OWN statements (M::ltail_eta: the same operations in the same order as the expression's pass -- bit for bit the reference's eta_i;
//     the fused linear predictor of the Poisson tail is NOT used: the expression's softplus is evaluated at the reference's eta, and so is this one);
//   * softplus by softplus_bounded (amwg_math.h: 39 operations, absolute error < kSoftplusBoundedAbs), two running sums per chain;
//   * the WAVEFRONT's pass (16 lanes per chain, four chains to a wavefront): the 64 lanes share out the OBSERVATIONS, a row -- once in registers -- is evaluated for
//     all four chains, whose parameters sit in scalar registers (M::kTailUniformState) or are read per lane from their LDS state; rows loaded a round ahead
//     (M::kTailRows) or where their first product needs them.
// The stepper gets the value with a bound eps on its distance from the expression evaluated in the REFERENCE's order (logit_tail_reference below: what this kernel
// evaluates when a uniform falls inside the bound, and what a launch leaves behind).  u = 2^-53, H = max_i |eta_i| (taken over the rows as they pass: the etas are the
// reference's own), Y = sum |y_i| (formed by the translator, rounded up), L = sum softplus(eta_i), Hm / Hc = the magnitudes / the number of the head's additions
// (M::ltail_head: HeadPair), n the observations, W = Hm + H Y + L + n >= every partial sum of magnitudes on either side (and >= n: the terms' absolute errors):
//   the reference's terms: exp_v8 is within an ulp of e^eta, log1p's derivative is below 1 and log1p_v8 is within an ulp of log1p: its softplus is within
//   2 u (1 + softplus) of the real one -- 2 u (n + L);  the product y eta rounds (unless y is 0 or 1): u H Y;  the term's subtraction: u (H Y + L) -- together
//   < 4 u W;  the reference's ONE running sum over the head's Hc terms and the n observations': (Hc + n) u W;
//   this pass: softplus_bounded, an ABSOLUTE error per observation: n kSoftplusBoundedAbs;  the head in the lanes' order Hc u Hm;  per-lane sums of n / 64 + 1 steps
//   (fused for sum eta y) and six butterfly additions on two sums (n / 64 + 7) u (H Y + L);  their difference and the closing P + tot: 2 u W.
//   In all  < u W (n + n / 64 + 2 Hc + 14) + n kSoftplusBoundedAbs;  the bound handed on is
//       eps = (u W (n + n / 32 + 2 Hc + 200) + n kSoftplusBoundedAbs) 1.25
//   (the same count and the same 1.25 as the Poisson tail's; L enters through this pass's own sum, whose relative error ~n u the slack covers many times over).
// H > 690 (exp_v8 nears its overflow, softplus_bounded leaves the range its bound is stated for), any non-finite value: eps is not finite and the stepper evaluates
// the expression.  (A NaN eta: fmax / fmin skip it, sum eta y carries it -- fma(NaN, y, .) is NaN whatever y.)  A non-finite y: the translator does not emit this plan.
// PER-DATASET CONSTANTS (M::kTailPerDataset, amwg_ptail.h TailPerDataset: translate_datasets, many datasets under ONE source): Y is not a literal of the text but the
// one slot of the f64 data array M::kTailConsts (key `#tail:consts`), formed by the translator from THAT dataset's values, rounded up the same way; M::ltail_sum_abs_y(d).
// Checked like the other bounds: tests/host/logit_bound_replay.cpp (the derivation in __float128) and tools/bound_audit.py --only logit (libamwg_audit.so
// evaluates the expression beside every certified value).
#pragma once
#include "amwg_user.h"      // (which includes this file at its end: TailApprox)
#include "amwg_ptail.h"     // ScalarState, wave_uniform
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)      // (device code throughout: the host build of a generated model -- tests/host -- sees nothing of it)
#include "amwg_kernel.h"    // butterfly
#include "amwg_math.h"
#include "amwg_rows.h"      // HeadPair
#include "amwg_types.h"

namespace amwg {

template <class M, int G, int BT>
__device__ __forceinline__ TailApprox logit_tail_approx(const StateView &S, const DataRef &d, const unsigned char *smem, int sub) {
  static_assert(G == 16, "the certified logistic tail runs four chains to a wavefront");
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int CW = 64 / G;
  const int lane = (int)(threadIdx.x & 63u);
  const HeadPair h = M::template ltail_head<G>(S, d, smem, sub);
  const double P = butterfly<1, G>(h.value), Hm = butterfly<1, G>(h.mag), Hc = butterfly<1, G>(h.cnt);
  // the four chains' states: LDS addresses, wave-uniform (the first lane of each chain's)
  typedef __attribute__((address_space(3))) const double *lds_f64;
  const uint32_t mine_off = (uint32_t)(uintptr_t)(lds_f64)S.base;
  const double *base[CW];
#pragma unroll
  for (int c = 0; c < CW; ++c) base[c] = (const double *)(lds_f64)(uintptr_t)(uint32_t)__builtin_amdgcn_readlane((int)mine_off, c * G);
  const SoftplusRegs K = softplus_regs();
  double s1[CW], ls[CW], hm = 0.0;
#pragma unroll
  for (int c = 0; c < CW; ++c) { s1[c] = 0.0; ls[c] = 0.0; }
  constexpr int n = M::kTailN;
  auto pass = [&](const auto &Sc) {
    auto consume = [&](const double (&eta)[CW], double y) {
      double sp[CW];
#pragma unroll
      for (int c = 0; c < CW; ++c) hm = __builtin_fmax(hm, __builtin_fabs(eta[c]));
#pragma unroll
      for (int c = 0; c < CW; ++c) sp[c] = softplus_bounded(eta[c], K);
#pragma unroll
      for (int c = 0; c < CW; ++c) { s1[c] = __builtin_fma(eta[c], y, s1[c]); ls[c] += sp[c]; }
    };
    if constexpr (M::kTailRows) {
      // a row is loaded a round AHEAD of its use (M::ltail_load: the translator has proved that the statements read nothing of the data but the observation's own
      // row): two row buffers, alternating -- the schedule of amwg_ptail.h, measured there
      constexpr int n_full = n / 64, rem = n % 64, pairs = n_full > 0 ? (n_full - 1) / 2 : 0, left = n_full - 2 * pairs;      // left: 0 (no full round), 1 or 2
      auto compute = [&](const typename M::TailRow &R, int i) {
        double eta[CW];
#pragma unroll
        for (int c = 0; c < CW; ++c) eta[c] = M::ltail_eta_row(Sc[c], R, i);
        consume(eta, M::ltail_y_row(R));
      };
      typename M::TailRow A, B;
      if constexpr (n_full > 0) {
        M::ltail_load(d, smem, lane, A);
        int i = lane;
        for (int k = 0; k < pairs; ++k, i += 128) {
          M::ltail_load(d, smem, i + 64, B);
          AMWG_STAGE_FENCE();
          compute(A, i);
          AMWG_STAGE_FENCE();
          M::ltail_load(d, smem, i + 128, A);
          AMWG_STAGE_FENCE();
          compute(B, i + 64);
          AMWG_STAGE_FENCE();
        }
        if constexpr (left == 2) {
          M::ltail_load(d, smem, i + 64, B);
          AMWG_STAGE_FENCE();
          compute(A, i);
          AMWG_STAGE_FENCE();
          compute(B, i + 64);
        } else {
          compute(A, i);
        }
      }
      if constexpr (rem > 0) {
        if (lane < rem) {
          M::ltail_load(d, smem, n_full * 64 + lane, A);
          compute(A, n_full * 64 + lane);
        }
      }
    } else {      // (some read of the data is not of the observation's own row: the plain loop -- every row is waited for where its first product needs it)
#pragma unroll 2
      for (int i = lane; i < n; i += 64) {
        const double y = M::ltail_y(d, smem, i);
        double eta[CW];
#pragma unroll
        for (int c = 0; c < CW; ++c) eta[c] = M::ltail_eta(Sc[c], d, smem, i);
        consume(eta, y);
      }
    }
  };
  if constexpr (M::kTailUniformState) {
    ScalarState<M::kStateN> Sc[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) {
#pragma unroll
      for (int p = 0; p < M::kStateN; ++p) Sc[c].v[p] = wave_uniform(base[c][p]);
    }
    pass(Sc);
  } else {
    StateView Sc[CW];      // (per-lane LDS reads: the loop gathers from the state by the data)
#pragma unroll
    for (int c = 0; c < CW; ++c) Sc[c].base = base[c];
    pass(Sc);
  }
  // every chain's totals over the wavefront; a lane keeps its own chain's.  H: the largest |eta| any of the four chains met (fmax skips a NaN: the sums carry it)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hm = __builtin_fmax(hm, __shfl_xor(hm, o));
  const int mine = lane / G;
  double tot = 0.0, L = 0.0;
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const double t = butterfly<1, 64>(s1[c] - ls[c]), l = butterfly<1, 64>(ls[c]);
    tot = mine == c ? t : tot;
    L = mine == c ? l : L;
  }
  double Y;
  if constexpr (TailPerDataset<M>::value) Y = M::ltail_sum_abs_y(d);
  else Y = M::ltail_sum_abs_y();
  const double H = hm;
  const double W = Hm + H * Y + L + (double)n;
  const double eps = (H <= 690.0) ? (W * ((double)n + (double)(n / 32) + 2.0 * Hc + 200.0) * 0x1p-53 + (double)n * kSoftplusBoundedAbs) * 1.25 : __builtin_inf();
  return TailApprox{P + tot, eps};
#else
  (void)S; (void)d; (void)smem; (void)sub;
  return TailApprox{0.0, __builtin_inf()};
#endif
}

// THE REFERENCE'S ORDER at G lanes per chain: the head as the closure states it (one lane's walk: M::ltail_head_sequence), then ONE running sum over the observations'
// terms -- the chain's lanes form the terms of a round of G observations side by side (the expression's own operations: y eta - log1p_exp_v8(eta) of the closure's
// eta) and the sum takes them in the order i = G k + lane, a broadcast per term: the same bits as the one-lane expression.  Slow, and run for ~1e-6 of the updates.
// Under the chain's own execution mask: the lanes it reads are its own.
template <class M, int G>
__device__ inline __attribute__((noinline)) double logit_tail_reference(const double *state, const DataRef *dp, const unsigned char *smem, int sub) {
  double acc = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
  const StateView S{state};
  const DataRef &d = *dp;
  acc = M::ltail_head_sequence(S, d, smem);
  constexpr int n = M::kTailN;
  const int base = (int)(threadIdx.x & 63u) & ~(G - 1);
  for (int k0 = 0; k0 < n; k0 += G) {
    const int cnt = n - k0 < G ? n - k0 : G, i = sub < cnt ? k0 + sub : k0;
    const double eta = M::ltail_eta(S, d, smem, i);
    const double term = M::ltail_y(d, smem, i) * eta - log1p_exp_v8(eta);
    for (int l = 0; l < cnt; ++l) acc += __shfl(term, base + l, 64);
  }
#else
  (void)state; (void)dp; (void)smem; (void)sub;
#endif
  return acc;
}

}  // namespace amwg
#endif
