// amwg_normal1.h -- the stepper of the Normal family at ONE LANE PER CHAIN, under the certified kernel's name (amwg_kernel.h amwg_step_kernel_cert<NormalModel, 1, BT>).
//
// step_body (amwg_kernel.h) is written for any model: any number of components, multidimensional parameters with their own shuffles, sweeps, binary components.  It
// keeps the chain's state, proposal scales, counters and the parameter table in LDS, walks the table for every slot and fetches the next slot's values a slot ahead.
// With a lane per chain and one wavefront per SIMD every instruction of that machinery costs an issue slot beside the fp64 work of the pass, and what it keeps alive
// across the pass cost the pass its registers (244 scalar registers travelled through vector lanes, 6 vector registers were parked).
//
// This family has two scalar components, mu and sigma, and nothing else.  Here a lane keeps both components' value, scale, counters and run totals in registers and
// selects by a compare on the component it updates; the components' constants are wave-uniform (scalar registers); the order of the two named steppers is the packed
// `perm` word.  LDS holds the data tile and nothing else.  What the lane DOES is step_body's, operation for operation, through the same functions -- rnorm_js, the
// uniform stream, NormalModel::log_post_approx, certified_test, log_post, adapt_scale, exp_v8 --: the same draws, decisions and stored words, bit for bit
// (tests/test_gpu_normal_lean.py: against the kernel that runs step_body with the expression in every update, and against the oracle).
#pragma once
#include "amwg_kernel.h"
#include "amwg_models.h"

namespace amwg {

#ifndef AMWG_LEAN_WAVE_BLOCK
#define AMWG_LEAN_WAVE_BLOCK 16
#endif
// rows per block of the wavefront's pass in the 256-thread class (NormalModel::log_post_approx WB).  16, as under step_body: with this stepper 32 rows compile (-DAMWG_LEAN_WAVE_BLOCK=32:
// 4 157 instructions for a block's 4 096 fp64 operations instead of 2 x 2 123, nothing parked inside the pass), but 12 words of the stepper's state then wait in accumulation
// registers around every pass and the remainder of 28 rows at n = 10^4 is three parts instead of two: measured, the pass was 0.3 % SLOWER and the benchmark no faster
// than with 16 rows, which need no parked register at all (profiles/README.md "Round 9")
constexpr int kLeanWaveBlock = AMWG_LEAN_WAVE_BLOCK;

template <int BT>
__device__ __forceinline__ void normal_one_lane_body(const StepArgs &a, unsigned char *smem) {
  using Model = NormalModel;
  constexpr int G = 1;
  constexpr int kPassU = BT >= 1024 ? 4 : 8;      // (the expression's pass: as step_body has it)
  constexpr int kRows = BT <= 256 ? kLeanWaveBlock : 8;
  const int tid = threadIdx.x, nt = blockDim.x;
  // ---- the invariants this body relies on (the host's plan keeps them; a launch that breaks one is refused, never run wrongly): two named parameters, each one
  // scalar component of real or int type, in the order of the state; every chain of the workgroup with a lane of its own
  {
    const int32_t *const t = a.pl.tab;      // base | len | top | multidim, [4][n_params]
    bool ok = a.pl.P == 2 && a.pl.n_params == 2 && a.pl.P_stepped == 2 && a.cpb == 0;
    if (ok) ok = t[0] == 0 && t[1] == 1 && t[2] == 1 && t[3] == 1 && t[6] == 0 && t[7] == 0 && (a.cc[0].type == kTypeReal || a.cc[0].type == kTypeInt) && (a.cc[1].type == kTypeReal || a.cc[1].type == kTypeInt);
    if (!ok) { device_error(a, kErrLeanShape); return; }
  }
  if (a.n_steps > 65535) { device_error(a, kErrLaunchTooLong); return; }      // run totals of a launch are 16-bit fields
  const unsigned char *data_lds = smem;      // (lds_layout: the data region comes first; the rest of the layout is not used here)
  Model::stage(smem, a.d, tid, nt, G);

  const int64_t chain_raw = (int64_t)blockIdx.x * nt + tid;
  const int64_t C = a.C;
  const bool live = chain_raw < C;
  const int64_t cl = live ? chain_raw : C - 1;      // dead lanes shadow the last chain and never store
  const bool writer = live;

  // ---- the components' constants: the same for every chain (scalar registers).  What only a batch boundary needs stays in memory until then.
  const double lower0 = a.cc[0].lower, upper0 = a.cc[0].upper, bsize0 = a.cc[0].batch_size;
  const double lower1 = a.cc[1].lower, upper1 = a.cc[1].upper, bsize1 = a.cc[1].batch_size;
  const bool int0 = a.cc[0].type == kTypeInt, int1 = a.cc[1].type == kTypeInt;
  const bool adapting0 = a.is_adapting[0] != 0, adapting1 = a.is_adapting[1] != 0;

  // ---- the chain: both components' value (the model's register mirror IS the state here), proposal sd = exp(prop_log_scale), counters, this launch's run totals
  Model::Cache cache = Model::cache_init();
  cache.mu = a.ch.state[cl];
  cache.sigma = a.ch.state[C + cl];
  cache.loaded = true;
  const StateView S{nullptr};      // (never read: the mirror is loaded)
  double sd0 = exp_v8(a.ch.prop_log_scale[cl]), sd1 = exp_v8(a.ch.prop_log_scale[C + cl]);      // the log scale itself stays in HBM: it only changes at batch boundaries
  int2 cnt0 = make_int2(a.ch.acceptance_count[cl], a.ch.iterations_since_adaption[cl]);
  int2 cnt1 = make_int2(a.ch.acceptance_count[C + cl], a.ch.iterations_since_adaption[C + cl]);
  uint32_t tot0 = 0u, tot1 = 0u;      // accepted << 16 | evaluated
  uint64_t perm = a.ch.perm[cl];
  CoopStream<G> rng;
  rng.init(a.seed, a.chain_offset + (uint64_t)cl, a.ch.rng_n[cl], tid);
  double lp_curr = a.ch.lp_curr[cl];
  __syncthreads();

  CrossWave xw{nullptr, 0};      // (one lane per chain: no exchange between wavefronts)
  auto expression = [&]() -> double { return log_post<Model, G, kPassU>(S, a, data_lds, 0, xw, cache); };
  auto set_state = [&](int comp, double v) { Model::on_set(cache, comp, v, 0, a.d); };
  if (a.init_lp) lp_curr = expression();      // ctor warm-up call, mcmc.js:961-963
  // the pair (lpA, epsA) of the current state and whether lp_curr is the expression's value of it: step_body "CERTIFIED DECISIONS"
  double lpA = lp_curr, epsA = 0.0;
  bool lp_exact = true;
  if (!a.init_lp) { epsA = a.ch.lp_eps[cl]; lp_exact = epsA == 0.0; }
#if defined(AMWG_AUDIT)
  constexpr bool kAudit = true;      // BOUND AUDIT: E beside A in every update (step_body has the account of it)
#else
  constexpr bool kAudit = false;
#endif
  [[maybe_unused]] double audE = 0.0, aud_max_v = 0.0, aud_max_d = 0.0;
  [[maybe_unused]] uint32_t aud_n = 0u, aud_bad = 0u;
#if defined(AMWG_X_PHASES)      // PHASE CLOCK: step_body's phase numbers (AMWG_PHASE is its macro)
  uint64_t ph_acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) ph_acc[q] = 0;
  uint64_t ph_last = __builtin_readcyclecounter();
#endif
  int64_t row = a.row0;
  int32_t next_rec = (int32_t)a.step0;      // steps until the first recorded step
  const bool recording = a.draws != nullptr;
  const int n_steps = a.n_steps;
  if constexpr (kAudit) { if (lp_exact) audE = lp_curr; else audE = expression(); }
  wave_priority(kStepperPriority);

  for (int step = 0; step < n_steps; ++step) {
    AMWG_PHASE(15);
    // ---- Sampler.sample: record the state BEFORE the step (mcmc.js:1020-1027)
    if (recording && step == next_rec) {
      double *const draws = cold_args()->draws;
      if (live) {
#if !defined(AMWG_X_NOREC)
        draws[(row * 2 + 0) * C + cl] = cache.mu;
        draws[(row * 2 + 1) * C + cl] = cache.sigma;
#endif
      }
      ++row;
      next_rec += cold_args()->thin;
    }
    // ---- AmwgStepper.step: in-place Durstenfeld shuffle of the two named steppers (mcmc.js:887, 228-236): one uniform
    {
      const int j = (int)__builtin_floor(rng.next() * 2.0);
      perm = perm_swap(perm, 1, j);
    }
    AMWG_PHASE(0);
    AMWG_PHASE(1);
#pragma unroll 1
    for (int slot = 0; slot < 2; ++slot) {
      const int comp = (int)perm_get(perm, slot);
      const bool first = comp == 0;
      AMWG_PHASE(14);
      // ---- OnedimMetropolisStepper.step (mcmc.js:517-553)
      const double cur = first ? cache.mu : cache.sigma;
      const int2 cnt = first ? cnt0 : cnt1;
      double prop = rnorm_js(rng, cur, first ? sd0 : sd1);
      if (first ? int0 : int1) prop = js_round(prop);
      const bool inb = !(prop < (first ? lower0 : lower1) || prop > (first ? upper0 : upper1));
      // the accept test's uniform (mcmc.js:528) is the next one of the stream whatever log_post returns: drawn now, and only for a proposal inside its bounds
      double u_accept = 0.0;
      if (inb) { set_state(comp, prop); u_accept = rng.next(); }
      AMWG_PHASE(8);
      AMWG_PHASE(9);
      bool accepted = false, certified = false;
      [[maybe_unused]] double aud_E_prop = 0.0;
      // (the pass is the WAVEFRONT's: the 64 chains of a wave are evaluated together, every lane taking part whether its own proposal needs a value or not --
      // control flow is uniform here: the slot loop is, and the lanes have come back together from their rnorm loops)
      if (__ballot(inb) != 0ull) {
        wave_priority(0);
        const Model::Approx r = Model::template log_post_approx<G, BT, kRows>(cache, S, a.mc, a.d, data_lds, 0);
        wave_priority(kStepperPriority);
        AMWG_PHASE(10);
        if (inb) {
          const double dA = r.value - lpA;
          const double eta = ((r.eps + epsA + __builtin_fabs(dA) * 0x1p-51) * 1.0625 + 0x1p-49) * a.bound_scale;
          const double ex = exp_v8(dA);
          if constexpr (kAudit) { if (a.audit_adversarial) u_accept = audit_place_u(ex, eta, u_accept, step + slot); }
          const int verdict = certified_test(dA, eta, ex, u_accept);      // (0 for a NaN anywhere)
          if constexpr (kAudit) {      // the expression's value of the proposal (the state holds it), beside the cheap one
            aud_E_prop = expression();
            const ChainArrays &ch = cold_args()->ch;
            const double rv = audit_ratio(r.value, r.eps, aud_E_prop);
            if (!(rv < 0.0)) { audit_max(aud_max_v, rv); audit_count_bin(ch, writer, 0, rv); }
            const double dE = aud_E_prop - audE;
            const double rd = audit_ratio(dA, (r.eps + epsA + __builtin_fabs(dA) * 0x1p-51) * 1.0625, dE);
            if (!(rd < 0.0)) { audit_max(aud_max_d, rd); audit_count_bin(ch, writer, 1, rd); }
            audit_verdict(aud_n, aud_bad, dE, verdict, u_accept);
          }
          if (verdict > 0) { certified = true; accepted = true; lpA = r.value; epsA = r.eps; lp_exact = false; }
          else if (verdict < 0) { certified = true; set_state(comp, cur); }
        }
      }
      if (!certified && inb) {
        // the cheap values could not decide: the expression, for the current state first if a cheap value has been standing in for it (ONE call site for both)
        double prop_lp = 0.0;
        for (int which = lp_exact ? 1 : 0; which < 2; ++which) {
          if (which == 0) set_state(comp, cur);
          const double v = expression();
          if (which == 0) { lp_curr = v; lp_exact = true; set_state(comp, prop); }
          else prop_lp = v;
        }
        // Math.exp(prop - curr) > Math.random() (mcmc.js:527-528) with step_body's shortcuts: the same decisions
        const double diff = prop_lp - lp_curr;
        if (diff >= 0.0) accepted = true;
        else if (diff < -746.0) accepted = false;
        else {
          const double lower = 1.0 + diff;
          if (u_accept < lower - 0x1p-50) accepted = true;
          else if (diff > -1.0 && u_accept > (lower + 0.5 * diff * diff) + 0x1p-50) accepted = false;
          else accepted = exp_v8(diff) > u_accept;
        }
        if (accepted) lp_curr = prop_lp;
        else set_state(comp, cur);
        lpA = lp_curr; epsA = 0.0;
      }
      // run totals (not in the reference; parity tests compare them with the oracle's)
      if (inb) { const uint32_t t = 1u + (accepted ? 0x10000u : 0u); tot0 += first ? t : 0u; tot1 += first ? 0u : t; }
      if constexpr (kAudit) { if (inb && accepted) audE = aud_E_prop; }
      AMWG_PHASE(11);
      // ---- Roberts-Rosenthal batch adaptation (mcmc.js:536-550); batch_count and the log scale live in HBM and are touched at a batch boundary only
      if (first ? adapting0 : adapting1) {
        int2 c = cnt;
        c.x += accepted ? 1 : 0;      // acceptance_count (mcmc.js:530)
        c.y += 1;                     // iterations_since_adaption (mcmc.js:537)
        if ((double)c.y >= (first ? bsize0 : bsize1)) {
          const cold_args_ptr ca = cold_args();
          const CompConst k = ca->cc[comp];
          const int64_t gi = (int64_t)comp * C + cl;
          int32_t *const g_bc = ca->ch.batch_count;
          double *const g_pls = ca->ch.prop_log_scale;
          const AdaptedScale ad = adapt_scale(k, g_bc[gi], g_pls[gi], c.x);
          c = make_int2(0, 0);
          const double sd = exp_v8_cold(ad.prop_log_scale);
          sd0 = first ? sd : sd0;
          sd1 = first ? sd1 : sd;
          if (writer) { g_bc[gi] = ad.batch_count; g_pls[gi] = ad.prop_log_scale; }
        }
        cnt0 = first ? c : cnt0;
        cnt1 = first ? cnt1 : c;
      }
      AMWG_PHASE(12);
    }
  }

  // what leaves the launch: the expression's value of the final state if the host asked for it, else the pair the stepper holds
  if (a.finalize_lp && !lp_exact) { lp_curr = expression(); lp_exact = true; }
  if (!lp_exact) lp_curr = lpA;
#if defined(AMWG_X_PHASES)
  if ((tid & 63) == 0 && live) {
    unsigned long long *const hh = cold_args()->ch.audit_hist + 64;
#pragma unroll
    for (int q = 0; q < 16; ++q) (void)atomicAdd(hh + q, (unsigned long long)ph_acc[q]);
  }
#endif
  if constexpr (kAudit) { if (writer) audit_store(cold_args()->ch.audit, C, cl, aud_max_v, aud_max_d, aud_n, aud_bad); }
  if (writer) {
    const cold_args_ptr ca = cold_args();
    ca->ch.lp_eps[cl] = lp_exact ? 0.0 : epsA;
    ca->ch.state[cl] = cache.mu;
    ca->ch.state[C + cl] = cache.sigma;
    ca->ch.acceptance_count[cl] = cnt0.x;
    ca->ch.acceptance_count[C + cl] = cnt1.x;
    ca->ch.iterations_since_adaption[cl] = cnt0.y;
    ca->ch.iterations_since_adaption[C + cl] = cnt1.y;
    ca->ch.accepts[cl] += (int32_t)(tot0 >> 16);
    ca->ch.accepts[C + cl] += (int32_t)(tot1 >> 16);
    ca->ch.inbounds[cl] += (int32_t)(tot0 & 0xffffu);
    ca->ch.inbounds[C + cl] += (int32_t)(tot1 & 0xffffu);
    ca->ch.perm[cl] = perm;
    ca->ch.rng_n[cl] = rng.consumed();
    ca->ch.lp_curr[cl] = lp_curr;
  }
}

template <int BT>
__device__ __forceinline__ void NormalModel::lean_one_lane(const StepArgs &a, unsigned char *smem) { normal_one_lane_body<BT>(a, smem); }

}  // namespace amwg
