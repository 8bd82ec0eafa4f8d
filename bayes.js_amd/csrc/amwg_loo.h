// amwg_loo.h -- the launcher behind amwg_last_sample_dataset_loo (amwg_loo.hip), over device pointers, so that the test library (amwg_selftest.hip:
// amwg_loo_check) drives the same kernels on arbitrary draws and data.  Internal to the shared objects, and not a source of the step kernels
// (tools/build_id.py).  The rule is stated in include/amwg.h; the terms and the split of the draws are WAIC's (amwg_terms.h).
//
// THE ROUTE.  S = rows * (C / D) draws per dataset, M = loo_tail_len(S), cap = max(64, M + 1 rounded up to a power of two) doubles of tail per observation; n = the
// dataset's observations (the Bernoulli family: n = 2, expanded afterwards).  The S x n terms are never stored: every pass below forms them again.
//   0 lppd         amwg_waic_run: lppd_i is WAIC's own, byte for byte.
//   1 select       loo_hist_kernel<Family>, the geometry of WAIC's partial kernel (a tile of 64 observations, a lane each; a run of draws staged in LDS and read as
//                  broadcasts).  Most significant digit first over select_key of the terms, 7 bits a pass: 128 x 64 counters in LDS, added to the observation's 128
//                  global counters with integer atomics; pass 0 also takes the smallest key (an integer atomic minimum) and flags a non-finite term.
//                  loo_pick_kernel, a thread per observation, finds the bin that holds rank M.  An observation is DONE as soon as everything at or below that bin
//                  fits the tail (the sort finishes the job), at the latest after the tenth pass, when the bin is one key: only then can ties overflow the tail, and
//                  the tail is the keys below it plus copies of it.  The host reads one counter per pass and stops when no observation is waiting.
//   2 compaction   loo_compact_kernel<Family>: a term at or below the threshold goes to tail[cursor++] (an integer cursor; the order is arbitrary, the sort makes it
//                  deterministic); a term above it adds exp_v8(a_0 - l) to the split's partial of B, merged over the four wavefronts in LDS in the order 0, 1, 2, 3.
//   3 sort + fit   loo_fit_kernel: a workgroup per observation (256 threads; one wavefront while the tail has at most 128 slots) sorts the tail in LDS (a bitonic
//                  network over the keys), adds the splits' partials in ascending order, forms the excesses in LDS, fits the generalised Pareto (wavefront w takes theta_j, j = w + 1, w + 5, ...; the lanes stride r; sums by
//                  a butterfly over the lanes and the wavefronts in the order 0, 1, 2, 3), smooths and writes elpd_loo_i and khat_i.
//   4 totals       on the host, in index order (amwg_loo_totals).
// Every sum is a function of the sorted tail, of (S, n) and of the observation's own terms: a dataset's bytes do not depend on its neighbours, on D, on the number
// of select passes its batch took, or on the scratch budget.
// SCRATCH per observation: cap doubles of tail, 512 bytes of counters, 48 bytes of state and a double per run of draws; allocated per call and freed before it
// returns; the datasets go in batches under the call's scratch budget (amwg_pointwise_plan, amwg_waic.h), and a dataset beyond the budget runs alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "amwg_waic.h"

constexpr int64_t kLooTailCap = 8192;                       // M + 1 at most: the tail (64 KB of doubles) one workgroup sorts and fits in LDS

// the smallest r with r * r >= v, in integers
inline int64_t loo_isqrt_up(int64_t v) {
  int64_t lo = 0, hi = 3037000500ll;
  while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (mid * mid >= v) hi = mid; else lo = mid + 1; }
  return lo;
}
// M = min(floor(S / 5), the smallest m3 with m3^2 >= 9 S)
inline int64_t loo_tail_len(int64_t S) {
  if (S > (int64_t)1 << 58) return S / 5;
  const int64_t a = S / 5, b = loo_isqrt_up(9 * S);
  return a < b ? a : b;
}

// what the last call did, for the measurement (tools/time_loo.py): select passes over the terms (the largest of its batches) and, when timing was asked for,
// milliseconds per phase summed over the batches
struct LooStats { int32_t passes, timed; float ms_lppd, ms_select, ms_compact, ms_fit; };

// events around a phase when timing is on
struct Phase {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t stream;
  Phase(hipStream_t s, bool timed) : stream(s) { if (timed) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventRecord(e0, stream); } }
  void end(float &into) {
    if (!e0) return;
    float ms = 0.f;
    (void)hipEventRecord(e1, stream);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    into += ms;
  }
  ~Phase() { if (e0) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); } }
};

constexpr uint32_t kFitSmall = 128;      // up to this many slots (S <= 1 800 or so) one wavefront sorts and fits: the network's compare loop has 64 pairs at most
inline unsigned fit_threads(uint32_t cap) { return cap <= kFitSmall ? 64u : 256u; }
inline uint32_t loo_cap(int64_t M) {
  uint32_t c = 64;
  while ((int64_t)c < M + 1) c <<= 1;
  return c;
}
inline int loo_thetas(int64_t M) { return 30 + (int)(loo_isqrt_up(M + 1) - 1); }      // 30 + floor(sqrt(M)): the largest r with r * r <= M is isqrt_up(M + 1) - 1

namespace amwg { struct LooState; }

#pragma GCC visibility push(hidden)
// Phase 1 of THE ROUTE for one batch of the plan: the states initialised, then select passes until no observation of the batch waits; *passes = how many.  obs_off:
// the batch's slice of the plan's offsets on the device; d_state [b.obs], d_hist [b.obs][128], d_pending [1]: the call's scratch.  Synchronises `stream`.
int amwg_loo_select(const PointwiseLaunch &K, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, const WaicDataset *d_sets, const PointwiseBatch &b,
                    const int64_t *obs_off, amwg::LooState *d_state, uint32_t *d_hist, int *d_pending, uint32_t M, uint32_t cap, hipStream_t stream, int *passes);
// AMWG_EINVAL "<call>: ..." unless the shape can be served: amwg_waic_shape's limits and loo_tail_len(S) + 1 <= kLooTailCap.  Host only.
int amwg_loo_shape(const char *call, int64_t rows, int PR, int64_t C, int D);
// The run over any PointwiseLaunch, as amwg_waic.h states it (PointwiseRunFn).  Host outputs: summary [D][4] (elpd_loo, se, p_loo, lppd), high [D] or nullptr,
// pointwise nullptr or [D][n_max][3] (elpd_loo_i, lppd_i, khat_i; NaN beyond n_d), tails nullptr or [D][n_max][M + 1] (the sorted smallest terms; NaN beyond n_d
// and for an observation with a non-finite term; the test library only).
int amwg_loo_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                 int32_t *high, double *pointwise, double *tails, size_t scratch_bytes, hipStream_t stream);
// amwg_loo_run for a built-in family, behind the checks of the pointers, the shape and the family
int amwg_loo_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, double *summary,
                    int32_t *high, double *pointwise, double *tails, size_t scratch_bytes, hipStream_t stream);
// the finish of include/amwg.h over one dataset's triples pw[n][3]: summary[4], *high (may be nullptr)
void amwg_loo_totals(const double *pw, int64_t n, double *summary, int32_t *high);
// phase timing of later calls on or off (events around the phases); the record of the last call that ended (a call gathers its own and publishes it once, under a
// lock: concurrent calls on several samplers do not share anything they write).  For the test library.
void amwg_loo_set_timing(int on);
int amwg_loo_timing();                                  // the switch as it stands
void amwg_loo_publish_stats(const LooStats &stats);      // the record of a call that ended (amwg_loo_predictive_run publishes its own: ms_lppd = 0, it has no such pass)
LooStats amwg_loo_last_stats();
#pragma GCC visibility pop
