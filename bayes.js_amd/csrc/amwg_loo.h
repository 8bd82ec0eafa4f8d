// amwg_loo.h -- the launcher behind amwg_last_sample_dataset_loo (amwg_loo.hip), over device pointers, so that the test library (amwg_selftest.hip:
// amwg_loo_check) drives the same kernels on arbitrary draws and data.  Internal to the shared objects, and not a source of the step kernels
// (tools/build_id.py).  The rule is stated in include/amwg.h; the terms and the split of the draws are WAIC's (amwg_terms.h).
//
// THE ROUTE.  S = rows * (C / D) draws per dataset, M = loo_tail_len(S), cap = max(64, M + 1 rounded up to a power of two) doubles of tail per observation; n = the
// dataset's observations (the Bernoulli family: n = 2, expanded afterwards).  The S x n terms are never stored: every pass below forms them again.
//   0 lppd         amwg_waic_launch: lppd_i is WAIC's own, byte for byte.
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
// returns; the datasets go in batches under kLooScratchBytes, and a dataset beyond the budget runs alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "amwg_waic.h"

constexpr size_t kLooScratchBytes = (size_t)256 << 20;      // the default scratch budget of a call: 256 MiB, as amwg_waic.h
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

#pragma GCC visibility push(hidden)
// AMWG_EINVAL "<call>: ..." unless the shape can be served: amwg_waic_shape's limits and loo_tail_len(S) + 1 <= kLooTailCap.  Host only.
int amwg_loo_shape(const char *call, int64_t rows, int PR, int64_t C, int D);
// draws [rows][PR][C] on the current device, D datasets of C / D columns each; sets [D] on the host.  Host outputs: summary [D][4] (elpd_loo, se, p_loo, lppd),
// high [D] or nullptr, pointwise nullptr or [D][n_max][3] (elpd_loo_i, lppd_i, khat_i; NaN beyond n_d), tails nullptr or [D][n_max][M + 1] (the sorted smallest
// terms; NaN beyond n_d and for an observation with a non-finite term; the test library only).  Returns after `stream` has drained.
int amwg_loo_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, double *summary,
                    int32_t *high, double *pointwise, double *tails, hipStream_t stream);
// amwg_loo_launch over any PointwiseLaunch (amwg_waic.h): the built-in families' kernels, or a closure's.  A closure: sets[d].n_obs = kTermN for every d.
int amwg_loo_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                 int32_t *high, double *pointwise, double *tails, hipStream_t stream);
// the finish of include/amwg.h over one dataset's triples pw[n][3]: summary[4], *high (may be nullptr)
void amwg_loo_totals(const double *pw, int64_t n, double *summary, int32_t *high);
// the scratch budget of later calls in bytes (0: kLooScratchBytes); returns the budget in force before.  For the test library: the product never calls it.
size_t amwg_loo_set_budget(size_t bytes);
// phase timing of later calls on or off (events around the phases); the record of the last call that ended (a call gathers its own and publishes it once, under a
// lock: concurrent calls on several samplers do not share anything they write).  For the test library.
void amwg_loo_set_timing(int on);
LooStats amwg_loo_last_stats();
#pragma GCC visibility pop
