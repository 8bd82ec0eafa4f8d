// amwg_loo_predictive.h -- the launcher behind amwg_last_sample_dataset_loo_predictive (amwg_loo_predictive.hip): PSIS-LOO predictive calibration per dataset --
// LOO-PIT, leave-one-out predictive mean and sd per observation -- over device pointers, so that the test library (amwg_selftest.hip: amwg_loo_predictive_check)
// drives the same kernels on arbitrary draws and data.  Internal to the shared objects, and not a source of the step kernels (tools/build_id.py).  The rule is
// stated in include/amwg.h; the terms are WAIC's (amwg_terms.h), the select, the sort and the fit LOO's (amwg_loo.h, amwg_loo_fit.h), F, Fm, mean and var the
// predictive call's (amwg_predictive_eval.h).
//
// THE ROUTE.  S, M, cap, n and the split of the draws are amwg_loo.h's.  Neither the S x n terms nor the S x n weights are ever stored, no pass over the terms is
// added to LOO's, and LOO's lppd pass is not run.
//   1 select       LOO's, unchanged (amwg_loo_select).
//   2 compaction   loo_pred_compact_kernel<Family>, the geometry of loo_compact_kernel: a tile of 64 observations, a lane each; a run of 256 draws staged in LDS
//                  TWICE, a thread each -- as the term's Draw and as the predictive Draw -- and read as broadcasts.  A lane takes its draws in register blocks of R
//                  (4; the Poisson family 2): R terms and R predictive evaluations, independent of each other, then per draw
//                    a key above the threshold: w = exp_v8(a_0 - l) into the SIX sums  sum w, w F, w Fm, w mean, w var, w (mean - c)^2  (c: the observation's mean
//                    under draw 0, which every lane forms for itself before the walk);
//                    a key the tail takes: the term to tail[cursor], the draw index to tail_ix[cursor] (one integer atomic; the order is arbitrary);
//                    the threshold's own key where ties overflow the tail (LooState::inclusive == 0): unweighted into the CLASS RECORD, the same six sums with w = 1,
//                    whose first is the count.  No tie-break picks which copies "are" in the tail.
//                  Both records are merged over the four wavefronts in LDS in the order 0, 1, 2, 3 and written to scratch [split][observation][2].
//   3 sort, fit,   loo_pred_fit_kernel<Family>: a workgroup per observation (fit_threads(cap), as LOO: khat_i is formed by the same code over the same bytes).  The
//     weight       bitonic network over (key, draw index) pairs in LDS -- equal keys end in index order, so the sums below do not depend on the cursor's order --; the
//                  excesses and the fit (amwg_loo_fit.h); the weight of every sorted slot into the LDS the excesses leave: exp_v8(lw~_{M-t}) below M on the smoothed
//                  route, exp_v8(a_0 - a_t) elsewhere.  THE CLASS MEANS: the thread that holds the first slot of a run of equal keys beginning below M adds the run's
//                  weights in ascending t and gives every slot the mean -- the rule's own order of additions, where a scan would add in a tree; runs are as long as a
//                  Metropolis chain's rejections, a handful of slots, and the worst case (one key all over the tail) is M additions by one thread.  Then the
//                  functionals of the buffered draws are evaluated again from their indices, a thread each (at most cap), each thread adds the splits k, k + T, ...
//                  of the two records, the workgroup's sums (block_sum) finish the six, the class record enters with its weight, and the five outputs are written.
//   4 finish       on the host: amwg_predictive_totals over (pit_hi, pit_lo, pred_mean, pred_sd) and the observations, and the count of khat_i > 0.7.
// The Bernoulli family runs on its two values and is expanded, as in LOO.
// LDS of the fit: (cap + 272) * 8 + cap * 4 bytes -- 100 480 at LOO's cap of 8 192 slots, inside the 160 KB of a workgroup: LOO's limit stands.
// SCRATCH per observation: LOO's (cap doubles of tail, 512 bytes of counters, 48 of state) plus 4 bytes per tail slot, and 96 bytes per run of draws; allocated per
// call under the call's budget, freed before it returns.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "amwg_loo.h"

#pragma GCC visibility push(hidden)
// The run, as amwg_waic.h states it (PointwiseRunFn), for a built-in family (K.builtin).  Host outputs: summary [D][4] (cover50, cover90, rmse, mean_mid), high [D]
// or nullptr, pointwise nullptr or [D][n_max][5] (pit_hi, pit_lo, pred_mean, pred_sd, khat_i; NaN beyond n_d); `extra` is not read.
int amwg_loo_predictive_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets,
                            double *summary, int32_t *high, double *pointwise, double *extra, size_t scratch_bytes, hipStream_t stream);
// ... behind the checks of the pointers, the shape (LOO's) and the family
int amwg_loo_predictive_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets,
                               double *summary, int32_t *high, double *pointwise, size_t scratch_bytes, hipStream_t stream);
#pragma GCC visibility pop
