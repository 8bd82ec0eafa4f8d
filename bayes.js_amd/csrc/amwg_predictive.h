// amwg_predictive.h -- the launcher behind amwg_last_sample_dataset_predictive (amwg_predictive.hip): posterior predictive calibration per dataset -- PIT, predictive
// mean and sd per observation -- over device draws and data in the sampler's layout, so that the test library (amwg_selftest.hip: amwg_predictive_check) drives the
// same kernels on arbitrary draws.  Internal to the shared objects, and not a source of the step kernels (tools/build_id.py).  The rule is stated in include/amwg.h,
// the two distribution functions and their bounds in amwg_cdf.h.
//
// THE ROUTE.  S = rows * (C / D) draws per dataset in WAIC's order; m = the dataset's observations to score (its own, or held-out ones packed by amwg_heldout_pack).
//   1 partials     predictive_partial_kernel<Family>: a workgroup of 256 threads serves a tile of Mt <= 64 observations and one of the dataset's `splits` contiguous
//                  runs of draws.  256 draws at a time are staged in LDS as the family's PREDICTIVE draw (the Normal family: mu and sigma -- not WAIC's c, den and
//                  reciprocal, which a CDF has no use for), a thread each; the observation stays in registers.
//                    A FULL TILE (Mt = 64; in-sample): a thread per observation, wavefront w walks the staged draws w, w + 4, ...; lane strides are compile-time.
//                    A SHORT TILE (K-fold): Np = Mt rounded up to a power of two, an observation is owned by 64 / Np lanes of every wavefront, lane unit =
//                    wave * (64 / Np) + lane / Np walks the staged draws unit, unit + 4 * 64 / Np, ...: with one observation all 256 threads work on it.
//                  Either way every lane of a wavefront that shares lane / Np reads the same LDS address (a broadcast).  THE ACCUMULATOR has no running maximum and
//                  no rescale, so a lane takes its draws in register blocks of R INDEPENDENT evaluations (R = 4; the Poisson family 2) summed pairwise: sum F, sum Fm,
//                  sum var, and sum (mean - K), sum (mean - K)^2 with K the mean of the lane's first draw (the shift keeps the variance over draws free of
//                  cancellation).  A block that reaches past the staged run evaluates the run's draw jb again and drops it by a select: one code path.
//                  At the end a lane holds the RECORD of six doubles (sum F, sum Fm, sum var, count, mean, M2).  The lanes of an observation merge by an xor butterfly
//                  over the lane distances Np ... 32 (amwg_lanes.h) -- Chan's formula on (count, mean, M2), applied to (lower lane, upper lane) in that order in
//                  both lanes -- and the four wavefronts through LDS in the order 0, 1, 2, 3, into scratch [split][observation].
//   2 finish       predictive_finish_kernel: a wavefront per observation -- lane k merges the splits k, k + 64, ... in ascending order, the 64 lanes by the same
//                  butterfly: a fixed tree, a function of the split count alone -- and writes pit_hi, pit_lo, pred_mean, pred_sd; a non-finite one makes all four NaN.
//   3 the finish of include/amwg.h on the host, in index order (amwg_predictive_totals).
// THE POISSON CDF's loop length differs per lane (about 9 sqrt(lambda) terms at the mode).  The lanes of a wavefront hold different observations of ONE draw (or, in
// a short tile, of 64 / Np draws), so their lambdas differ by the covariates and their loops by the square root of that; the early stop caps every lane's loop and the
// wavefront issues the longest of its 64: DESIGN.md section 6 gives the cost.
// MATRIX INSTRUCTIONS do not fit: an eta by fp64 MFMA would not be the term's eta (another order of additions), and exp / erfc dominate.
// splits = waic_splits(S, m), a function of those two alone: a dataset's bytes do not depend on its neighbours, on D, or on the scratch budget.
// SCRATCH: splits * m records of 48 bytes per dataset; the datasets go in batches under the call's budget (kPointwiseScratchBytes by default); freed on return.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "amwg_host.h"
#include "amwg_waic.h"

#pragma GCC visibility push(hidden)
// The run.  draws [rows][PR][C] on the current device; M: the family with its arrays on the device in the sampler's layout (the sampler's own: amwg_waic_describe;
// held-out ones: amwg_heldout_pack); sets [D] on the host; index: the Poisson family's positions on the device at WaicDataset::off_xb, or nullptr for 0 ... m_d - 1.
// summary [D][4] = cover50, cover90, rmse, mean_mid; pointwise nullptr or [D][m_max][4].  Returns after `stream` has drained.
int amwg_predictive_run(const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &M, const WaicDataset *sets, const int32_t *index,
                        double *summary, double *pointwise, size_t scratch_bytes, hipStream_t stream);
// THE FINISH of include/amwg.h over one dataset: pw [m][4], the observations y [m] -> summary[4]
void amwg_predictive_totals(const double *pw, const double *y, int64_t m, double *summary);
#pragma GCC visibility pop
