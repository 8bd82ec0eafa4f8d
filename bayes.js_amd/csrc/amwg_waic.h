// amwg_waic.h -- the launcher behind amwg_last_sample_dataset_waic (amwg_waic.hip), over device pointers, so that the test library (amwg_selftest.hip:
// amwg_waic_check) drives the same kernels on arbitrary draws and data.  Internal to the shared objects, and not a source of the step kernels
// (tools/build_id.py).  The rule is stated in include/amwg.h.
//
// THE ROUTE.  S = rows * (C / D) draws per dataset, in the order s = row * (C / D) + chain; n = the dataset's observations (the Bernoulli family: n = 2, the two
// values an observation can take -- its pointwise pairs are picked from those two afterwards).
//   1 partials     waic_partial_kernel<Family>: a workgroup of 256 threads serves a tile of 64 observations and one of the dataset's `splits` contiguous runs
//                  of draws.  256 draws at a time, a thread each, the workgroup forms what an evaluation needs of a draw -- the Normal family: mu, c, den and its
//                  Reciprocal, one log and one division per draw -- and stages it in LDS; lane l of each of the four wavefronts owns observation tile * 64 + l,
//                  wavefront w walks the staged draws w, w + 4, ..., every lane reading the same LDS address (a broadcast): no cross-lane operation per evaluation.
//                  Per evaluation: the family's term, exp_v8(-|l - m|) into a running (m, sum exp(l - m)), and d = l - K into (sum d, sum d^2), K the running
//                  mean as it stood when the 64 staged draws began (the first term of the very first): (count, mean, M2) are updated once per staged run by
//                  Chan's formula.  The four wavefronts' partials are merged in LDS in the order 0, 1, 2, 3 and written to scratch [split][observation].
//   2 finish       waic_merge_kernel: a thread per observation merges the splits in ascending order -- (m, sum) by rescaling, (count, mean, M2) by Chan's
//                  formula -- and writes lppd_i = m + log(sum) - log(S), p_i = M2 / (S - 1); a non-finite M2 (a non-finite term, or terms whose squares overflow)
//                  gives NaN for both.
//   3 totals       on the host, in index order (amwg_waic_totals).
// splits = waic_splits(S, n), a function of those two alone: a dataset's bytes do not depend on its neighbours, on D, or on the scratch budget.
// SCRATCH: splits * n partials of 32 bytes per dataset, allocated per call and freed before it returns; the datasets go in batches under kWaicScratchBytes, and a
// dataset whose partials exceed the budget runs alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "amwg_pointwise_types.h"      // WaicDataset, UserTermsArg

struct amwg_sampler;

constexpr size_t kWaicScratchBytes = (size_t)256 << 20;      // the default scratch budget of a call: 256 MiB, as amwg_hpd.h

// the family and its arrays on the device, in the sampler's own layout (DataRef, amwg_types.h)
struct WaicModel {
  int32_t model, G, exact_division, reserved;      // AMWG_MODEL_*; the hierarchical family's groups; amwg_options::exact_division
  double neg_half_log_2pi;                         // ModelConsts::neg_half_log_2pi
  const double *x, *y, *lfact;                     // NORMAL x | HIER y | GLM X column-major [7][n]; GLM counts; GLM lfactorial(y_i), +inf for a negative count
  const uint8_t *xb;                               // BETA_BERN x as bytes | HIER group labels
  const uint8_t *invalid;                          // BETA_BERN: 1 where x_i is neither 0 nor 1, laid out like xb; nullptr: no such observation anywhere
};

// HOW A CALL LAUNCHES THE KERNELS THAT EVALUATE THE MODEL (amwg_pointwise.h): the instantiations for a built-in family (amwg_waic_family_kernels,
// amwg_loo_family_kernels), or the entries of a closure's code object (amwg_pointwise_user_kernels).  Everything else of a call is the same code for both.
struct PointwiseLaunch {
  bool bern = false;                     // the family of two observations per dataset (its pairs are picked by x_i afterwards)
  const WaicModel *family = nullptr;     // the built-in family's model (nullptr: a closure)
  std::function<hipError_t(dim3, hipStream_t, const double *, int64_t, int, int64_t, int64_t, int, const WaicDataset *, const int64_t *, void *)> waic_partial;
  std::function<hipError_t(dim3, hipStream_t, const double *, int64_t, int, int64_t, int64_t, const WaicDataset *, double *, int64_t)> waic_loglik;
  std::function<hipError_t(dim3, hipStream_t, const double *, int64_t, int, int64_t, int64_t, int, const WaicDataset *, const int64_t *, void *, uint32_t *, int)> loo_hist;
  std::function<hipError_t(dim3, hipStream_t, const double *, int64_t, int, int64_t, int64_t, int, const WaicDataset *, const int64_t *, const int64_t *, void *, double *, uint32_t, double *)> loo_compact;
};
// the pointwise code object of a translated closure, loaded on the sampler's device (amwg_rtc.hip load_pointwise), and its model argument
struct UserPointwise {
  hipFunction_t waic_partial = nullptr, waic_loglik = nullptr, loo_hist = nullptr, loo_compact = nullptr;
  amwg::UserTermsArg arg{};
  int32_t n_obs = 0, state_n = 0;      // kTermN, kStateN of the terms text
};

#pragma GCC visibility push(hidden)
void amwg_waic_family_kernels(PointwiseLaunch &K, const WaicModel &model);      // (keeps &model: the launch must not outlive it)
void amwg_loo_family_kernels(PointwiseLaunch &K, const WaicModel &model);
void amwg_pointwise_user_kernels(PointwiseLaunch &K, const UserPointwise &u);
// amwg_waic_launch behind its family checks: the same call over any PointwiseLaunch.  A closure: sets[d].n_obs = kTermN for every d.
int amwg_waic_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                  int32_t *high, double *pointwise, double *loglik, hipStream_t stream);
// AMWG_EINVAL "<call>: ..." unless the shape can be served: amwg_dataset_quantiles_shape's limits and at least 2 draws per dataset.  Host only.
int amwg_waic_shape(const char *call, int64_t rows, int PR, int64_t C, int D);
// draws [rows][PR][C] on the current device, D datasets of C / D columns each; sets [D] on the host.  Host outputs: summary [D][4] (elpd_waic, se, p_waic, lppd),
// high [D] or nullptr, pointwise nullptr or [D][n_max][2] (NaN beyond n_d; n_max the largest n_obs), loglik nullptr or [D][S][n_max] (the terms themselves; the test
// library only).  Returns after `stream` has drained.
int amwg_waic_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, double *summary,
                     int32_t *high, double *pointwise, double *loglik, hipStream_t stream);
// sets [D] and model of a sampler's own data, as the launchers take them; the sampler's device is current (one copy from it when D > 1)
int amwg_waic_describe(amwg_sampler *s, std::vector<WaicDataset> &sets, WaicModel &model);
// the same for a closure sampler whose pointwise text is set: compiles and loads the code object on first use; every dataset has kTermN observations
int amwg_pointwise_describe_user(amwg_sampler *s, std::vector<WaicDataset> &sets, UserPointwise &u);
// the finish of include/amwg.h over one dataset's pairs pw[n][2]: summary[4], *high (may be nullptr)
void amwg_waic_totals(const double *pw, int64_t n, double *summary, int32_t *high);
// the scratch budget of later calls in bytes (0: kWaicScratchBytes); returns the budget in force before.  For the test library: the product never calls it.
size_t amwg_waic_set_budget(size_t bytes);
#pragma GCC visibility pop
