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
// SCRATCH: splits * n partials of 32 bytes per dataset, allocated per call and freed before it returns; the datasets go in batches under the call's scratch budget
// (kPointwiseScratchBytes by default), and a dataset whose partials exceed the budget runs alone.
//
// WHAT WAIC AND PSIS-LOO SHARE ON THE HOST (amwg_pointwise_host.hip) is declared here too: how a call launches the kernels that evaluate the model (PointwiseLaunch),
// the batches under the budget, the device outputs of a call, and the one body of the two amwg_last_sample_dataset_* entries.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "amwg_host.h"                 // DevBuf
#include "amwg_pointwise_types.h"      // WaicDataset, UserTermsArg

struct amwg_sampler;

constexpr size_t kPointwiseScratchBytes = (size_t)256 << 20;      // the default scratch budget of a WAIC or LOO call: 256 MiB, as amwg_hpd.h

// the family and its arrays on the device, in the sampler's own layout (DataRef, amwg_types.h)
struct WaicModel {
  int32_t model, G, exact_division, reserved;      // AMWG_MODEL_*; the hierarchical family's groups; amwg_options::exact_division
  double neg_half_log_2pi;                         // ModelConsts::neg_half_log_2pi
  const double *x, *y, *lfact;                     // NORMAL x | HIER y | GLM X column-major [7][n]; GLM counts; GLM lfactorial(y_i), +inf for a negative count
  const uint8_t *xb;                               // BETA_BERN x as bytes | HIER group labels
  const uint8_t *invalid;                          // BETA_BERN: 1 where x_i is neither 0 nor 1, laid out like xb; nullptr: no such observation anywhere
};

// HOW A CALL LAUNCHES THE KERNELS THAT EVALUATE THE MODEL (amwg_pointwise.h), as plain data: the instantiations for a built-in family (amwg_pointwise_family), or the
// entries of a closure's code object (amwg_pointwise_describe_user).  The two take the same argument lists, the model in the same slot; everything else of a call is
// the same code for both.
// The four grouped twins (leave-one-group-out) stand kPwGrouped after the kernel they replace.
enum PointwiseKernel { kPwWaicPartial, kPwWaicLoglik, kPwLooHist, kPwLooCompact, kPwWaicFold, kPwGrouped, kPwKernels = kPwGrouped + 4 };      // (the first four: the order of amwg_sampler::pw_fn)
struct PointwiseGroups;
struct PointwiseLaunch {
  bool bern = false;                   // the family of two observations per dataset (its pairs are picked by x_i afterwards)
  bool builtin = false;                // a built-in family: `family` is the model argument and fn[] are addresses of the kernels' instantiations (hipLaunchKernel);
  WaicModel family{};                  // a closure: `user`, and fn[] are the hipFunction_t of its code object (hipModuleLaunchKernel)
  amwg::UserTermsArg user{};
  const void *fn[kPwKernels] = {};
  const PointwiseGroups *groups = nullptr;      // a grouped call (amwg_pointwise_groups): the walking kernels are fn[kPwGrouped + k] and take the groups after `sets`
  void *model_arg() const { return builtin ? (void *)&family : (void *)&user; }      // the model's slot of an args[] list
};

// the batches of a call: consecutive datasets whose scratch fits the budget together (a dataset beyond it runs alone)
struct PointwiseBatch { int d0, d1; int64_t tiles, splits, n_most, obs; };      // datasets [d0, d1): the largest tiles, splits and n among them; their observations
struct PointwisePlan {
  std::vector<int64_t> off;      // off[d]: observations before d in its batch; off[D + d]: partials (splits * n per dataset) before it
  std::vector<PointwiseBatch> batches;
  int64_t most_obs = 0, most_parts = 0;      // of the largest batch
};
// the device side of a call's outputs: sets [D], pw [D][n_max][2] and, when asked for, extra [D][n_max * extra_per_obs], both filled with NaN
struct PointwiseOut {
  int64_t n_max = 0;      // the largest n_obs
  size_t pw_count = 0, extra_count = 0;
  DevBuf sets, pw, extra;
};

// THE GROUPS OF A GROUPED CALL (include/amwg.h, leave-one-group-out).  From the joint terms on, a group is what an observation is to an ungrouped call: the plan, the
// merge, pick and fit kernels, the outputs and the totals take `by_group` -- the datasets with n_obs = G_d -- for `sets`; only the walking kernels read the
// observations' own sets and the CSR (GroupSet, amwg_pointwise_types.h), uploaded once per call.
struct PointwiseGroups {
  std::vector<WaicDataset> by_group;      // [D], host: the call's `sets`
  std::vector<GroupSet> gsets;            // [D], host
  std::vector<int32_t> csr;               // every dataset's start, member and deal, back to back
  DevBuf d_sets, d_gsets, d_csr;          // the observations' sets [D], gsets and csr on the device
};

// the built-in families, in the order of AMWG_MODEL_* from AMWG_MODEL_NORMAL on: the one list the two units expand into their instantiations
template <int... MODEL> struct PointwiseModels {};
typedef PointwiseModels<AMWG_MODEL_NORMAL, AMWG_MODEL_BETA_BERN, AMWG_MODEL_HIER_NORMAL, AMWG_MODEL_POIS_GLM> BuiltinModels;
static_assert(AMWG_MODEL_BETA_BERN == AMWG_MODEL_NORMAL + 1 && AMWG_MODEL_HIER_NORMAL == AMWG_MODEL_NORMAL + 2 && AMWG_MODEL_POIS_GLM == AMWG_MODEL_NORMAL + 3, "BuiltinModels is indexed by model - AMWG_MODEL_NORMAL");

#pragma GCC visibility push(hidden)
// the address of a built-in family's instantiation, model one of BuiltinModels (amwg_waic.hip: k = 0 the partial kernel, 1 loglik, 2 the fold; amwg_loo.hip: k = 0 hist, 1 compact)
const void *amwg_waic_family_fn(int model, int k);
const void *amwg_loo_family_fn(int model, int k);
// ... of its grouped twin of kernel k < 4 (amwg_grouped.hip; nullptr for the Bernoulli family, which the grouped calls refuse)
const void *amwg_grouped_family_fn(int model, int k);
// K of a built-in family.  AMWG_EINVAL "<call>: ..." for an unknown model, draws of fewer components than the family reads, the hierarchical family on D != 1.
int amwg_pointwise_family(const char *call, const WaicModel &model, int PR, int D, PointwiseLaunch &K);
// The groups of D datasets from their labels back to back (n_d each), by the rule of include/amwg.h, uploaded on `stream`; K.groups = &g, which must outlive the
// run.  AMWG_EINVAL "<call>: ..." for the Bernoulli family; nothing is launched.  labels are not NULL: amwg_pointwise_labels is the one refusal of NULL labels, which
// the bodies of the grouped entries ask before they open a device or compile a closure's text.  The groups' own device memory (below) is no part of the scratch
// budget: it lives for the whole call, across its batches.  amwg_group_csr: one dataset's start [G + 1], member [n] and
// deal [G] from its labels alone -> G (host only)
int amwg_pointwise_groups(const char *call, PointwiseLaunch &K, const WaicDataset *sets, int D, const int32_t *labels, hipStream_t stream, PointwiseGroups &g);
int amwg_pointwise_labels(const char *call, const int32_t *labels);
int32_t amwg_group_csr(const int32_t *labels, int32_t n, std::vector<int32_t> &start, std::vector<int32_t> &member, std::vector<int32_t> &deal);
// entry k of K over `grid` workgroups of kThreads; args: the kernel's argument list, K.model_arg() in the model's slot
hipError_t amwg_pointwise_go(const PointwiseLaunch &K, int k, dim3 grid, hipStream_t stream, void **args);
hipError_t amwg_pointwise_fill_nan(double *out, int64_t count, hipStream_t stream);
// the Bernoulli family: out[d][i][width] = two[d][x_i == 1 ? 0 : 1][width] for i < n_d; an invalid x_i: NaN
hipError_t amwg_pointwise_bern_expand(const PointwiseLaunch &K, const WaicDataset *d_sets, int D, const double *two, double *out, int64_t n_max, int64_t width, hipStream_t stream);
// obs_bytes of scratch per observation and part_bytes per partial; scratch_bytes: the budget (0: kPointwiseScratchBytes).  A new batch starts when the batch is not
// empty and the next dataset would exceed the budget.
PointwisePlan amwg_pointwise_plan(const PointwiseLaunch &K, const WaicDataset *sets, int D, int64_t S, size_t obs_bytes, size_t part_bytes, size_t scratch_bytes);
// AMWG_EINVAL for an n_obs < 0; else n_max, sets uploaded, the outputs allocated and filled (extra_per_obs = 0: no extra).  amwg_pointwise_fetch: after the stream
// has drained, pw [D][n_max][2] and extra to the host
int amwg_pointwise_begin(const char *call, const WaicDataset *sets, int D, int64_t extra_per_obs, hipStream_t stream, PointwiseOut &o);
int amwg_pointwise_fetch(const PointwiseOut &o, double *pw, double *extra);
// The run of a statistic over any PointwiseLaunch: amwg_waic_run, amwg_loo_run.  draws [rows][PR][C] on the current device, D datasets of C / D columns each; sets [D]
// on the host (a closure: n_obs = kTermN for every d).  The caller has checked the pointers and the shape (amwg_waic_shape, amwg_loo_shape).  scratch_bytes: the budget
// of this call (0: the default; the product passes 0).  Returns after `stream` has drained.
typedef int (*PointwiseRunFn)(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                              int32_t *high, double *pointwise, double *extra, size_t scratch_bytes, hipStream_t stream);
typedef int (*PointwiseShapeFn)(const char *call, int64_t rows, int PR, int64_t C, int D);
// the body of amwg_last_sample_dataset_waic and amwg_last_sample_dataset_loo: the refusals, the sampler's datasets and model described, `run`.  grouped: the body of
// their _grouped twins -- labels as amwg_pointwise_groups takes them, n_groups_out [D] or nullptr, pointwise [D][G_max][..]
int amwg_pointwise_entry(const char *call, amwg_sampler *s, double *summary, int32_t *high, double *pointwise, PointwiseShapeFn shape, PointwiseRunFn run,
                         bool grouped = false, const int32_t *labels = nullptr, int32_t *n_groups_out = nullptr);
// Host outputs: summary [D][4] (elpd_waic, se, p_waic, lppd), high [D] or nullptr, pointwise nullptr or [D][n_max][2] (NaN beyond n_d; n_max the largest n_obs), loglik
// nullptr or [D][S][n_max] (the terms themselves; the test library only).
int amwg_waic_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                  int32_t *high, double *pointwise, double *loglik, size_t scratch_bytes, hipStream_t stream);
// AMWG_EINVAL "<call>: ..." unless the shape can be served: amwg_dataset_quantiles_shape's limits and at least 2 draws per dataset.  Host only.
int amwg_waic_shape(const char *call, int64_t rows, int PR, int64_t C, int D);
// amwg_waic_run for a built-in family, behind the checks of the pointers, the shape and the family
int amwg_waic_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, double *summary,
                     int32_t *high, double *pointwise, double *loglik, size_t scratch_bytes, hipStream_t stream);
// sets [D] and model of a sampler's own data, as the launchers take them; the sampler's device is current (one copy from it when D > 1)
int amwg_waic_describe(amwg_sampler *s, std::vector<WaicDataset> &sets, WaicModel &model);
// the same for a closure sampler whose pointwise text is set: compiles and loads the code object on first use; every dataset has kTermN observations
int amwg_pointwise_describe_user(amwg_sampler *s, std::vector<WaicDataset> &sets, PointwiseLaunch &K);
// the finish of include/amwg.h over one dataset's pairs pw[n][2]: summary[4], *high (may be nullptr)
void amwg_waic_totals(const double *pw, int64_t n, double *summary, int32_t *high);

// ---- WAIC FOLDED WINDOW BY WINDOW (amwg_waic_fold.hip): amwg_set_waic arms it for a sampler's summarising calls, the test library (amwg_waic_fold_check) drives the
// same three steps over any array cut into windows.
//   begin    the records [dataset][split][observation] of 32 bytes (amwg_pointwise.h: fold_splits of (window_rows * C / D, n_d)) allocated and zeroed
//   window   waic_fold_body<Family> over the rows of one window, enqueued behind the fold of the same window: every workgroup continues its split's records
//   finish   a thread per observation merges its splits in ascending order, the counts from the indices (fold_count), and writes lppd_i and p_i by the stored call's
//            rules; the Bernoulli family's two observations are expanded; the totals on the host (amwg_waic_totals)
// The records cannot be batched under a scratch budget: they live from the first window to the query.  A dataset's bytes depend on its own draws and data, on
// (rows, C / D) and on window_rows.
struct WaicFold {
  bool armed = false, folded = false;      // amwg_set_waic; the records are those of the sampler's last summarising call
  PointwiseLaunch K;
  std::vector<WaicDataset> sets;           // [D], host
  std::vector<int64_t> off;                // [D]: records before dataset d
  int D = 0, PR = 0;
  int64_t C = 0, window_rows = 0, total_rows = 0, tiles = 0, splits = 0, n_most = 0;      // the largest tiles, splits and n among the datasets
  DevBuf d_sets, d_off, d_state;           // (never copied: the map of amwg_waic_fold.hip holds it in place)
  size_t state_bytes = 0;
};
// the device bytes of the records of D datasets under windows of window_rows rows (the split rule, restated for amwg_waic_info and the tests)
size_t amwg_waic_fold_bytes(const PointwiseLaunch &K, const WaicDataset *sets, int D, int64_t window_rows, int64_t cpd);
// AMWG_EINVAL "<call>: ..." unless amwg_waic_shape serves (total_rows, PR, C, D) and window_rows >= 1; the records allocated and zeroed on `stream`
int amwg_waic_fold_begin(const char *call, const PointwiseLaunch &K, const WaicDataset *sets, int D, int PR, int64_t C, int64_t window_rows, int64_t total_rows,
                         hipStream_t stream, WaicFold &f);
// rows [g0, g0 + nrows) of the call stand in window[0 .. nrows)[PR][C]; g0 a multiple of window_rows, nrows <= window_rows.  Enqueued on `stream`; no synchronisation
int amwg_waic_fold_window(const WaicFold &f, const double *window, int64_t g0, int64_t nrows, hipStream_t stream);
// the outputs of amwg_waic_run from the records.  Returns after `stream` has drained
int amwg_waic_fold_finish(const char *call, const WaicFold &f, double *summary, int32_t *high, double *pointwise, hipStream_t stream);
// the fold armed for `s` (amwg_set_waic), or nullptr; amwg_sample_summarize_async, before its launches: the sampler described, the records of this call begun -> the
// arm, or nullptr (none armed); amwg_destroy
WaicFold *amwg_waic_armed(const amwg_sampler *s);
int amwg_waic_begin(amwg_sampler *s, int64_t window_rows, int64_t rows, WaicFold **arm);
void amwg_waic_forget(const amwg_sampler *s);
#pragma GCC visibility pop
