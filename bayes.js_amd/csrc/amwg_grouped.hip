// amwg_grouped.hip -- WAIC and PSIS-LOO over GROUPS of observations (leave-one-group-out: amwg_last_sample_dataset_waic_grouped / _loo_grouped, include/amwg.h): the
// built-in families' instantiations of the four grouped kernels of amwg_pointwise.h -- the WAIC partial kernel, the test library's loglik kernel, LOO's select and
// compaction kernels, each with a lane per group walking the staged draws in blocks of R.  Everything else of a grouped call is the ungrouped call's code with G for
// n: the host path (amwg_pointwise_host.hip), the merge, pick and fit kernels and the totals (amwg_waic.hip, amwg_loo.hip).  The Bernoulli family is served through
// the two values an observation takes, which says nothing about a sum over a group: the grouped calls refuse it, and it has no instantiation here.
// Part of libamwg.so; not a source of the step kernels (tools/build_id.py).
#include <hip/hip_runtime.h>

#include "amwg_loo.h"
#include "amwg_terms.h"
#include "amwg_waic.h"

using namespace amwg;

namespace {

template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_partial_grouped_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                        const WaicDataset *__restrict__ sets, const GroupSet *__restrict__ gsets, const int32_t *__restrict__ csr,
                                                                        const int64_t *__restrict__ part_off, Part *__restrict__ parts) {
  waic_partial_grouped_body<Family<MODEL>>(draws, rows, PR, C, cpd, d0, M, sets, gsets, csr, part_off, parts);
}

template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_loglik_grouped_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, const WaicModel M,
                                                                       const WaicDataset *__restrict__ sets, const GroupSet *__restrict__ gsets, const int32_t *__restrict__ csr,
                                                                       double *__restrict__ out, int64_t g_max) {
  waic_loglik_grouped_body<Family<MODEL>>(draws, rows, PR, C, cpd, M, sets, gsets, csr, out, g_max);
}

// (the atomics are loo_hist_body's and loo_compact_body's, on the same integers: amwg_loo.hip)
template <int MODEL>
__global__ void __launch_bounds__(kThreads) loo_hist_grouped_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                    const WaicDataset *__restrict__ sets, const GroupSet *__restrict__ gsets, const int32_t *__restrict__ csr,
                                                                    const int64_t *__restrict__ obs_off, LooState *__restrict__ state, uint32_t *__restrict__ hist, int pass) {
  loo_hist_grouped_body<Family<MODEL>>(draws, rows, PR, C, cpd, d0, M, sets, gsets, csr, obs_off, state, hist, pass);
}

template <int MODEL>
__global__ void __launch_bounds__(kThreads) loo_compact_grouped_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                       const WaicDataset *__restrict__ sets, const GroupSet *__restrict__ gsets, const int32_t *__restrict__ csr,
                                                                       const int64_t *__restrict__ obs_off, const int64_t *__restrict__ part_off, LooState *__restrict__ state,
                                                                       double *__restrict__ tail, uint32_t cap, double *__restrict__ parts) {
  loo_compact_grouped_body<Family<MODEL>>(draws, rows, PR, C, cpd, d0, M, sets, gsets, csr, obs_off, part_off, state, tail, cap, parts);
}

template <int MODEL> const void *grouped_fn(int k) {
  const void *const fn[4] = {reinterpret_cast<const void *>(&waic_partial_grouped_kernel<MODEL>), reinterpret_cast<const void *>(&waic_loglik_grouped_kernel<MODEL>),
                             reinterpret_cast<const void *>(&loo_hist_grouped_kernel<MODEL>), reinterpret_cast<const void *>(&loo_compact_grouped_kernel<MODEL>)};
  return fn[k];
}

}  // namespace

const void *amwg_grouped_family_fn(int model, int k) {
  switch (model) {
    case AMWG_MODEL_NORMAL: return grouped_fn<AMWG_MODEL_NORMAL>(k);
    case AMWG_MODEL_HIER_NORMAL: return grouped_fn<AMWG_MODEL_HIER_NORMAL>(k);
    case AMWG_MODEL_POIS_GLM: return grouped_fn<AMWG_MODEL_POIS_GLM>(k);
    default: return nullptr;
  }
}
