// amwg_waic.hip -- WAIC per dataset on the device from the stored draws (amwg_last_sample_dataset_waic; part of libamwg.so).  include/amwg.h states the rule,
// amwg_waic.h the route: a thread owns an observation and walks the draws, the draw-invariant values come from LDS as broadcasts, the draws are split over
// wavefronts and workgroups by a function of (S, n) alone, and the partials are merged in a fixed order.  The terms are the reference's, bit for bit (amwg_terms.h,
// shared with amwg_loo.hip: amwg_ld.h, amwg_div.h, exp_log_v8); the accumulations are bounded, not pinned.  The exponential of the log-sum-exp is exp_v8 (fdlibm's, below 1 ulp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "amwg_dataset_quantiles.h"
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_terms.h"
#include "amwg_waic.h"

using namespace amwg;

namespace {

// parts[part_off[z] + split * n + i], z = the dataset's place in the batch (amwg_pointwise.h)
template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_partial_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                const WaicDataset *__restrict__ sets, const int64_t *__restrict__ part_off, Part *__restrict__ parts) {
  waic_partial_body<Family<MODEL>>(draws, rows, PR, C, cpd, d0, M, sets, part_off, parts);
}

// the same terms over one window of a summarising call, continued from and written back to state[state_off[d] + split * n + i] (amwg_pointwise.h; amwg_waic_fold.hip)
template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_fold_kernel(const double *__restrict__ window, int64_t nrows, int64_t g0, int64_t window_rows, int PR, int64_t C, int64_t cpd,
                                                             const WaicModel M, const WaicDataset *__restrict__ sets, const int64_t *__restrict__ state_off, Part *__restrict__ state) {
  waic_fold_body<Family<MODEL>>(window, nrows, g0, window_rows, PR, C, cpd, M, sets, state_off, state);
}

// out[(d * out_stride + i) * 2 + (0 | 1)] = lppd_i | p_i for i < n: the splits merged in ascending order
// (model-free: bern = the family of two observations per dataset; stage = the staged run length of the partial kernel is no part of it)
__global__ void __launch_bounds__(kThreads) waic_merge_kernel(int64_t rows, int64_t cpd, int d0, const WaicDataset *__restrict__ sets, int bern, const int64_t *__restrict__ part_off,
                                                              const Part *__restrict__ parts, double *__restrict__ out, int64_t out_stride) {
  const int d = d0 + (int)blockIdx.y;
  const WaicDataset ds = sets[d];
  const int64_t n = bern ? (ds.n_obs > 0 ? 2 : 0) : ds.n_obs, S = rows * cpd, splits = waic_splits(S, n);
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const Part *p = parts + part_off[blockIdx.y] + i;
  Part a = p[0];
  double cnt = (double)(split_begin(S, splits, 1) - split_begin(S, splits, 0));
  for (int64_t k = 1; k < splits; ++k) merge_parts(a, cnt, p[k * n], (double)(split_begin(S, splits, k + 1) - split_begin(S, splits, k)));
  const double Sd = (double)S;
  double lppd = a.m + log_v8(a.sum) - log_v8(Sd), pv = a.M2 / (Sd - 1.0);
  if (!(__builtin_fabs(a.M2) < kInf) || !(__builtin_fabs(lppd) < kInf)) { lppd = __builtin_nan(""); pv = __builtin_nan(""); }
  out[(d * out_stride + i) * 2] = lppd;
  out[(d * out_stride + i) * 2 + 1] = pv;
}

// the terms themselves, out[(d * S + s) * n_max + i]: the test library's view of what the partial kernel accumulates (amwg_pointwise.h)
template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_loglik_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, const WaicModel M,
                                                               const WaicDataset *__restrict__ sets, double *__restrict__ out, int64_t n_max) {
  waic_loglik_body<Family<MODEL>, WaicModel, MODEL == AMWG_MODEL_BETA_BERN>(draws, rows, PR, C, cpd, M, sets, out, n_max);
}

int run_kernels(const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, const WaicDataset *d_sets, int64_t n_max,
                double *d_pw, double *d_loglik, size_t scratch_bytes, hipStream_t stream) {
  int64_t cpd = C / D;      // (not const: the args[] lists point at it)
  const int64_t S = rows * cpd;
  DevBuf two, off, parts;
  if (K.bern) HIP_TRY(two.alloc((size_t)D * 4 * 8));
  double *out = K.bern ? two.as<double>() : d_pw;
  const int64_t out_stride = K.bern ? 2 : n_max;
  const PointwisePlan plan = amwg_pointwise_plan(K, sets, D, S, 0, sizeof(Part), scratch_bytes);
  HIP_TRY(off.alloc((size_t)D * 8));
  HIP_TRY(hipMemcpyAsync(off.p, plan.off.data() + D, (size_t)D * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(parts.alloc((size_t)plan.most_parts * sizeof(Part)));
  Part *d_parts = parts.as<Part>();
  // a grouped call: `sets` and d_sets count groups; the walking kernels take the observations' sets and the groups in their place
  const int walk = K.groups ? kPwGrouped : 0;
  const WaicDataset *obs_sets = K.groups ? K.groups->d_sets.as<WaicDataset>() : d_sets;
  const GroupSet *gsets = K.groups ? K.groups->d_gsets.as<GroupSet>() : nullptr;
  const int32_t *csr = K.groups ? K.groups->d_csr.as<int32_t>() : nullptr;
  for (const PointwiseBatch &b : plan.batches) {
    if (b.tiles == 0) continue;
    int d0 = b.d0;
    const int64_t *part_off = off.as<int64_t>() + d0;
    void *args[] = {&draws, &rows, &PR, &C, &cpd, &d0, K.model_arg(), &d_sets, &part_off, &d_parts};
    void *grouped_args[] = {&draws, &rows, &PR, &C, &cpd, &d0, K.model_arg(), &obs_sets, &gsets, &csr, &part_off, &d_parts};
    HIP_TRY(amwg_pointwise_go(K, walk + kPwWaicPartial, dim3((unsigned)b.tiles, (unsigned)b.splits, (unsigned)(b.d1 - d0)), stream, K.groups ? grouped_args : args));
    hipLaunchKernelGGL(waic_merge_kernel, dim3((unsigned)((b.n_most + kThreads - 1) / kThreads), (unsigned)(b.d1 - d0)), dim3(kThreads), 0, stream, rows, cpd, d0, d_sets, K.bern ? 1 : 0,
                       part_off, d_parts, out, out_stride);
    HIP_TRY(hipGetLastError());
  }
  if (K.bern) HIP_TRY(amwg_pointwise_bern_expand(K, d_sets, D, two.as<double>(), d_pw, n_max, 2, stream));
  if (d_loglik && K.groups) {      // [D][S][G_max]: a tile of 64 groups per workgroup, the draws in as many rows of workgroups as a grid takes
    void *args[] = {&draws, &rows, &PR, &C, &cpd, K.model_arg(), &obs_sets, &gsets, &csr, &d_loglik, &n_max};
    const int64_t rows_of_blocks = (S + kWaves - 1) / kWaves;
    HIP_TRY(amwg_pointwise_go(K, kPwGrouped + kPwWaicLoglik, dim3((unsigned)((n_max + kTile - 1) / kTile), (unsigned)(rows_of_blocks < 65535 ? rows_of_blocks : 65535), (unsigned)D), stream, args));
  } else if (d_loglik) {
    void *args[] = {&draws, &rows, &PR, &C, &cpd, K.model_arg(), &d_sets, &d_loglik, &n_max};
    HIP_TRY(amwg_pointwise_go(K, kPwWaicLoglik, dim3((unsigned)((n_max + kThreads - 1) / kThreads), (unsigned)S, (unsigned)D), stream, args));
  }
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is freed on return)
  return AMWG_OK;
}

template <int... MODEL> const void *family_fn(PointwiseModels<MODEL...>, int model, int k) {
  const void *const fn[][3] = {{reinterpret_cast<const void *>(&waic_partial_kernel<MODEL>), reinterpret_cast<const void *>(&waic_loglik_kernel<MODEL>),
                                reinterpret_cast<const void *>(&waic_fold_kernel<MODEL>)}...};
  return fn[model - AMWG_MODEL_NORMAL][k];
}

}  // namespace

const void *amwg_waic_family_fn(int model, int k) { return family_fn(BuiltinModels{}, model, k); }

int amwg_waic_shape(const char *call, int64_t rows, int PR, int64_t C, int D) {
  TRYB(amwg_dataset_quantiles_shape(call, rows, PR, C, D, 1));
  if (rows * (C / D) < 2) return amwg_fail(AMWG_EINVAL, "%s: fewer than 2 draws per dataset (rows %lld, chains per dataset %lld)", call, (long long)rows, (long long)(C / D));
  return AMWG_OK;
}

void amwg_waic_totals(const double *pw, int64_t n, double *summary, int32_t *high) {
  double lppd = 0.0, p = 0.0, elpd = 0.0;
  int32_t h = 0;
  for (int64_t i = 0; i < n; ++i) {
    lppd += pw[2 * i];
    p += pw[2 * i + 1];
    elpd += pw[2 * i] - pw[2 * i + 1];
    h += pw[2 * i + 1] > 0.4 ? 1 : 0;
  }
  const double centre = elpd / (double)n;
  double ss = 0.0;
  for (int64_t i = 0; i < n; ++i) { const double e = (pw[2 * i] - pw[2 * i + 1]) - centre; ss += e * e; }
  summary[0] = elpd;
  summary[1] = n == 1 ? (double)NAN : std::sqrt((double)n * ss / (double)(n - 1));
  summary[2] = p;
  summary[3] = lppd;
  if (high) *high = h;
}

int amwg_waic_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, double *summary,
                     int32_t *high, double *pointwise, double *loglik, size_t scratch_bytes, hipStream_t stream) {
  if (!draws || !sets || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_waic_shape(call, rows, PR, C, D));
  PointwiseLaunch K;
  TRYB(amwg_pointwise_family(call, model, PR, D, K));
  return amwg_waic_run(call, draws, rows, PR, C, D, K, sets, summary, high, pointwise, loglik, scratch_bytes, stream);
}

int amwg_waic_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                  int32_t *high, double *pointwise, double *loglik, size_t scratch_bytes, hipStream_t stream) {
  PointwiseOut o;
  TRYB(amwg_pointwise_begin(call, sets, D, loglik ? rows * (C / D) : 0, stream, o));
  TRYB(run_kernels(draws, rows, PR, C, D, K, sets, o.sets.as<WaicDataset>(), o.n_max, o.pw.as<double>(), loglik ? o.extra.as<double>() : nullptr, scratch_bytes, stream));
  std::vector<double> own;
  double *pw = pointwise;
  if (!pw) { own.resize(o.pw_count ? o.pw_count : 1); pw = own.data(); }
  TRYB(amwg_pointwise_fetch(o, pw, loglik));
  for (int d = 0; d < D; ++d) amwg_waic_totals(pw + (size_t)d * (size_t)o.n_max * 2, sets[d].n_obs, summary + (size_t)d * 4, high ? high + d : nullptr);
  return AMWG_OK;
}

extern "C" int amwg_last_sample_dataset_waic(amwg_sampler *s, double *summary, int32_t *high, double *pointwise) {
  static const char *call = "amwg_last_sample_dataset_waic";
  if (s && summary && amwg_summarised(s)) {      // the draws were not kept: only what was folded while they passed can answer
    const WaicFold *f = amwg_waic_armed(s);
    if (!f || !f->folded)
      return amwg_fail(AMWG_EINVAL, "%s: the last sample call was amwg_sample_summarize, which kept no draw, and no WAIC fold was armed for it (amwg_set_waic before the call)", call);
    HIP_TRY(hipSetDevice(s->device));
    return amwg_waic_fold_finish(call, *f, summary, high, pointwise, s->stream);
  }
  return amwg_pointwise_entry(call, s, summary, high, pointwise, amwg_waic_shape, amwg_waic_run);
}

extern "C" int amwg_last_sample_dataset_waic_grouped(amwg_sampler *s, const int32_t *labels, double *summary, int32_t *high, double *pointwise, int32_t *n_groups_out) {
  return amwg_pointwise_entry("amwg_last_sample_dataset_waic_grouped", s, summary, high, pointwise, amwg_waic_shape, amwg_waic_run, true, labels, n_groups_out);
}
