// amwg_waic.hip -- WAIC per dataset on the device from the stored draws (amwg_last_sample_dataset_waic; part of libamwg.so).  include/amwg.h states the rule,
// amwg_waic.h the route: a thread owns an observation and walks the draws, the draw-invariant values come from LDS as broadcasts, the draws are split over
// wavefronts and workgroups by a function of (S, n) alone, and the partials are merged in a fixed order.  The terms are the reference's, bit for bit (amwg_terms.h,
// shared with amwg_loo.hip: amwg_ld.h, amwg_div.h, exp_log_v8); the accumulations are bounded, not pinned.  The exponential of the log-sum-exp is exp_v8 (fdlibm's, below 1 ulp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amwg_dataset.h"
#include "amwg_dataset_quantiles.h"
#include "amwg_div.h"
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_ld.h"
#include "amwg_sampler.h"
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

__global__ void __launch_bounds__(kThreads) waic_fill_nan_kernel(double *out, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < count) out[k] = __builtin_nan("");
}

// the Bernoulli family: observation i takes the pair of its value; an invalid x_i has the term -inf in every draw: NaN
__global__ void __launch_bounds__(kThreads) waic_bern_expand_kernel(const WaicModel M, const WaicDataset *__restrict__ sets, const double *__restrict__ two, double *__restrict__ out,
                                                                    int64_t n_max) {
  const int d = blockIdx.y;
  const WaicDataset ds = sets[d];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= ds.n_obs) return;
  const bool invalid = M.invalid && M.invalid[ds.off_xb + i];
  const int k = M.xb[ds.off_xb + i] ? 0 : 1;
  out[(d * n_max + i) * 2] = invalid ? __builtin_nan("") : two[(d * 2 + k) * 2];
  out[(d * n_max + i) * 2 + 1] = invalid ? __builtin_nan("") : two[(d * 2 + k) * 2 + 1];
}

// the terms themselves, out[(d * S + s) * n_max + i]: the test library's view of what the partial kernel accumulates (amwg_pointwise.h)
template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_loglik_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, const WaicModel M,
                                                               const WaicDataset *__restrict__ sets, double *__restrict__ out, int64_t n_max) {
  waic_loglik_body<Family<MODEL>, WaicModel, MODEL == AMWG_MODEL_BETA_BERN>(draws, rows, PR, C, cpd, M, sets, out, n_max);
}

size_t g_budget = kWaicScratchBytes;

int run_kernels(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, const WaicDataset *d_sets,
                int64_t n_max, double *d_pw, double *d_loglik, hipStream_t stream) {
  const bool bern = K.bern;
  const int64_t cpd = C / D, S = rows * cpd;
  DevBuf two, off, parts;
  if (bern) HIP_TRY(two.alloc((size_t)D * 4 * 8));
  double *out = bern ? two.as<double>() : d_pw;
  const int64_t out_stride = bern ? 2 : n_max;
  // the batches: consecutive datasets whose partials fit the budget together (a dataset beyond it runs alone)
  std::vector<int64_t> n_eff((size_t)D), part_off((size_t)D);
  std::vector<int> batch_end;
  size_t largest = 0;
  {
    size_t in_batch = 0;
    for (int d = 0; d < D; ++d) {
      n_eff[(size_t)d] = bern ? (sets[d].n_obs > 0 ? 2 : 0) : sets[d].n_obs;
      const size_t bytes = (size_t)waic_splits(S, n_eff[(size_t)d]) * (size_t)n_eff[(size_t)d] * sizeof(Part);
      if (in_batch && in_batch + bytes > g_budget) { batch_end.push_back(d); in_batch = 0; }
      part_off[(size_t)d] = (int64_t)(in_batch / sizeof(Part));
      in_batch += bytes;
      largest = in_batch > largest ? in_batch : largest;
    }
    batch_end.push_back(D);
  }
  HIP_TRY(off.alloc((size_t)D * 8));
  HIP_TRY(hipMemcpyAsync(off.p, part_off.data(), (size_t)D * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(parts.alloc(largest));
  int d0 = 0;
  for (const int d1 : batch_end) {
    int64_t tiles = 0, splits = 0, n_most = 0;
    for (int d = d0; d < d1; ++d) {
      const int64_t n = n_eff[(size_t)d], t = (n + kTile - 1) / kTile, sp = waic_splits(S, n);
      tiles = t > tiles ? t : tiles; splits = sp > splits ? sp : splits; n_most = n > n_most ? n : n_most;
    }
    if (tiles > 0) {
      HIP_TRY(K.waic_partial(dim3((unsigned)tiles, (unsigned)splits, (unsigned)(d1 - d0)), stream, draws, rows, PR, C, cpd, d0, d_sets, off.as<int64_t>() + d0, parts.as<Part>()));
      hipLaunchKernelGGL(waic_merge_kernel, dim3((unsigned)((n_most + kThreads - 1) / kThreads), (unsigned)(d1 - d0)), dim3(kThreads), 0, stream, rows, cpd, d0, d_sets, bern ? 1 : 0,
                         off.as<int64_t>() + d0, parts.as<Part>(), out, out_stride);
      HIP_TRY(hipGetLastError());
    }
    d0 = d1;
  }
  if (bern) {
    hipLaunchKernelGGL(waic_bern_expand_kernel, dim3((unsigned)((n_max + kThreads - 1) / kThreads), (unsigned)D), dim3(kThreads), 0, stream, *K.family, d_sets, two.as<double>(), d_pw, n_max);
    HIP_TRY(hipGetLastError());
  }
  if (d_loglik) {
    HIP_TRY(K.waic_loglik(dim3((unsigned)((n_max + kThreads - 1) / kThreads), (unsigned)S, (unsigned)D), stream, draws, rows, PR, C, cpd, d_sets, d_loglik, n_max));
  }
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is freed on return)
  (void)call;
  return AMWG_OK;
}

template <int MODEL>
void family_kernels(PointwiseLaunch &K, const WaicModel &model) {
  K.waic_partial = [model](dim3 grid, hipStream_t stream, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicDataset *sets, const int64_t *part_off, void *parts) {
    hipLaunchKernelGGL(waic_partial_kernel<MODEL>, grid, dim3(kThreads), 0, stream, draws, rows, PR, C, cpd, d0, model, sets, part_off, static_cast<Part *>(parts));
    return hipGetLastError();
  };
  K.waic_loglik = [model](dim3 grid, hipStream_t stream, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, const WaicDataset *sets, double *out, int64_t n_max) {
    hipLaunchKernelGGL(waic_loglik_kernel<MODEL>, grid, dim3(kThreads), 0, stream, draws, rows, PR, C, cpd, model, sets, out, n_max);
    return hipGetLastError();
  };
}

}  // namespace

size_t amwg_waic_set_budget(size_t bytes) {
  const size_t before = g_budget;
  g_budget = bytes ? bytes : kWaicScratchBytes;
  return before;
}

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

void amwg_waic_family_kernels(PointwiseLaunch &K, const WaicModel &model) {
  K.bern = model.model == AMWG_MODEL_BETA_BERN;
  K.family = &model;
  switch (model.model) {
    case AMWG_MODEL_NORMAL: family_kernels<AMWG_MODEL_NORMAL>(K, model); break;
    case AMWG_MODEL_BETA_BERN: family_kernels<AMWG_MODEL_BETA_BERN>(K, model); break;
    case AMWG_MODEL_HIER_NORMAL: family_kernels<AMWG_MODEL_HIER_NORMAL>(K, model); break;
    default: family_kernels<AMWG_MODEL_POIS_GLM>(K, model); break;
  }
}

// a closure's code object (amwg_rtc.hip load_pointwise): the four entries of amwg_pointwise.h, launched with the closure's model argument
void amwg_pointwise_user_kernels(PointwiseLaunch &K, const UserPointwise &u) {
  K.bern = false;
  K.family = nullptr;
  const UserPointwise U = u;
  auto go = [](hipFunction_t fn, dim3 grid, hipStream_t stream, void **args) { return hipModuleLaunchKernel(fn, grid.x, grid.y, grid.z, kThreads, 1, 1, 0, stream, args, nullptr); };
  K.waic_partial = [U, go](dim3 grid, hipStream_t stream, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicDataset *sets, const int64_t *part_off, void *parts) {
    UserTermsArg M = U.arg;
    void *args[] = {&draws, &rows, &PR, &C, &cpd, &d0, &M, &sets, &part_off, &parts};
    return go(U.waic_partial, grid, stream, args);
  };
  K.waic_loglik = [U, go](dim3 grid, hipStream_t stream, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, const WaicDataset *sets, double *out, int64_t n_max) {
    UserTermsArg M = U.arg;
    void *args[] = {&draws, &rows, &PR, &C, &cpd, &M, &sets, &out, &n_max};
    return go(U.waic_loglik, grid, stream, args);
  };
  K.loo_hist = [U, go](dim3 grid, hipStream_t stream, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicDataset *sets, const int64_t *obs_off, void *state,
                       uint32_t *hist, int pass) {
    UserTermsArg M = U.arg;
    void *args[] = {&draws, &rows, &PR, &C, &cpd, &d0, &M, &sets, &obs_off, &state, &hist, &pass};
    return go(U.loo_hist, grid, stream, args);
  };
  K.loo_compact = [U, go](dim3 grid, hipStream_t stream, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicDataset *sets, const int64_t *obs_off,
                          const int64_t *part_off, void *state, double *tail, uint32_t cap, double *parts) {
    UserTermsArg M = U.arg;
    void *args[] = {&draws, &rows, &PR, &C, &cpd, &d0, &M, &sets, &obs_off, &part_off, &state, &tail, &cap, &parts};
    return go(U.loo_compact, grid, stream, args);
  };
}

int amwg_waic_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, double *summary,
                     int32_t *high, double *pointwise, double *loglik, hipStream_t stream) {
  if (!draws || !sets || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_waic_shape(call, rows, PR, C, D));
  const int need = model.model == AMWG_MODEL_NORMAL ? 2 : model.model == AMWG_MODEL_BETA_BERN ? 1 : model.model == AMWG_MODEL_HIER_NORMAL ? model.G + 2 : model.model == AMWG_MODEL_POIS_GLM ? 9 : -1;
  if (need < 0) return amwg_fail(AMWG_EINVAL, "%s: unknown model %d", call, model.model);
  if (PR < need) return amwg_fail(AMWG_EINVAL, "%s: the family reads %d components of a draw, the draws hold %d", call, need, PR);
  if (model.model == AMWG_MODEL_HIER_NORMAL && D != 1) return amwg_fail(AMWG_EINVAL, "%s: the hierarchical family runs on one dataset", call);
  PointwiseLaunch K;
  amwg_waic_family_kernels(K, model);
  return amwg_waic_run(call, draws, rows, PR, C, D, K, sets, summary, high, pointwise, loglik, stream);
}

int amwg_waic_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                  int32_t *high, double *pointwise, double *loglik, hipStream_t stream) {
  if (!draws || !sets || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_waic_shape(call, rows, PR, C, D));
  int64_t n_max = 0;
  for (int d = 0; d < D; ++d) {
    if (sets[d].n_obs < 0) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: n_obs < 0", call, d);
    n_max = sets[d].n_obs > n_max ? sets[d].n_obs : n_max;
  }
  const int64_t S = rows * (C / D);
  const size_t pw_count = (size_t)D * (size_t)n_max * 2;
  DevBuf d_sets, d_pw, d_ll;
  HIP_TRY(d_sets.alloc((size_t)D * sizeof(WaicDataset)));
  HIP_TRY(hipMemcpyAsync(d_sets.p, sets, (size_t)D * sizeof(WaicDataset), hipMemcpyHostToDevice, stream));
  HIP_TRY(d_pw.alloc(pw_count * 8));
  if (pw_count) {
    hipLaunchKernelGGL(waic_fill_nan_kernel, dim3((unsigned)((pw_count + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, d_pw.as<double>(), (int64_t)pw_count);
    HIP_TRY(hipGetLastError());
  }
  const size_t ll_count = loglik ? (size_t)D * (size_t)S * (size_t)n_max : 0;
  if (loglik) {
    HIP_TRY(d_ll.alloc(ll_count * 8));
    if (ll_count) {
      hipLaunchKernelGGL(waic_fill_nan_kernel, dim3((unsigned)((ll_count + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, d_ll.as<double>(), (int64_t)ll_count);
      HIP_TRY(hipGetLastError());
    }
  }
  double *dl = loglik ? d_ll.as<double>() : nullptr;
  const WaicDataset *ds = d_sets.as<WaicDataset>();
  TRYB(run_kernels(call, draws, rows, PR, C, D, K, sets, ds, n_max, d_pw.as<double>(), dl, stream));
  std::vector<double> own;
  double *pw = pointwise;
  if (!pw) { own.resize(pw_count ? pw_count : 1); pw = own.data(); }
  if (pw_count) HIP_TRY(hipMemcpy(pw, d_pw.p, pw_count * 8, hipMemcpyDeviceToHost));
  if (ll_count) HIP_TRY(hipMemcpy(loglik, d_ll.p, ll_count * 8, hipMemcpyDeviceToHost));
  for (int d = 0; d < D; ++d) amwg_waic_totals(pw + (size_t)d * (size_t)n_max * 2, sets[d].n_obs, summary + (size_t)d * 4, high ? high + d : nullptr);
  return AMWG_OK;
}

// the sampler's datasets and family as the launchers take them (shared with amwg_last_sample_dataset_loo); the sampler's device is current
int amwg_waic_describe(amwg_sampler *s, std::vector<WaicDataset> &sets, WaicModel &m) {
  const int D = s->n_datasets;
  sets.assign((size_t)D, WaicDataset{});
  if (D == 1) {
    sets[0] = WaicDataset{s->ds_n_obs.empty() ? s->d.n_obs : s->ds_n_obs[0], s->mc.data_mid_range, 0, 0, 0, 0};
  } else {
    std::vector<DatasetConsts> consts((size_t)D);
    HIP_TRY(hipMemcpy(consts.data(), s->d_ds_consts, (size_t)D * sizeof(DatasetConsts), hipMemcpyDeviceToHost));
    for (int d = 0; d < D; ++d) sets[(size_t)d] = WaicDataset{consts[(size_t)d].n_obs, consts[(size_t)d].data_mid_range, consts[(size_t)d].off_x, consts[(size_t)d].off_y, consts[(size_t)d].off_lfact, consts[(size_t)d].off_xb};
  }
  m.model = s->model; m.G = s->d.G; m.exact_division = s->mc.exact_division;
  m.neg_half_log_2pi = s->mc.neg_half_log_2pi;
  m.x = s->d.x; m.y = s->d.y; m.lfact = s->d.lfact; m.xb = s->d.xb;
  m.invalid = s->model == AMWG_MODEL_BETA_BERN ? static_cast<const uint8_t *>(s->d.arr[1]) : nullptr;      // (amwg_create.hip upload_bernoulli_data)
  return AMWG_OK;
}

// ... and of a closure whose pointwise text is set (amwg_set_pointwise): the code object compiled and loaded on first use, every dataset with kTermN observations
int amwg_pointwise_describe_user(amwg_sampler *s, std::vector<WaicDataset> &sets, UserPointwise &u) {
  TRYB(load_pointwise(s, s->user_arch.c_str()));
  u.waic_partial = s->pw_fn[0]; u.waic_loglik = s->pw_fn[1]; u.loo_hist = s->pw_fn[2]; u.loo_compact = s->pw_fn[3];
  u.arg.d = s->d;
  u.arg.table = s->n_datasets > 1 ? s->d_user_ds_table : nullptr;
  u.arg.row_stride = s->user_ds_row_stride;
  u.arg.reserved = 0;
  u.n_obs = s->pw_n_obs; u.state_n = s->pw_state_n;
  sets.assign((size_t)s->n_datasets, WaicDataset{s->pw_n_obs, 0, 0, 0, 0, 0});
  return AMWG_OK;
}

extern "C" int amwg_set_pointwise(amwg_sampler *s, const char *terms_source) {
  static const char *call = "amwg_set_pointwise";
  if (!s || !terms_source) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (!s->user) return amwg_fail(AMWG_EINVAL, "%s: the pointwise terms of a built-in family are known to the library; the text is for amwg_create_user* samplers only", call);
  auto int_after = [&](const char *key) -> long {
    const char *q = strstr(terms_source, key);
    return q ? strtol(q + strlen(key), nullptr, 10) : -1;
  };
  const long n = int_after("kTermN = "), p = int_after("kStateN = ");
  if (!strstr(terms_source, "struct UserTerms") || n < 1 || n >= (1l << 31)) return amwg_fail(AMWG_EINVAL, "%s: the text does not define struct amwg::UserTerms with kTermN >= 1 (translate.js, options.pointwise)", call);
  if (p != s->P) return amwg_fail(AMWG_EINVAL, "%s: the text was made for a state of %ld components, the sampler's has %d", call, p, s->P);
  HIP_TRY(hipSetDevice(s->device));
  if (s->pw_module) { (void)hipModuleUnload(s->pw_module); s->pw_module = nullptr; }
  s->pw_terms = terms_source;
  s->pw_n_obs = (int)n; s->pw_state_n = (int)p;
  return AMWG_OK;
}

extern "C" int64_t amwg_pointwise_n_obs(const amwg_sampler *s) { return s && s->user && !s->pw_terms.empty() ? s->pw_n_obs : 0; }

extern "C" int amwg_last_sample_dataset_waic(amwg_sampler *s, double *summary, int32_t *high, double *pointwise) {
  static const char *call = "amwg_last_sample_dataset_waic";
  if (!s || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (s->user && s->pw_terms.empty()) return amwg_fail(AMWG_EINVAL, "%s: the pointwise terms of a closure are not known to the library; built-in families only", call);
  TRYB(amwg_refuse_summarised(s, call));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "%s: no sample() call yet", call);
  const int D = s->n_datasets, PR = s->P + s->D;
  TRYB(amwg_waic_shape(call, s->last_rows, PR, s->C, D));
  if (s->mc.group_local) return amwg_fail(AMWG_EINVAL, "%s: a group_local sampler keeps its observations as a lane-major tile; the pointwise terms need them in index order", call);
  HIP_TRY(hipSetDevice(s->device));
  std::vector<WaicDataset> sets;
  if (s->user) {
    UserPointwise u;
    TRYB(amwg_pointwise_describe_user(s, sets, u));
    PointwiseLaunch K;
    amwg_pointwise_user_kernels(K, u);
    return amwg_waic_run(call, s->last_draws, s->last_rows, PR, s->C, D, K, sets.data(), summary, high, pointwise, nullptr, s->stream);
  }
  WaicModel m{};
  TRYB(amwg_waic_describe(s, sets, m));
  return amwg_waic_launch(call, s->last_draws, s->last_rows, PR, s->C, D, m, sets.data(), summary, high, pointwise, nullptr, s->stream);
}
