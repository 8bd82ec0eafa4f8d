// amwg_waic.hip -- WAIC per dataset on the device from the stored draws (amwg_last_sample_dataset_waic; part of libamwg.so).  include/amwg.h states the rule,
// amwg_waic.h the route: a thread owns an observation and walks the draws, the draw-invariant values come from LDS as broadcasts, the draws are split over
// wavefronts and workgroups by a function of (S, n) alone, and the partials are merged in a fixed order.  The terms are the reference's, bit for bit (amwg_terms.h,
// shared with amwg_loo.hip: amwg_ld.h, amwg_div.h, exp_log_v8); the accumulations are bounded, not pinned.  The exponential of the log-sum-exp is exp_v8 (fdlibm's, below 1 ulp).
#include <hip/hip_runtime.h>

#include <cmath>
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

struct Part { double m, sum, mean, M2; };      // max term and sum exp(l - m); mean and sum (l - mean)^2.  The count is a function of the indices.
__device__ __forceinline__ void merge_parts(Part &a, double &na, const Part &b, double nb) {
  if (nb == 0.0) return;
  if (na == 0.0) { a = b; na = nb; return; }
  const double M = b.m > a.m ? b.m : a.m;
  a.sum = a.sum * exp_v8_cold(a.m - M) + b.sum * exp_v8_cold(b.m - M);
  a.m = M;
  const double nt = na + nb, delta = b.mean - a.mean;
  a.mean = a.mean + delta * (nb / nt);
  a.M2 = a.M2 + b.M2 + delta * delta * (na * nb / nt);
  na = nt;
}

// parts[part_off[z] + split * n + i], z = the dataset's place in the batch
template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_partial_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                const WaicDataset *__restrict__ sets, const int64_t *__restrict__ part_off, Part *__restrict__ parts) {
  typedef Family<MODEL> F;
  __shared__ typename F::Draw stage[kStage];
  __shared__ Part wave_part[kWaves - 1][kTile];
  const int d = d0 + (int)blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WaicDataset ds = sets[d];
  const int64_t n = F::n_eff(ds), S = rows * cpd, splits = waic_splits(S, n);
  if ((int64_t)blockIdx.x * kTile >= n || (int64_t)blockIdx.y >= splits) return;      // (uniform over the workgroup)
  const int64_t s_begin = split_begin(S, splits, blockIdx.y), s_end = split_begin(S, splits, (int64_t)blockIdx.y + 1);
  const int64_t i = (int64_t)blockIdx.x * kTile + lane;
  const bool active = i < n;
  const typename F::Obs o = F::load_obs(M, ds, active ? i : n - 1);
  Part a{-kInf, 0.0, 0.0, 0.0};
  double cnt = 0.0;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += kStage) {
    const int L = (int)(s_end - s0 < kStage ? s_end - s0 : kStage);
    __syncthreads();
    if (tid < L) stage[tid] = draw_at<F>(draws, PR, C, cpd, d, s0 + tid, M, ds);
    __syncthreads();
    if (wave >= L) continue;      // (uniform over the wavefront; the barriers above are reached by all: L does not depend on the wavefront)
    const double K = cnt == 0.0 ? F::term(o, stage[wave], i, draws, C) : a.mean;
    double s1 = 0.0, s2 = 0.0;
    int nb = 0;
    for (int j = wave; j < L; j += kWaves) {
      const double l = F::term(o, stage[j], i, draws, C);
      const double dm = l - a.m;
      const double e = waic_exp(-__builtin_fabs(dm));
      const bool up = dm > 0.0;
      a.sum = up ? __builtin_fma(a.sum, e, 1.0) : a.sum + e;
      a.m = up ? l : a.m;
      const double dk = l - K;
      s1 += dk;
      s2 = __builtin_fma(dk, dk, s2);
      ++nb;
    }
    const double nbd = (double)nb, q = s1 / nbd;
    double M2b = s2 - s1 * q;
    M2b = M2b < 0.0 ? 0.0 : M2b;      // (a NaN stays a NaN)
    const double mean_b = K + q;
    if (cnt == 0.0) { a.mean = mean_b; a.M2 = M2b; cnt = nbd; }
    else {
      const double nt = cnt + nbd, delta = mean_b - a.mean;
      a.mean = a.mean + delta * (nbd / nt);
      a.M2 = a.M2 + M2b + delta * delta * (cnt * nbd / nt);
      cnt = nt;
    }
  }
  __syncthreads();
  if (wave > 0) wave_part[wave - 1][lane] = a;
  __syncthreads();
  if (wave != 0 || !active) return;
  // the draws of the split went round the four wavefronts: wavefront w took those with (s - s0) % 4 == w of every staged run
  const int64_t len = s_end - s_begin, full = len / kStage, rest = len % kStage;
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const double nw = (double)(full * (kStage / kWaves) + (rest > w ? (rest - w + kWaves - 1) / kWaves : 0));
    merge_parts(a, cnt, wave_part[w - 1][lane], nw);
  }
  parts[part_off[blockIdx.z] + (int64_t)blockIdx.y * n + i] = a;
}

// out[(d * out_stride + i) * 2 + (0 | 1)] = lppd_i | p_i for i < n: the splits merged in ascending order
template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_merge_kernel(int64_t rows, int64_t cpd, int d0, const WaicDataset *__restrict__ sets, const int64_t *__restrict__ part_off,
                                                              const Part *__restrict__ parts, double *__restrict__ out, int64_t out_stride) {
  typedef Family<MODEL> F;
  const int d = d0 + (int)blockIdx.y;
  const WaicDataset ds = sets[d];
  const int64_t n = F::n_eff(ds), S = rows * cpd, splits = waic_splits(S, n);
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

// the terms themselves, out[(d * S + s) * n_max + i]: the test library's view of what the partial kernel accumulates (the same device functions)
template <int MODEL>
__global__ void __launch_bounds__(kThreads) waic_loglik_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, const WaicModel M,
                                                               const WaicDataset *__restrict__ sets, double *__restrict__ out, int64_t n_max) {
  typedef Family<MODEL> F;
  const int d = blockIdx.z;
  const WaicDataset ds = sets[d];
  const int64_t S = rows * cpd, s = blockIdx.y, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= ds.n_obs) return;
  const typename F::Draw w = draw_at<F>(draws, PR, C, cpd, d, s, M, ds);
  double l;
  if constexpr (MODEL == AMWG_MODEL_BETA_BERN) {
    const bool invalid = M.invalid && M.invalid[ds.off_xb + i];
    l = invalid ? -kInf : F::term(F::load_obs(M, ds, M.xb[ds.off_xb + i] ? 0 : 1), w, i, draws, C);
  } else {
    l = F::term(F::load_obs(M, ds, i), w, i, draws, C);
  }
  out[((int64_t)d * S + s) * n_max + i] = l;
}

size_t g_budget = kWaicScratchBytes;

template <int MODEL>
int run_family(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, const WaicDataset *d_sets,
               int64_t n_max, double *d_pw, double *d_loglik, hipStream_t stream) {
  const bool bern = MODEL == AMWG_MODEL_BETA_BERN;
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
      hipLaunchKernelGGL(waic_partial_kernel<MODEL>, dim3((unsigned)tiles, (unsigned)splits, (unsigned)(d1 - d0)), dim3(kThreads), 0, stream, draws, rows, PR, C, cpd, d0, model,
                         d_sets, off.as<int64_t>() + d0, parts.as<Part>());
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(waic_merge_kernel<MODEL>, dim3((unsigned)((n_most + kThreads - 1) / kThreads), (unsigned)(d1 - d0)), dim3(kThreads), 0, stream, rows, cpd, d0, d_sets,
                         off.as<int64_t>() + d0, parts.as<Part>(), out, out_stride);
      HIP_TRY(hipGetLastError());
    }
    d0 = d1;
  }
  if (bern) {
    hipLaunchKernelGGL(waic_bern_expand_kernel, dim3((unsigned)((n_max + kThreads - 1) / kThreads), (unsigned)D), dim3(kThreads), 0, stream, model, d_sets, two.as<double>(), d_pw, n_max);
    HIP_TRY(hipGetLastError());
  }
  if (d_loglik) {
    hipLaunchKernelGGL(waic_loglik_kernel<MODEL>, dim3((unsigned)((n_max + kThreads - 1) / kThreads), (unsigned)S, (unsigned)D), dim3(kThreads), 0, stream, draws, rows, PR, C, cpd,
                       model, d_sets, d_loglik, n_max);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is freed on return)
  (void)call;
  return AMWG_OK;
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

int amwg_waic_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, double *summary,
                     int32_t *high, double *pointwise, double *loglik, hipStream_t stream) {
  if (!draws || !sets || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_waic_shape(call, rows, PR, C, D));
  const int need = model.model == AMWG_MODEL_NORMAL ? 2 : model.model == AMWG_MODEL_BETA_BERN ? 1 : model.model == AMWG_MODEL_HIER_NORMAL ? model.G + 2 : model.model == AMWG_MODEL_POIS_GLM ? 9 : -1;
  if (need < 0) return amwg_fail(AMWG_EINVAL, "%s: unknown model %d", call, model.model);
  if (PR < need) return amwg_fail(AMWG_EINVAL, "%s: the family reads %d components of a draw, the draws hold %d", call, need, PR);
  if (model.model == AMWG_MODEL_HIER_NORMAL && D != 1) return amwg_fail(AMWG_EINVAL, "%s: the hierarchical family runs on one dataset", call);
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
  switch (model.model) {
    case AMWG_MODEL_NORMAL: TRYB(run_family<AMWG_MODEL_NORMAL>(call, draws, rows, PR, C, D, model, sets, ds, n_max, d_pw.as<double>(), dl, stream)); break;
    case AMWG_MODEL_BETA_BERN: TRYB(run_family<AMWG_MODEL_BETA_BERN>(call, draws, rows, PR, C, D, model, sets, ds, n_max, d_pw.as<double>(), dl, stream)); break;
    case AMWG_MODEL_HIER_NORMAL: TRYB(run_family<AMWG_MODEL_HIER_NORMAL>(call, draws, rows, PR, C, D, model, sets, ds, n_max, d_pw.as<double>(), dl, stream)); break;
    default: TRYB(run_family<AMWG_MODEL_POIS_GLM>(call, draws, rows, PR, C, D, model, sets, ds, n_max, d_pw.as<double>(), dl, stream)); break;
  }
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

extern "C" int amwg_last_sample_dataset_waic(amwg_sampler *s, double *summary, int32_t *high, double *pointwise) {
  static const char *call = "amwg_last_sample_dataset_waic";
  if (!s || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (s->user) return amwg_fail(AMWG_EINVAL, "%s: the pointwise terms of a closure are not known to the library; built-in families only", call);
  TRYB(amwg_refuse_summarised(s, call));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "%s: no sample() call yet", call);
  const int D = s->n_datasets, PR = s->P + s->D;
  TRYB(amwg_waic_shape(call, s->last_rows, PR, s->C, D));
  if (s->mc.group_local) return amwg_fail(AMWG_EINVAL, "%s: a group_local sampler keeps its observations as a lane-major tile; the pointwise terms need them in index order", call);
  HIP_TRY(hipSetDevice(s->device));
  std::vector<WaicDataset> sets;
  WaicModel m{};
  TRYB(amwg_waic_describe(s, sets, m));
  return amwg_waic_launch(call, s->last_draws, s->last_rows, PR, s->C, D, m, sets.data(), summary, high, pointwise, nullptr, s->stream);
}
