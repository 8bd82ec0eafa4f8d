// amwg_loo.hip -- PSIS-LOO per dataset on the device from the stored draws (amwg_last_sample_dataset_loo; part of libamwg.so).  include/amwg.h states the rule,
// amwg_loo.h the route: a radix select over the recomputed terms finds each observation's M + 1 smallest, one more pass compacts them and sums the rest, a workgroup
// per observation sorts the tail in LDS, fits the generalised Pareto and forms the smoothed sum.  The terms are WAIC's (amwg_terms.h), bit for bit; the excesses are
// pinned to the bit (exp_v8 of differences of sorted terms); the accumulations are bounded, not pinned, and deterministic: the only atomics are on integers.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <vector>

#include "amwg_host.h"
#include "amwg_loo.h"
#include "amwg_loo_fit.h"
#include "amwg_select.h"
#include "amwg_terms.h"

using namespace amwg;

namespace {

__global__ void __launch_bounds__(kThreads) loo_init_kernel(LooState *state, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < count) state[k] = LooState{0, 0, kMaxKey, 0, 0, 0, 0, 0, 0};
}

// one digit of the select (amwg_pointwise.h).  The atomics of the two kernels that walk the terms are there now, and as before every one is on an integer:
// atomicAdd(&cnt[...], 1u) on the LDS counters, atomicAdd(&h[...], c) on the global ones, atomicMin((unsigned long long *)&state[o_at].minkey, ...) and
// atomicOr(&state[o_at].bad, 1u) on the state's integer fields, atomicAdd(&state[o_at].cursor, 1u) for the tail slots
template <int MODEL>
__global__ void __launch_bounds__(kThreads) loo_hist_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                            const WaicDataset *__restrict__ sets, const int64_t *__restrict__ obs_off, LooState *__restrict__ state,
                                                            uint32_t *__restrict__ hist, int pass) {
  loo_hist_body<Family<MODEL>>(draws, rows, PR, C, cpd, d0, M, sets, obs_off, state, hist, pass);
}

// after a pass: the bin that holds rank M, per observation; *pending counts the observations that need another pass
__global__ void __launch_bounds__(kThreads) loo_pick_kernel(int d0, const WaicDataset *__restrict__ sets, int bern, const int64_t *__restrict__ obs_off, LooState *__restrict__ state,
                                                            const uint32_t *__restrict__ hist, int pass, uint32_t Mlen, uint32_t cap, int *__restrict__ pending) {
  const int d = d0 + (int)blockIdx.y;
  const int64_t n = bern ? (sets[d].n_obs > 0 ? 2 : 0) : sets[d].n_obs;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t o_at = obs_off[blockIdx.y] + i;
  LooState st = state[o_at];
  if (st.done) return;
  const uint32_t *h = hist + o_at * kBins;
  const int nb = pass_bins(pass), shift = pass_shift(pass);
  uint32_t cum = 0, c = 0;
  int b = 0;
  for (;; ++b) {
    c = h[b];
    if (st.lo + cum + c > Mlen || b == nb - 1) break;
    cum += c;
  }
  st.lo += cum;
  st.in = c;
  st.prefix |= (uint64_t)b << shift;
  if (st.lo + c <= cap) {
    st.done = 1; st.inclusive = 1;
    st.thr = st.prefix | (shift ? (((uint64_t)1 << shift) - 1) : 0);
  } else if (pass == kPasses - 1) {      // the bin is one key, held by more draws than the tail has room for
    st.done = 1; st.inclusive = 0;
    st.thr = st.prefix;
  } else {
    atomicAdd(pending, 1);
  }
  state[o_at] = st;
}

// the terms at or below the threshold into the tail, the others into the split's partial of B (amwg_pointwise.h)
template <int MODEL>
__global__ void __launch_bounds__(kThreads) loo_compact_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                               const WaicDataset *__restrict__ sets, const int64_t *__restrict__ obs_off, const int64_t *__restrict__ part_off,
                                                               LooState *__restrict__ state, double *__restrict__ tail, uint32_t cap, double *__restrict__ parts) {
  loo_compact_body<Family<MODEL>>(draws, rows, PR, C, cpd, d0, M, sets, obs_off, part_off, state, tail, cap, parts);
}

// (the workgroup's sums, the bitonic network, the excesses and the fit: amwg_loo_fit.h, shared with amwg_loo_predictive.hip)
// One workgroup per observation -- 256 threads, or one wavefront for a tail of at most kFitSmall slots (fit_threads) --: the tail sorted in LDS, the fit, the smoothed sum.  out[(d * out_stride + i) * 2 + (0 | 1)] = elpd_loo_i | khat_i; the sorted
// tail's first M + 1 go to tails_out[(d * out_stride + i) * (M + 1) + t] when asked for.  Dynamic LDS: (cap + kFitExtra) * 8 bytes.
__global__ void __launch_bounds__(kThreads) loo_fit_kernel(int64_t rows, int64_t cpd, int d0, const WaicDataset *__restrict__ sets, int bern, const int64_t *__restrict__ obs_off,
                                                           const int64_t *__restrict__ part_off, const LooState *__restrict__ state, double *__restrict__ tail, uint32_t cap,
                                                           const double *__restrict__ parts, uint32_t Mlen, int mm, double *__restrict__ out, int64_t out_stride,
                                                           double *__restrict__ tails_out) {
  extern __shared__ uint64_t lds[];
  uint64_t *keys = lds;
  double *Lj = reinterpret_cast<double *>(lds + cap), *Wj = Lj + kMaxTheta, *red = Wj + kMaxTheta;
  const int d = d0 + (int)blockIdx.y, tid = threadIdx.x;
  const uint32_t T = blockDim.x;
  const WaicDataset ds = sets[d];
  const int64_t n = bern ? (ds.n_obs > 0 ? 2 : 0) : ds.n_obs, S = rows * cpd, splits = waic_splits(S, n), i = blockIdx.x;
  if (i >= n) return;      // (uniform over the workgroup)
  const int64_t o_at = obs_off[blockIdx.y] + i;
  const LooState st = state[o_at];
  double *my_tail = tail + o_at * cap;
  const uint32_t taken = st.cursor < cap ? st.cursor : cap;
  const uint32_t nv = st.inclusive ? taken : Mlen + 1;      // the slots that hold terms
  for (uint32_t t = tid; t < cap; t += T) keys[t] = t < taken ? select_key(my_tail[t]) : (!st.inclusive && t <= Mlen ? st.thr : kMaxKey);
  __syncthreads();
  loo_sort<false>(keys, nullptr, cap);
  double *res = out + (d * out_stride + i) * 2;
  if (st.bad) {      // a NaN or an infinity among the terms: NaN (the launcher filled the tails with NaN)
    if (tid == 0) { res[0] = __builtin_nan(""); res[1] = __builtin_nan(""); }
    return;
  }
  for (uint32_t t = tid; t < nv; t += T) my_tail[t] = select_value(keys[t]);      // the raw log weights are read from here below
  if (tails_out) for (uint32_t t = tid; t <= Mlen; t += T) tails_out[(d * out_stride + i) * ((int64_t)Mlen + 1) + t] = select_value(keys[t]);
  const double a0 = select_value(keys[0]), aM = select_value(keys[Mlen]);
  // B = sum_{t >= M} exp(a_0 - a_t): the splits' partials in ascending order, the copies of the threshold the tail had no room for, the sorted slots from M on
  double rest = 0.0;
  {
    const double *p = parts + part_off[blockIdx.y] + i;
    for (int64_t k = 0; k < splits; ++k) rest += p[k * n];
    if (!st.inclusive) rest += (double)(st.lo + st.in - (Mlen + 1)) * exp_v8(a0 - select_value(st.thr));
  }
  double v = 0.0;
  for (uint32_t t = Mlen + tid; t < nv; t += T) v += exp_v8(a0 - select_value(keys[t]));
  const double B = rest + block_sum(v, red);
  const double Sd = (double)S, Md = (double)Mlen;
  const LooFit f = loo_gpd_fit(keys, Lj, Wj, red, Mlen, mm, a0, aM);      // (the excesses now stand where the keys stood)
  const bool raw = f.raw;
  const double khat = f.khat, sigma = f.sigma, ec = f.ec;
  double elpd = 0.0;
  if (!raw) {
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t t = tid; t < Mlen; t += T) {
      const double r = (double)(Mlen - t), lp = log1p_v8(-((r - 0.5) / Md));
      const double q = khat == 0.0 ? -sigma * lp : sigma * expm1_v8(-khat * lp) / khat;
      const double lq = log_v8(q + ec), lwt = lq > 0.0 ? 0.0 : lq;      // (a NaN stays a NaN)
      s1 += exp_v8(lwt - (a0 - my_tail[t]));
      s2 += exp_v8(lwt);
    }
    const double S1 = block_sum(s1, red), S2 = block_sum(s2, red);
    elpd = a0 + (log_v8((Sd - Md) + S1) - log_v8(B + S2));      // (the difference of the logarithms first: identical draws give a_0 itself)
  }
  if (raw) {      // no fit: the plain importance-sampling estimate, log S - log sum_s exp(-l_s) taken at a_0
    double h = 0.0;
    for (uint32_t t = tid; t < Mlen; t += T) h += exp_v8(a0 - my_tail[t]);
    elpd = a0 + (log_v8(Sd) - log_v8(B + block_sum(h, red)));
  }
  if (tid == 0) { res[0] = elpd; res[1] = khat; }
}

std::atomic<int> g_timing{0};      // the test library's switch
std::mutex g_stats_lock;
LooStats g_stats{};                // the last call's record, published once when it ends

int run_kernels(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, const WaicDataset *d_sets,
                int64_t n_max, double *d_pw, double *d_tails, LooStats &stats, size_t scratch_bytes, hipStream_t stream) {
  const bool bern = K.bern;
  int64_t cpd = C / D;      // (not const, nor cap: the args[] lists point at them)
  const int64_t S = rows * cpd, M = loo_tail_len(S);
  uint32_t cap = loo_cap(M);
  const int mm = loo_thetas(M);
  const size_t fit_lds = ((size_t)cap + kFitExtra) * 8;
  if (fit_lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(loo_fit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fit_lds);
    if (e != hipSuccess) return amwg_fail(AMWG_EHIP, "%s: a tail of %lld terms needs %zu bytes of LDS in one workgroup: %s", call, (long long)(M + 1), fit_lds, hipGetErrorString(e));
  }
  DevBuf two, two_tails, offs, state, hist, tail, parts, pending;
  if (bern) {
    HIP_TRY(two.alloc((size_t)D * 4 * 8));
    if (d_tails) {
      HIP_TRY(two_tails.alloc((size_t)D * 2 * (size_t)(M + 1) * 8));
      HIP_TRY(amwg_pointwise_fill_nan(two_tails.as<double>(), (int64_t)D * 2 * (M + 1), stream));
    }
  }
  double *out = bern ? two.as<double>() : d_pw;
  double *tails_out = d_tails ? (bern ? two_tails.as<double>() : d_tails) : nullptr;
  const int64_t out_stride = bern ? 2 : n_max;
  const PointwisePlan plan = amwg_pointwise_plan(K, sets, D, S, (size_t)cap * 8 + (size_t)kBins * 4 + sizeof(LooState), 8, scratch_bytes);
  HIP_TRY(offs.alloc((size_t)D * 16));
  HIP_TRY(hipMemcpyAsync(offs.p, plan.off.data(), (size_t)D * 16, hipMemcpyHostToDevice, stream));
  HIP_TRY(state.alloc((size_t)plan.most_obs * sizeof(LooState)));
  HIP_TRY(hist.alloc((size_t)plan.most_obs * kBins * 4));
  HIP_TRY(tail.alloc((size_t)plan.most_obs * cap * 8));
  HIP_TRY(parts.alloc((size_t)plan.most_parts * 8));
  HIP_TRY(pending.alloc(sizeof(int)));
  LooState *d_state = state.as<LooState>();
  uint32_t *d_hist = hist.as<uint32_t>();
  double *d_tail = tail.as<double>(), *d_parts = parts.as<double>();
  // a grouped call: `sets` and d_sets count groups; the walking kernels take the observations' sets and the groups in their place
  const int walk_fn = K.groups ? kPwGrouped : 0;
  const WaicDataset *obs_sets = K.groups ? K.groups->d_sets.as<WaicDataset>() : d_sets;
  const GroupSet *gsets = K.groups ? K.groups->d_gsets.as<GroupSet>() : nullptr;
  const int32_t *csr = K.groups ? K.groups->d_csr.as<int32_t>() : nullptr;
  for (const PointwiseBatch &b : plan.batches) {
    if (b.tiles == 0) continue;
    int d0 = b.d0;
    const int64_t *obs_off = offs.as<int64_t>() + d0, *part_off = offs.as<int64_t>() + D + d0;
    const dim3 walk((unsigned)b.tiles, (unsigned)b.splits, (unsigned)(b.d1 - d0));
    void *compact_args[] = {&draws, &rows, &PR, &C, &cpd, &d0, K.model_arg(), &d_sets, &obs_off, &part_off, &d_state, &d_tail, &cap, &d_parts};
    void *grouped_compact_args[] = {&draws, &rows, &PR, &C, &cpd, &d0, K.model_arg(), &obs_sets, &gsets, &csr, &obs_off, &part_off, &d_state, &d_tail, &cap, &d_parts};
    {
      Phase ph(stream, stats.timed != 0);
      int passes = 0;
      TRYB(amwg_loo_select(K, draws, rows, PR, C, cpd, d_sets, b, obs_off, d_state, d_hist, pending.as<int>(), (uint32_t)M, cap, stream, &passes));
      stats.passes = passes > stats.passes ? passes : stats.passes;
      ph.end(stats.ms_select);
    }
    {
      Phase ph(stream, stats.timed != 0);
      HIP_TRY(amwg_pointwise_go(K, walk_fn + kPwLooCompact, walk, stream, K.groups ? grouped_compact_args : compact_args));
      ph.end(stats.ms_compact);
    }
    {
      Phase ph(stream, stats.timed != 0);
      hipLaunchKernelGGL(loo_fit_kernel, dim3((unsigned)b.n_most, (unsigned)(b.d1 - d0)), dim3(fit_threads(cap)), fit_lds, stream, rows, cpd, d0, d_sets, bern ? 1 : 0, obs_off, part_off,
                         d_state, d_tail, cap, d_parts, (uint32_t)M, mm, out, out_stride, tails_out);
      HIP_TRY(hipGetLastError());
      ph.end(stats.ms_fit);
    }
  }
  if (bern) {
    HIP_TRY(amwg_pointwise_bern_expand(K, d_sets, D, two.as<double>(), d_pw, n_max, 2, stream));
    if (d_tails) HIP_TRY(amwg_pointwise_bern_expand(K, d_sets, D, two_tails.as<double>(), d_tails, n_max, M + 1, stream));
  }
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is freed on return)
  return AMWG_OK;
}

}  // namespace

int amwg_loo_select(const PointwiseLaunch &K, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, const WaicDataset *d_sets, const PointwiseBatch &b,
                    const int64_t *obs_off, LooState *d_state, uint32_t *d_hist, int *d_pending, uint32_t M, uint32_t cap, hipStream_t stream, int *passes) {
  const int bern = K.bern ? 1 : 0;
  int d0 = b.d0, pass = 0;
  const dim3 walk((unsigned)b.tiles, (unsigned)b.splits, (unsigned)(b.d1 - d0)), per_obs_grid((unsigned)((b.n_most + kThreads - 1) / kThreads), (unsigned)(b.d1 - d0));
  const int walk_fn = K.groups ? kPwGrouped : 0;
  const WaicDataset *obs_sets = K.groups ? K.groups->d_sets.as<WaicDataset>() : d_sets;
  const GroupSet *gsets = K.groups ? K.groups->d_gsets.as<GroupSet>() : nullptr;
  const int32_t *csr = K.groups ? K.groups->d_csr.as<int32_t>() : nullptr;
  void *hist_args[] = {&draws, &rows, &PR, &C, &cpd, &d0, K.model_arg(), &d_sets, &obs_off, &d_state, &d_hist, &pass};
  void *grouped_hist_args[] = {&draws, &rows, &PR, &C, &cpd, &d0, K.model_arg(), &obs_sets, &gsets, &csr, &obs_off, &d_state, &d_hist, &pass};
  hipLaunchKernelGGL(loo_init_kernel, dim3((unsigned)((b.obs + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, d_state, b.obs);
  HIP_TRY(hipGetLastError());
  *passes = 0;
  for (pass = 0; pass < kPasses; ++pass) {      // (hist_args reads `pass`)
    int waiting = 0;
    HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)b.obs * kBins * 4, stream));
    HIP_TRY(hipMemsetAsync(d_pending, 0, sizeof(int), stream));
    HIP_TRY(amwg_pointwise_go(K, walk_fn + kPwLooHist, walk, stream, K.groups ? grouped_hist_args : hist_args));
    hipLaunchKernelGGL(loo_pick_kernel, per_obs_grid, dim3(kThreads), 0, stream, d0, d_sets, bern, obs_off, d_state, d_hist, pass, M, cap, d_pending);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&waiting, d_pending, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    ++*passes;
    if (!waiting) break;
  }
  return AMWG_OK;
}

namespace {

template <int... MODEL> const void *family_fn(PointwiseModels<MODEL...>, int model, int k) {
  const void *const fn[][2] = {{reinterpret_cast<const void *>(&loo_hist_kernel<MODEL>), reinterpret_cast<const void *>(&loo_compact_kernel<MODEL>)}...};
  return fn[model - AMWG_MODEL_NORMAL][k];
}

}  // namespace

const void *amwg_loo_family_fn(int model, int k) { return family_fn(BuiltinModels{}, model, k); }

void amwg_loo_set_timing(int on) { g_timing.store(on); }
int amwg_loo_timing() { return g_timing.load(); }
void amwg_loo_publish_stats(const LooStats &stats) {
  std::lock_guard<std::mutex> hold(g_stats_lock);
  g_stats = stats;
}
LooStats amwg_loo_last_stats() {
  std::lock_guard<std::mutex> hold(g_stats_lock);
  return g_stats;
}

int amwg_loo_shape(const char *call, int64_t rows, int PR, int64_t C, int D) {
  TRYB(amwg_waic_shape(call, rows, PR, C, D));
  const int64_t S = rows * (C / D), M = loo_tail_len(S);
  if (M + 1 > kLooTailCap)
    return amwg_fail(AMWG_EINVAL, "%s: %lld draws per dataset make a tail of %lld + 1 terms, more than the %lld doubles (64 KB) of tail one workgroup sorts and fits in LDS", call, (long long)S,
                     (long long)M, (long long)kLooTailCap);
  return AMWG_OK;
}

void amwg_loo_totals(const double *pw, int64_t n, double *summary, int32_t *high) {
  double elpd = 0.0, lppd = 0.0;
  int32_t h = 0;
  for (int64_t i = 0; i < n; ++i) {
    elpd += pw[3 * i];
    lppd += pw[3 * i + 1];
    h += pw[3 * i + 2] > 0.7 ? 1 : 0;
  }
  const double centre = elpd / (double)n;
  double ss = 0.0;
  for (int64_t i = 0; i < n; ++i) { const double e = pw[3 * i] - centre; ss += e * e; }
  summary[0] = elpd;
  summary[1] = n == 1 ? (double)NAN : std::sqrt((double)n * ss / (double)(n - 1));
  summary[2] = lppd - elpd;
  summary[3] = lppd;
  if (high) *high = h;
}

int amwg_loo_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets, double *summary,
                    int32_t *high, double *pointwise, double *tails, size_t scratch_bytes, hipStream_t stream) {
  if (!draws || !sets || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_loo_shape(call, rows, PR, C, D));
  PointwiseLaunch K;
  TRYB(amwg_pointwise_family(call, model, PR, D, K));
  return amwg_loo_run(call, draws, rows, PR, C, D, K, sets, summary, high, pointwise, tails, scratch_bytes, stream);
}

int amwg_loo_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                 int32_t *high, double *pointwise, double *tails, size_t scratch_bytes, hipStream_t stream) {
  int64_t n_max = 0;
  for (int d = 0; d < D; ++d) n_max = sets[d].n_obs > n_max ? sets[d].n_obs : n_max;
  const int64_t M = loo_tail_len(rows * (C / D));
  LooStats stats{0, g_timing.load(), 0.f, 0.f, 0.f, 0.f};      // this call's own; nothing shared is written while it runs
  // lppd_i: WAIC's, which also refuses an n_obs < 0
  const size_t pairs = (size_t)D * (size_t)(n_max > 0 ? n_max : 1);
  std::vector<double> wsum((size_t)D * 4), wpw(pairs * 2), got(pairs * 2);
  {
    Phase ph(stream, stats.timed != 0);
    TRYB(amwg_waic_run(call, draws, rows, PR, C, D, K, sets, wsum.data(), nullptr, wpw.data(), nullptr, scratch_bytes, stream));
    ph.end(stats.ms_lppd);
  }
  PointwiseOut o;
  TRYB(amwg_pointwise_begin(call, sets, D, tails ? M + 1 : 0, stream, o));
  TRYB(run_kernels(call, draws, rows, PR, C, D, K, sets, o.sets.as<WaicDataset>(), n_max, o.pw.as<double>(), tails ? o.extra.as<double>() : nullptr, stats, scratch_bytes, stream));
  amwg_loo_publish_stats(stats);
  TRYB(amwg_pointwise_fetch(o, got.data(), tails));
  // the triples: (elpd_loo_i, WAIC's lppd_i, khat_i); all three NaN where either pass found the terms of (d, i) unfit
  std::vector<double> own;
  double *pw = pointwise;
  if (!pw) { own.resize(pairs * 3); pw = own.data(); }
  for (size_t k = 0; k < (size_t)D * (size_t)n_max; ++k) {
    const bool nan = std::isnan(wpw[2 * k]) || std::isnan(got[2 * k]);
    pw[3 * k] = nan ? (double)NAN : got[2 * k];
    pw[3 * k + 1] = nan ? (double)NAN : wpw[2 * k];
    pw[3 * k + 2] = nan ? (double)NAN : got[2 * k + 1];
  }
  for (int d = 0; d < D; ++d) amwg_loo_totals(pw + (size_t)d * (size_t)n_max * 3, sets[d].n_obs, summary + (size_t)d * 4, high ? high + d : nullptr);
  return AMWG_OK;
}

extern "C" int amwg_last_sample_dataset_loo(amwg_sampler *s, double *summary, int32_t *high, double *pointwise) {
  return amwg_pointwise_entry("amwg_last_sample_dataset_loo", s, summary, high, pointwise, amwg_loo_shape, amwg_loo_run);
}

extern "C" int amwg_last_sample_dataset_loo_grouped(amwg_sampler *s, const int32_t *labels, double *summary, int32_t *high, double *pointwise, int32_t *n_groups_out) {
  return amwg_pointwise_entry("amwg_last_sample_dataset_loo_grouped", s, summary, high, pointwise, amwg_loo_shape, amwg_loo_run, true, labels, n_groups_out);
}
