// amwg_loo_predictive.hip -- PSIS-LOO predictive calibration per dataset on the device from the stored draws (amwg_last_sample_dataset_loo_predictive; part of
// libamwg.so): per observation the LOO-PIT, the leave-one-out predictive mean and sd, and khat_i.  include/amwg.h states the rule, amwg_loo_predictive.h the route.
// The weight of a draw is carried from LOO's tail to the predictive functionals without the S x n weights ever standing in memory.  The accumulations are bounded,
// not pinned, and deterministic: the only atomics are on integers.  Not a source of the step kernels (tools/build_id.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "amwg_host.h"
#include "amwg_loo_fit.h"
#include "amwg_loo_predictive.h"
#include "amwg_predictive.h"
#include "amwg_predictive_eval.h"
#include "amwg_sampler.h"
#include "amwg_select.h"
#include "amwg_terms.h"

using namespace amwg;

namespace {

constexpr int kSums = 6;      // sum w, sum w F, sum w Fm, sum w mean, sum w var, sum w (mean - c)^2
struct Six { double v[kSums]; };

__device__ __forceinline__ void add_six(double (&a)[kSums], double w, const Eval &e, double c) {
  const double dm = e.mean - c;
  a[0] += w; a[1] += w * e.F; a[2] += w * e.Fm; a[3] += w * e.mean; a[4] += w * e.var; a[5] += w * (dm * dm);
}

// observation i as the predictive evaluation reads it; the Bernoulli family: i = 0 stands for x = 1 and i = 1 for x = 0, as in Family<AMWG_MODEL_BETA_BERN>
template <int MODEL> __device__ __forceinline__ typename Pred<MODEL>::Obs pred_obs(const WaicModel &M, const WaicDataset &ds, int64_t i) {
  if constexpr (MODEL == AMWG_MODEL_BETA_BERN) return typename Pred<MODEL>::Obs{i == 0 ? 1 : 0, 0};
  else return Pred<MODEL>::load_obs(M, ds, i);
}
template <int MODEL> __device__ __forceinline__ typename Pred<MODEL>::Draw pred_draw(const double *draws, int PR, int64_t C, int64_t cpd, int d, int64_t s, const WaicModel &M) {
  const int64_t row = s / cpd, base = row * PR * C + (int64_t)d * cpd + (s - row * cpd);
  return Pred<MODEL>::make_draw(draws + base, C, M, base);
}

// phase 2.  tail[(obs_off[z] + i) * cap + slot] and tail_ix[...]: the terms the tail takes and their draws; parts[(part_off[z] + split * n + i) * 2 + (0 | 1)]: the
// weighted sums of the terms above the threshold | the class record of the threshold's own key
template <int MODEL>
__global__ void __launch_bounds__(kThreads) loo_pred_compact_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                    const WaicDataset *__restrict__ sets, const int64_t *__restrict__ obs_off, const int64_t *__restrict__ part_off,
                                                                    LooState *__restrict__ state, double *__restrict__ tail, uint32_t *__restrict__ tail_ix, uint32_t cap,
                                                                    Six *__restrict__ parts) {
  typedef Family<MODEL> F;
  typedef Pred<MODEL> P;
  constexpr int R = P::R;
  static_assert(stage_len<F>() == kStage && sizeof(typename P::Draw) * kStage <= (size_t)kStageBytes, "256 draws are staged in both forms");
  __shared__ typename F::Draw stage[kStage];
  __shared__ typename P::Draw pstage[kStage];
  __shared__ double wave_s[kWaves - 1][2 * kSums][kTile];
  const int d = d0 + (int)blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WaicDataset ds = sets[d];
  const int64_t n = F::n_eff(ds), S = rows * cpd, splits = waic_splits(S, n);
  if ((int64_t)blockIdx.x * kTile >= n || (int64_t)blockIdx.y >= splits) return;      // (uniform over the workgroup)
  const int64_t s_begin = split_begin(S, splits, blockIdx.y), s_end = split_begin(S, splits, (int64_t)blockIdx.y + 1);
  const int64_t i = (int64_t)blockIdx.x * kTile + lane;
  const bool active = i < n;
  const int64_t ii = active ? i : n - 1, o_at = obs_off[blockIdx.z] + ii;
  const LooState st = state[o_at];
  const double a0 = select_value(st.minkey);
  const typename F::Obs fo = F::load_obs(M, ds, ii);
  const typename P::Obs po = pred_obs<MODEL>(M, ds, ii);
  const double c = P::eval(po, pred_draw<MODEL>(draws, PR, C, cpd, d, 0, M), ii, draws, C).mean;      // the shift: the observation's mean under draw 0
  double *my_tail = tail + o_at * cap;
  uint32_t *my_ix = tail_ix + o_at * cap;
  double sw[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t s0 = s_begin; s0 < s_end; s0 += kStage) {
    const int L = (int)(s_end - s0 < kStage ? s_end - s0 : kStage);
    __syncthreads();
    if (tid < L) {
      stage[tid] = draw_at<F>(draws, PR, C, cpd, d, s0 + tid, M, ds);
      pstage[tid] = pred_draw<MODEL>(draws, PR, C, cpd, d, s0 + tid, M);
    }
    __syncthreads();
    for (int jb = wave; jb < L; jb += kWaves * R) {
      double l[R];
      Eval e[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {      // R independent terms and evaluations; a block that reaches past the run evaluates draw jb again, dropped below
        const int at = jb + kWaves * r < L ? jb + kWaves * r : jb;
        l[r] = F::term(M, fo, stage[at], ii, draws, C);
        e[r] = P::eval(po, pstage[at], ii, draws, C);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (jb + kWaves * r >= L) break;
        const uint64_t key = select_key(l[r]);
        const bool take = st.inclusive ? key <= st.thr : key < st.thr;
        if (take) {
          if (active) {
            const uint32_t at = atomicAdd(&state[o_at].cursor, 1u);
            if (at < cap) { my_tail[at] = l[r]; my_ix[at] = (uint32_t)(s0 + jb + kWaves * r); }      // (the select's counts say at < cap; the comparison keeps a wrong count inside the buffers)
          }
        } else if (key > st.thr) {
          add_six(sw, waic_exp(a0 - l[r]), e[r], c);
        } else {
          add_six(sc, 1.0, e[r], c);
        }
      }
    }
  }
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) { wave_s[wave - 1][k][lane] = sw[k]; wave_s[wave - 1][kSums + k][lane] = sc[k]; }
  }
  __syncthreads();
  if (wave != 0 || !active) return;
#pragma unroll
  for (int w = 1; w < kWaves; ++w)
#pragma unroll
    for (int k = 0; k < kSums; ++k) { sw[k] += wave_s[w - 1][k][lane]; sc[k] += wave_s[w - 1][kSums + k][lane]; }
  Six *out = parts + (part_off[blockIdx.z] + (int64_t)blockIdx.y * n + i) * 2;
#pragma unroll
  for (int k = 0; k < kSums; ++k) { out[0].v[k] = sw[k]; out[1].v[k] = sc[k]; }
}

// phase 3.  One workgroup per observation, fit_threads(cap) threads.  out[(d * out_stride + i) * 5 ...] = pit_hi, pit_lo, pred_mean, pred_sd, khat_i.
// Dynamic LDS: (cap + kFitExtra) * 8 bytes as loo_fit_kernel, then cap * 4 of draw indices.
template <int MODEL>
__global__ void __launch_bounds__(kThreads) loo_pred_fit_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                const WaicDataset *__restrict__ sets, const int64_t *__restrict__ obs_off, const int64_t *__restrict__ part_off,
                                                                const LooState *__restrict__ state, double *__restrict__ tail, const uint32_t *__restrict__ tail_ix, uint32_t cap,
                                                                const Six *__restrict__ parts, uint32_t Mlen, int mm, double *__restrict__ out, int64_t out_stride) {
  typedef Family<MODEL> F;
  typedef Pred<MODEL> P;
  extern __shared__ uint64_t lds[];
  uint64_t *keys = lds;
  double *W = reinterpret_cast<double *>(lds);      // the weights take the place of the excesses, which took the place of the keys
  double *Lj = reinterpret_cast<double *>(lds + cap), *Wj = Lj + kMaxTheta, *red = Wj + kMaxTheta;
  uint32_t *ix = reinterpret_cast<uint32_t *>(lds + cap + kFitExtra);
  const int d = d0 + (int)blockIdx.y, tid = threadIdx.x;
  const uint32_t T = blockDim.x;
  const WaicDataset ds = sets[d];
  const int64_t n = F::n_eff(ds), S = rows * cpd, splits = waic_splits(S, n), i = blockIdx.x;
  if (i >= n) return;      // (uniform over the workgroup)
  const int64_t o_at = obs_off[blockIdx.y] + i;
  const LooState st = state[o_at];
  double *my_tail = tail + o_at * cap;
  const uint32_t *my_ix = tail_ix + o_at * cap;
  const uint32_t taken = st.cursor < cap ? st.cursor : cap;      // the slots that hold terms of draws; ties that overflow: the keys below the threshold
  const uint32_t nv = st.inclusive ? taken : Mlen + 1;           // ... and with the copies of the threshold that stand for its class up to rank M
  for (uint32_t t = tid; t < cap; t += T) {
    keys[t] = t < taken ? select_key(my_tail[t]) : (!st.inclusive && t <= Mlen ? st.thr : kMaxKey);
    ix[t] = t < taken ? my_ix[t] : 0xffffffffu;
  }
  __syncthreads();
  loo_sort<true>(keys, ix, cap);
  double *res = out + (d * out_stride + i) * 5;
  if (st.bad) {      // a NaN or an infinity among the terms
    if (tid == 0) for (int k = 0; k < 5; ++k) res[k] = __builtin_nan("");
    return;
  }
  for (uint32_t t = tid; t < nv; t += T) my_tail[t] = select_value(keys[t]);
  const double a0 = select_value(keys[0]), aM = select_value(keys[Mlen]), Md = (double)Mlen;
  const LooFit f = loo_gpd_fit(keys, Lj, Wj, red, Mlen, mm, a0, aM);
  __syncthreads();
  // the weight of every sorted slot.  Below M on the smoothed route: LOO's lw~_r, r = M - t, the expression of loo_fit_kernel
  for (uint32_t t = tid; t < nv; t += T) {
    double w;
    if (!f.raw && t < Mlen) {
      const double r = (double)(Mlen - t), lp = log1p_v8(-((r - 0.5) / Md));
      const double q = f.khat == 0.0 ? -f.sigma * lp : f.sigma * expm1_v8(-f.khat * lp) / f.khat;
      const double lq = log_v8(q + f.ec), lwt = lq > 0.0 ? 0.0 : lq;      // (a NaN stays a NaN)
      w = exp_v8(lwt);
    } else {
      w = exp_v8(a0 - my_tail[t]);      // (written above by this thread)
    }
    W[t] = w;
  }
  __syncthreads();      // (the sorted terms in my_tail are the workgroup's own writes: visible behind the barrier)
  // the class means: runs of equal keys among the terms of draws that begin below M; the threshold's overflowing class is weighted at the end
  if (!f.raw) {
    const uint32_t heads = taken < Mlen ? taken : Mlen;
    for (uint32_t t = tid; t < heads; t += T) {
      const uint64_t k = select_key(my_tail[t]);
      if (t > 0 && select_key(my_tail[t - 1]) == k) continue;
      uint32_t e = t + 1;
      double sum = W[t];
      while (e < taken && select_key(my_tail[e]) == k) { if (e < Mlen) sum += W[e]; ++e; }
      if (e - t == 1) continue;
      if (e > Mlen) sum += (double)(e - Mlen) * exp_v8(a0 - select_value(k));
      const double w = sum / (double)(e - t);
      for (uint32_t u = t; u < e; ++u) W[u] = w;
    }
  }
  __syncthreads();
  // the functionals of the buffered draws from their indices, then the splits' records: thread k takes the slots and the splits k, k + T, ...
  const typename P::Obs po = pred_obs<MODEL>(M, ds, i);
  const double c = P::eval(po, pred_draw<MODEL>(draws, PR, C, cpd, d, 0, M), i, draws, C).mean;
  double s[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, cl[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint32_t t = tid; t < taken; t += T) {
    const int64_t at = ix[t];
    if (at >= S) continue;      // (never: a slot below `taken` holds a draw)
    add_six(s, W[t], P::eval(po, pred_draw<MODEL>(draws, PR, C, cpd, d, at, M), i, draws, C), c);
  }
  const Six *p = parts + (part_off[blockIdx.y] + i) * 2;
  for (int64_t k = tid; k < splits; k += T) {
#pragma unroll
    for (int q = 0; q < kSums; ++q) { s[q] += p[k * n * 2].v[q]; cl[q] += p[k * n * 2 + 1].v[q]; }
  }
#pragma unroll
  for (int q = 0; q < kSums; ++q) s[q] = block_sum(s[q], red);
  if (!st.inclusive) {      // (uniform over the workgroup)
#pragma unroll
    for (int q = 0; q < kSums; ++q) cl[q] = block_sum(cl[q], red);
  }
  if (tid != 0) return;
  if (!st.inclusive) {      // the threshold's class: m_c slots below M (taken ... M - 1), st.in members in all
    const double thr_w = exp_v8(a0 - select_value(st.thr));
    double w = thr_w;
    if (!f.raw && taken < Mlen) {
      double sum = 0.0;
      for (uint32_t t = taken; t < Mlen; ++t) sum += W[t];
      w = (sum + (double)(st.in - (Mlen - taken)) * thr_w) / (double)st.in;
    }
#pragma unroll
    for (int q = 0; q < kSums; ++q) s[q] += w * cl[q];
  }
  const double hi = s[1] / s[0], lo = s[2] / s[0], mean = s[3] / s[0], dm = mean - c, var = (s[4] + s[5]) / s[0] - dm * dm;
  const double sd = __builtin_sqrt(var < 0.0 ? 0.0 : var);      // (a NaN stays a NaN)
  const bool finite = __builtin_fabs(hi) < kInf && __builtin_fabs(lo) < kInf && __builtin_fabs(mean) < kInf && __builtin_fabs(sd) < kInf;
  const double r[5] = {hi, lo, mean, sd, f.khat};
#pragma unroll
  for (int k = 0; k < 5; ++k) res[k] = finite ? r[k] : __builtin_nan("");
}

// y[d * y_stride + j] = observation j as the finish on the host reads it
template <int MODEL>
__global__ void __launch_bounds__(kThreads) loo_pred_y_kernel(const WaicModel M, const WaicDataset *__restrict__ sets, double *__restrict__ y, int64_t y_stride) {
  const int d = blockIdx.y;
  const WaicDataset ds = sets[d];
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j < ds.n_obs) y[d * y_stride + j] = Pred<MODEL>::y_of(Pred<MODEL>::load_obs(M, ds, j));
}

template <int... MODEL> const void *kernel_fn(PointwiseModels<MODEL...>, int model, int k) {
  const void *const fn[][3] = {{reinterpret_cast<const void *>(&loo_pred_compact_kernel<MODEL>), reinterpret_cast<const void *>(&loo_pred_fit_kernel<MODEL>),
                                reinterpret_cast<const void *>(&loo_pred_y_kernel<MODEL>)}...};
  return fn[model - AMWG_MODEL_NORMAL][k];
}

}  // namespace

int amwg_loo_predictive_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets,
                            double *summary, int32_t *high, double *pointwise, double *, size_t scratch_bytes, hipStream_t stream) {
  if (!K.builtin || K.groups) return amwg_fail(AMWG_EINVAL, "%s: built-in families over observations only", call);
  WaicModel M = K.family;
  const bool bern = K.bern, timed = amwg_loo_timing() != 0;
  int64_t cpd = C / D, n_max = 0;      // (not const, nor cap: the args[] lists point at them)
  for (int d = 0; d < D; ++d) {
    if (sets[d].n_obs < 0) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: n_obs < 0", call, d);
    n_max = sets[d].n_obs > n_max ? sets[d].n_obs : n_max;
  }
  const int64_t S = rows * cpd, Mlen = loo_tail_len(S);
  uint32_t cap = loo_cap(Mlen), Mu = (uint32_t)Mlen;
  int mm = loo_thetas(Mlen);
  const void *compact = kernel_fn(BuiltinModels{}, M.model, 0), *fit = kernel_fn(BuiltinModels{}, M.model, 1), *yfn = kernel_fn(BuiltinModels{}, M.model, 2);
  const size_t fit_lds = ((size_t)cap + kFitExtra) * 8 + (size_t)cap * 4;
  if (fit_lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fit_lds);
    if (e != hipSuccess) return amwg_fail(AMWG_EHIP, "%s: a tail of %lld terms needs %zu bytes of LDS in one workgroup: %s", call, (long long)(Mlen + 1), fit_lds, hipGetErrorString(e));
  }
  // ---- the outputs on the device, filled with NaN
  const size_t obs_count = (size_t)D * (size_t)n_max;
  DevBuf d_sets_buf, d_pw, d_y, two, offs, state, hist, tail, tail_ix, parts, pending;
  HIP_TRY(d_sets_buf.alloc((size_t)D * sizeof(WaicDataset)));
  HIP_TRY(hipMemcpyAsync(d_sets_buf.p, sets, (size_t)D * sizeof(WaicDataset), hipMemcpyHostToDevice, stream));
  const WaicDataset *d_sets = d_sets_buf.as<WaicDataset>();
  HIP_TRY(d_pw.alloc((obs_count ? obs_count : 1) * 40));
  HIP_TRY(amwg_pointwise_fill_nan(d_pw.as<double>(), (int64_t)obs_count * 5, stream));
  HIP_TRY(d_y.alloc((obs_count ? obs_count : 1) * 8));
  HIP_TRY(amwg_pointwise_fill_nan(d_y.as<double>(), (int64_t)obs_count, stream));
  if (bern) {
    HIP_TRY(two.alloc((size_t)D * 2 * 40));
    HIP_TRY(amwg_pointwise_fill_nan(two.as<double>(), (int64_t)D * 10, stream));
  }
  double *out = bern ? two.as<double>() : d_pw.as<double>(), *d_y_out = d_y.as<double>();
  int64_t out_stride = bern ? 2 : n_max;
  // ---- the scratch of the largest batch under the budget
  const PointwisePlan plan = amwg_pointwise_plan(K, sets, D, S, (size_t)cap * 12 + (size_t)kBins * 4 + sizeof(LooState), 2 * sizeof(Six), scratch_bytes);
  HIP_TRY(offs.alloc((size_t)D * 16));
  HIP_TRY(hipMemcpyAsync(offs.p, plan.off.data(), (size_t)D * 16, hipMemcpyHostToDevice, stream));
  HIP_TRY(state.alloc((size_t)plan.most_obs * sizeof(LooState)));
  HIP_TRY(hist.alloc((size_t)plan.most_obs * kBins * 4));
  HIP_TRY(tail.alloc((size_t)plan.most_obs * cap * 8));
  HIP_TRY(tail_ix.alloc((size_t)plan.most_obs * cap * 4));
  HIP_TRY(parts.alloc((size_t)plan.most_parts * 2 * sizeof(Six)));
  HIP_TRY(pending.alloc(sizeof(int)));
  LooState *d_state = state.as<LooState>();
  double *d_tail = tail.as<double>();
  uint32_t *d_ix = tail_ix.as<uint32_t>();
  Six *d_parts = parts.as<Six>();
  LooStats stats{0, timed ? 1 : 0, 0.f, 0.f, 0.f, 0.f};      // this call's own, published once when it ends (amwg_loo.h)
  for (const PointwiseBatch &b : plan.batches) {
    if (b.tiles == 0) continue;
    int d0 = b.d0, passes = 0;
    const int64_t *obs_off = offs.as<int64_t>() + d0, *part_off = offs.as<int64_t>() + D + d0;
    {
      Phase ph(stream, timed);
      TRYB(amwg_loo_select(K, draws, rows, PR, C, cpd, d_sets, b, obs_off, d_state, hist.as<uint32_t>(), pending.as<int>(), Mu, cap, stream, &passes));
      stats.passes = passes > stats.passes ? passes : stats.passes;
      ph.end(stats.ms_select);
    }
    {
      Phase ph(stream, timed);
      void *args[] = {&draws, &rows, &PR, &C, &cpd, &d0, &M, &d_sets, &obs_off, &part_off, &d_state, &d_tail, &d_ix, &cap, &d_parts};
      (void)hipLaunchKernel(compact, dim3((unsigned)b.tiles, (unsigned)b.splits, (unsigned)(b.d1 - d0)), dim3(kThreads), args, 0, stream);
      HIP_TRY(hipGetLastError());
      ph.end(stats.ms_compact);
    }
    {
      Phase ph(stream, timed);
      void *args[] = {&draws, &rows, &PR, &C, &cpd, &d0, &M, &d_sets, &obs_off, &part_off, &d_state, &d_tail, &d_ix, &cap, &d_parts, &Mu, &mm, &out, &out_stride};
      (void)hipLaunchKernel(fit, dim3((unsigned)b.n_most, (unsigned)(b.d1 - d0)), dim3(fit_threads(cap)), args, fit_lds, stream);
      HIP_TRY(hipGetLastError());
      ph.end(stats.ms_fit);
    }
  }
  if (bern) HIP_TRY(amwg_pointwise_bern_expand(K, d_sets, D, two.as<double>(), d_pw.as<double>(), n_max, 5, stream));
  if (obs_count) {
    void *args[] = {&M, &d_sets, &d_y_out, &n_max};
    (void)hipLaunchKernel(yfn, dim3((unsigned)((n_max + kThreads - 1) / kThreads), (unsigned)D), dim3(kThreads), args, 0, stream);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is freed on return)
  amwg_loo_publish_stats(stats);
  // ---- the finish: the predictive call's, over the first four values, and the count of high khat
  std::vector<double> own, y(obs_count ? obs_count : 1), four((size_t)(n_max ? n_max : 1) * 4);
  double *pw = pointwise;
  if (!pw) { own.resize(obs_count ? obs_count * 5 : 1); pw = own.data(); }
  if (obs_count) {
    HIP_TRY(hipMemcpy(pw, d_pw.p, obs_count * 40, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(y.data(), d_y.p, obs_count * 8, hipMemcpyDeviceToHost));
  }
  for (int d = 0; d < D; ++d) {
    const double *row = pw + (size_t)d * (size_t)n_max * 5;
    int32_t h = 0;
    for (int64_t j = 0; j < sets[d].n_obs; ++j) {
      for (int k = 0; k < 4; ++k) four[(size_t)j * 4 + k] = row[j * 5 + k];
      h += row[j * 5 + 4] > 0.7 ? 1 : 0;
    }
    amwg_predictive_totals(four.data(), y.data() + (size_t)d * (size_t)n_max, sets[d].n_obs, summary + (size_t)d * 4);
    if (high) high[d] = h;
  }
  return AMWG_OK;
}

int amwg_loo_predictive_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &model, const WaicDataset *sets,
                               double *summary, int32_t *high, double *pointwise, size_t scratch_bytes, hipStream_t stream) {
  if (!draws || !sets || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_loo_shape(call, rows, PR, C, D));
  PointwiseLaunch K;
  TRYB(amwg_pointwise_family(call, model, PR, D, K));
  return amwg_loo_predictive_run(call, draws, rows, PR, C, D, K, sets, summary, high, pointwise, nullptr, scratch_bytes, stream);
}

extern "C" int amwg_last_sample_dataset_loo_predictive(amwg_sampler *s, double *summary, int32_t *high, double *pointwise) {
  static const char *call = "amwg_last_sample_dataset_loo_predictive";
  if (!s || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (s->user) return amwg_fail(AMWG_EINVAL, "%s: the predictive distribution of a closure is not known to the library; built-in families only", call);
  return amwg_pointwise_entry(call, s, summary, high, pointwise, amwg_loo_shape, amwg_loo_predictive_run);
}
