// amwg_loo.hip -- PSIS-LOO per dataset on the device from the stored draws (amwg_last_sample_dataset_loo; part of libamwg.so).  include/amwg.h states the rule,
// amwg_loo.h the route: a radix select over the recomputed terms finds each observation's M + 1 smallest, one more pass compacts them and sums the rest, a workgroup
// per observation sorts the tail in LDS, fits the generalised Pareto and forms the smoothed sum.  The terms are WAIC's (amwg_terms.h), bit for bit; the excesses are
// pinned to the bit (exp_v8 of differences of sorted terms); the accumulations are bounded, not pinned, and deterministic: the only atomics are on integers.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <vector>

#include "amwg_dataset.h"
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_loo.h"
#include "amwg_sampler.h"
#include "amwg_select.h"
#include "amwg_terms.h"

using namespace amwg;

namespace {

constexpr int kMaxTheta = 128;                                    // 30 + floor(sqrt(M)) <= 120 for M < kLooTailCap
constexpr int kFitExtra = 2 * kMaxTheta + 16;                     // doubles of LDS of the fit beside the tail: L_j, w_j, the wavefronts' partial sums
__global__ void __launch_bounds__(kThreads) loo_init_kernel(LooState *state, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < count) state[k] = LooState{0, 0, kMaxKey, 0, 0, 0, 0, 0, 0};
}

__global__ void __launch_bounds__(kThreads) loo_fill_nan_kernel(double *out, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < count) out[k] = __builtin_nan("");
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

// the sum of v over the workgroup's threads (one wavefront, or four), the same double in every thread: a butterfly over the lanes, then the wavefronts in the
// order 0, 1, 2, 3
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return blockDim.x == 64 ? red[0] : ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One workgroup per observation -- 256 threads, or one wavefront for a tail of at most kFitSmall slots (fit_threads) --: the tail sorted in LDS, the fit, the smoothed sum.  out[(d * out_stride + i) * 2 + (0 | 1)] = elpd_loo_i | khat_i; the sorted
// tail's first M + 1 go to tails_out[(d * out_stride + i) * (M + 1) + t] when asked for.  Dynamic LDS: (cap + kFitExtra) * 8 bytes.
__global__ void __launch_bounds__(kThreads) loo_fit_kernel(int64_t rows, int64_t cpd, int d0, const WaicDataset *__restrict__ sets, int bern, const int64_t *__restrict__ obs_off,
                                                           const int64_t *__restrict__ part_off, const LooState *__restrict__ state, double *__restrict__ tail, uint32_t cap,
                                                           const double *__restrict__ parts, uint32_t Mlen, int mm, double *__restrict__ out, int64_t out_stride,
                                                           double *__restrict__ tails_out) {
  extern __shared__ uint64_t lds[];
  uint64_t *keys = lds;
  double *X = reinterpret_cast<double *>(lds);      // the excesses take the place of the keys: x_r at X[M - r]
  double *Lj = reinterpret_cast<double *>(lds + cap), *Wj = Lj + kMaxTheta, *red = Wj + kMaxTheta;
  const int d = d0 + (int)blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t T = blockDim.x;
  const int waves = (int)(T >> 6);
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
  for (uint32_t kk = 2; kk <= cap; kk <<= 1) {
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (cap >> 1); t += T) {
        const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = a | j;
        const bool up = (a & kk) == 0;
        const uint64_t x = keys[a], y = keys[l];
        if ((x > y) == up) { keys[a] = y; keys[l] = x; }
      }
      __syncthreads();
    }
  }
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
  bool raw = Mlen < 5;
  double khat = kInf, elpd = 0.0;
  if (!raw) {
    const double ec = exp_v8(a0 - aM);
    __syncthreads();
    for (uint32_t t = tid; t < Mlen; t += T) X[t] = exp_v8(a0 - select_value(keys[t])) - ec;      // (slot t is read and written by the same thread)
    __syncthreads();
    const double xM = X[0], xs = X[Mlen - (Mlen + 2) / 4];      // x_M; x* = x_{floor(M / 4 + 0.5)}
    raw = !(xs > 0.0) || !(xM > 0.0);
    if (!raw) {
      const double mmd = (double)mm;
      for (int j = wave + 1; j <= mm; j += waves) {
        const double theta = 1.0 / xM + (1.0 - ::sqrt(mmd / ((double)j - 0.5))) / (3.0 * xs);
        double s = 0.0;
        for (uint32_t t = lane; t < Mlen; t += 64) s += log1p_v8(-theta * X[t]);
        const double k = wave_sum(s) / Md;
        if (lane == 0) Lj[j - 1] = Md * (log_v8(-theta / k) - k - 1.0);
      }
      __syncthreads();
      if (tid < mm) {
        double z = 0.0;
        for (int q = 0; q < mm; ++q) z += exp_v8(Lj[q] - Lj[tid]);
        Wj[tid] = 1.0 / z;
      }
      __syncthreads();
      double th = 0.0;
      for (int j = 1; j <= mm; ++j) th += (1.0 / xM + (1.0 - ::sqrt(mmd / ((double)j - 0.5))) / (3.0 * xs)) * Wj[j - 1];
      double s = 0.0;
      for (uint32_t t = tid; t < Mlen; t += T) s += log1p_v8(-th * X[t]);
      const double kp = block_sum(s, red) / Md, sigma = -kp / th;
      khat = (Md * kp + 5.0) / (Md + 10.0);
      raw = !(__builtin_fabs(khat) < kInf);
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
    }
  }
  if (raw) {      // no fit: the plain importance-sampling estimate, log S - log sum_s exp(-l_s) taken at a_0
    double h = 0.0;
    for (uint32_t t = tid; t < Mlen; t += T) h += exp_v8(a0 - my_tail[t]);
    elpd = a0 + (log_v8(Sd) - log_v8(B + block_sum(h, red)));
    khat = kInf;
  }
  if (tid == 0) { res[0] = elpd; res[1] = khat; }
}

// the Bernoulli family: observation i takes the values of its x (two[d][0] for x = 1, two[d][1] for x = 0), `width` doubles each; an invalid x_i: NaN
__global__ void __launch_bounds__(kThreads) loo_bern_expand_kernel(const WaicModel M, const WaicDataset *__restrict__ sets, const double *__restrict__ two, double *__restrict__ out,
                                                                   int64_t n_max, int64_t width) {
  const int d = blockIdx.y;
  const WaicDataset ds = sets[d];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= ds.n_obs) return;
  const bool invalid = M.invalid && M.invalid[ds.off_xb + i];
  const int k = M.xb[ds.off_xb + i] ? 0 : 1;
  for (int64_t t = 0; t < width; ++t) out[(d * n_max + i) * width + t] = invalid ? __builtin_nan("") : two[(d * 2 + k) * width + t];
}

size_t g_budget = kLooScratchBytes;
std::atomic<int> g_timing{0};      // the test library's switch
std::mutex g_stats_lock;
LooStats g_stats{};                // the last call's record, published once when it ends

struct Phase {      // events around a phase when timing is on
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t stream;
  Phase(hipStream_t s, bool timed) : stream(s) { if (timed) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventRecord(e0, stream); } }
  void end(float &into) {
    if (!e0) return;
    float ms = 0.f;
    (void)hipEventRecord(e1, stream);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    into += ms;
  }
  ~Phase() { if (e0) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); } }
};

constexpr uint32_t kFitSmall = 128;      // up to this many slots (S <= 1 800 or so) one wavefront sorts and fits: the network's compare loop has 64 pairs at most
inline unsigned fit_threads(uint32_t cap) { return cap <= kFitSmall ? 64u : (unsigned)kThreads; }
inline uint32_t loo_cap(int64_t M) {
  uint32_t c = 64;
  while ((int64_t)c < M + 1) c <<= 1;
  return c;
}
inline int loo_thetas(int64_t M) { return 30 + (int)(loo_isqrt_up(M + 1) - 1); }      // 30 + floor(sqrt(M)): the largest r with r * r <= M is isqrt_up(M + 1) - 1

int run_kernels(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, const WaicDataset *d_sets,
                int64_t n_max, double *d_pw, double *d_tails, LooStats &stats, hipStream_t stream) {
  const bool bern = K.bern;
  const int64_t cpd = C / D, S = rows * cpd, M = loo_tail_len(S);
  const uint32_t cap = loo_cap(M);
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
      const int64_t count = (int64_t)D * 2 * (M + 1);
      HIP_TRY(two_tails.alloc((size_t)count * 8));
      hipLaunchKernelGGL(loo_fill_nan_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, two_tails.as<double>(), count);
      HIP_TRY(hipGetLastError());
    }
  }
  double *out = bern ? two.as<double>() : d_pw;
  double *tails_out = d_tails ? (bern ? two_tails.as<double>() : d_tails) : nullptr;
  const int64_t out_stride = bern ? 2 : n_max;
  // the batches: consecutive datasets whose scratch fits the budget together (a dataset beyond it runs alone)
  const size_t per_obs = (size_t)cap * 8 + (size_t)kBins * 4 + sizeof(LooState);
  std::vector<int64_t> n_eff((size_t)D), off((size_t)D * 2);      // off[d]: observations before d in its batch; off[D + d]: partials before it
  std::vector<int> batch_end;
  int64_t most_obs = 0, most_parts = 0;
  {
    size_t in_batch = 0;
    int64_t obs = 0, prt = 0;
    for (int d = 0; d < D; ++d) {
      const int64_t n = bern ? (sets[d].n_obs > 0 ? 2 : 0) : sets[d].n_obs;
      n_eff[(size_t)d] = n;
      const int64_t np = waic_splits(S, n) * n;
      const size_t bytes = (size_t)n * per_obs + (size_t)np * 8;
      if (in_batch && in_batch + bytes > g_budget) { batch_end.push_back(d); in_batch = 0; obs = 0; prt = 0; }
      off[(size_t)d] = obs; off[(size_t)D + (size_t)d] = prt;
      in_batch += bytes; obs += n; prt += np;
      most_obs = obs > most_obs ? obs : most_obs; most_parts = prt > most_parts ? prt : most_parts;
    }
    batch_end.push_back(D);
  }
  HIP_TRY(offs.alloc((size_t)D * 16));
  HIP_TRY(hipMemcpyAsync(offs.p, off.data(), (size_t)D * 16, hipMemcpyHostToDevice, stream));
  HIP_TRY(state.alloc((size_t)most_obs * sizeof(LooState)));
  HIP_TRY(hist.alloc((size_t)most_obs * kBins * 4));
  HIP_TRY(tail.alloc((size_t)most_obs * cap * 8));
  HIP_TRY(parts.alloc((size_t)most_parts * 8));
  HIP_TRY(pending.alloc(sizeof(int)));
  const int64_t *obs_off = offs.as<int64_t>(), *part_off = offs.as<int64_t>() + D;
  int d0 = 0;
  for (const int d1 : batch_end) {
    int64_t tiles = 0, splits = 0, n_most = 0, obs = 0;
    for (int d = d0; d < d1; ++d) {
      const int64_t n = n_eff[(size_t)d], t = (n + kTile - 1) / kTile, sp = waic_splits(S, n);
      tiles = t > tiles ? t : tiles; splits = sp > splits ? sp : splits; n_most = n > n_most ? n : n_most; obs += n;
    }
    if (tiles > 0) {
      const dim3 walk((unsigned)tiles, (unsigned)splits, (unsigned)(d1 - d0)), per_obs_grid((unsigned)((n_most + kThreads - 1) / kThreads), (unsigned)(d1 - d0));
      hipLaunchKernelGGL(loo_init_kernel, dim3((unsigned)((obs + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, state.as<LooState>(), obs);
      HIP_TRY(hipGetLastError());
      {
        Phase ph(stream, stats.timed != 0);
        int passes = 0;
        for (int pass = 0; pass < kPasses; ++pass) {
          int waiting = 0;
          HIP_TRY(hipMemsetAsync(hist.p, 0, (size_t)obs * kBins * 4, stream));
          HIP_TRY(hipMemsetAsync(pending.p, 0, sizeof(int), stream));
          HIP_TRY(K.loo_hist(walk, stream, draws, rows, PR, C, cpd, d0, d_sets, obs_off + d0, state.as<LooState>(), hist.as<uint32_t>(), pass));
          hipLaunchKernelGGL(loo_pick_kernel, per_obs_grid, dim3(kThreads), 0, stream, d0, d_sets, bern ? 1 : 0, obs_off + d0, state.as<LooState>(), hist.as<uint32_t>(), pass,
                             (uint32_t)M, cap, pending.as<int>());
          HIP_TRY(hipGetLastError());
          HIP_TRY(hipMemcpyAsync(&waiting, pending.p, sizeof(int), hipMemcpyDeviceToHost, stream));
          HIP_TRY(hipStreamSynchronize(stream));
          ++passes;
          if (!waiting) break;
        }
        stats.passes = passes > stats.passes ? passes : stats.passes;
        ph.end(stats.ms_select);
      }
      {
        Phase ph(stream, stats.timed != 0);
        HIP_TRY(K.loo_compact(walk, stream, draws, rows, PR, C, cpd, d0, d_sets, obs_off + d0, part_off + d0, state.as<LooState>(), tail.as<double>(), cap, parts.as<double>()));
        ph.end(stats.ms_compact);
      }
      {
        Phase ph(stream, stats.timed != 0);
        hipLaunchKernelGGL(loo_fit_kernel, dim3((unsigned)n_most, (unsigned)(d1 - d0)), dim3(fit_threads(cap)), fit_lds, stream, rows, cpd, d0, d_sets, bern ? 1 : 0, obs_off + d0,
                           part_off + d0, state.as<LooState>(), tail.as<double>(), cap, parts.as<double>(), (uint32_t)M, mm, out, out_stride, tails_out);
        HIP_TRY(hipGetLastError());
        ph.end(stats.ms_fit);
      }
    }
    d0 = d1;
  }
  if (bern) {
    const dim3 grid((unsigned)((n_max + kThreads - 1) / kThreads), (unsigned)D);
    hipLaunchKernelGGL(loo_bern_expand_kernel, grid, dim3(kThreads), 0, stream, *K.family, d_sets, two.as<double>(), d_pw, n_max, (int64_t)2);
    HIP_TRY(hipGetLastError());
    if (d_tails) {
      hipLaunchKernelGGL(loo_bern_expand_kernel, grid, dim3(kThreads), 0, stream, *K.family, d_sets, two_tails.as<double>(), d_tails, n_max, M + 1);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is freed on return)
  (void)call;
  return AMWG_OK;
}

template <int MODEL>
void family_kernels(PointwiseLaunch &K, const WaicModel &model) {
  K.loo_hist = [model](dim3 grid, hipStream_t stream, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicDataset *sets, const int64_t *obs_off, void *state,
                       uint32_t *hist, int pass) {
    hipLaunchKernelGGL(loo_hist_kernel<MODEL>, grid, dim3(kThreads), 0, stream, draws, rows, PR, C, cpd, d0, model, sets, obs_off, static_cast<LooState *>(state), hist, pass);
    return hipGetLastError();
  };
  K.loo_compact = [model](dim3 grid, hipStream_t stream, const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicDataset *sets, const int64_t *obs_off,
                          const int64_t *part_off, void *state, double *tail, uint32_t cap, double *parts) {
    hipLaunchKernelGGL(loo_compact_kernel<MODEL>, grid, dim3(kThreads), 0, stream, draws, rows, PR, C, cpd, d0, model, sets, obs_off, part_off, static_cast<LooState *>(state), tail, cap, parts);
    return hipGetLastError();
  };
}

}  // namespace

void amwg_loo_family_kernels(PointwiseLaunch &K, const WaicModel &model) {
  switch (model.model) {
    case AMWG_MODEL_NORMAL: family_kernels<AMWG_MODEL_NORMAL>(K, model); break;
    case AMWG_MODEL_BETA_BERN: family_kernels<AMWG_MODEL_BETA_BERN>(K, model); break;
    case AMWG_MODEL_HIER_NORMAL: family_kernels<AMWG_MODEL_HIER_NORMAL>(K, model); break;
    default: family_kernels<AMWG_MODEL_POIS_GLM>(K, model); break;
  }
}

size_t amwg_loo_set_budget(size_t bytes) {
  const size_t before = g_budget;
  g_budget = bytes ? bytes : kLooScratchBytes;
  return before;
}
void amwg_loo_set_timing(int on) { g_timing.store(on); }
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
                    int32_t *high, double *pointwise, double *tails, hipStream_t stream) {
  PointwiseLaunch K;
  amwg_waic_family_kernels(K, model);
  amwg_loo_family_kernels(K, model);
  return amwg_loo_run(call, draws, rows, PR, C, D, K, sets, summary, high, pointwise, tails, stream);
}

int amwg_loo_run(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const PointwiseLaunch &K, const WaicDataset *sets, double *summary,
                 int32_t *high, double *pointwise, double *tails, hipStream_t stream) {
  if (!draws || !sets || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_loo_shape(call, rows, PR, C, D));
  int64_t n_max = 0;
  for (int d = 0; d < D; ++d) n_max = sets[d].n_obs > n_max ? sets[d].n_obs : n_max;
  const int64_t S = rows * (C / D), M = loo_tail_len(S);
  LooStats stats{0, g_timing.load(), 0.f, 0.f, 0.f, 0.f};      // this call's own; nothing shared is written while it runs
  // lppd_i: WAIC's, which also checks the family, its components and the sizes
  const size_t pairs = (size_t)D * (size_t)(n_max > 0 ? n_max : 1);
  std::vector<double> wsum((size_t)D * 4), wpw(pairs * 2), got(pairs * 2);
  {
    Phase ph(stream, stats.timed != 0);
    if (K.family) TRYB(amwg_waic_launch(call, draws, rows, PR, C, D, *K.family, sets, wsum.data(), nullptr, wpw.data(), nullptr, stream));
    else TRYB(amwg_waic_run(call, draws, rows, PR, C, D, K, sets, wsum.data(), nullptr, wpw.data(), nullptr, stream));
    ph.end(stats.ms_lppd);
  }
  const size_t pw_count = (size_t)D * (size_t)n_max * 2, tl_count = tails ? (size_t)D * (size_t)n_max * (size_t)(M + 1) : 0;
  DevBuf d_sets, d_pw, d_tl;
  HIP_TRY(d_sets.alloc((size_t)D * sizeof(WaicDataset)));
  HIP_TRY(hipMemcpyAsync(d_sets.p, sets, (size_t)D * sizeof(WaicDataset), hipMemcpyHostToDevice, stream));
  HIP_TRY(d_pw.alloc(pw_count * 8));
  if (pw_count) {
    hipLaunchKernelGGL(loo_fill_nan_kernel, dim3((unsigned)((pw_count + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, d_pw.as<double>(), (int64_t)pw_count);
    HIP_TRY(hipGetLastError());
  }
  if (tails) {
    HIP_TRY(d_tl.alloc(tl_count * 8));
    if (tl_count) {
      hipLaunchKernelGGL(loo_fill_nan_kernel, dim3((unsigned)((tl_count + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, d_tl.as<double>(), (int64_t)tl_count);
      HIP_TRY(hipGetLastError());
    }
  }
  double *dt = tails ? d_tl.as<double>() : nullptr;
  const WaicDataset *ds = d_sets.as<WaicDataset>();
  TRYB(run_kernels(call, draws, rows, PR, C, D, K, sets, ds, n_max, d_pw.as<double>(), dt, stats, stream));
  {
    std::lock_guard<std::mutex> hold(g_stats_lock);
    g_stats = stats;
  }
  if (pw_count) HIP_TRY(hipMemcpy(got.data(), d_pw.p, pw_count * 8, hipMemcpyDeviceToHost));
  if (tl_count) HIP_TRY(hipMemcpy(tails, d_tl.p, tl_count * 8, hipMemcpyDeviceToHost));
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
  static const char *call = "amwg_last_sample_dataset_loo";
  if (!s || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (s->user && s->pw_terms.empty()) return amwg_fail(AMWG_EINVAL, "%s: the pointwise terms of a closure are not known to the library; built-in families only", call);
  TRYB(amwg_refuse_summarised(s, call));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "%s: no sample() call yet", call);
  const int D = s->n_datasets, PR = s->P + s->D;
  TRYB(amwg_loo_shape(call, s->last_rows, PR, s->C, D));
  if (s->mc.group_local) return amwg_fail(AMWG_EINVAL, "%s: a group_local sampler keeps its observations as a lane-major tile; the pointwise terms need them in index order", call);
  HIP_TRY(hipSetDevice(s->device));
  std::vector<WaicDataset> sets;
  if (s->user) {
    UserPointwise u;
    TRYB(amwg_pointwise_describe_user(s, sets, u));
    PointwiseLaunch K;
    amwg_pointwise_user_kernels(K, u);
    return amwg_loo_run(call, s->last_draws, s->last_rows, PR, s->C, D, K, sets.data(), summary, high, pointwise, nullptr, s->stream);
  }
  WaicModel m{};
  TRYB(amwg_waic_describe(s, sets, m));
  return amwg_loo_launch(call, s->last_draws, s->last_rows, PR, s->C, D, m, sets.data(), summary, high, pointwise, nullptr, s->stream);
}
