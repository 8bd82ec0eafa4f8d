// amwg_pointwise.h -- the kernels of WAIC (amwg_waic.hip) and PSIS-LOO (amwg_loo.hip) that evaluate the model, as ONE text over the family class F and its model
// argument MA: WAIC's partial kernel and loglik kernel, LOO's histogram kernel and compaction kernel.  amwg_waic.hip and amwg_loo.hip instantiate it for the four
// built-in families (Family<MODEL>, WaicModel: amwg_terms.h); hiprtc instantiates the very same text for the pointwise terms of a translated closure (UserTerms:
// translate.js pointwisePlan; UserTermsArg) as the extern "C" entries at the end of this file, in one code object (amwg_rtc.hip compile_pointwise).  What does not
// depend on the model -- merge, pick, fit, fill, totals -- stays in the two .hip files and serves both.
//
// A family class F has: Draw (what an evaluation needs of a draw; staged in LDS), Obs (what it needs of an observation; registers), n_eff(ds), make_draw(at, C, M, ds),
// set_base(w, base), load_obs(M, ds, i) and term(M, o, w, i, draws, C).  M is the model argument as dataset d sees it: dataset_model(MA, d).
//
// STAGED RUN LENGTH.  stage_len<F>() draws are staged at a time: 256 (a thread each) wherever 256 Draws fit in 48 KiB of LDS, else the largest multiple of kWaves that
// fits -- a function of sizeof(Draw) alone, so the bytes of a dataset still depend on its own draws and data, on (rows, C / D) and, for a closure, on its text.  A Draw
// of which fewer than kWaves fit does not compile.
// Device code; not a source of the step kernels (tools/build_id.py).
#pragma once
#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#endif

#include "amwg_stdint.h"
#include "amwg_ld.h"
#include "amwg_select.h"
#include "amwg_types.h"
#include "amwg_pointwise_types.h"

namespace amwg {

constexpr int kThreads = 256;      // a workgroup: four wavefronts
constexpr int kTile = 64;          // observations per workgroup, a lane each
constexpr int kWaves = kThreads / 64;
constexpr int kStage = 256;        // draws staged in LDS at a time, a thread each (stage_len: fewer for a large Draw)
constexpr int kStageBytes = 48 * 1024;
constexpr int64_t kTargetBlocks = 2048;      // workgroups per dataset the split aims at (256 CUs x 8)
constexpr int64_t kMinRun = 256;             // draws per split at least: one staged run

constexpr int stage_len_of(size_t draw_bytes) {
  return (size_t)kStageBytes / draw_bytes >= (size_t)kStage ? kStage : (int)((size_t)kStageBytes / draw_bytes) / kWaves * kWaves;
}
template <class F> constexpr int stage_len() { return stage_len_of(sizeof(typename F::Draw)); }

// the number of contiguous runs a dataset's S draws are cut into, from S and its n alone
__host__ __device__ inline int64_t waic_splits(int64_t S, int64_t n) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  int64_t want = tiles > 0 ? kTargetBlocks / tiles : 1;
  want = want < 1 ? 1 : want;
  int64_t by_len = S / kMinRun;
  by_len = by_len < 1 ? 1 : by_len;
  return want < by_len ? want : by_len;
}
__host__ __device__ inline int64_t split_begin(int64_t S, int64_t splits, int64_t k) { return S / splits * k + (S % splits) * k / splits; }

// exp_v8 with its rare arguments out of line (0, beyond -708, the sliver at ln2 / 2): the loop's code holds the common path only
__device__ __forceinline__ double waic_exp(double a) {
  if (__builtin_expect(exp_is_rare(a), 0)) return exp_v8_cold(a);
  const ExpParts e = exp_parts(a, ExpLogLiterals{});
  return set_hi_word(e.y, hi_word(e.y) + (e.k << 20));
}

// the model argument as dataset d sees it
template <class MA> __device__ __forceinline__ const MA &dataset_model(const MA &M, int) { return M; }
__device__ __forceinline__ DataRef dataset_model(const UserTermsArg &M, int d) {
  DataRef v = M.d;
  if (M.table) {
    const void *const *row = M.table + (int64_t)d * (int64_t)M.row_stride;      // (a uniform address: scalar loads)
#pragma unroll
    for (int j = 0; j < kInlineUserArrays; ++j) v.arr[j] = row[j];
    v.arr_ext = row + kInlineUserArrays;
  }
  return v;
}

template <class F, class M>
__device__ __forceinline__ typename F::Draw draw_at(const double *draws, int PR, int64_t C, int64_t cpd, int d, int64_t s, const M &Md, const WaicDataset &ds) {
  const int64_t row = s / cpd, base = row * PR * C + (int64_t)d * cpd + (s - row * cpd);
  typename F::Draw w = F::make_draw(draws + base, C, Md, ds);
  F::set_base(w, base);
  return w;
}

// ---- WAIC
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
template <class F, class MA>
__device__ __forceinline__ void waic_partial_body(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const MA &M,
                                                  const WaicDataset *__restrict__ sets, const int64_t *__restrict__ part_off, Part *__restrict__ parts) {
  constexpr int kRun = stage_len<F>();
  static_assert(kRun >= kWaves, "the Draw of this model is too large: fewer than kWaves of them fit in the 48 KiB of LDS a workgroup stages draws in");
  __shared__ typename F::Draw stage[kRun];
  __shared__ Part wave_part[kWaves - 1][kTile];
  const int d = d0 + (int)blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WaicDataset ds = sets[d];
  const int64_t n = F::n_eff(ds), S = rows * cpd, splits = waic_splits(S, n);
  if ((int64_t)blockIdx.x * kTile >= n || (int64_t)blockIdx.y >= splits) return;      // (uniform over the workgroup)
  const auto &Md = dataset_model(M, d);
  const int64_t s_begin = split_begin(S, splits, blockIdx.y), s_end = split_begin(S, splits, (int64_t)blockIdx.y + 1);
  const int64_t i = (int64_t)blockIdx.x * kTile + lane;
  const bool active = i < n;
  const typename F::Obs o = F::load_obs(Md, ds, active ? i : n - 1);
  Part a{-kInf, 0.0, 0.0, 0.0};
  double cnt = 0.0;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += kRun) {
    const int L = (int)(s_end - s0 < kRun ? s_end - s0 : kRun);
    __syncthreads();
    if (tid < L) stage[tid] = draw_at<F>(draws, PR, C, cpd, d, s0 + tid, Md, ds);
    __syncthreads();
    if (wave >= L) continue;      // (uniform over the wavefront; the barriers above are reached by all: L does not depend on the wavefront)
    const double K = cnt == 0.0 ? F::term(Md, o, stage[wave], active ? i : n - 1, draws, C) : a.mean;
    double s1 = 0.0, s2 = 0.0;
    int nb = 0;
    for (int j = wave; j < L; j += kWaves) {
      const double l = F::term(Md, o, stage[j], active ? i : n - 1, draws, C);
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
  const int64_t len = s_end - s_begin, full = len / kRun, rest = len % kRun;
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const double nw = (double)(full * (kRun / kWaves) + (rest > w ? (rest - w + kWaves - 1) / kWaves : 0));
    merge_parts(a, cnt, wave_part[w - 1][lane], nw);
  }
  parts[part_off[blockIdx.z] + (int64_t)blockIdx.y * n + i] = a;
}

// the terms themselves, out[(d * S + s) * n_max + i]: the test library's view of what the partial kernel accumulates (the same device functions).  BERN: the family
// of two observations, picked by x_i (amwg_terms.h)
template <class F, class MA, bool BERN>
__device__ __forceinline__ void waic_loglik_body(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, const MA &M,
                                                 const WaicDataset *__restrict__ sets, double *__restrict__ out, int64_t n_max) {
  const int d = blockIdx.z;
  const WaicDataset ds = sets[d];
  const int64_t S = rows * cpd, s = blockIdx.y, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= ds.n_obs) return;
  const auto &Md = dataset_model(M, d);
  const typename F::Draw w = draw_at<F>(draws, PR, C, cpd, d, s, Md, ds);
  double l;
  if constexpr (BERN) {
    const bool invalid = Md.invalid && Md.invalid[ds.off_xb + i];
    l = invalid ? -kInf : F::term(Md, F::load_obs(Md, ds, Md.xb[ds.off_xb + i] ? 0 : 1), w, i, draws, C);
  } else {
    l = F::term(Md, F::load_obs(Md, ds, i), w, i, draws, C);
  }
  out[((int64_t)d * S + s) * n_max + i] = l;
}

// ---- PSIS-LOO
constexpr int kDigitBits = 7, kBins = 1 << kDigitBits;      // 128 x 64 counters of 4 bytes: 32 KB of LDS beside the staged draws
constexpr int kPasses = (64 + kDigitBits - 1) / kDigitBits;      // 10: nine digits of 7 bits and the last bit
constexpr uint64_t kMaxKey = ~(uint64_t)0;

struct LooState {
  uint64_t prefix, thr, minkey;      // the digits chosen so far (low bits 0); the threshold key once done; the smallest key
  uint32_t lo, in, done, inclusive, bad, cursor;      // keys below the bin, keys in it; 1: take keys <= thr, 0: keys < thr and copies of thr; a non-finite term; tail slots taken
};

__host__ __device__ inline int pass_shift(int pass) { const int s = 64 - kDigitBits * (pass + 1); return s < 0 ? 0 : s; }
__host__ __device__ inline int pass_bins(int pass) { return 64 - kDigitBits * pass >= kDigitBits ? kBins : 1 << (64 - kDigitBits * pass); }

// one digit of the select: hist[(obs_off[z] + i) * kBins + bin] += the terms of (d, i) whose key agrees with the prefix, by the bin of this pass's digit
template <class F, class MA>
__device__ __forceinline__ void loo_hist_body(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const MA &M,
                                              const WaicDataset *__restrict__ sets, const int64_t *__restrict__ obs_off, LooState *__restrict__ state,
                                              uint32_t *__restrict__ hist, int pass) {
  constexpr int kRun = stage_len<F>();
  static_assert(kRun >= kWaves, "the Draw of this model is too large: fewer than kWaves of them fit in the 48 KiB of LDS a workgroup stages draws in");
  __shared__ typename F::Draw stage[kRun];
  __shared__ uint32_t cnt[kBins * kTile];      // [bin][lane]: a wavefront's 64 lanes fall into 64 different banks whatever their bins
  const int d = d0 + (int)blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WaicDataset ds = sets[d];
  const int64_t n = F::n_eff(ds), S = rows * cpd, splits = waic_splits(S, n);
  if ((int64_t)blockIdx.x * kTile >= n || (int64_t)blockIdx.y >= splits) return;      // (uniform over the workgroup)
  const auto &Md = dataset_model(M, d);
  const int64_t s_begin = split_begin(S, splits, blockIdx.y), s_end = split_begin(S, splits, (int64_t)blockIdx.y + 1);
  const int64_t i = (int64_t)blockIdx.x * kTile + lane;
  const bool active = i < n;
  const int64_t o_at = obs_off[blockIdx.z] + (active ? i : n - 1);
  const LooState st = state[o_at];
  const bool counting = active && !st.done;
  if (!__syncthreads_or(counting ? 1 : 0)) return;      // every observation of the tile is done
  for (int k = tid; k < kBins * kTile; k += kThreads) cnt[k] = 0;
  const typename F::Obs o = F::load_obs(Md, ds, active ? i : n - 1);
  const int shift = pass_shift(pass), shift_prev = 64 - kDigitBits * pass;
  const uint32_t mask = (uint32_t)pass_bins(pass) - 1u;
  uint64_t kmin = kMaxKey;
  bool bad = false;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += kRun) {
    const int L = (int)(s_end - s0 < kRun ? s_end - s0 : kRun);
    __syncthreads();
    if (tid < L) stage[tid] = draw_at<F>(draws, PR, C, cpd, d, s0 + tid, Md, ds);
    __syncthreads();
    for (int j = wave; j < L; j += kWaves) {
      const double l = F::term(Md, o, stage[j], active ? i : n - 1, draws, C);
      const uint64_t key = select_key(l);
      if (pass == 0) {
        kmin = key < kmin ? key : kmin;
        bad = bad || !(__builtin_fabs(l) < kInf);
      }
      const bool match = pass == 0 || ((key ^ st.prefix) >> shift_prev) == 0;
      if (counting && match) atomicAdd(&cnt[(((uint32_t)(key >> shift)) & mask) * kTile + lane], 1u);
    }
  }
  __syncthreads();
  uint32_t *h = hist + obs_off[blockIdx.z] * kBins;
  for (int k = tid; k < kBins * kTile; k += kThreads) {
    const uint32_t c = cnt[k];
    if (c) atomicAdd(&h[((int64_t)blockIdx.x * kTile + (k & (kTile - 1))) * kBins + (k >> 6)], c);      // (a lane that counted is an observation below n)
  }
  if (pass == 0 && active) {
    atomicMin((unsigned long long *)&state[o_at].minkey, (unsigned long long)kmin);
    if (bad) atomicOr(&state[o_at].bad, 1u);
  }
}

// the terms at or below the threshold into the tail, the others into the split's partial of B = sum exp(a_0 - l): parts[part_off[z] + split * n + i]
template <class F, class MA>
__device__ __forceinline__ void loo_compact_body(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const MA &M,
                                                 const WaicDataset *__restrict__ sets, const int64_t *__restrict__ obs_off, const int64_t *__restrict__ part_off,
                                                 LooState *__restrict__ state, double *__restrict__ tail, uint32_t cap, double *__restrict__ parts) {
  constexpr int kRun = stage_len<F>();
  static_assert(kRun >= kWaves, "the Draw of this model is too large: fewer than kWaves of them fit in the 48 KiB of LDS a workgroup stages draws in");
  __shared__ typename F::Draw stage[kRun];
  __shared__ double wave_b[kWaves - 1][kTile];
  const int d = d0 + (int)blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WaicDataset ds = sets[d];
  const int64_t n = F::n_eff(ds), S = rows * cpd, splits = waic_splits(S, n);
  if ((int64_t)blockIdx.x * kTile >= n || (int64_t)blockIdx.y >= splits) return;      // (uniform over the workgroup)
  const auto &Md = dataset_model(M, d);
  const int64_t s_begin = split_begin(S, splits, blockIdx.y), s_end = split_begin(S, splits, (int64_t)blockIdx.y + 1);
  const int64_t i = (int64_t)blockIdx.x * kTile + lane;
  const bool active = i < n;
  const int64_t o_at = obs_off[blockIdx.z] + (active ? i : n - 1);
  const LooState st = state[o_at];
  const double a0 = select_value(st.minkey);
  const typename F::Obs o = F::load_obs(Md, ds, active ? i : n - 1);
  double *my_tail = tail + o_at * cap;
  double b = 0.0;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += kRun) {
    const int L = (int)(s_end - s0 < kRun ? s_end - s0 : kRun);
    __syncthreads();
    if (tid < L) stage[tid] = draw_at<F>(draws, PR, C, cpd, d, s0 + tid, Md, ds);
    __syncthreads();
    for (int j = wave; j < L; j += kWaves) {
      const double l = F::term(Md, o, stage[j], active ? i : n - 1, draws, C);
      const uint64_t key = select_key(l);
      const bool take = st.inclusive ? key <= st.thr : key < st.thr;
      if (take) {
        if (active) {
          const uint32_t at = atomicAdd(&state[o_at].cursor, 1u);
          if (at < cap) my_tail[at] = l;      // (the counts of the select say at < cap; the comparison keeps a wrong count inside the buffer)
        }
      } else if (key > st.thr) {
        b += waic_exp(a0 - l);
      }
    }
  }
  __syncthreads();
  if (wave > 0) wave_b[wave - 1][lane] = b;
  __syncthreads();
  if (wave != 0 || !active) return;
#pragma unroll
  for (int w = 1; w < kWaves; ++w) b += wave_b[w - 1][lane];
  parts[part_off[blockIdx.z] + (int64_t)blockIdx.y * n + i] = b;
}

}  // namespace amwg

// ---- a translated closure's pointwise terms (hiprtc; the program is `source`, the UserTerms text, then this header under AMWG_POINTWISE_USER: amwg_rtc.hip)
#if defined(AMWG_POINTWISE_USER)
namespace amwg {
struct UserFamily {
  typedef UserTerms::Draw Draw;
  struct Obs {};
  __device__ static int64_t n_eff(const WaicDataset &ds) { return ds.n_obs; }
  __device__ static Draw make_draw(const double *at, int64_t C, const DataRef &d, const WaicDataset &) { return UserTerms::make_draw(at, C, d); }
  __device__ static void set_base(Draw &w, int64_t base) { UserTerms::set_base(w, base); }
  __device__ static Obs load_obs(const DataRef &, const WaicDataset &, int64_t) { return Obs{}; }
  __device__ __forceinline__ static double term(const DataRef &d, const Obs &, const Draw &w, int64_t i, const double *draws, int64_t C) {
    return UserTerms::term(w, d, UserTerms::kTermStart + (int)i, draws, C);
  }
};
}  // namespace amwg

extern "C" __global__ void __launch_bounds__(amwg::kThreads) amwg_pw_waic_partial(const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const amwg::UserTermsArg M,
                                                                                  const WaicDataset *sets, const int64_t *part_off, amwg::Part *parts) {
  amwg::waic_partial_body<amwg::UserFamily>(draws, rows, PR, C, cpd, d0, M, sets, part_off, parts);
}
extern "C" __global__ void __launch_bounds__(amwg::kThreads) amwg_pw_waic_loglik(const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, const amwg::UserTermsArg M,
                                                                                 const WaicDataset *sets, double *out, int64_t n_max) {
  amwg::waic_loglik_body<amwg::UserFamily, amwg::UserTermsArg, false>(draws, rows, PR, C, cpd, M, sets, out, n_max);
}
extern "C" __global__ void __launch_bounds__(amwg::kThreads) amwg_pw_loo_hist(const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const amwg::UserTermsArg M,
                                                                              const WaicDataset *sets, const int64_t *obs_off, amwg::LooState *state, uint32_t *hist, int pass) {
  amwg::loo_hist_body<amwg::UserFamily>(draws, rows, PR, C, cpd, d0, M, sets, obs_off, state, hist, pass);
}
extern "C" __global__ void __launch_bounds__(amwg::kThreads) amwg_pw_loo_compact(const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const amwg::UserTermsArg M,
                                                                                 const WaicDataset *sets, const int64_t *obs_off, const int64_t *part_off, amwg::LooState *state,
                                                                                 double *tail, uint32_t cap, double *parts) {
  amwg::loo_compact_body<amwg::UserFamily>(draws, rows, PR, C, cpd, d0, M, sets, obs_off, part_off, state, tail, cap, parts);
}
#endif
