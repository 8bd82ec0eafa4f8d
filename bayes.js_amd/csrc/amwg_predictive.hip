// amwg_predictive.hip -- posterior predictive calibration per dataset on the device (amwg_last_sample_dataset_predictive; part of libamwg.so): per observation the
// probability integral transform, the predictive mean and the predictive sd over the stored draws.  include/amwg.h states the rule, amwg_predictive.h the route,
// amwg_cdf.h the two distribution functions.  The accumulations are bounded, not pinned, and deterministic.  Not a source of the step kernels (tools/build_id.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "amwg_cdf.h"
#include "amwg_fold.h"
#include "amwg_heldout.h"
#include "amwg_host.h"
#include "amwg_lanes.h"
#include "amwg_ld.h"
#include "amwg_pointwise.h"
#include "amwg_predictive.h"
#include "amwg_predictive_eval.h"
#include "amwg_waic.h"

using namespace amwg;

namespace {

struct Rec { double sF, sFm, sV, n, mean, M2; };          // sums of F, Fm, var; (count, mean, M2) of the location over the draws.  An empty one is all zero

// b after a: plain sums, and Chan's formula
__device__ __forceinline__ Rec rec_merge(const Rec &a, const Rec &b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double nt = a.n + b.n, delta = b.mean - a.mean;
  return Rec{a.sF + b.sF, a.sFm + b.sFm, a.sV + b.sV, nt, a.mean + delta * (b.n / nt), a.M2 + b.M2 + delta * delta * (a.n * b.n / nt)};
}

// one step of the butterfly: the records of lane and lane ^ OFF merged as (lower lane, upper lane), the same bytes in both
template <int OFF> __device__ __forceinline__ Rec butterfly_step(const Rec &a, int lane) {
  Rec lo, hi;
  lane_pair<OFF>(a.sF, lane, lo.sF, hi.sF); lane_pair<OFF>(a.sFm, lane, lo.sFm, hi.sFm); lane_pair<OFF>(a.sV, lane, lo.sV, hi.sV);
  lane_pair<OFF>(a.n, lane, lo.n, hi.n); lane_pair<OFF>(a.mean, lane, lo.mean, hi.mean); lane_pair<OFF>(a.M2, lane, lo.M2, hi.M2);
  return rec_merge(lo, hi);
}
// the lane distances from Np up (Np is uniform over the workgroup, and all 64 lanes are here)
__device__ __forceinline__ Rec butterfly_from(Rec a, int Np, int lane) {
  if (Np <= 1) a = butterfly_step<1>(a, lane);
  if (Np <= 2) a = butterfly_step<2>(a, lane);
  if (Np <= 4) a = butterfly_step<4>(a, lane);
  if (Np <= 8) a = butterfly_step<8>(a, lane);
  if (Np <= 16) a = butterfly_step<16>(a, lane);
  if (Np <= 32) a = butterfly_step<32>(a, lane);
  return a;
}

// the split's draws walked by one lane: FULL -- a thread per observation, compile-time strides; else the observation spread over 64 / Np lanes
template <int MODEL, bool FULL>
__device__ __forceinline__ void walk(const double *__restrict__ draws, int PR, int64_t C, int64_t cpd, int d, const WaicModel &M, const WaicDataset &ds,
                                     const int32_t *__restrict__ index, int Mt, int64_t s_begin, int64_t s_end, typename Pred<MODEL>::Draw *stage, Rec (*wave_part)[kTile],
                                     Rec *__restrict__ out, double *__restrict__ y_out) {
  typedef Pred<MODEL> F;
  constexpr int R = F::R;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int Np = kTile;
  if (!FULL) { Np = 1; while (Np < Mt) Np <<= 1; }
  const int sub = FULL ? 1 : kTile / Np, slot = FULL ? lane : lane & (Np - 1), unit = FULL ? wave : wave * sub + lane / Np, units = FULL ? kWaves : kWaves * sub;
  const int64_t j = (int64_t)blockIdx.x * kTile + (slot < Mt ? slot : Mt - 1);      // (a lane beyond the tile's observations repeats the last: its partners hold the same slot)
  const typename F::Obs o = F::load_obs(M, ds, j);
  const int64_t pos = MODEL == AMWG_MODEL_POIS_GLM && index ? (int64_t)index[ds.off_xb + j] : j;
  double sF = 0.0, sFm = 0.0, sV = 0.0, s1 = 0.0, s2 = 0.0, K = 0.0;
  int n = 0;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += kStage) {
    const int L = (int)(s_end - s0 < kStage ? s_end - s0 : kStage);
    __syncthreads();
    if (tid < L) {
      const int64_t s = s0 + tid, row = s / cpd, base = row * PR * C + (int64_t)d * cpd + (s - row * cpd);
      stage[tid] = F::make_draw(draws + base, C, M, base);
    }
    __syncthreads();
    for (int jb = unit; jb < L; jb += units * R) {
      double f[R], fm[R], v[R], dm[R], q[R];
      Eval e[R];
#pragma unroll
      for (int r = 0; r < R; ++r) e[r] = F::eval(o, stage[jb + units * r < L ? jb + units * r : jb], pos, draws, C);      // R independent evaluations
      if (n == 0) K = e[0].mean;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool in = jb + units * r < L;
        f[r] = in ? e[r].F : 0.0; fm[r] = in ? e[r].Fm : 0.0; v[r] = in ? e[r].var : 0.0;
        dm[r] = in ? e[r].mean - K : 0.0;
        q[r] = dm[r] * dm[r];
        n += in ? 1 : 0;
      }
#pragma unroll
      for (int w = 1; w < R; w <<= 1)
#pragma unroll
        for (int r = 0; r + w < R; r += 2 * w) { f[r] += f[r + w]; fm[r] += fm[r + w]; v[r] += v[r + w]; dm[r] += dm[r + w]; q[r] += q[r + w]; }
      sF += f[0]; sFm += fm[0]; sV += v[0]; s1 += dm[0]; s2 += q[0];
    }
  }
  Rec a{sF, sFm, sV, (double)n, 0.0, 0.0};
  if (n > 0) {
    const double c = s1 / a.n, M2 = s2 - s1 * c;
    a.mean = K + c;
    a.M2 = M2 < 0.0 ? 0.0 : M2;      // (a NaN stays a NaN)
  }
  if (!FULL) a = butterfly_from(a, Np, lane);
  __syncthreads();
  if (wave > 0 && lane < Np) wave_part[wave - 1][lane] = a;
  __syncthreads();
  if (wave != 0 || lane >= Mt) return;      // (lane < Mt: the lane is its own slot, and the slot holds an observation)
#pragma unroll
  for (int w = 1; w < kWaves; ++w) a = rec_merge(a, wave_part[w - 1][lane]);
  out[j] = a;
  if (blockIdx.y == 0) y_out[j] = F::y_of(o);
}

// parts[part_off[z] + split * m + j], z = the dataset's place in the batch; y[d * y_stride + j] = observation j as the finish on the host reads it
template <int MODEL>
__global__ void __launch_bounds__(kThreads) predictive_partial_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                      const WaicDataset *__restrict__ sets, const int32_t *__restrict__ index,
                                                                      const int64_t *__restrict__ part_off, Rec *__restrict__ parts, double *__restrict__ y, int64_t y_stride) {
  static_assert(sizeof(typename Pred<MODEL>::Draw) * kStage <= (size_t)kStageBytes, "256 staged draws fit the 48 KiB of LDS");
  __shared__ typename Pred<MODEL>::Draw stage[kStage];
  __shared__ Rec wave_part[kWaves - 1][kTile];
  const int d = d0 + (int)blockIdx.z;
  const WaicDataset ds = sets[d];
  const int64_t m = ds.n_obs, S = rows * cpd, splits = waic_splits(S, m);
  if ((int64_t)blockIdx.x * kTile >= m || (int64_t)blockIdx.y >= splits) return;      // (uniform over the workgroup)
  const int64_t left = m - (int64_t)blockIdx.x * kTile;
  const int64_t s_begin = split_begin(S, splits, blockIdx.y), s_end = split_begin(S, splits, (int64_t)blockIdx.y + 1);
  Rec *out = parts + part_off[blockIdx.z] + (int64_t)blockIdx.y * m;
  double *y_out = y + (int64_t)d * y_stride;
  if (left >= kTile) walk<MODEL, true>(draws, PR, C, cpd, d, M, ds, index, kTile, s_begin, s_end, stage, wave_part, out, y_out);
  else walk<MODEL, false>(draws, PR, C, cpd, d, M, ds, index, (int)left, s_begin, s_end, stage, wave_part, out, y_out);
}

// out[(d * out_stride + j) * 4 ...] = pit_hi, pit_lo, pred_mean, pred_sd for j < m_d.  A WAVEFRONT per observation: lane k merges the splits k, k + 64, ... in
// ascending order, then the 64 lanes merge by the butterfly: a fixed tree, a function of the split count alone
__global__ void __launch_bounds__(kThreads) predictive_finish_kernel(int64_t rows, int64_t cpd, int d0, const WaicDataset *__restrict__ sets, const int64_t *__restrict__ part_off,
                                                                     const Rec *__restrict__ parts, double *__restrict__ out, int64_t out_stride) {
  const int d = d0 + (int)blockIdx.y;
  const int64_t m = sets[d].n_obs, S = rows * cpd, splits = waic_splits(S, m);
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (j >= m) return;      // (uniform over the wavefront)
  const Rec *p = parts + part_off[blockIdx.y] + j;
  Rec a{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t k = lane; k < splits; k += 64) a = rec_merge(a, p[k * m]);
  a = butterfly_from(a, 1, lane);
  if (lane != 0) return;
  const double Sd = (double)S;
  double r[4] = {a.sF / Sd, a.sFm / Sd, a.mean, __builtin_sqrt(a.sV / Sd + a.M2 / Sd)};
  const bool finite = __builtin_fabs(r[0]) < kInf && __builtin_fabs(r[1]) < kInf && __builtin_fabs(r[2]) < kInf && __builtin_fabs(r[3]) < kInf;
  double *o = out + ((int64_t)d * out_stride + j) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = finite ? r[k] : __builtin_nan("");
}

template <int... MODEL> const void *partial_fn(PointwiseModels<MODEL...>, int model) {
  const void *const fn[] = {reinterpret_cast<const void *>(&predictive_partial_kernel<MODEL>)...};
  return fn[model - AMWG_MODEL_NORMAL];
}

}  // namespace

void amwg_predictive_totals(const double *pw, const double *y, int64_t m, double *summary) {
  double in50 = 0.0, in90 = 0.0, ss = 0.0, mids = 0.0;
  bool nan = m == 0;
  for (int64_t j = 0; j < m; ++j) {
    const double mid = (pw[4 * j] + pw[4 * j + 1]) / 2, e = y[j] - pw[4 * j + 2];
    nan = nan || mid != mid || e != e || pw[4 * j + 3] != pw[4 * j + 3];
    in50 += 0.25 <= mid && mid <= 0.75 ? 1.0 : 0.0;
    in90 += 0.05 <= mid && mid <= 0.95 ? 1.0 : 0.0;
    ss += e * e;
    mids += mid;
  }
  const double md = (double)m;
  summary[0] = nan ? (double)NAN : in50 / md;
  summary[1] = nan ? (double)NAN : in90 / md;
  summary[2] = nan ? (double)NAN : std::sqrt(ss / md);
  summary[3] = nan ? (double)NAN : mids / md;
}

int amwg_predictive_run(const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &M_in, const WaicDataset *sets, const int32_t *index,
                        double *summary, double *pointwise, size_t scratch_bytes, hipStream_t stream) {
  WaicModel M = M_in;
  int64_t cpd = C / D;      // (not const: the args[] list points at it)
  const int64_t S = rows * cpd;
  int64_t m_max = 0;
  for (int d = 0; d < D; ++d) m_max = sets[d].n_obs > m_max ? sets[d].n_obs : m_max;
  // ---- the outputs, and the batches under the budget: 48 bytes per (split, observation)
  DevBuf d_sets, d_pw, d_y, d_off, d_parts;
  HIP_TRY(d_sets.alloc((size_t)D * sizeof(WaicDataset)));
  HIP_TRY(hipMemcpyAsync(d_sets.p, sets, (size_t)D * sizeof(WaicDataset), hipMemcpyHostToDevice, stream));
  const size_t obs_count = (size_t)D * (size_t)m_max;
  HIP_TRY(d_pw.alloc(obs_count * 32));
  HIP_TRY(amwg_pointwise_fill_nan(d_pw.as<double>(), (int64_t)obs_count * 4, stream));
  HIP_TRY(d_y.alloc(obs_count * 8));
  HIP_TRY(amwg_pointwise_fill_nan(d_y.as<double>(), (int64_t)obs_count, stream));
  const size_t budget = scratch_bytes ? scratch_bytes : kPointwiseScratchBytes;
  struct Batch { int d0, d1; int64_t tiles, splits, m_most; };
  constexpr int kMaxGridYZ = 65535;
  std::vector<Batch> batches;
  std::vector<int64_t> part_off((size_t)D, 0);
  int64_t most_parts = 0, prt = 0;
  Batch b{0, 0, 0, 0, 0};
  for (int d = 0; d < D; ++d) {
    const int64_t m = sets[d].n_obs, sp = waic_splits(S, m), np = sp * m, t = (m + kTile - 1) / kTile;
    if ((prt && (size_t)(prt + np) * sizeof(Rec) > budget) || d - b.d0 >= kMaxGridYZ) { b.d1 = d; batches.push_back(b); b = Batch{d, d, 0, 0, 0}; prt = 0; }      // (the batch's datasets are a grid dimension)
    part_off[(size_t)d] = prt;
    prt += np;
    b.tiles = t > b.tiles ? t : b.tiles; b.splits = sp > b.splits ? sp : b.splits; b.m_most = m > b.m_most ? m : b.m_most;
    most_parts = prt > most_parts ? prt : most_parts;
  }
  b.d1 = D;
  batches.push_back(b);
  HIP_TRY(d_off.alloc((size_t)D * 8));
  HIP_TRY(hipMemcpyAsync(d_off.p, part_off.data(), (size_t)D * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(d_parts.alloc((size_t)most_parts * sizeof(Rec)));
  const WaicDataset *sets_dev = d_sets.as<WaicDataset>();
  Rec *parts = d_parts.as<Rec>();
  double *out = d_pw.as<double>(), *y_dev = d_y.as<double>();
  const void *fn = partial_fn(BuiltinModels{}, M.model);
  for (const Batch &bt : batches) {
    if (bt.tiles == 0) continue;
    int d0 = bt.d0;
    int64_t y_stride = m_max;
    const int64_t *off_dev = d_off.as<int64_t>() + d0;
    void *args[] = {&draws, &rows, &PR, &C, &cpd, &d0, &M, &sets_dev, &index, &off_dev, &parts, &y_dev, &y_stride};
    (void)hipLaunchKernel(fn, dim3((unsigned)bt.tiles, (unsigned)bt.splits, (unsigned)(bt.d1 - d0)), dim3(kThreads), args, 0, stream);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(predictive_finish_kernel, dim3((unsigned)((bt.m_most + kWaves - 1) / kWaves), (unsigned)(bt.d1 - d0)), dim3(kThreads), 0, stream, rows, cpd, d0, sets_dev,
                       off_dev, parts, out, m_max);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is freed on return)
  std::vector<double> own, y(obs_count ? obs_count : 1);
  double *pw = pointwise;
  if (!pw) { own.resize(obs_count ? obs_count * 4 : 1); pw = own.data(); }
  if (obs_count) {
    HIP_TRY(hipMemcpy(pw, d_pw.p, obs_count * 32, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(y.data(), d_y.p, obs_count * 8, hipMemcpyDeviceToHost));
  }
  for (int d = 0; d < D; ++d) amwg_predictive_totals(pw + (size_t)d * (size_t)m_max * 4, y.data() + (size_t)d * (size_t)m_max, sets[d].n_obs, summary + (size_t)d * 4);
  return AMWG_OK;
}

extern "C" int amwg_last_sample_dataset_predictive(amwg_sampler *s, const amwg_model_desc *held, const int32_t *index, double *summary, double *pointwise) {
  static const char *call = "amwg_last_sample_dataset_predictive";
  if (!s || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (s->user) return amwg_fail(AMWG_EINVAL, "%s: the predictive distribution of a closure is not known to the library; built-in families only", call);
  TRYB(amwg_need_stored_draws(s, call));
  const int D = s->n_datasets, PR = s->P + s->D;
  TRYB(amwg_waic_shape(call, s->last_rows, PR, s->C, D));
  if (s->mc.group_local) return amwg_fail(AMWG_EINVAL, "%s: a group_local sampler keeps its observations as a lane-major tile; the pointwise terms need them in index order", call);
  if (held) TRYB(amwg_heldout_validate(call, s->model, s->d.G, s->d.K, D, held, index));
  WaicModel base{};
  base.model = s->model; base.G = s->d.G; base.exact_division = s->mc.exact_division;
  base.neg_half_log_2pi = s->mc.neg_half_log_2pi;
  PointwiseLaunch K;
  TRYB(amwg_pointwise_family(call, base, PR, D, K));      // (the components a draw must hold)
  HIP_TRY(hipSetDevice(s->device));
  if (held) {
    HeldArrays h;
    TRYB(amwg_heldout_pack(base, D, held, index, s->stream, h));
    return amwg_predictive_run(s->last_draws, s->last_rows, PR, s->C, D, h.M, h.sets.data(), h.index, summary, pointwise, 0, s->stream);
  }
  std::vector<WaicDataset> sets;      // in-sample: the sampler's own arrays where they lie
  TRYB(amwg_waic_describe(s, sets, base));
  return amwg_predictive_run(s->last_draws, s->last_rows, PR, s->C, D, base, sets.data(), nullptr, summary, pointwise, 0, s->stream);
}
