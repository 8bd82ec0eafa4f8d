// amwg_heldout.hip -- held-out predictive density per dataset on the device (amwg_last_sample_dataset_heldout; part of libamwg.so): the scoring step of K-fold
// cross-validation and of exact refits.  include/amwg.h states the rule, amwg_heldout.h the route: FEW OBSERVATIONS x MANY DRAWS -- an observation is owned by
// 64 / Np lanes of every wavefront, which share the staged draws between them, keep (m, sum exp(l - m)) over register blocks of R terms and merge by a cross-lane
// butterfly.  The terms are Family<MODEL>::term of amwg_terms.h over held-out arrays packed as the sampler packs its own: WAIC's doubles, bit for bit.  The
// accumulations are bounded, not pinned, and deterministic.  Not a source of the step kernels (tools/build_id.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "amwg_fold.h"
#include "amwg_heldout.h"
#include "amwg_host.h"
#include "amwg_lanes.h"
#include "amwg_terms.h"
#include "amwg_waic.h"

using namespace amwg;

namespace {

struct Lse { double m, sum; };      // max term and sum exp(l - m); an empty one is (-inf, 0)

// sum as it stands under the larger maximum M (m == M: as it is -- and (-inf, 0) under -inf stays 0, where exp(-inf + inf) would be NaN)
__device__ __forceinline__ double rescaled(double sum, double m, double M) { return m == M ? sum : sum * exp_v8_cold(m - M); }
// max, two rescales, one add: the same bytes whichever way round the two come
__device__ __forceinline__ Lse lse_merge(const Lse &a, const Lse &b) {
  const double M = b.m > a.m ? b.m : a.m;
  return Lse{M, rescaled(a.sum, a.m, M) + rescaled(b.sum, b.m, M)};
}

// one step of the butterfly: a merged with the Lse of lane ^ OFF, in every lane.  OFF = 16, 32: v_permlane16_swap / v_permlane32_swap with both operands the same
// register leave the lane's own value in one result and the partner's in the other; which is which depends on the lane and does not matter to a symmetric merge
template <int OFF> __device__ __forceinline__ Lse butterfly_step(const Lse &a) {
  if constexpr (OFF < 16) {
    return lse_merge(a, Lse{dpp_xor<OFF>(a.m), dpp_xor<OFF>(a.sum)});
  } else {
    const uint32_t w[4] = {(uint32_t)f64_bits(a.m), (uint32_t)(f64_bits(a.m) >> 32), (uint32_t)f64_bits(a.sum), (uint32_t)(f64_bits(a.sum) >> 32)};
    uint32_t x[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (OFF == 32) { const auto r = __builtin_amdgcn_permlane32_swap(w[k], w[k], false, false); x[k] = r[0]; y[k] = r[1]; }
      else { const auto r = __builtin_amdgcn_permlane16_swap(w[k], w[k], false, false); x[k] = r[0]; y[k] = r[1]; }
    }
    return lse_merge(Lse{bits_f64(((uint64_t)x[1] << 32) | x[0]), bits_f64(((uint64_t)x[3] << 32) | x[2])},
                     Lse{bits_f64(((uint64_t)y[1] << 32) | y[0]), bits_f64(((uint64_t)y[3] << 32) | y[2])});
  }
}

// held-out observation j as the family's Obs.  The Bernoulli family: every x_j directly -- the family's observation 0 is x = 1, its observation 1 is x = 0; an x
// that is neither has the term -inf under every draw
template <int MODEL> struct HeldObs {
  __device__ static typename Family<MODEL>::Obs load(const WaicModel &M, const WaicDataset &ds, int64_t j, bool &invalid) {
    invalid = false;
    return Family<MODEL>::load_obs(M, ds, j);
  }
};
template <> struct HeldObs<AMWG_MODEL_BETA_BERN> {
  __device__ static Family<AMWG_MODEL_BETA_BERN>::Obs load(const WaicModel &M, const WaicDataset &ds, int64_t j, bool &invalid) {
    invalid = M.invalid && M.invalid[ds.off_xb + j];
    return Family<AMWG_MODEL_BETA_BERN>::load_obs(M, ds, M.xb[ds.off_xb + j] ? 0 : 1);
  }
};

// parts[part_off[z] + split * m + j], z = the dataset's place in the batch.  sets, M: the HELD-OUT data; index: the Poisson family's positions, at ds.off_xb
template <int MODEL>
__global__ void __launch_bounds__(kThreads) heldout_partial_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, int d0, const WaicModel M,
                                                                   const WaicDataset *__restrict__ sets, const int32_t *__restrict__ index, const int64_t *__restrict__ part_off,
                                                                   Lse *__restrict__ parts) {
  typedef Family<MODEL> F;
  constexpr int kRun = stage_len<F>(), R = group_block<F>();
  static_assert(kRun >= kWaves && kRun <= kThreads, "a staged run is filled a thread per draw");
  __shared__ typename F::Draw stage[kRun];
  __shared__ Lse wave_part[kWaves - 1][kTile];
  const int d = d0 + (int)blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WaicDataset ds = sets[d];
  const int64_t m = ds.n_obs, S = rows * cpd, splits = heldout_splits(S, m);
  if ((int64_t)blockIdx.x * kTile >= m || (int64_t)blockIdx.y >= splits) return;      // (uniform over the workgroup)
  const int64_t left = m - (int64_t)blockIdx.x * kTile;
  const int Mt = left < kTile ? (int)left : kTile;
  int Np = 1;
  while (Np < Mt) Np <<= 1;
  const int sub = kTile / Np, slot = lane & (Np - 1), unit = wave * sub + lane / Np, units = kWaves * sub;
  const bool active = slot < Mt;
  const int64_t j = (int64_t)blockIdx.x * kTile + (active ? slot : Mt - 1);      // (a lane beyond the tile's observations repeats the last: its partners hold the same slot)
  bool invalid;
  const typename F::Obs o = HeldObs<MODEL>::load(M, ds, j, invalid);
  const int64_t pos = MODEL == AMWG_MODEL_POIS_GLM ? (int64_t)index[ds.off_xb + j] : j;
  const int64_t s_begin = split_begin(S, splits, blockIdx.y), s_end = split_begin(S, splits, (int64_t)blockIdx.y + 1);
  Lse a{-kInf, 0.0};
  bool bad = false;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += kRun) {
    const int L = (int)(s_end - s0 < kRun ? s_end - s0 : kRun);
    __syncthreads();
    if (tid < L) stage[tid] = draw_at<F>(draws, PR, C, cpd, d, s0 + tid, M, ds);
    __syncthreads();
    for (int jb = unit; jb < L; jb += units * R) {
      if (jb + units * (R - 1) < L) {      // a full block: the maximum first, one rescale, R independent exponentials
        double l[R], e[R];
        double mn = a.m;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double t = F::term(M, o, stage[jb + units * r], pos, draws, C);
          l[r] = invalid ? -kInf : t;
          bad = bad || !(__builtin_fabs(l[r]) < kInf);
          mn = l[r] > mn ? l[r] : mn;      // (a NaN term never becomes the maximum; `bad` carries it)
        }
        if (mn != a.m) a.sum = a.sum * waic_exp(a.m - mn);
        a.m = mn;
#pragma unroll
        for (int r = 0; r < R; ++r) e[r] = waic_exp(l[r] - mn);
#pragma unroll
        for (int w = 1; w < R; w <<= 1)
#pragma unroll
          for (int r = 0; r + w < R; r += 2 * w) e[r] = e[r] + e[r + w];
        a.sum = a.sum + e[0];
      } else {                             // the last, short block of a staged run: term by term
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (jb + units * r >= L) break;
          const double t = F::term(M, o, stage[jb + units * r], pos, draws, C);
          const double l = invalid ? -kInf : t;
          bad = bad || !(__builtin_fabs(l) < kInf);
          if (l > a.m) { a.sum = a.sum * waic_exp(a.m - l); a.m = l; }
          a.sum = a.sum + waic_exp(l - a.m);
        }
      }
    }
  }
  if (bad) a.sum = __builtin_nan("");      // (rescales and adds carry it to the finish)
  // the sub lanes of the observation, every wavefront at once (Np is uniform over the workgroup, and all 64 lanes are here)
  if (Np <= 1) a = butterfly_step<1>(a);
  if (Np <= 2) a = butterfly_step<2>(a);
  if (Np <= 4) a = butterfly_step<4>(a);
  if (Np <= 8) a = butterfly_step<8>(a);
  if (Np <= 16) a = butterfly_step<16>(a);
  if (Np <= 32) a = butterfly_step<32>(a);
  __syncthreads();
  if (wave > 0 && lane < Np) wave_part[wave - 1][lane] = a;
  __syncthreads();
  if (wave != 0 || lane >= Mt) return;      // (lane < Mt: the lane is its own slot, and the slot holds an observation)
#pragma unroll
  for (int w = 1; w < kWaves; ++w) a = lse_merge(a, wave_part[w - 1][lane]);
  parts[part_off[blockIdx.z] + (int64_t)blockIdx.y * m + j] = a;
}

// out[d * out_stride + j] = lppd_j for j < m_d.  A WAVEFRONT per observation: with few observations a thread per observation would walk up to 2 048 splits alone
// (a trace at m = 1 showed that walk taking five times the partial kernel).  Lane k merges the splits k, k + 64, ... in ascending order, then the 64 lanes merge by
// the butterfly of the partial kernel: a fixed tree, a function of the split count alone
__global__ void __launch_bounds__(kThreads) heldout_finish_kernel(int64_t rows, int64_t cpd, int d0, const WaicDataset *__restrict__ sets, const int64_t *__restrict__ part_off,
                                                                  const Lse *__restrict__ parts, double *__restrict__ out, int64_t out_stride) {
  const int d = d0 + (int)blockIdx.y;
  const int64_t m = sets[d].n_obs, S = rows * cpd, splits = heldout_splits(S, m);
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (j >= m) return;      // (uniform over the wavefront)
  const Lse *p = parts + part_off[blockIdx.y] + j;
  Lse a{-kInf, 0.0};
  for (int64_t k = lane; k < splits; k += 64) a = lse_merge(a, p[k * m]);
  a = butterfly_step<1>(a); a = butterfly_step<2>(a); a = butterfly_step<4>(a); a = butterfly_step<8>(a); a = butterfly_step<16>(a); a = butterfly_step<32>(a);
  if (lane != 0) return;
  double lppd = a.m + log_v8(a.sum) - log_v8((double)S);
  if (!(__builtin_fabs(lppd) < kInf)) lppd = __builtin_nan("");
  out[d * out_stride + j] = lppd;
}

template <int... MODEL> const void *partial_fn(PointwiseModels<MODEL...>, int model) {
  const void *const fn[] = {reinterpret_cast<const void *>(&heldout_partial_kernel<MODEL>)...};
  return fn[model - AMWG_MODEL_NORMAL];
}

// one array of every dataset back to back on 256-byte boundaries, as amwg_create.hip lays the sampler's (upload_datasets); off[d] in elements
template <class T, class Fill> int pack(int D, const amwg_model_desc *held, size_t per_obs, Fill fill, std::vector<int64_t> &off, DevBuf &dev, hipStream_t stream, std::vector<T> &host) {
  constexpr size_t align = 256 / sizeof(T);
  size_t total = 0;
  off.assign((size_t)D, 0);
  for (int d = 0; d < D; ++d) { off[(size_t)d] = (int64_t)total; total += ((size_t)held[d].n_obs * per_obs + align - 1) / align * align; }
  host.assign(total ? total : 1, T(0));
  for (int d = 0; d < D; ++d) fill(d, host.data() + off[(size_t)d]);
  HIP_TRY(dev.alloc(host.size() * sizeof(T)));
  HIP_TRY(hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, stream));      // (`host` outlives the stream's drain: the caller's)
  return AMWG_OK;
}

}  // namespace

int amwg_heldout_validate(const char *call, int model, int G, int K, int D, const amwg_model_desc *held, const int32_t *index) {
  if (model < AMWG_MODEL_NORMAL || model > AMWG_MODEL_POIS_GLM) return amwg_fail(AMWG_EINVAL, "%s: unknown model %d", call, model);
  if (model == AMWG_MODEL_HIER_NORMAL && D != 1) return amwg_fail(AMWG_EINVAL, "%s: the hierarchical family runs on one dataset", call);
  for (int d = 0; d < D; ++d) {
    const amwg_model_desc &h = held[d];
    if (h.model != model) return amwg_fail(AMWG_EINVAL, "%s: held-out dataset %d is of model %d, the sampler's is %d", call, d, h.model, model);
    if (h.K != K || h.G != G) return amwg_fail(AMWG_EINVAL, "%s: held-out dataset %d has K = %d, G = %d, the sampler has K = %d, G = %d", call, d, h.K, h.G, K, G);
    if (h.n_obs < 0) return amwg_fail(AMWG_EINVAL, "%s: held-out dataset %d: n_obs < 0", call, d);
    if (h.n_obs > 0 && !h.x) return amwg_fail(AMWG_EINVAL, "%s: held-out dataset %d: a null x", call, d);
    if (model == AMWG_MODEL_POIS_GLM && h.n_obs > 0 && !h.y) return amwg_fail(AMWG_EINVAL, "%s: held-out dataset %d: the Poisson family needs y", call, d);
    if (model == AMWG_MODEL_HIER_NORMAL) {
      if (h.n_obs > 0 && !h.g) return amwg_fail(AMWG_EINVAL, "%s: held-out dataset %d: the hierarchical family needs g", call, d);
      for (int i = 0; i < h.n_obs; ++i)
        if (h.g[i] < 0 || h.g[i] >= G) return amwg_fail(AMWG_EINVAL, "%s: held-out dataset %d: label g[%d] = %d outside 0..%d", call, d, i, h.g[i], G - 1);
    }
    if (index) {      // (read by the Poisson family alone)
      for (int i = 0; i < h.n_obs; ++i)
        if (model == AMWG_MODEL_POIS_GLM && index[i] < 0) return amwg_fail(AMWG_EINVAL, "%s: held-out dataset %d: index[%d] = %d is negative (a position in the original series)", call, d, i, index[i]);
      index += h.n_obs;
    }
  }
  return AMWG_OK;
}

void amwg_heldout_totals(const double *lppd, int64_t m, double *summary) {
  double elpd = 0.0;
  for (int64_t j = 0; j < m; ++j) elpd += lppd[j];
  const double centre = elpd / (double)m;
  double ss = 0.0;
  for (int64_t j = 0; j < m; ++j) { const double e = lppd[j] - centre; ss += e * e; }
  summary[0] = elpd;
  summary[1] = m < 2 ? (double)NAN : std::sqrt((double)m * ss / (double)(m - 1));
}

int amwg_heldout_pack(const WaicModel &base, int D, const amwg_model_desc *held, const int32_t *index, hipStream_t stream, HeldArrays &h) {
  const int model = base.model;
  WaicModel &M = h.M;
  M = base;
  M.x = M.y = M.lfact = nullptr; M.xb = M.invalid = nullptr;
  std::vector<WaicDataset> &sets = h.sets;
  sets.assign((size_t)D, WaicDataset{});
  std::vector<int64_t> off;
  std::vector<double> &hx = h.hx, &hy = h.hy, &hlf = h.hlf;
  std::vector<uint8_t> &hxb = h.hxb, &hbad = h.hbad;
  std::vector<int32_t> &hidx = h.hidx;
  DevBuf &dx = h.dx, &dy = h.dy, &dlf = h.dlf, &dxb = h.dxb, &dbad = h.dbad, &didx = h.didx;
  int64_t &m_max = h.m_max;
  m_max = 0;
  for (int d = 0; d < D; ++d) { sets[(size_t)d] = WaicDataset{held[d].n_obs, 1, 0, 0, 0, 0}; m_max = held[d].n_obs > m_max ? held[d].n_obs : m_max; }
  if (model == AMWG_MODEL_NORMAL || model == AMWG_MODEL_HIER_NORMAL) {
    TRYB(pack<double>(D, held, 1, [&](int d, double *dst) { for (int i = 0; i < held[d].n_obs; ++i) dst[i] = held[d].x[i]; }, off, dx, stream, hx));
    for (int d = 0; d < D; ++d) {
      sets[(size_t)d].off_x = off[(size_t)d];
      bool mid = true;      // (the division by an invariant is the IEEE quotient wherever its condition holds: the condition is asked of the held-out values)
      for (int i = 0; i < held[d].n_obs; ++i) mid = mid && (held[d].x[i] == 0.0 || mid_range(std::fabs(held[d].x[i])));
      sets[(size_t)d].data_mid_range = mid ? 1 : 0;
    }
    M.x = dx.as<double>();
    if (model == AMWG_MODEL_HIER_NORMAL) {
      TRYB(pack<uint8_t>(D, held, 1, [&](int d, uint8_t *dst) { for (int i = 0; i < held[d].n_obs; ++i) dst[i] = (uint8_t)held[d].g[i]; }, off, dxb, stream, hxb));
      for (int d = 0; d < D; ++d) sets[(size_t)d].off_xb = off[(size_t)d];
      M.xb = dxb.as<uint8_t>();
    }
  } else if (model == AMWG_MODEL_BETA_BERN) {
    TRYB(pack<uint8_t>(D, held, 1, [&](int d, uint8_t *dst) { for (int i = 0; i < held[d].n_obs; ++i) dst[i] = held[d].x[i] == 1 ? 1 : 0; }, off, dxb, stream, hxb));
    TRYB(pack<uint8_t>(D, held, 1, [&](int d, uint8_t *dst) { for (int i = 0; i < held[d].n_obs; ++i) dst[i] = !(held[d].x[i] == 1 || held[d].x[i] == 0); }, off, dbad, stream, hbad));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_xb = off[(size_t)d];
    M.xb = dxb.as<uint8_t>(); M.invalid = dbad.as<uint8_t>();
  } else {      // the Poisson family: X column-major [7][m_d], the counts, lfactorial of the counts (+inf for a negative one) as amwg_create.hip forms it, the positions
    TRYB(pack<double>(D, held, 7, [&](int d, double *dst) { const int N = held[d].n_obs; for (int i = 0; i < N; ++i) for (int k = 0; k < 7; ++k) dst[(size_t)k * N + i] = held[d].x[(size_t)i * 7 + k]; }, off, dx, stream, hx));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_x = off[(size_t)d];
    TRYB(pack<double>(D, held, 1, [&](int d, double *dst) { for (int i = 0; i < held[d].n_obs; ++i) dst[i] = held[d].y[i]; }, off, dy, stream, hy));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_y = off[(size_t)d];
    TRYB(pack<double>(D, held, 1, [&](int d, double *dst) { for (int i = 0; i < held[d].n_obs; ++i) dst[i] = held[d].y[i] < 0 ? (double)INFINITY : lfactorial_js(held[d].y[i]); }, off, dlf, stream, hlf));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_lfact = off[(size_t)d];
    std::vector<int64_t> before((size_t)D, 0);
    for (int d = 1; d < D; ++d) before[(size_t)d] = before[(size_t)d - 1] + held[d - 1].n_obs;
    TRYB(pack<int32_t>(D, held, 1, [&](int d, int32_t *dst) { for (int i = 0; i < held[d].n_obs; ++i) dst[i] = index ? index[before[(size_t)d] + i] : i; }, off, didx, stream, hidx));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_xb = off[(size_t)d];
    M.x = dx.as<double>(); M.y = dy.as<double>(); M.lfact = dlf.as<double>();
  }
  h.index = didx.as<int32_t>();
  return AMWG_OK;
}

int amwg_heldout_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &base, const amwg_model_desc *held, const int32_t *index,
                        double *summary, double *pointwise, size_t scratch_bytes, hipStream_t stream) {
  int64_t cpd = C / D;      // (not const: the args[] list points at it)
  const int64_t S = rows * cpd;
  // ---- the held-out data as the family reads the sampler's own
  HeldArrays h;
  TRYB(amwg_heldout_pack(base, D, held, index, stream, h));
  const int model = base.model;
  WaicModel M = h.M;
  const std::vector<WaicDataset> &sets = h.sets;
  const int64_t m_max = h.m_max;
  const int32_t *d_index = h.index;
  // ---- the outputs, and the batches under the budget: 16 bytes per (split, observation)
  DevBuf d_sets, d_pw, d_off, d_parts;
  HIP_TRY(d_sets.alloc((size_t)D * sizeof(WaicDataset)));
  HIP_TRY(hipMemcpyAsync(d_sets.p, sets.data(), (size_t)D * sizeof(WaicDataset), hipMemcpyHostToDevice, stream));
  const size_t pw_count = (size_t)D * (size_t)m_max;
  HIP_TRY(d_pw.alloc(pw_count * 8));
  HIP_TRY(amwg_pointwise_fill_nan(d_pw.as<double>(), (int64_t)pw_count, stream));
  const size_t budget = scratch_bytes ? scratch_bytes : kPointwiseScratchBytes;
  struct Batch { int d0, d1; int64_t tiles, splits, m_most; };
  constexpr int kMaxGridYZ = 65535;
  std::vector<Batch> batches;
  std::vector<int64_t> part_off((size_t)D, 0);
  int64_t most_parts = 0, prt = 0;
  Batch b{0, 0, 0, 0, 0};
  for (int d = 0; d < D; ++d) {
    const int64_t m = held[d].n_obs, np = heldout_splits(S, m) * m;
    if ((prt && (size_t)(prt + np) * sizeof(Lse) > budget) || d - b.d0 >= kMaxGridYZ) { b.d1 = d; batches.push_back(b); b = Batch{d, d, 0, 0, 0}; prt = 0; }      // (the batch's datasets are a grid dimension)
    part_off[(size_t)d] = prt;
    prt += np;
    const int64_t t = (m + kTile - 1) / kTile, sp = heldout_splits(S, m);
    b.tiles = t > b.tiles ? t : b.tiles; b.splits = sp > b.splits ? sp : b.splits; b.m_most = m > b.m_most ? m : b.m_most;
    most_parts = prt > most_parts ? prt : most_parts;
  }
  b.d1 = D;
  batches.push_back(b);
  HIP_TRY(d_off.alloc((size_t)D * 8));
  HIP_TRY(hipMemcpyAsync(d_off.p, part_off.data(), (size_t)D * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(d_parts.alloc((size_t)most_parts * sizeof(Lse)));
  const WaicDataset *sets_dev = d_sets.as<WaicDataset>();
  Lse *parts = d_parts.as<Lse>();
  double *out = d_pw.as<double>();
  const void *fn = partial_fn(BuiltinModels{}, model);
  for (const Batch &bt : batches) {
    if (bt.tiles == 0) continue;
    int d0 = bt.d0;
    const int64_t *off_dev = d_off.as<int64_t>() + d0;
    void *args[] = {&draws, &rows, &PR, &C, &cpd, &d0, &M, &sets_dev, &d_index, &off_dev, &parts};
    (void)hipLaunchKernel(fn, dim3((unsigned)bt.tiles, (unsigned)bt.splits, (unsigned)(bt.d1 - d0)), dim3(kThreads), args, 0, stream);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(heldout_finish_kernel, dim3((unsigned)((bt.m_most + kWaves - 1) / kWaves), (unsigned)(bt.d1 - d0)), dim3(kThreads), 0, stream, rows, cpd, d0, sets_dev,
                       off_dev, parts, out, m_max);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch and the held-out arrays are freed on return)
  std::vector<double> own;
  double *pw = pointwise;
  if (!pw) { own.resize(pw_count ? pw_count : 1); pw = own.data(); }
  if (pw_count) HIP_TRY(hipMemcpy(pw, d_pw.p, pw_count * 8, hipMemcpyDeviceToHost));
  for (int d = 0; d < D; ++d) amwg_heldout_totals(pw + (size_t)d * (size_t)m_max, held[d].n_obs, summary + (size_t)d * 2);
  return AMWG_OK;
}

extern "C" int amwg_last_sample_dataset_heldout(amwg_sampler *s, const amwg_model_desc *held, const int32_t *index, double *summary, double *pointwise) {
  static const char *call = "amwg_last_sample_dataset_heldout";
  if (!s || !held || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (s->user) return amwg_fail(AMWG_EINVAL, "%s: built-in families only: the data lengths of a translated closure are part of its compiled text", call);
  TRYB(amwg_need_stored_draws(s, call));
  const int D = s->n_datasets, PR = s->P + s->D;
  TRYB(amwg_waic_shape(call, s->last_rows, PR, s->C, D));
  if (s->mc.group_local) return amwg_fail(AMWG_EINVAL, "%s: a group_local sampler keeps its observations as a lane-major tile; the pointwise terms need them in index order", call);
  TRYB(amwg_heldout_validate(call, s->model, s->d.G, s->d.K, D, held, index));
  WaicModel base{};
  base.model = s->model; base.G = s->d.G; base.exact_division = s->mc.exact_division;
  base.neg_half_log_2pi = s->mc.neg_half_log_2pi;
  PointwiseLaunch K;
  TRYB(amwg_pointwise_family(call, base, PR, D, K));      // (the components a draw must hold)
  HIP_TRY(hipSetDevice(s->device));
  return amwg_heldout_launch(call, s->last_draws, s->last_rows, PR, s->C, D, base, held, index, summary, pointwise, 0, s->stream);
}
