// amwg_summaries.hip -- posterior quantiles on the device (part of libamwg.so; separate translation unit because
// the rocPRIM/hipCUB sort templates are slow to compile).  The reference's users compute these in R on the returned
// arrays (tests/test_mcmc_js.R); with 10^5 chains the draws are better summarised where they are.
// Pooled over all chains: gather + radix sort (amwg_last_sample_quantiles).  Per dataset of a dataset sampler: a radix select in place
// (amwg_last_sample_dataset_quantiles, at the end of this file).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>

#include "amwg_dataset_quantiles.h"
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_sampler.h"
#include "amwg_select.h"

namespace {

// draws [row][PR][C] -> contiguous values of one recorded component
__global__ void gather_component_kernel(const double *draws, int64_t rows, int PR, int64_t C, int p, double *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C) return;
  out[i] = draws[((i / C) * PR + p) * C + (i % C)];
}

// R's default quantile (type 7): h = (n-1) q; x[floor h] + (h - floor h) (x[floor h + 1] - x[floor h])
__global__ void pick_quantiles_kernel(const double *sorted, int64_t n, const double *probs, int n_probs, double *out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_probs) return;
  const double q = probs[k];
  if (!(q >= 0.0 && q <= 1.0)) { out[k] = __builtin_nan(""); return; }
  const double h = (double)(n - 1) * q;
  const int64_t lo = (int64_t)floor(h);
  const int64_t hi = lo + 1 < n ? lo + 1 : lo;
  out[k] = sorted[lo] + (h - (double)lo) * (sorted[hi] - sorted[lo]);
}

}  // namespace

extern "C" int amwg_last_sample_quantiles(amwg_sampler *s, const double *probs, int32_t n_probs, double *out) {
  if (!s || !probs || !out || n_probs < 1) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_quantiles: bad argument");
  TRYB(amwg_refuse_pooled(s, "amwg_last_sample_quantiles"));
  TRYB(amwg_refuse_summarised(s, "amwg_last_sample_quantiles"));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_quantiles: no sample() call yet");
  const int PR = s->P + s->D;
  const int64_t n = s->last_rows * s->C;
  if (n > 2147483647) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_quantiles: more than 2^31 values per component");      // (the sort counts in int)
  DevBuf vals, sorted, dprobs, dout, tmp;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(vals.alloc((size_t)n * 8));
  HIP_TRY(sorted.alloc((size_t)n * 8));
  HIP_TRY(dprobs.alloc((size_t)n_probs * 8));
  HIP_TRY(dout.alloc((size_t)n_probs * 8));
  HIP_TRY(hipMemcpyAsync(dprobs.p, probs, (size_t)n_probs * 8, hipMemcpyHostToDevice, s->stream));
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, vals.as<double>(), sorted.as<double>(), (int)n, 0, 64, s->stream));
  HIP_TRY(tmp.alloc(tmp_bytes));
  for (int p = 0; p < PR; ++p) {
    hipLaunchKernelGGL(gather_component_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->last_draws, s->last_rows, PR, s->C, p, vals.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp.p, tmp_bytes, vals.as<double>(), sorted.as<double>(), (int)n, 0, 64, s->stream));
    hipLaunchKernelGGL(pick_quantiles_kernel, dim3((unsigned)((n_probs + 63) / 64)), dim3(64), 0, s->stream, sorted.as<double>(), n, dprobs.as<double>(), n_probs, dout.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out + (size_t)p * n_probs, dout.p, (size_t)n_probs * 8, hipMemcpyDeviceToHost, s->stream));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMWG_OK;
}

// ---- a dataset sampler (amwg_create_datasets): quantiles per dataset.  A dataset's values of one recorded component are `rows` runs of cpd doubles inside
// draws [row][PR][C], and a caller wants a handful of order statistics of each of the D x PR segments: a radix SELECT, most significant digit first, reads them
// where they lie and sorts nothing.  One workgroup per (recorded value p, dataset d), the launch shape of dataset_moments_kernel (amwg_diag.hip); eight passes
// of 8-bit digits over the monotone u64 key of the fp64 pattern.  All ranks wanted (the distinct lo and hi of R's type-7 rule, as in pick_quantiles_kernel)
// travel through the passes together: ranks that still share a key prefix form a GROUP with one 256-bin histogram in LDS over the elements under that prefix;
// after a pass each rank takes the bin that holds it, groups split, and after the eighth pass a group's prefix is the key of its ranks.
namespace {

constexpr int kSelThreads = 512;            // 8 wavefronts.  At 40 VGPRs the registers allow four workgroups per CU; LDS (1 832 B + 1 KB per rank) allows four
                                            // up to 38 ranks and three at the 48 ranks of a full launch (50 984 B of 160 KB)
constexpr int kSelProbs = 24;               // probabilities per launch: <= 48 ranks = 48 KB of histograms (the host chunks longer lists)
constexpr int kSelRanks = 2 * kSelProbs;
constexpr int kSelLoads = 4;                // elements a thread has in flight

// (select_key, select_value, wave_count and select_scan: amwg_select.h, shared with the thresholds of amwg_hpd.hip)

// out[d][p][k0 + k] for k < kc <= kSelProbs; dynamic LDS: 2 kc histograms of 256 u32
__global__ void __launch_bounds__(kSelThreads) dataset_select_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd,
                                                                     const double *__restrict__ probs, int n_probs, int k0, int kc, double *__restrict__ out) {
  extern __shared__ uint32_t hist[];                   // [groups][256]: counts, then their exclusive scan
  __shared__ uint32_t cand[kSelRanks];                 // rank wanted by (probability k, lo | hi) = entry 2k | 2k + 1; ~0u: none (q outside [0, 1])
  __shared__ uint8_t first[kSelRanks], idx[kSelRanks]; // first occurrence of its rank; position of the entry's rank among the distinct ranks, ascending
  __shared__ uint32_t rank[kSelRanks], digit[kSelRanks];      // the distinct ranks, ascending; the digit each took in this pass
  __shared__ int grp[kSelRanks];                       // group of a rank: groups are runs of neighbouring ranks, prefixes ascending
  __shared__ uint64_t gprefix[kSelRanks];              // the digits a group's ranks have taken so far
  __shared__ uint32_t gbase[kSelRanks];                // elements whose key prefix is smaller than the group's
  __shared__ double val[kSelRanks];
  __shared__ int sR, sG;
  const int p = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t n = (uint32_t)(rows * cpd), cpd32 = (uint32_t)cpd;      // n <= 2^31 - 1 (the host refuses more)
  const double *col = draws + (int64_t)p * C + (int64_t)d * cpd;
  const int64_t row_stride = (int64_t)PR * C;

  // the ranks: h = (n - 1) q, lo = floor h, hi = min(lo + 1, n - 1)
  double q = 0, h = 0;
  int64_t lo = 0;
  bool valid = false;
  uint32_t want = ~0u;
  if (tid < 2 * kc) {
    q = probs[k0 + (tid >> 1)];
    valid = q >= 0.0 && q <= 1.0;
    h = (double)((int64_t)n - 1) * q;
    lo = valid ? (int64_t)floor(h) : 0;
    const int64_t hi = lo + 1 < (int64_t)n ? lo + 1 : lo;
    if (valid) want = (uint32_t)((tid & 1) ? hi : lo);
    cand[tid] = want;
  }
  __syncthreads();
  if (tid < 2 * kc) {
    bool f = valid;
    for (int t = 0; t < tid; ++t) f = f && cand[t] != want;
    first[tid] = f;
  }
  __syncthreads();
  if (tid < 2 * kc && valid) {
    int pos = 0;
    for (int t = 0; t < 2 * kc; ++t) pos += (first[t] && cand[t] < want) ? 1 : 0;
    idx[tid] = (uint8_t)pos;
    if (first[tid]) { rank[pos] = want; grp[pos] = 0; }
  }
  if (tid == 0) {
    int r = 0;
    for (int t = 0; t < 2 * kc; ++t) r += first[t];
    sR = r;
    sG = 1;
    gprefix[0] = 0;
    gbase[0] = 0;
  }
  __syncthreads();
  const int R = sR;

  for (int pass = 0; pass < 8 && R > 0; ++pass) {
    const int G = sG, shift = 56 - 8 * pass;
    for (int i = tid; i < G * 256; i += kSelThreads) hist[i] = 0;
    __syncthreads();
    // histograms: consecutive lanes read consecutive columns of a run
    for (uint32_t base = 0; base < n; base += kSelLoads * kSelThreads) {
      uint64_t key[kSelLoads];
      bool act[kSelLoads];
#pragma unroll
      for (int u = 0; u < kSelLoads; ++u) {
        const uint32_t i = base + (uint32_t)(u * kSelThreads + tid);
        act[u] = i < n;
        key[u] = 0;
        if (act[u]) { const uint32_t r = i / cpd32; key[u] = select_key(col[(int64_t)r * row_stride + (i - r * cpd32)]); }
      }
#pragma unroll
      for (int u = 0; u < kSelLoads; ++u) {
        const uint64_t hp = pass ? key[u] >> (shift + 8) : 0;
        int a = 0, b = G;                              // the first group whose prefix is >= hp
        while (a < b) { const int m = (a + b) >> 1; if (gprefix[m] < hp) a = m + 1; else b = m; }
        const bool in_group = act[u] && a < G && gprefix[a] == hp;
        wave_count(hist, in_group, (uint32_t)a * 256u + (uint32_t)((key[u] >> shift) & 255u));
      }
    }
    __syncthreads();
    // exclusive scan of each group's bins, a wavefront per group, four bins per lane
    for (int g = wave; g < G; g += kSelThreads / 64) select_scan(hist + g * 256, lane);
    __syncthreads();
    // each rank takes the bin that holds it: the last bin whose exclusive count is <= the rank's position inside its group
    uint64_t new_prefix = 0;
    uint32_t new_base = 0;
    if (tid < R) {
      const int g = grp[tid];
      const uint32_t *hb = hist + g * 256, t = rank[tid] - gbase[g];
      int a = 0, b = 255;
      while (a < b) { const int m = (a + b + 1) >> 1; if (hb[m] <= t) a = m; else b = m - 1; }
      digit[tid] = (uint32_t)a;
      new_prefix = (gprefix[g] << 8) | (uint64_t)a;
      new_base = gbase[g] + hb[a];
    }
    __syncthreads();
    // groups split where neighbouring ranks took different digits (kSelRanks <= 64: the first wavefront holds every rank)
    bool head = false;
    int new_group = 0;
    uint64_t heads = 0;
    if (wave == 0) {
      head = tid < R && (tid == 0 || grp[tid] != grp[tid - 1] || digit[tid] != digit[tid - 1]);
      heads = __ballot(head);
      new_group = __popcll(heads & ((2ull << lane) - 1ull)) - 1;
    }
    __syncthreads();
    if (tid < R) {
      grp[tid] = new_group;
      if (head) { gprefix[new_group] = new_prefix; gbase[new_group] = new_base; }
    }
    if (tid == 0) sG = __popcll(heads);
    __syncthreads();
  }

  if (tid < R) val[tid] = select_value(gprefix[grp[tid]]);
  __syncthreads();
  if (tid < 2 * kc && !(tid & 1)) {
    double r = __builtin_nan("");
    if (valid) { const double xlo = val[idx[tid]], xhi = val[idx[tid + 1]]; r = xlo + (h - (double)lo) * (xhi - xlo); }
    out[((size_t)d * PR + p) * (size_t)n_probs + (size_t)(k0 + (tid >> 1))] = r;
  }
}

}  // namespace

int amwg_dataset_quantiles_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int n_probs) {
  if (n_probs < 1 || rows < 1 || PR < 1 || C < 1 || D < 1 || D > 65535 || C % D != 0)
    return amwg_fail(AMWG_EINVAL, "%s: bad shape (rows %lld, values %d, chains %lld, datasets %d -- at most 65535, dividing the chains --, probabilities %d)", call, (long long)rows, PR, (long long)C, D, n_probs);
  if (rows > 2147483647 / (C / D)) return amwg_fail(AMWG_EINVAL, "%s: more than 2^31 - 1 values per dataset and component", call);
  return AMWG_OK;
}

int amwg_dataset_quantiles_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const double *probs, int n_probs, double *out,
                                  hipStream_t stream) {
  static_assert(kSelRanks <= 64, "the regrouping step holds every rank in one wavefront");
  if (!draws || !probs || !out) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_dataset_quantiles_shape(call, rows, PR, C, D, n_probs));
  const int64_t cpd = C / D;
  const size_t n_out = (size_t)D * (size_t)PR * (size_t)n_probs;
  DevBuf dprobs, dout;
  HIP_TRY(dprobs.alloc((size_t)n_probs * 8));
  HIP_TRY(dout.alloc(n_out * 8));
  HIP_TRY(hipMemcpyAsync(dprobs.p, probs, (size_t)n_probs * 8, hipMemcpyHostToDevice, stream));
  for (int k0 = 0; k0 < n_probs; k0 += kSelProbs) {
    const int kc = n_probs - k0 < kSelProbs ? n_probs - k0 : kSelProbs;
    hipLaunchKernelGGL(dataset_select_kernel, dim3((unsigned)PR, (unsigned)D), dim3(kSelThreads), (size_t)(2 * kc) * 256 * sizeof(uint32_t), stream, draws, rows, PR, C, cpd,
                       dprobs.as<double>(), n_probs, k0, kc, dout.as<double>());
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(out, dout.p, n_out * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return AMWG_OK;
}

extern "C" int amwg_last_sample_dataset_quantiles(amwg_sampler *s, const double *probs, int32_t n_probs, double *out) {
  if (!s || !probs || !out || n_probs < 1) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_dataset_quantiles: bad argument");
  TRYB(amwg_refuse_summarised(s, "amwg_last_sample_dataset_quantiles"));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_dataset_quantiles: no sample() call yet");
  HIP_TRY(hipSetDevice(s->device));
  return amwg_dataset_quantiles_launch("amwg_last_sample_dataset_quantiles", s->last_draws, s->last_rows, s->P + s->D, s->C, s->n_datasets, probs, n_probs, out, s->stream);
}
