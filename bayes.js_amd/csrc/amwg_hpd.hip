// amwg_hpd.hip -- highest-density intervals per dataset on the device (amwg_last_sample_dataset_hpd; part of libamwg.so).  include/amwg.h states the rule,
// amwg_hpd.h the route: per probability the two order statistics t_lo = x_(k-1), t_hi = x_(g) by radix select where the draws lie, the two tails of k keys
// compacted into scratch, each tail sorted by a bitonic network (keys only), and the narrowest of the k widths by a block argmin.  Nothing but the tails is
// gathered or sorted, and the draws stay on the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "amwg_dataset_quantiles.h"
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_hpd.h"
#include "amwg_sampler.h"
#include "amwg_select.h"

namespace {

constexpr int kThrThreads = 512;            // the thresholds: 8 wavefronts per (value, dataset), the geometry of dataset_select_kernel with two ranks
constexpr int kThrLoads = 4;                // elements a thread has in flight
constexpr int kCompThreads = 256, kCompLoads = 16;      // compaction: a workgroup takes 4096 consecutive elements of a slice
constexpr int kSortMaxThreads = 1024;       // the LDS sort: a thread per pair of keys up to this, then several pairs per thread
constexpr int kStepThreads = 256;           // a global bitonic step and the fill: one element (pair) per thread
constexpr int kArgThreads = 256;
constexpr int64_t kMaxBatch = 16384;        // pairs per batch at most: two tails per pair ride in gridDim.y
constexpr uint64_t kMaxKey = ~0ull;         // the pad.  (Only a NaN pattern has this key, and a slice that holds one answers NaN whatever the sort does.)

// thr[d][p][0 | 1] = key of x_(r_lo) | x_(r_hi) of the slice (value p, dataset d); bad[d][p] = a draw of the slice is NaN or +-inf.  Eight passes of 8-bit digits,
// most significant first.  Each rank carries the digits it has taken and the count of keys below that prefix; while both ranks share a prefix (G = 1) one
// histogram serves both, afterwards each has its own over the elements under its prefix.
__global__ void __launch_bounds__(kThrThreads) hpd_threshold_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, uint32_t r_lo, uint32_t r_hi,
                                                                    uint64_t *__restrict__ thr, uint32_t *__restrict__ bad) {
  __shared__ uint32_t hist[2 * 256];
  __shared__ uint64_t prefix[2];
  __shared__ uint32_t below[2];
  __shared__ int s_bad;
  const int p = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t n = (uint32_t)(rows * cpd), cpd32 = (uint32_t)cpd;      // n <= 2^31 - 1 (the host refuses more)
  const double *col = draws + (int64_t)p * C + (int64_t)d * cpd;
  const int64_t row_stride = (int64_t)PR * C;
  if (tid < 2) { prefix[tid] = 0; below[tid] = 0; }
  if (tid == 0) s_bad = 0;
  __syncthreads();
  bool non_finite = false;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    const uint64_t pre0 = prefix[0], pre1 = prefix[1];
    const int G = pre0 == pre1 ? 1 : 2;
    hist[tid] = 0;      // (kThrThreads = 2 x 256)
    __syncthreads();
    // histograms: consecutive lanes read consecutive columns of a run
    for (uint32_t base = 0; base < n; base += kThrLoads * kThrThreads) {
      uint64_t key[kThrLoads];
      bool act[kThrLoads];
#pragma unroll
      for (int u = 0; u < kThrLoads; ++u) {
        const uint32_t i = base + (uint32_t)(u * kThrThreads + tid);
        act[u] = i < n;
        key[u] = 0;
        if (act[u]) {
          const uint32_t r = i / cpd32;
          const double v = col[(int64_t)r * row_stride + (i - r * cpd32)];
          if (pass == 0 && (((uint64_t)__double_as_longlong(v) >> 52) & 0x7ffull) == 0x7ffull) non_finite = true;
          key[u] = select_key(v);
        }
      }
#pragma unroll
      for (int u = 0; u < kThrLoads; ++u) {
        const uint64_t hp = pass ? key[u] >> (shift + 8) : 0;
        const int a = hp == pre0 ? 0 : 1;
        const bool in_group = act[u] && (a == 0 || hp == pre1);
        wave_count(hist, in_group, (uint32_t)a * 256u + (uint32_t)((key[u] >> shift) & 255u));
      }
    }
    __syncthreads();
    if (wave < G) select_scan(hist + wave * 256, lane);
    __syncthreads();
    // each rank takes the bin that holds it: the last bin whose exclusive count is <= the rank's position under its prefix
    if (tid < 2) {
      const uint32_t *hb = hist + (G == 1 ? 0 : tid) * 256, t = (tid ? r_hi : r_lo) - below[tid];
      int a = 0, b = 255;
      while (a < b) { const int m = (a + b + 1) >> 1; if (hb[m] <= t) a = m; else b = m - 1; }
      prefix[tid] = (prefix[tid] << 8) | (uint64_t)a;
      below[tid] += hb[a];
    }
    if (pass == 0 && non_finite) s_bad = 1;
    __syncthreads();
  }
  const size_t pair = (size_t)d * PR + p;
  if (tid < 2) thr[pair * 2 + tid] = prefix[tid];
  if (tid == 0) bad[pair] = (uint32_t)s_bad;
}

// dst[cursor ..] takes the keys of the lanes with `take`, one atomic per wavefront: the first such lane moves the cursor by their number.  Called by whole
// wavefronts.  A position at or past `cap` is not written (the thresholds guarantee fewer than cap takers; the guard keeps a wrong count inside the scratch).
__device__ inline void hpd_push(uint64_t *dst, uint32_t *cursor, uint32_t cap, bool take, uint64_t key) {
  const uint64_t m = __ballot(take);
  if (!m) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((unsigned long long)m) - 1;
  uint32_t start = 0;
  if (lane == leader) start = atomicAdd(cursor, (uint32_t)__popcll(m));
  start = __shfl(start, leader);
  if (take) {
    const uint32_t pos = start + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < cap) dst[pos] = key;
  }
}

// scratch [pair of the batch][lo | hi][npad]; cursors [pair of the batch][lo | hi], zero at the start.  Grid (chunks of a slice, pairs of the batch).
__global__ void __launch_bounds__(kCompThreads) hpd_compact_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd, size_t pair0,
                                                                   const uint64_t *__restrict__ thr, uint32_t k, uint32_t npad, uint64_t *__restrict__ scratch,
                                                                   uint32_t *__restrict__ cursors) {
  const size_t pair = pair0 + blockIdx.y;
  const int p = (int)(pair % (size_t)PR), tid = threadIdx.x;
  const int64_t d = (int64_t)(pair / (size_t)PR);
  const uint32_t n = (uint32_t)(rows * cpd), cpd32 = (uint32_t)cpd;
  const double *col = draws + (int64_t)p * C + d * cpd;
  const int64_t row_stride = (int64_t)PR * C;
  const uint64_t k_lo = thr[pair * 2], k_hi = thr[pair * 2 + 1];
  uint64_t *lo = scratch + (size_t)blockIdx.y * 2 * npad, *hi = lo + npad;
  uint32_t *cur = cursors + (size_t)blockIdx.y * 2;
  const uint64_t first = (uint64_t)blockIdx.x * (kCompLoads * kCompThreads);
#pragma unroll 4
  for (int u = 0; u < kCompLoads; ++u) {
    const uint64_t i64 = first + (uint64_t)(u * kCompThreads + tid);
    const bool act = i64 < n;
    uint64_t key = 0;
    if (act) { const uint32_t i = (uint32_t)i64, r = i / cpd32; key = select_key(col[(int64_t)r * row_stride + (i - r * cpd32)]); }
    hpd_push(lo, cur, k, act && key < k_lo, key);
    hpd_push(hi, cur + 1, k, act && key > k_hi, key);
  }
}

// what the cursors left open: copies of the tail's threshold up to k, maximal keys up to npad.  Grid (npad / kStepThreads rounded up, 2 x pairs of the batch).
__global__ void __launch_bounds__(kStepThreads) hpd_fill_kernel(size_t pair0, const uint64_t *__restrict__ thr, const uint32_t *__restrict__ cursors, uint32_t k, uint32_t npad,
                                                                uint64_t *__restrict__ scratch) {
  const uint64_t i = (uint64_t)blockIdx.x * kStepThreads + threadIdx.x;
  if (i >= npad) return;
  const uint32_t taken = cursors[blockIdx.y] < k ? cursors[blockIdx.y] : k;
  if (i < taken) return;
  scratch[(size_t)blockIdx.y * npad + i] = i < k ? thr[(pair0 + (blockIdx.y >> 1)) * 2 + (blockIdx.y & 1)] : kMaxKey;
}

// The steps (kk, j) of the bitonic network whose partner distance j is below `chunk`, for kk = kk_lo .. kk_hi, on `chunk` keys held in LDS: element i of a tail
// is compared with i ^ j, ascending where (i & kk) == 0.  With chunk = npad, kk_lo = 2, kk_hi = npad this is the whole sort.  chunk and npad are powers of two,
// chunk <= npad.  Grid (npad / chunk, 2 x pairs of the batch); dynamic LDS chunk x 8 bytes.
__global__ void __launch_bounds__(kSortMaxThreads) hpd_bitonic_lds_kernel(uint64_t *__restrict__ scratch, uint32_t npad, uint32_t chunk, uint64_t kk_lo, uint64_t kk_hi) {
  extern __shared__ uint64_t keys[];
  const uint32_t tid = threadIdx.x, T = blockDim.x, first = blockIdx.x * chunk;
  uint64_t *a = scratch + (size_t)blockIdx.y * npad + first;
  for (uint32_t i = tid; i < chunk; i += T) keys[i] = a[i];
  __syncthreads();
  for (uint64_t kk = kk_lo; kk <= kk_hi; kk <<= 1) {
    for (uint32_t j = (uint32_t)((kk >> 1) < (uint64_t)(chunk >> 1) ? (kk >> 1) : (uint64_t)(chunk >> 1)); j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (chunk >> 1); t += T) {
        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
        const bool up = (((uint64_t)first + i) & kk) == 0;
        const uint64_t x = keys[i], y = keys[l];
        if ((x > y) == up) { keys[i] = y; keys[l] = x; }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < chunk; i += T) a[i] = keys[i];
}

// one step (kk, j) with j >= the LDS chunk, in global memory.  Grid (npad / 2 / kStepThreads rounded up, 2 x pairs of the batch).
__global__ void __launch_bounds__(kStepThreads) hpd_bitonic_step_kernel(uint64_t *__restrict__ scratch, uint32_t npad, uint64_t kk, uint32_t j) {
  const uint64_t t64 = (uint64_t)blockIdx.x * kStepThreads + threadIdx.x;
  if (t64 >= (npad >> 1)) return;
  const uint32_t t = (uint32_t)t64, i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
  uint64_t *a = scratch + (size_t)blockIdx.y * npad;
  const bool up = ((uint64_t)i & kk) == 0;
  const uint64_t x = a[i], y = a[l];
  if ((x > y) == up) { a[i] = y; a[l] = x; }
}

// res[pair][0 | 1] = (x_(i*), x_(i* + g)): i* the smallest i < k whose w_i = value(hi[i]) - value(lo[i]) is minimal; (NaN, NaN) for a slice with a non-finite draw.
// A thread meets its i in ascending order and keeps the first of equal widths; the tree keeps the smaller i of equal widths.  One workgroup per pair.
__global__ void __launch_bounds__(kArgThreads) hpd_argmin_kernel(const uint64_t *__restrict__ scratch, uint32_t k, uint32_t npad, size_t pair0, const uint32_t *__restrict__ bad,
                                                                 double *__restrict__ res) {
  __shared__ double sw[kArgThreads];
  __shared__ uint32_t si[kArgThreads];
  const int tid = threadIdx.x;
  const size_t pair = pair0 + blockIdx.x;
  const uint64_t *lo = scratch + (size_t)blockIdx.x * 2 * npad, *hi = lo + npad;
  double bw = 0.0;
  uint32_t bi = ~0u;      // ~0u: none yet
  for (uint32_t i = tid; i < k; i += kArgThreads) {
    const double w = select_value(hi[i]) - select_value(lo[i]);
    if (bi == ~0u || w < bw) { bw = w; bi = i; }
  }
  sw[tid] = bw;
  si[tid] = bi;
  __syncthreads();
  for (int o = kArgThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double ow = sw[tid + o];
      const uint32_t oi = si[tid + o];
      if (oi != ~0u && (si[tid] == ~0u || ow < sw[tid] || (ow == sw[tid] && oi < si[tid]))) { sw[tid] = ow; si[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool nan = bad[pair] != 0 || si[0] == ~0u;
    res[pair * 2] = nan ? __builtin_nan("") : select_value(lo[si[0]]);
    res[pair * 2 + 1] = nan ? __builtin_nan("") : select_value(hi[si[0]]);
  }
}

size_t g_budget = kHpdScratchBytes;

uint64_t pow2_at_least(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

struct ProbPlan { bool valid; int64_t g, k; uint64_t npad; int64_t batch; };

}  // namespace

size_t amwg_hpd_set_budget(size_t bytes) {
  const size_t before = g_budget;
  g_budget = bytes ? bytes : kHpdScratchBytes;
  return before;
}

int amwg_hpd_lds_keys(int64_t *keys) {
  int dev = 0, lds = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  if (lds < 1024) return amwg_fail(AMWG_EHIP, "amwg_hpd: the device reports %d bytes of LDS per workgroup", lds);
  int64_t c = 128;
  while (c * 2 * 8 <= (int64_t)lds) c *= 2;
  *keys = c;
  return AMWG_OK;
}

int amwg_hpd_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int n_probs) {
  TRYB(amwg_dataset_quantiles_shape(call, rows, PR, C, D, n_probs));
  if (rows * (C / D) < 2) return amwg_fail(AMWG_EINVAL, "%s: fewer than 2 values per dataset and value (rows %lld, chains per dataset %lld)", call, (long long)rows, (long long)(C / D));
  return AMWG_OK;
}

int amwg_hpd_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const double *probs, int n_probs, double *out, hipStream_t stream) {
  if (!draws || !probs || !out) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_hpd_shape(call, rows, PR, C, D, n_probs));
  const int64_t cpd = C / D, N = rows * cpd;
  const size_t pairs = (size_t)D * (size_t)PR;
  for (size_t i = 0; i < pairs * (size_t)n_probs * 2; ++i) out[i] = __builtin_nan("");
  // the rule's g per probability, and what its tails need
  std::vector<ProbPlan> plan((size_t)n_probs);
  size_t scratch_bytes = 0;
  int64_t max_batch = 0;
  for (int q = 0; q < n_probs; ++q) {
    ProbPlan &pl = plan[(size_t)q];
    const double p = probs[q];
    pl.valid = p > 0.0 && p < 1.0;
    if (!pl.valid) continue;
    int64_t g = (int64_t)std::floor(p * (double)N);
    g = g < 1 ? 1 : g > N - 1 ? N - 1 : g;
    pl.g = g;
    pl.k = N - g;
    pl.npad = pow2_at_least((uint64_t)pl.k);
    const size_t per_pair = (size_t)pl.npad * 2 * 8;
    int64_t batch = (int64_t)(g_budget / per_pair);
    batch = batch < 1 ? 1 : batch;      // (a pair whose two tails exceed the budget runs alone)
    batch = batch > kMaxBatch ? kMaxBatch : batch;
    batch = (size_t)batch > pairs ? (int64_t)pairs : batch;
    pl.batch = batch;
    if ((size_t)batch * per_pair > scratch_bytes) scratch_bytes = (size_t)batch * per_pair;
    if (batch > max_batch) max_batch = batch;
  }
  if (!max_batch) return AMWG_OK;      // every probability is NaN or outside (0, 1)
  int64_t lds_keys = 0;
  TRYB(amwg_hpd_lds_keys(&lds_keys));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(hpd_bitonic_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_keys * 8)));
  DevBuf thr, bad, res, cur, scratch;
  HIP_TRY(thr.alloc(pairs * 2 * 8));
  HIP_TRY(bad.alloc(pairs * 4));
  HIP_TRY(res.alloc(pairs * 2 * 8));
  HIP_TRY(cur.alloc((size_t)max_batch * 2 * 4));
  HIP_TRY(scratch.alloc(scratch_bytes));
  std::vector<double> host_res(pairs * 2);
  for (int q = 0; q < n_probs; ++q) {
    const ProbPlan &pl = plan[(size_t)q];
    if (!pl.valid) continue;
    const uint32_t k = (uint32_t)pl.k, npad = (uint32_t)pl.npad;      // k <= N - 1 < 2^31, so npad <= 2^31
    const uint32_t chunk = (uint64_t)lds_keys < pl.npad ? (uint32_t)lds_keys : npad;
    const unsigned sort_threads = chunk / 2 < 64 ? 64u : chunk / 2 > (uint32_t)kSortMaxThreads ? (unsigned)kSortMaxThreads : chunk / 2;
    hipLaunchKernelGGL(hpd_threshold_kernel, dim3((unsigned)PR, (unsigned)D), dim3(kThrThreads), 0, stream, draws, rows, PR, C, cpd, (uint32_t)(pl.k - 1), (uint32_t)pl.g,
                       thr.as<uint64_t>(), bad.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    for (size_t pair0 = 0; pair0 < pairs; pair0 += (size_t)pl.batch) {
      const unsigned nb = (unsigned)(pairs - pair0 < (size_t)pl.batch ? pairs - pair0 : (size_t)pl.batch);
      HIP_TRY(hipMemsetAsync(cur.p, 0, (size_t)nb * 2 * 4, stream));
      hipLaunchKernelGGL(hpd_compact_kernel, dim3((unsigned)((N + kCompLoads * kCompThreads - 1) / (kCompLoads * kCompThreads)), nb), dim3(kCompThreads), 0, stream, draws, rows, PR, C,
                         cpd, pair0, thr.as<uint64_t>(), k, npad, scratch.as<uint64_t>(), cur.as<uint32_t>());
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(hpd_fill_kernel, dim3((unsigned)((pl.npad + kStepThreads - 1) / kStepThreads), 2 * nb), dim3(kStepThreads), 0, stream, pair0, thr.as<uint64_t>(),
                         cur.as<uint32_t>(), k, npad, scratch.as<uint64_t>());
      HIP_TRY(hipGetLastError());
      if (npad >= 2) {
        hipLaunchKernelGGL(hpd_bitonic_lds_kernel, dim3(npad / chunk, 2 * nb), dim3(sort_threads), (size_t)chunk * 8, stream, scratch.as<uint64_t>(), npad, chunk, (uint64_t)2,
                           (uint64_t)chunk);
        HIP_TRY(hipGetLastError());
        for (uint64_t kk = (uint64_t)chunk * 2; kk <= pl.npad; kk <<= 1) {      // tails longer than the LDS: the far partners in global memory, the near ones per chunk
          for (uint64_t j = kk >> 1; j >= chunk; j >>= 1) {
            hipLaunchKernelGGL(hpd_bitonic_step_kernel, dim3((unsigned)((pl.npad / 2 + kStepThreads - 1) / kStepThreads), 2 * nb), dim3(kStepThreads), 0, stream,
                               scratch.as<uint64_t>(), npad, kk, (uint32_t)j);
            HIP_TRY(hipGetLastError());
          }
          hipLaunchKernelGGL(hpd_bitonic_lds_kernel, dim3(npad / chunk, 2 * nb), dim3(sort_threads), (size_t)chunk * 8, stream, scratch.as<uint64_t>(), npad, chunk, kk, kk);
          HIP_TRY(hipGetLastError());
        }
      }
      hipLaunchKernelGGL(hpd_argmin_kernel, dim3(nb), dim3(kArgThreads), 0, stream, scratch.as<uint64_t>(), k, npad, pair0, bad.as<uint32_t>(), res.as<double>());
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(host_res.data(), res.p, pairs * 2 * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (size_t pair = 0; pair < pairs; ++pair) {
      out[(pair * (size_t)n_probs + (size_t)q) * 2] = host_res[pair * 2];
      out[(pair * (size_t)n_probs + (size_t)q) * 2 + 1] = host_res[pair * 2 + 1];
    }
  }
  return AMWG_OK;
}

extern "C" int amwg_last_sample_dataset_hpd(amwg_sampler *s, const double *probs, int32_t n_probs, double *out) {
  if (!s || !probs || !out || n_probs < 1) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_dataset_hpd: bad argument");
  TRYB(amwg_refuse_summarised(s, "amwg_last_sample_dataset_hpd"));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_dataset_hpd: no sample() call yet");
  TRYB(amwg_hpd_shape("amwg_last_sample_dataset_hpd", s->last_rows, s->P + s->D, s->C, s->n_datasets, n_probs));
  HIP_TRY(hipSetDevice(s->device));
  return amwg_hpd_launch("amwg_last_sample_dataset_hpd", s->last_draws, s->last_rows, s->P + s->D, s->C, s->n_datasets, probs, n_probs, out, s->stream);
}
