// amwg_histogram.hip -- posterior histograms over caller-given edges, on the device (part of libamwg.so): the kernel, its launcher, the histogram a sampler arms for
// its summarising calls (amwg_set_histogram) and the call that returns the counts (amwg_last_sample_dataset_histogram).  amwg_histogram.h states the bin rule.
// Counts are integers and integer adds commute: the counts of an array do not depend on how it is cut into windows, slices or workgroups, nor on scheduling.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <unordered_map>

#include "amwg_fold.h"
#include "amwg_histogram.h"
#include "amwg_host.h"
#include "amwg_sampler.h"

using namespace amwg;

namespace {

constexpr int kHistThreads = 256;      // 4 wavefronts.  LDS at bins = 4096: 4097 edges x 8 B + 4099 counters x 4 B = 49 172 B -> three workgroups (12 wavefronts) per CU
constexpr int kHistWaves = kHistThreads / 64;
constexpr int kHistLoads = 4;          // rows a thread has in flight
constexpr int64_t kHistTargetGroups = 1024;      // workgroups wanted where the input is large enough: four per CU
constexpr int64_t kHistMinValues = 2048;         // ... and no workgroup for fewer values than two rounds of its threads' loads

// cnt[slot] += 1 for every lane with `active`.  The draws of one posterior pile into a few bins, so the 64 lanes of a wave instruction often name the same
// counter, and an LDS atomic serialises the lanes that do.  dataset_select_kernel's scheme (amwg_summaries.hip) takes that away: the first lane still waiting
// broadcasts its slot, the lanes that agree are counted by a ballot and ONE lane adds the count.  Repeated until no lane waits, its trip count is the number of
// distinct slots in the wavefront -- measured 5 x slower on draws spread over 256 bins than on the same draws in two.  So: kHistRounds rounds of it, which serve the one or two crowded counters, and the lanes still waiting then add 1 each, to counters that are mostly distinct.
// Every lane of the wavefront must arrive here.
constexpr int kHistRounds = 2;
__device__ inline void wave_count(uint32_t *cnt, bool active, uint32_t slot) {
  const int lane = threadIdx.x & 63;
  uint64_t todo = __ballot(active);
#pragma unroll
  for (int round = 0; round < kHistRounds && todo; ++round) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t ls = (uint32_t)__builtin_amdgcn_readlane((int)slot, leader);
    const uint64_t same = __ballot(active && slot == ls);
    if (lane == leader) atomicAdd(&cnt[ls], (uint32_t)__popcll(same));
    active = active && slot != ls;
    todo &= ~same;
  }
  if (active) atomicAdd(&cnt[slot], 1u);
}

// the slot of x among the edges e[0 .. bins] (LDS): a binary search for the number of edges <= x -- comparisons only, no arithmetic on x.
// slots: [0, bins) the bins, bins = under, bins + 1 = over, bins + 2 = nan
__device__ inline uint32_t hist_slot(const double *e, int bins, double x) {
  if (x != x) return (uint32_t)bins + 2u;
  int lo = 0, hi = bins + 1;      // the answer lies in [lo, hi]
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (e[m] <= x) lo = m + 1; else hi = m;
  }
  return lo == 0 ? (uint32_t)bins : (lo == bins + 1 ? (uint32_t)bins + 1u : (uint32_t)(lo - 1));
}
// The same slot where the edges are (nearly) a uniform grid: a guess k = floor((x - e0) s), s = bins / (e_bins - e0), corrected by comparisons with the edges until
// e[k] <= x < e[k + 1].  The comparisons decide, never the arithmetic: whatever the guess, the loops end at the bin of the rule (x lies in [e0, e_bins) when they
// start).  The guess only sets their trip count, and the host takes this path only for edges whose own guesses are at most one bin off (amwg_histogram_uniform):
// the guess is monotone in x, so between two edges it is at most two bins off.
__device__ inline uint32_t hist_slot_uniform(const double *e, int bins, double e0, double s, double x) {
  if (x != x) return (uint32_t)bins + 2u;
  if (x < e0) return (uint32_t)bins;
  if (x >= e[bins]) return (uint32_t)bins + 1u;
  double t = (x - e0) * s;
  t = t < (double)(bins - 1) ? t : (double)(bins - 1);      // (an infinite product too)
  int k = (int)t;
  while (k > 0 && x < e[k]) --k;
  while (k < bins - 1 && x >= e[k + 1]) ++k;
  return (uint32_t)k;
}

// Workgroup (p, d, z) counts the values of recorded value p and dataset d in rows [rs rps, (rs + 1) rps) and the dataset's columns [cs cps, (cs + 1) cps), where
// z = rs n_cs + cs, into u32 counters in LDS, and at the end adds its non-zero counters to counts[d][p][bins + 3].  A wavefront walks rows with the column as the
// lane index (consecutive lanes = consecutive chains: a row is one 512-byte run); where the columns are fewer than 64, the wavefront's lanes cover 64 / columns
// rows at a time -- one integer division per THREAD, none per element.  Dynamic LDS: (bins + 1) doubles, then (bins + 3) u32.
__global__ void __launch_bounds__(kHistThreads) dataset_histogram_kernel(const double *__restrict__ draws, int64_t rows, int PR, int64_t C, int64_t cpd,
                                                                         const double *__restrict__ edges, int bins, int guess, int n_cs, int64_t rps, int64_t cps,
                                                                         unsigned long long *__restrict__ counts) {
  extern __shared__ double hist_lds[];
  double *e = hist_lds;
  uint32_t *cnt = reinterpret_cast<uint32_t *>(hist_lds + bins + 1);
  const int p = blockIdx.x, d = blockIdx.y, rs = (int)blockIdx.z / n_cs, cs = (int)blockIdx.z - rs * n_cs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i <= bins; i += kHistThreads) e[i] = edges[(size_t)p * (size_t)(bins + 1) + (size_t)i];
  for (int i = tid; i < bins + 3; i += kHistThreads) cnt[i] = 0;
  __syncthreads();
  const double e0 = e[0], scale = (double)bins / (e[bins] - e0);      // (used when `guess`: hist_slot_uniform)

  const int64_t r_lo = (int64_t)rs * rps, r_hi = r_lo + rps < rows ? r_lo + rps : rows;
  const int64_t c_lo = (int64_t)cs * cps, c_hi = c_lo + cps < cpd ? c_lo + cps : cpd;
  const int64_t width = c_hi - c_lo;
  if (width > 0 && r_lo < r_hi) {      // (workgroup-uniform; the host launches no empty slice)
    const int cw = width < 64 ? (int)width : 64;      // columns a wavefront covers at a time
    const int rpw = 64 / cw, sub = lane / cw, c0 = lane - sub * cw;      // ... and rows; this lane's row and column among them
    const bool lane_on = sub < rpw;
    const int64_t rstep = (int64_t)kHistWaves * rpw, my_r = (int64_t)wave * rpw + sub, row_stride = (int64_t)PR * C;
    const double *src = draws + (int64_t)p * C + (int64_t)d * cpd;
    for (int64_t ct = c_lo; ct < c_hi; ct += cw) {
      const int64_t col = ct + c0;
      const bool col_ok = lane_on && col < c_hi;
      for (int64_t rb = r_lo; rb < r_hi; rb += rstep * kHistLoads) {
        double v[kHistLoads];
        bool on[kHistLoads];
#pragma unroll
        for (int u = 0; u < kHistLoads; ++u) {
          const int64_t r = rb + (int64_t)u * rstep + my_r;
          on[u] = col_ok && r < r_hi;
          v[u] = on[u] ? src[r * row_stride + col] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kHistLoads; ++u) wave_count(cnt, on[u], guess ? hist_slot_uniform(e, bins, e0, scale, v[u]) : hist_slot(e, bins, v[u]));
      }
    }
  }
  __syncthreads();
  unsigned long long *cell = counts + ((size_t)d * (size_t)PR + (size_t)p) * (size_t)(bins + 3);
  for (int i = tid; i < bins + 3; i += kHistThreads) {
    const uint32_t c = cnt[i];
    if (c) atomicAdd(&cell[i], (unsigned long long)c);
  }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the histogram armed per sampler.  Beside the handle, not in it: amwg_sampler.h is one of the sources the step kernels' id is formed from
std::mutex g_hist_mu;
std::unordered_map<const amwg_sampler *, HistArm> g_hist;
void free_arm(HistArm &a) {
  if (a.d_edges) (void)hipFree(a.d_edges);
  if (a.d_counts) (void)hipFree(a.d_counts);
  a = HistArm();
}

}  // namespace

// Row slices first (whole rows stay whole runs), column slices -- in units of 64 columns -- where the rows are too few: a window of a summarising call on one dataset
// is 64 rows of 65 536 chains.
void amwg_histogram_grid(int64_t rows, int PR, int64_t C, int D, int *row_slices, int *column_slices, int64_t *rows_per_slice, int64_t *columns_per_slice) {
  const int64_t cpd = C / D, base = (int64_t)PR * D;
  const int64_t want = ceil_div(kHistTargetGroups, base), useful = rows * cpd / kHistMinValues > 1 ? rows * cpd / kHistMinValues : 1;
  const int64_t slices = want < useful ? want : useful;
  const int64_t rpw = cpd < 64 ? 64 / cpd : 1, round_rows = (int64_t)kHistWaves * kHistLoads * rpw;      // rows of one round of a workgroup's loads
  int64_t n_rs = ceil_div(rows, round_rows) < slices ? ceil_div(rows, round_rows) : slices;
  const int64_t rps = ceil_div(rows, n_rs);
  n_rs = ceil_div(rows, rps);
  const int64_t tiles = ceil_div(cpd, 64);
  int64_t n_cs = ceil_div(slices, n_rs) < tiles ? ceil_div(slices, n_rs) : tiles;
  const int64_t cps = ceil_div(tiles, n_cs) * 64;
  n_cs = ceil_div(cpd, cps);
  *row_slices = (int)n_rs;
  *column_slices = (int)n_cs;
  *rows_per_slice = rps;
  *columns_per_slice = cps;
}

int amwg_histogram_edges_check(const char *call, const double *edges, int PR, int bins) {
  if (!edges) return amwg_fail(AMWG_EINVAL, "%s: null edges", call);
  if (bins < 1 || bins > kHistMaxBins) return amwg_fail(AMWG_EINVAL, "%s: %d bins (1 to %d)", call, bins, kHistMaxBins);
  for (int p = 0; p < PR; ++p) {
    const double *e = edges + (size_t)p * (size_t)(bins + 1);
    for (int i = 0; i <= bins; ++i) {
      if (!std::isfinite(e[i])) return amwg_fail(AMWG_EINVAL, "%s: edge %d of recorded value %d is not finite", call, i, p);
      if (i > 0 && !(e[i - 1] < e[i])) return amwg_fail(AMWG_EINVAL, "%s: the edges of recorded value %d are not strictly ascending at edge %d (%.17g, then %.17g)", call, p, i, e[i - 1], e[i]);
    }
  }
  return AMWG_OK;
}

int amwg_histogram_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int bins) {
  if (bins < 1 || bins > kHistMaxBins) return amwg_fail(AMWG_EINVAL, "%s: %d bins (1 to %d)", call, bins, kHistMaxBins);
  if (rows < 1 || PR < 1 || C < 1 || D < 1 || D > 65535 || C % D != 0)
    return amwg_fail(AMWG_EINVAL, "%s: bad shape (rows %lld, values %d, chains %lld, datasets %d -- at most 65535, dividing the chains)", call, (long long)rows, PR, (long long)C, D);
  if (rows > INT64_MAX / 8 / PR / C) return amwg_fail(AMWG_EINVAL, "%s: array too large", call);
  int n_rs, n_cs;
  int64_t rps, cps;
  amwg_histogram_grid(rows, PR, C, D, &n_rs, &n_cs, &rps, &cps);
  if (rps > (int64_t)4294967295 / cps) return amwg_fail(AMWG_EINVAL, "%s: 2^32 or more values in one workgroup's slice of %lld rows x %lld columns (its counters are 32 bits wide)", call, (long long)rps, (long long)cps);
  return AMWG_OK;
}

bool amwg_histogram_uniform(const double *edges, int PR, int bins) {
  for (int p = 0; p < PR; ++p) {
    const double *e = edges + (size_t)p * (size_t)(bins + 1);
    const double s = (double)bins / (e[bins] - e[0]);
    if (!std::isfinite(s)) return false;
    for (int i = 0; i <= bins; ++i) {
      const double g = std::floor((e[i] - e[0]) * s);
      if (!(g >= (double)(i - 1) && g <= (double)(i + 1))) return false;
    }
  }
  return true;
}

int amwg_histogram_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const double *d_edges, int bins, bool uniform,
                          uint64_t *d_counts, hipStream_t stream) {
  if (!draws || !d_edges || !d_counts) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  TRYB(amwg_histogram_shape(call, rows, PR, C, D, bins));
  int n_rs, n_cs;
  int64_t rps, cps;
  amwg_histogram_grid(rows, PR, C, D, &n_rs, &n_cs, &rps, &cps);
  const size_t lds = (size_t)(bins + 1) * sizeof(double) + (size_t)(bins + 3) * sizeof(uint32_t);
  hipLaunchKernelGGL(dataset_histogram_kernel, dim3((unsigned)PR, (unsigned)D, (unsigned)(n_rs * n_cs)), dim3(kHistThreads), lds, stream, draws, rows, PR, C, C / D, d_edges, bins, uniform ? 1 : 0, n_cs,
                     rps, cps, reinterpret_cast<unsigned long long *>(d_counts));
  HIP_TRY(hipGetLastError());
  return AMWG_OK;
}

HistArm *amwg_histogram_armed(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_hist_mu);
  auto it = g_hist.find(s);      // (pointers into an unordered_map stay valid while other entries come and go)
  return it == g_hist.end() || it->second.bins < 1 ? nullptr : &it->second;
}

int amwg_histogram_begin(amwg_sampler *s, HistArm **arm) {
  HistArm *a = amwg_histogram_armed(s);
  *arm = a;
  if (!a) return AMWG_OK;
  const size_t cells = (size_t)s->n_datasets * (size_t)(s->P + s->D) * (size_t)(a->bins + 3);
  HIP_TRY(hipMemsetAsync(a->d_counts, 0, cells * 8, s->stream));      // (each summarising call starts afresh)
  a->folded = true;
  return AMWG_OK;
}

void amwg_histogram_forget(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_hist_mu);
  auto it = g_hist.find(s);
  if (it == g_hist.end()) return;
  free_arm(it->second);
  g_hist.erase(it);
}

extern "C" {

int amwg_set_histogram(amwg_sampler *s, const double *edges, int32_t bins) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_set_histogram: null sampler");
  const bool disarm = !edges && bins == 0;
  if (!disarm) {
    if (!edges) return amwg_fail(AMWG_EINVAL, "amwg_set_histogram: null edges (NULL, 0 disarms)");
    if (bins < 1 || bins > kHistMaxBins) return amwg_fail(AMWG_EINVAL, "amwg_set_histogram: %d bins (1 to %d; NULL, 0 disarms)", (int)bins, kHistMaxBins);
    TRYB(amwg_histogram_edges_check("amwg_set_histogram", edges, s->P + s->D, bins));
  }
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));      // (a summarising call still in flight adds to the counts that go away)
  amwg_histogram_forget(s);
  if (disarm) return AMWG_OK;
  const int PR = s->P + s->D;
  const size_t edge_bytes = (size_t)PR * (size_t)(bins + 1) * 8, count_bytes = (size_t)s->n_datasets * (size_t)PR * (size_t)(bins + 3) * 8;
  HistArm a;
  if (hipMalloc(reinterpret_cast<void **>(&a.d_edges), edge_bytes) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&a.d_counts), count_bytes) != hipSuccess ||
      hipMemcpy(a.d_edges, edges, edge_bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemset(a.d_counts, 0, count_bytes) != hipSuccess) {
    free_arm(a);
    return amwg_fail(AMWG_EHIP, "amwg_set_histogram: cannot place %zu bytes of edges and counts on the device", edge_bytes + count_bytes);
  }
  a.bins = bins;
  a.uniform = amwg_histogram_uniform(edges, PR, bins);
  a.bytes = edge_bytes + count_bytes;
  std::lock_guard<std::mutex> lock(g_hist_mu);
  g_hist[s] = a;
  return AMWG_OK;
}

int amwg_histogram_info(const amwg_sampler *s, int32_t *bins, size_t *bytes) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_histogram_info: null sampler");
  const HistArm *a = amwg_histogram_armed(s);
  if (bins) *bins = a ? a->bins : 0;
  if (bytes) *bytes = a ? a->bytes : 0;
  return AMWG_OK;
}

int amwg_last_sample_dataset_histogram(amwg_sampler *s, const double *edges, int32_t bins, uint64_t *counts) {
  const char *call = "amwg_last_sample_dataset_histogram";
  if (!s || !counts) return amwg_fail(AMWG_EINVAL, "%s: null %s", call, !s ? "sampler" : "counts");
  if (edges && (bins < 1 || bins > kHistMaxBins)) return amwg_fail(AMWG_EINVAL, "%s: %d bins (1 to %d)", call, (int)bins, kHistMaxBins);
  const int PR = s->P + s->D, D = s->n_datasets;
  if (amwg_summarised(s)) {      // the draws were not kept: only what was counted while they passed can be returned
    const HistArm *a = amwg_histogram_armed(s);
    if (edges || !a || !a->folded || a->bins != bins)
      return amwg_fail(AMWG_EINVAL, "%s: the last sample call was amwg_sample_summarize, which kept no draw: %s", call,
                       edges ? "edges cannot be given afterwards -- arm them with amwg_set_histogram before the call, and pass NULL here"
                       : !a || !a->folded ? "no histogram was armed for it (amwg_set_histogram before the call)"
                                          : "the number of bins differs from the one armed with amwg_set_histogram");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(counts, a->d_counts, (size_t)D * (size_t)PR * (size_t)(bins + 3) * 8, hipMemcpyDeviceToHost));
    return AMWG_OK;
  }
  if (!edges) return amwg_fail(AMWG_EINVAL, "%s: null edges (NULL asks for the counts of a summarising call under the edges of amwg_set_histogram; the last sample call was none)", call);
  TRYB(amwg_histogram_edges_check(call, edges, PR, bins));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "%s: no sample() call yet", call);
  TRYB(amwg_histogram_shape(call, s->last_rows, PR, s->C, D, bins));
  HIP_TRY(hipSetDevice(s->device));
  const size_t edge_bytes = (size_t)PR * (size_t)(bins + 1) * 8, count_bytes = (size_t)D * (size_t)PR * (size_t)(bins + 3) * 8;
  DevBuf de, dc;
  HIP_TRY(de.alloc(edge_bytes));
  HIP_TRY(dc.alloc(count_bytes));
  HIP_TRY(hipMemcpyAsync(de.p, edges, edge_bytes, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemsetAsync(dc.p, 0, count_bytes, s->stream));
  TRYB(amwg_histogram_launch(call, s->last_draws, s->last_rows, PR, s->C, D, de.as<double>(), bins, amwg_histogram_uniform(edges, PR, bins), dc.as<uint64_t>(), s->stream));
  HIP_TRY(hipMemcpyAsync(counts, dc.p, count_bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMWG_OK;
}

}  // extern "C"
