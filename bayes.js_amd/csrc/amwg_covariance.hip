// amwg_covariance.hip -- posterior covariance matrices over a subset of the recorded values, on the device (part of libamwg.so): the co-moment kernels that run
// beside the fold of a window, the kernel that turns per-chain co-moments into a matrix per dataset, their launchers, the covariance a sampler arms for its
// summarising calls (amwg_set_covariance) and the call that returns the matrices (amwg_last_sample_dataset_covariance).  amwg_covariance.h states the arithmetic.
// No atomics: a co-moment (pair, chain) belongs to one thread of one launch, an entry of a matrix to one workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <numeric>
#include <unordered_map>

#include "amwg_covariance.h"
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_sampler.h"

using namespace amwg;

namespace {

// the place of the pair (a, b), a < b, of K ascending values among the co-moments: the upper triangle without its diagonal, row by row
__host__ __device__ inline size_t pair_at(int a, int b, int K) { return (size_t)a * (size_t)(2 * K - a - 1) / 2 + (size_t)(b - a - 1); }

// ---- the co-moments of a window.  One thread per chain, the chain the fastest index: a wavefront's 64 loads of one row of one value are one 512-byte run.  A thread
// carries the running means of a TILE of values and the tile's co-moments in registers from the first row of the window to the last: read once, written once.  The
// means are not stored: they are the fold's own acc[4] recurrence (welford_add's mean line, the same operations on the same inputs, so the same bits), recomputed
// here from acc[4] as the fold of the PREVIOUS window left it -- this kernel runs before the fold of its window.  The recurrence carries an fp64 division per value
// and row; the loads do not depend on it, so A rows are fetched ahead of the dependent updates.  A row's index among the kept draws is g0 + r: a window may begin
// anywhere.
//
// Tiles.  comoment_tile_kernel<T, A>: T values and their T (T - 1) / 2 pairs -- K <= 8 is one tile (T = 2, 4 or 8); larger K is cut into tiles of 4, and
// comoment_cross_kernel<T, A> takes two different tiles and their T x T pairs.  Each launch of a tile (pair) recomputes its means and reads its values' rows once.
// A tile that reaches past K repeats the last value: what it computes for the repeats is not stored.
//                                  means + co-moments + rows ahead (doubles)   VGPRs (no scratch; DESIGN.md section 3 has the compiler's report)
//   comoment_tile_kernel<2, 8>      2 +  1 + 16                                  58
//   comoment_tile_kernel<4, 4>      4 +  6 + 16                                  72
//   comoment_tile_kernel<8, 2>      8 + 28 + 16                                 124
//   comoment_cross_kernel<4, 2>     8 + 16 + 16                                 100
// At most 128, so that a SIMD holds four waves of each.  A load's address is a wavefront-uniform base (SGPRs) plus the lane: a pointer per value in VGPRs cost the
// <8, 2> kernel 30 registers.
template <int T, int A>
__global__ void __launch_bounds__(256) comoment_tile_kernel(const double *__restrict__ window, int64_t g0, int64_t nrows, int PR, int64_t C, const int32_t *__restrict__ vals,
                                                            int K, const double *__restrict__ mean0, double *__restrict__ co) {
  const size_t c0 = (size_t)blockIdx.x * 256;      // the workgroup's first chain: with the value's offset it is wavefront-uniform, a load's address is that + lane
  const uint32_t l = threadIdx.x;
  if (c0 + l >= (size_t)C) return;
  const size_t c = c0 + l;
  const int base = (int)blockIdx.y * T;
  const size_t stat = (size_t)PR * (size_t)C;
  size_t at[T];      // (uniform)
  double m[T], cm[T * (T - 1) / 2];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    at[t] = (size_t)vals[base + t < K ? base + t : K - 1] * (size_t)C + c0;
    m[t] = (mean0 + at[t])[l];
  }
#pragma unroll
  for (int b = 1, q = 0; b < T; ++b)
#pragma unroll
    for (int a = 0; a < b; ++a, ++q) cm[q] = base + b < K ? co[pair_at(base + a, base + b, K) * (size_t)C + (size_t)c] : 0.0;
  for (int64_t r = 0; r < nrows; r += A) {
    double x[A][T];
#pragma unroll
    for (int u = 0; u < A; ++u)
#pragma unroll
      for (int t = 0; t < T; ++t) x[u][t] = r + u < nrows ? (window + (at[t] + (size_t)(r + u) * stat))[l] : 0.0;
#pragma unroll
    for (int u = 0; u < A; ++u) {
      if (r + u >= nrows) break;
      const double k = (double)(g0 + r + u + 1);      // the row's 1-based index among the chain's kept draws
      double dx[T];
#pragma unroll
      for (int b = 0, q = 0; b < T; ++b) {
        dx[b] = x[u][b] - m[b];
        m[b] += dx[b] / k;
        const double e = x[u][b] - m[b];
#pragma unroll
        for (int a = 0; a < b; ++a, ++q) cm[q] += dx[a] * e;
      }
    }
  }
#pragma unroll
  for (int b = 1, q = 0; b < T; ++b)
#pragma unroll
    for (int a = 0; a < b; ++a, ++q)
      if (base + b < K) co[pair_at(base + a, base + b, K) * (size_t)C + (size_t)c] = cm[q];
}

// tiles ta < tb (blockIdx.y, blockIdx.z; the other workgroups of the square grid leave at once): the pairs (i in ta, j in tb), i the smaller index as everywhere
template <int T, int A>
__global__ void __launch_bounds__(256) comoment_cross_kernel(const double *__restrict__ window, int64_t g0, int64_t nrows, int PR, int64_t C, const int32_t *__restrict__ vals,
                                                             int K, const double *__restrict__ mean0, double *__restrict__ co) {
  const size_t c0 = (size_t)blockIdx.x * 256;
  const uint32_t l = threadIdx.x;
  if (blockIdx.z <= blockIdx.y || c0 + l >= (size_t)C) return;
  const size_t c = c0 + l;
  const int bi = (int)blockIdx.y * T, bj = (int)blockIdx.z * T;
  const size_t stat = (size_t)PR * (size_t)C;
  size_t at[2 * T];      // (uniform)
  double m[2 * T], cm[T * T];
#pragma unroll
  for (int t = 0; t < 2 * T; ++t) {
    const int k = t < T ? bi + t : bj + t - T;
    at[t] = (size_t)vals[k < K ? k : K - 1] * (size_t)C + c0;
    m[t] = (mean0 + at[t])[l];
  }
#pragma unroll
  for (int a = 0; a < T; ++a)      // (bi + a < K always: tile ta is not the last)
#pragma unroll
    for (int b = 0; b < T; ++b) cm[a * T + b] = bj + b < K ? co[pair_at(bi + a, bj + b, K) * (size_t)C + (size_t)c] : 0.0;
  for (int64_t r = 0; r < nrows; r += A) {
    double x[A][2 * T];
#pragma unroll
    for (int u = 0; u < A; ++u)
#pragma unroll
      for (int t = 0; t < 2 * T; ++t) x[u][t] = r + u < nrows ? (window + (at[t] + (size_t)(r + u) * stat))[l] : 0.0;
#pragma unroll
    for (int u = 0; u < A; ++u) {
      if (r + u >= nrows) break;
      const double k = (double)(g0 + r + u + 1);
      double dx[T];
#pragma unroll
      for (int a = 0; a < T; ++a) {
        dx[a] = x[u][a] - m[a];
        m[a] += dx[a] / k;
      }
#pragma unroll
      for (int b = 0; b < T; ++b) {
        const double dj = x[u][T + b] - m[T + b];
        m[T + b] += dj / k;
        const double e = x[u][T + b] - m[T + b];
#pragma unroll
        for (int a = 0; a < T; ++a) cm[a * T + b] += dx[a] * e;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < T; ++a)
#pragma unroll
    for (int b = 0; b < T; ++b)
      if (bj + b < K) co[pair_at(bi + a, bj + b, K) * (size_t)C + (size_t)c] = cm[a * T + b];
}

// ---- per (dataset d, pair a <= b of the ascending values): the matrix entry from the per-chain means (acc[4]), co-moments and -- on the diagonal -- the whole-chain
// M2 (acc[5]), in fold_moments_kernel's order: thread t takes the dataset's chains t, t + 256, ..., block_sum's halving tree adds the 256 partial sums.  On the
// diagonal every operation is fold_moments_kernel's own, so sqrt(cov_ii) is its sd.  Workgroup (d, a, b); those with b < a leave at once.
__global__ void __launch_bounds__(256) covariance_finish_kernel(const double *__restrict__ acc, const double *__restrict__ co, int64_t rows, int PR, int64_t C, int64_t cpd,
                                                                const int32_t *__restrict__ vals, int K, double *__restrict__ cov) {
  __shared__ double red[256];
  const int d = blockIdx.x, a = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, nt = blockDim.x;
  if (b < a) return;
  const size_t off = (size_t)d * (size_t)cpd;
  const double *mi = acc + ((size_t)4 * PR + vals[a]) * C + off, *mj = acc + ((size_t)4 * PR + vals[b]) * C + off;
  const double *w = a == b ? acc + ((size_t)5 * PR + vals[a]) * C + off : co + pair_at(a, b, K) * (size_t)C + off;
  double si = 0, sj = 0, s2 = 0;
  for (int64_t c = tid; c < cpd; c += nt) { si += mi[c]; sj += mj[c]; s2 += w[c]; }
  const double gi = block_sum(si, red) / (double)cpd, gj = block_sum(sj, red) / (double)cpd, within = block_sum(s2, red);
  double sb = 0;
  for (int64_t c = tid; c < cpd; c += nt) sb += (mi[c] - gi) * (mj[c] - gj);
  const double ss = within + (double)rows * block_sum(sb, red);
  const double n = (double)rows * (double)cpd;
  if (tid == 0) {
    const double v = ss / (n - 1);
    cov[((size_t)d * K + a) * K + b] = v;
    cov[((size_t)d * K + b) * K + a] = v;
  }
}

bool mul_fits(size_t a, size_t b, size_t *out) { return !__builtin_mul_overflow(a, b, out); }

// ---- the covariance armed per sampler.  Beside the handle, not in it: amwg_sampler.h is one of the sources the step kernels' id is formed from
std::mutex g_cov_mu;
std::unordered_map<const amwg_sampler *, CovArm> g_cov;
void free_arm(CovArm &a) {
  if (a.d_values) (void)hipFree(a.d_values);
  if (a.d_co) (void)hipFree(a.d_co);
  a = CovArm();
}

// cov_sorted [D][K][K] (ascending values) -> cov [D][K][K] in the caller's order: entry (i, j) is (where[i], where[j])
void put_back(const double *cov_sorted, int D, int K, const std::vector<int32_t> &where, double *cov) {
  for (int d = 0; d < D; ++d)
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j) cov[((size_t)d * K + i) * K + j] = cov_sorted[((size_t)d * K + where[i]) * K + where[j]];
}

}  // namespace

size_t amwg_covariance_pairs(int32_t K) { return (size_t)K * (size_t)(K - 1) / 2; }

void amwg_covariance_order(const int32_t *values, int32_t K, std::vector<int32_t> *sorted, std::vector<int32_t> *where) {
  std::vector<int32_t> by(K);      // by[r]: the place in `values` of the r-th smallest
  std::iota(by.begin(), by.end(), 0);
  std::sort(by.begin(), by.end(), [&](int32_t x, int32_t y) { return values[x] < values[y]; });
  sorted->resize(K);
  where->resize(K);
  for (int32_t r = 0; r < K; ++r) { (*sorted)[r] = values[by[r]]; (*where)[by[r]] = r; }
}

int amwg_covariance_values_check(const char *call, const int32_t *values, int32_t K, int PR) {
  if (!values) return amwg_fail(AMWG_EINVAL, "%s: null values", call);
  if (K < 1 || K > PR) return amwg_fail(AMWG_EINVAL, "%s: %d values (1 to %d, the recorded values)", call, (int)K, PR);
  std::vector<char> seen(PR, 0);
  for (int32_t k = 0; k < K; ++k) {
    if (values[k] < 0 || values[k] >= PR) return amwg_fail(AMWG_EINVAL, "%s: value %d of the list is %d, outside the recorded values [0, %d)", call, (int)k, (int)values[k], PR);
    if (seen[values[k]]) return amwg_fail(AMWG_EINVAL, "%s: recorded value %d is listed twice", call, (int)values[k]);
    seen[values[k]] = 1;
  }
  return AMWG_OK;
}

int amwg_covariance_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int32_t K) {
  if (rows < 1 || PR < 1 || PR > 65535 || C < 1 || D < 1 || D > 65535 || C % D != 0)
    return amwg_fail(AMWG_EINVAL, "%s: bad shape (rows %lld, values %d, chains %lld, datasets %d -- at most 65535, dividing the chains)", call, (long long)rows, PR, (long long)C, D);
  if (K < 1 || K > PR) return amwg_fail(AMWG_EINVAL, "%s: %d values (1 to %d, the recorded values)", call, (int)K, PR);
  if (rows < 2 && C / D < 2) return amwg_fail(AMWG_EINVAL, "%s: a covariance needs at least 2 draws per dataset (got %lld kept draws x %lld chains)", call, (long long)rows, (long long)(C / D));
  size_t row_bytes, bytes;
  if (!mul_fits((size_t)PR * 8, (size_t)C, &row_bytes) || !mul_fits(row_bytes, (size_t)rows, &bytes) || !mul_fits(row_bytes, (size_t)kFoldStats, &bytes) ||
      !mul_fits(amwg_covariance_pairs(K) * 8, (size_t)C, &bytes) || !mul_fits((size_t)K * (size_t)K * 8, (size_t)D, &bytes))
    return amwg_fail(AMWG_EINVAL, "%s: array too large (a byte count beyond size_t)", call);
  return AMWG_OK;
}

int amwg_comoment_window(const double *window, int64_t g0, int64_t nrows, int PR, int64_t C, const int32_t *d_values, int32_t K, const double *acc, double *d_co,
                         hipStream_t stream) {
  if (!window || !d_values || !acc || g0 < 0 || nrows < 1 || PR < 1 || PR > 65535 || C < 1 || K < 1 || K > PR)
    return amwg_fail(AMWG_EINVAL, "internal: co-moments of rows [%lld, +%lld) of %d of %d values x %lld chains", (long long)g0, (long long)nrows, (int)K, PR, (long long)C);
  if (K == 1) return AMWG_OK;      // (no pair: the diagonal comes from the fold's own M2)
  if (!d_co) return amwg_fail(AMWG_EINVAL, "internal: no co-moments");
  const unsigned gx = (unsigned)((C + 255) / 256);
  const double *mean0 = acc + (size_t)4 * (size_t)PR * (size_t)C;
  if (K <= 2) hipLaunchKernelGGL((comoment_tile_kernel<2, 8>), dim3(gx, 1), dim3(256), 0, stream, window, g0, nrows, PR, C, d_values, (int)K, mean0, d_co);
  else if (K <= 4) hipLaunchKernelGGL((comoment_tile_kernel<4, 4>), dim3(gx, 1), dim3(256), 0, stream, window, g0, nrows, PR, C, d_values, (int)K, mean0, d_co);
  else if (K <= 8) hipLaunchKernelGGL((comoment_tile_kernel<8, 2>), dim3(gx, 1), dim3(256), 0, stream, window, g0, nrows, PR, C, d_values, (int)K, mean0, d_co);
  else {
    const unsigned tiles = (unsigned)((K + 3) / 4);      // (<= 16384: K <= PR <= 65535)
    hipLaunchKernelGGL((comoment_tile_kernel<4, 4>), dim3(gx, tiles), dim3(256), 0, stream, window, g0, nrows, PR, C, d_values, (int)K, mean0, d_co);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((comoment_cross_kernel<4, 2>), dim3(gx, tiles, tiles), dim3(256), 0, stream, window, g0, nrows, PR, C, d_values, (int)K, mean0, d_co);
  }
  HIP_TRY(hipGetLastError());
  return AMWG_OK;
}

int amwg_covariance_finish(const double *acc, const double *d_co, int64_t rows, int PR, int64_t C, int D, const int32_t *d_values, int32_t K, double *d_cov,
                           hipStream_t stream) {
  if (!acc || !d_values || !d_cov || (K > 1 && !d_co) || K < 1 || K > PR || PR > 65535 || D < 1 || D > 65535 || C % D != 0)
    return amwg_fail(AMWG_EINVAL, "internal: covariance of %d of %d values, %lld chains in %d datasets", (int)K, PR, (long long)C, D);
  hipLaunchKernelGGL(covariance_finish_kernel, dim3((unsigned)D, (unsigned)K, (unsigned)K), dim3(256), 0, stream, acc, d_co, rows, PR, C, C / D, d_values, (int)K, d_cov);
  HIP_TRY(hipGetLastError());
  return AMWG_OK;
}

int amwg_covariance_of_array(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const int32_t *values, int32_t K, int64_t window_rows,
                             double *cov, hipStream_t stream) {
  if (!draws || !cov) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (window_rows < 0) return amwg_fail(AMWG_EINVAL, "%s: bad shape (window_rows %lld)", call, (long long)window_rows);
  TRYB(amwg_covariance_shape(call, rows, PR, C, D, K));
  TRYB(amwg_covariance_values_check(call, values, K, PR));
  std::vector<int32_t> sorted, where;
  amwg_covariance_order(values, K, &sorted, &where);
  const size_t row_elems = (size_t)PR * (size_t)C, acc_bytes = (size_t)kFoldStats * row_elems * 8, co_bytes = amwg_covariance_pairs(K) * (size_t)C * 8;
  const size_t cov_elems = (size_t)D * (size_t)K * (size_t)K;
  DevBuf acc, co, dv, dc;
  HIP_TRY(acc.alloc(acc_bytes));
  HIP_TRY(co.alloc(co_bytes));
  HIP_TRY(dv.alloc((size_t)K * 4));
  HIP_TRY(dc.alloc(cov_elems * 8));
  HIP_TRY(hipMemcpyAsync(dv.p, sorted.data(), (size_t)K * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(acc.p, 0, acc_bytes, stream));      // (the zeroed per-chain scratch a summarising call starts from too)
  HIP_TRY(hipMemsetAsync(co.p, 0, co_bytes ? co_bytes : 8, stream));
  const int64_t w = window_rows > 0 ? window_rows : rows;
  for (int64_t g0 = 0; g0 < rows; g0 += w) {      // (window after window, as launch_steps folds them: the co-moments first, they start from the means of the fold before)
    const int64_t n = rows - g0 < w ? rows - g0 : w;
    TRYB(amwg_comoment_window(draws + (size_t)g0 * row_elems, g0, n, PR, C, dv.as<int32_t>(), K, acc.as<double>(), co.as<double>(), stream));
    TRYB(amwg_fold_window(draws + (size_t)g0 * row_elems, g0, n, rows / 2, PR, C, acc.as<double>(), stream));
  }
  TRYB(amwg_covariance_finish(acc.as<double>(), co.as<double>(), rows, PR, C, D, dv.as<int32_t>(), K, dc.as<double>(), stream));
  std::vector<double> cs(cov_elems);
  HIP_TRY(hipMemcpyAsync(cs.data(), dc.p, cov_elems * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  put_back(cs.data(), D, K, where, cov);
  return AMWG_OK;
}

CovArm *amwg_covariance_armed(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_cov_mu);
  auto it = g_cov.find(s);      // (pointers into an unordered_map stay valid while other entries come and go)
  return it == g_cov.end() || it->second.n_values < 1 ? nullptr : &it->second;
}

int amwg_covariance_begin(amwg_sampler *s, CovArm **arm) {
  CovArm *a = amwg_covariance_armed(s);
  *arm = a;
  if (!a) return AMWG_OK;
  const size_t co_bytes = amwg_covariance_pairs(a->n_values) * (size_t)s->C * 8;
  if (co_bytes) HIP_TRY(hipMemsetAsync(a->d_co, 0, co_bytes, s->stream));      // (each summarising call starts afresh)
  a->folded = true;
  return AMWG_OK;
}

void amwg_covariance_forget(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_cov_mu);
  auto it = g_cov.find(s);
  if (it == g_cov.end()) return;
  free_arm(it->second);
  g_cov.erase(it);
}

extern "C" {

int amwg_set_covariance(amwg_sampler *s, const int32_t *values, int32_t n_values) {
  const char *call = "amwg_set_covariance";
  if (!s) return amwg_fail(AMWG_EINVAL, "%s: null sampler", call);
  const bool disarm = !values && n_values == 0;
  const int PR = s->P + s->D;
  size_t co_bytes = 0;
  if (!disarm) {
    if (!values) return amwg_fail(AMWG_EINVAL, "%s: null values (NULL, 0 disarms)", call);
    TRYB(amwg_covariance_values_check(call, values, n_values, PR));
    if (!mul_fits(amwg_covariance_pairs(n_values) * 8, (size_t)s->C, &co_bytes)) return amwg_fail(AMWG_EINVAL, "%s: array too large (a byte count beyond size_t)", call);
  }
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));      // (a summarising call still in flight adds to the co-moments that go away)
  amwg_covariance_forget(s);
  if (disarm) return AMWG_OK;
  CovArm a;
  std::vector<int32_t> sorted;
  amwg_covariance_order(values, n_values, &sorted, &a.where);
  a.values.assign(values, values + n_values);
  const size_t list_bytes = (size_t)n_values * 4;
  if (hipMalloc(reinterpret_cast<void **>(&a.d_values), list_bytes) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&a.d_co), co_bytes ? co_bytes : 8) != hipSuccess ||
      hipMemcpy(a.d_values, sorted.data(), list_bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemset(a.d_co, 0, co_bytes ? co_bytes : 8) != hipSuccess) {
    free_arm(a);
    return amwg_fail(AMWG_EHIP, "%s: cannot place %zu bytes of co-moments and values on the device", call, co_bytes + list_bytes);
  }
  a.n_values = n_values;
  a.bytes = co_bytes + list_bytes;
  std::lock_guard<std::mutex> lock(g_cov_mu);
  g_cov[s] = a;
  return AMWG_OK;
}

int amwg_covariance_info(const amwg_sampler *s, int32_t *n_values, size_t *bytes) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_covariance_info: null sampler");
  const CovArm *a = amwg_covariance_armed(s);
  if (n_values) *n_values = a ? a->n_values : 0;
  if (bytes) *bytes = a ? a->bytes : 0;
  return AMWG_OK;
}

int amwg_last_sample_dataset_covariance(amwg_sampler *s, const int32_t *values, int32_t n_values, double *cov) {
  const char *call = "amwg_last_sample_dataset_covariance";
  if (!s || !cov) return amwg_fail(AMWG_EINVAL, "%s: null %s", call, !s ? "sampler" : "cov");
  if (n_values < 1) return amwg_fail(AMWG_EINVAL, "%s: %d values (at least 1)", call, (int)n_values);
  const int PR = s->P + s->D, D = s->n_datasets;
  if (amwg_summarised(s)) {      // the draws were not kept: only what was folded while they passed can be returned
    const CovArm *a = amwg_covariance_armed(s);
    if (values || !a || !a->folded || a->n_values != n_values)
      return amwg_fail(AMWG_EINVAL, "%s: the last sample call was amwg_sample_summarize, which kept no draw: %s", call,
                       values ? "values cannot be given afterwards -- arm them with amwg_set_covariance before the call, and pass NULL here"
                       : !a || !a->folded ? "no covariance was armed for it (amwg_set_covariance before the call)"
                                          : "the number of values differs from the one armed with amwg_set_covariance");
    const FoldSummary *f = amwg_summary_of(s);
    if (!f || !f->acc) return amwg_fail(AMWG_EINVAL, "internal: a summarised sampler without accumulators");
    TRYB(amwg_covariance_shape(call, s->last_rows, PR, s->C, D, n_values));
    HIP_TRY(hipSetDevice(s->device));
    const size_t cov_elems = (size_t)D * (size_t)n_values * (size_t)n_values;
    DevBuf dc;
    HIP_TRY(dc.alloc(cov_elems * 8));
    TRYB(amwg_covariance_finish(f->acc, a->d_co, s->last_rows, PR, s->C, D, a->d_values, n_values, dc.as<double>(), s->stream));
    std::vector<double> cs(cov_elems);
    HIP_TRY(hipMemcpyAsync(cs.data(), dc.p, cov_elems * 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    put_back(cs.data(), D, n_values, a->where, cov);
    return AMWG_OK;
  }
  if (!values) return amwg_fail(AMWG_EINVAL, "%s: null values (NULL asks for the matrix of a summarising call over the values of amwg_set_covariance; the last sample call was none)", call);
  TRYB(amwg_covariance_values_check(call, values, n_values, PR));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "%s: no sample() call yet", call);
  TRYB(amwg_covariance_shape(call, s->last_rows, PR, s->C, D, n_values));
  HIP_TRY(hipSetDevice(s->device));
  return amwg_covariance_of_array(call, s->last_draws, s->last_rows, PR, s->C, D, values, n_values, 0, cov, s->stream);
}

}  // extern "C"
