// amwg_autocov.hip -- autocovariance along the chains at lags 0 .. L over a subset of the recorded values, on the device (part of libamwg.so): the lag-sum and
// carry kernels that run beside the fold of a window, the kernels that turn the per-chain sums into autocovariances per dataset, their launchers, the
// autocovariance a sampler arms for its summarising calls (amwg_set_autocovariance) and the call that returns the result
// (amwg_last_sample_dataset_autocovariance).  amwg_autocov.h states the arithmetic and the state.
// No atomics: a sum (lag, value, chain) belongs to one thread of one launch, an output to one workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <unordered_map>

#include "amwg_autocov.h"
#include "amwg_covariance.h"      // (the checks and the ordering of a list of recorded values)
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_sampler.h"

using namespace amwg;

namespace {

constexpr int kLagTile = 8;      // consecutive lags per thread
constexpr int kAhead = 4;        // rows fetched ahead of the dependent adds

// ---- the lagged sums of a window.  One thread per chain, the chain the fastest index: a wavefront's 64 loads of one row of one value are one 512-byte run.
// blockIdx = (chains / 256, tile, value); tile i owns the lags l0 = 8 i .. l0 + 7 (those <= L).  A thread keeps the tile's 8 sums and a sliding register window
// w[j] = y_(g - l0 - j) from the first row of the window to the last: per row two loads -- x_g and the x entering the tile, x_(g - l0) -- for 16 fp64 operations;
// tile 0 needs the first load only and carries Y.  x_(g - l0) is read from the window when g - l0 >= g0, else from the ring (rows g0 - L .. g0 - 1 at slot
// g mod L: the carry kernel of the windows before left them there); a window may be shorter than L, so a lag may reach back over several windows.  The pilot is
// head[0], or row 0 of the window that holds it.  kAhead rows are fetched ahead of the adds, which depend on one another; a load's address is a
// wavefront-uniform base plus the lane.  Registers: 8 sums + 8 of the window + 2 kAhead fetched doubles, 66 VGPRs, no scratch.
__global__ void __launch_bounds__(256) autocov_lag_kernel(const double *__restrict__ window, int64_t g0, int64_t nrows, int PR, int64_t C, const int32_t *__restrict__ vals,
                                                          int K, int L, double *__restrict__ state) {
  const size_t c0 = (size_t)blockIdx.x * 256;
  const uint32_t lane = threadIdx.x;
  if (c0 + lane >= (size_t)C) return;
  const int k = (int)blockIdx.z, l0 = (int)blockIdx.y * kLagTile;
  const size_t stat = (size_t)PR * (size_t)C, KC = (size_t)K * (size_t)C, kc = (size_t)k * (size_t)C + c0;      // (uniform)
  double *S = state, *Y = state + (size_t)(L + 1) * KC;
  const double *ring = Y + KC, *head = ring + (size_t)L * KC;
  const double *wv = window + ((size_t)vals[k] * (size_t)C + c0);
  const double a = g0 > 0 ? (head + kc)[lane] : wv[lane];
  double s[kLagTile], w[kLagTile];
#pragma unroll
  for (int j = 0; j < kLagTile; ++j) s[j] = l0 + j <= L ? (S + ((size_t)(l0 + j) * KC + kc))[lane] : 0.0;
  double ysum = l0 == 0 ? (Y + kc)[lane] : 0.0;
  // before row g0: w[j] = y_(g0 - 1 - l0 - j), so that the shift of the first row puts every value in its place (w[7] leaves unused)
#pragma unroll
  for (int j = 0; j < kLagTile; ++j) {
    const int64_t i = g0 - 1 - l0 - j;
    w[j] = (i >= 0 && l0 + j + 1 <= L) ? (ring + ((size_t)(i % L) * KC + kc))[lane] - a : 0.0;
  }
  int64_t e = g0 - l0;                                  // the row entering the tile with row g0
  int64_t slot = ((e % L) + L) % L;                     // e mod L, kept in step with e
  for (int64_t r = 0; r < nrows; r += kAhead) {
    double xt[kAhead], xe[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      xt[u] = xe[u] = a;
      if (r + u < nrows) {
        xt[u] = (wv + (size_t)(r + u) * stat)[lane];
        if (l0 > 0) {
          if (e >= g0) xe[u] = (wv + (size_t)(e - g0) * stat)[lane];
          else if (e >= 0) xe[u] = (ring + ((size_t)slot * KC + kc))[lane];
        }
      }
      ++e;
      slot = slot + 1 == L ? 0 : slot + 1;
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (r + u >= nrows) break;
      const int64_t g = g0 + r + u;
      const double yt = xt[u] - a;
#pragma unroll
      for (int j = kLagTile - 1; j > 0; --j) w[j] = w[j - 1];
      w[0] = l0 > 0 ? xe[u] - a : yt;
      if (l0 == 0) ysum += yt;
      const int64_t last = g - l0 < (int64_t)(L - l0) ? g - l0 : (int64_t)(L - l0);      // the tile's lags j <= last exist at this row
#pragma unroll
      for (int j = 0; j < kLagTile; ++j)
        if (j <= last) s[j] += yt * w[j];
    }
  }
#pragma unroll
  for (int j = 0; j < kLagTile; ++j)
    if (l0 + j <= L) (S + ((size_t)(l0 + j) * KC + kc))[lane] = s[j];
  if (l0 == 0) (Y + kc)[lane] = ysum;
}

// ---- after the lag sums of the same window, on the same stream (so no slot is overwritten that they still read): the window's last m = min(nrows, L) rows go to
// the ring, row g to slot g mod L, and its rows g < L to head[g].  blockIdx = (chains / 256, value, z < m): ring row nrows - m + z, head row z.
__global__ void __launch_bounds__(256) autocov_carry_kernel(const double *__restrict__ window, int64_t g0, int64_t nrows, int PR, int64_t C, const int32_t *__restrict__ vals,
                                                            int K, int L, double *__restrict__ state) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= (size_t)C) return;
  const int k = blockIdx.y;
  const int64_t z = blockIdx.z, m = nrows < L ? nrows : (int64_t)L;
  const size_t stat = (size_t)PR * (size_t)C, KC = (size_t)K * (size_t)C, kc = (size_t)k * (size_t)C + c;
  double *ring = state + (size_t)(L + 2) * KC, *head = ring + (size_t)L * KC;
  const double *wv = window + ((size_t)vals[k] * (size_t)C + c);
  const int64_t r = nrows - m + z;
  ring[(size_t)((g0 + r) % L) * KC + kc] = wv[(size_t)r * stat];
  if (g0 + z < L && z < nrows) head[(size_t)(g0 + z) * KC + kc] = wv[(size_t)z * stat];
}

// ---- per chain and value, after the last window: gamma [L + 1][K][C] and m [K][C] (amwg_autocov.h); H and T run over the lags, so a thread walks them in order
__global__ void __launch_bounds__(256) autocov_chain_kernel(const double *__restrict__ state, int64_t n, int64_t C, int K, int L, double *__restrict__ gamma,
                                                            double *__restrict__ mean) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= (size_t)C) return;
  const size_t KC = (size_t)K * (size_t)C, kc = (size_t)blockIdx.y * (size_t)C + c;
  const double *S = state, *Y = state + (size_t)(L + 1) * KC, *ring = Y + KC, *head = ring + (size_t)L * KC;
  const double a = head[kc], y = Y[kc], yb = y / (double)n;
  mean[kc] = a + yb;
  double H = 0.0, T = 0.0;
  int64_t slot = (n - 1) % L;      // of row n - 1 - l
  for (int l = 0; l <= L; ++l) {
    gamma[(size_t)l * KC + kc] = ((S[(size_t)l * KC + kc] - yb * ((y - H) + (y - T))) + (double)(n - l) * (yb * yb)) / (double)n;
    if (l < L) {
      H += head[(size_t)l * KC + kc] - a;
      T += ring[(size_t)slot * KC + kc] - a;
      slot = slot == 0 ? L - 1 : slot - 1;
    }
  }
}

// ---- per (dataset d, value k, z): z <= L the autocovariance at lag z; z = L + 1 the mean and the between-chain variance.  fold_moments_kernel's order: thread t
// takes the dataset's chains t, t + 256, ..., block_sum's halving tree adds the 256 partial sums.
__global__ void __launch_bounds__(256) autocov_dataset_kernel(const double *__restrict__ gamma, const double *__restrict__ mean, int64_t C, int64_t cpd, int K, int L,
                                                              double *__restrict__ acov, double *__restrict__ gmean, double *__restrict__ between) {
  __shared__ double red[256];
  const int d = blockIdx.x, k = blockIdx.y, z = blockIdx.z, tid = threadIdx.x, nt = blockDim.x;
  const size_t KC = (size_t)K * (size_t)C, off = (size_t)k * (size_t)C + (size_t)d * (size_t)cpd;
  const double *g = gamma + ((size_t)(z <= L ? z : 0) * KC + off), *m = mean + off;
  double sg = 0;
  for (int64_t c = tid; c < cpd; c += nt) sg += g[c];
  const double ac = block_sum(sg, red) / (double)cpd;
  if (z <= L) {
    if (tid == 0) acov[((size_t)d * K + k) * (size_t)(L + 1) + z] = ac;
    return;
  }
  double sm = 0;
  for (int64_t c = tid; c < cpd; c += nt) sm += m[c];
  const double gm = block_sum(sm, red) / (double)cpd;
  double sb = 0;
  for (int64_t c = tid; c < cpd; c += nt) { const double dm = m[c] - gm; sb += dm * dm; }
  const double tot = block_sum(sb, red);
  if (tid == 0) {
    const bool finite = fabs(ac) < std::numeric_limits<double>::infinity();      // (acov_0: false for a NaN too)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    gmean[(size_t)d * K + k] = finite ? gm : nan;
    between[(size_t)d * K + k] = !finite ? nan : cpd > 1 ? tot / (double)(cpd - 1) : 0.0;
  }
}

bool mul_fits(size_t a, size_t b, size_t *out) { return !__builtin_mul_overflow(a, b, out); }

// ---- the autocovariance armed per sampler.  Beside the handle, not in it: amwg_sampler.h is one of the sources the step kernels' id is formed from
std::mutex g_acf_mu;
std::unordered_map<const amwg_sampler *, AutocovArm> g_acf;
void free_arm(AutocovArm &a) {
  if (a.d_values) (void)hipFree(a.d_values);
  if (a.d_state) (void)hipFree(a.d_state);
  a = AutocovArm();
}

}  // namespace

int amwg_autocov_lag_check(const char *call, int32_t L) {
  if (L < 1 || L > kAutocovMaxLag) return amwg_fail(AMWG_EINVAL, "%s: max_lag %d (1 to %d)", call, (int)L, (int)kAutocovMaxLag);
  return AMWG_OK;
}

bool amwg_autocov_state_elems(int32_t K, int64_t C, int32_t L, size_t *elems) {
  size_t kc, bytes;
  if (!mul_fits((size_t)K, (size_t)C, &kc) || !mul_fits(kc, (size_t)(3 * (size_t)L + 2), elems) || !mul_fits(*elems, 8, &bytes)) return false;
  return true;
}

int amwg_autocov_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int32_t K, int32_t L) {
  if (rows < 1 || PR < 1 || PR > 65535 || C < 1 || D < 1 || D > 65535 || C % D != 0)
    return amwg_fail(AMWG_EINVAL, "%s: bad shape (rows %lld, values %d, chains %lld, datasets %d -- at most 65535, dividing the chains)", call, (long long)rows, PR, (long long)C, D);
  if (K < 1 || K > PR) return amwg_fail(AMWG_EINVAL, "%s: %d values (1 to %d, the recorded values)", call, (int)K, PR);
  TRYB(amwg_autocov_lag_check(call, L));
  if ((int64_t)L >= rows) return amwg_fail(AMWG_EINVAL, "%s: max_lag %d needs more than %d kept draws per chain (got %lld)", call, (int)L, (int)L, (long long)rows);
  size_t row_bytes, bytes, elems;
  if (!mul_fits((size_t)PR * 8, (size_t)C, &row_bytes) || !mul_fits(row_bytes, (size_t)rows, &bytes) || !amwg_autocov_state_elems(K, C, L, &elems) ||
      !mul_fits((size_t)K * (size_t)(L + 2) * 8, (size_t)D, &bytes))
    return amwg_fail(AMWG_EINVAL, "%s: array too large (a byte count beyond size_t)", call);
  return AMWG_OK;
}

int amwg_autocov_window(const double *window, int64_t g0, int64_t nrows, int PR, int64_t C, const int32_t *d_values, int32_t K, int32_t L, double *state,
                        hipStream_t stream) {
  if (!window || !d_values || !state || g0 < 0 || nrows < 1 || PR < 1 || PR > 65535 || C < 1 || K < 1 || K > PR || L < 1 || L > kAutocovMaxLag)
    return amwg_fail(AMWG_EINVAL, "internal: lag sums of rows [%lld, +%lld) of %d of %d values x %lld chains, max_lag %d", (long long)g0, (long long)nrows, (int)K, PR, (long long)C, (int)L);
  const unsigned gx = (unsigned)((C + 255) / 256);
  const int tiles = L / kLagTile + 1;      // lags 0 .. L
  const int64_t m = nrows < L ? nrows : (int64_t)L;
  hipLaunchKernelGGL(autocov_lag_kernel, dim3(gx, (unsigned)tiles, (unsigned)K), dim3(256), 0, stream, window, g0, nrows, PR, C, d_values, (int)K, (int)L, state);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(autocov_carry_kernel, dim3(gx, (unsigned)K, (unsigned)m), dim3(256), 0, stream, window, g0, nrows, PR, C, d_values, (int)K, (int)L, state);
  HIP_TRY(hipGetLastError());
  return AMWG_OK;
}

int amwg_autocov_collect(const double *state, int64_t rows, int64_t C, int D, int32_t K, int32_t L, const std::vector<int32_t> &where, double *acov, double *mean,
                         double *between, hipStream_t stream) {
  if (!state || !acov || !mean || !between || rows <= L || C < 1 || D < 1 || D > 65535 || C % D != 0 || K < 1 || K > 65535 || L < 1 || L > kAutocovMaxLag || (int32_t)where.size() != K)
    return amwg_fail(AMWG_EINVAL, "internal: autocovariance of %d values, %lld chains of %lld rows in %d datasets, max_lag %d", (int)K, (long long)C, (long long)rows, D, (int)L);
  const size_t KC = (size_t)K * (size_t)C, DK = (size_t)D * (size_t)K, out_elems = DK * (size_t)(L + 3);
  DevBuf per_chain, out;      // gamma [L + 1][K][C], m [K][C]; acov [D][K][L + 1], mean [D][K], between [D][K]
  HIP_TRY(per_chain.alloc((size_t)(L + 2) * KC * 8));
  HIP_TRY(out.alloc(out_elems * 8));
  double *gamma = per_chain.as<double>(), *m = gamma + (size_t)(L + 1) * KC;
  double *d_acov = out.as<double>(), *d_mean = d_acov + DK * (size_t)(L + 1), *d_between = d_mean + DK;
  hipLaunchKernelGGL(autocov_chain_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)K), dim3(256), 0, stream, state, rows, C, (int)K, (int)L, gamma, m);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(autocov_dataset_kernel, dim3((unsigned)D, (unsigned)K, (unsigned)(L + 2)), dim3(256), 0, stream, gamma, m, C, C / D, (int)K, (int)L, d_acov, d_mean, d_between);
  HIP_TRY(hipGetLastError());
  std::vector<double> host(out_elems);
  HIP_TRY(hipMemcpyAsync(host.data(), out.p, out_elems * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  const double *ha = host.data(), *hm = ha + DK * (size_t)(L + 1), *hb = hm + DK;
  for (int d = 0; d < D; ++d)
    for (int k = 0; k < K; ++k) {      // (the device worked on the ascending list)
      const size_t to = (size_t)d * K + k, from = (size_t)d * K + where[k];
      std::copy(ha + from * (size_t)(L + 1), ha + (from + 1) * (size_t)(L + 1), acov + to * (size_t)(L + 1));
      mean[to] = hm[from];
      between[to] = hb[from];
    }
  return AMWG_OK;
}

int amwg_autocov_of_array(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const int32_t *values, int32_t K, int32_t L, int64_t window_rows,
                          double *acov, double *mean, double *between, hipStream_t stream) {
  if (!draws || !acov || !mean || !between) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (window_rows < 0) return amwg_fail(AMWG_EINVAL, "%s: bad shape (window_rows %lld)", call, (long long)window_rows);
  TRYB(amwg_autocov_shape(call, rows, PR, C, D, K, L));
  TRYB(amwg_covariance_values_check(call, values, K, PR));
  std::vector<int32_t> sorted, where;
  amwg_covariance_order(values, K, &sorted, &where);
  size_t elems = 0;
  (void)amwg_autocov_state_elems(K, C, L, &elems);      // (fits: amwg_autocov_shape)
  const size_t row_elems = (size_t)PR * (size_t)C;
  DevBuf st, dv;
  HIP_TRY(st.alloc(elems * 8));
  HIP_TRY(dv.alloc((size_t)K * 4));
  HIP_TRY(hipMemcpyAsync(dv.p, sorted.data(), (size_t)K * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(st.p, 0, elems * 8, stream));      // (the zeroed state a summarising call starts from too)
  const int64_t w = window_rows > 0 ? window_rows : rows;
  for (int64_t g0 = 0; g0 < rows; g0 += w) {      // (window after window, as launch_steps enqueues them)
    const int64_t n = rows - g0 < w ? rows - g0 : w;
    TRYB(amwg_autocov_window(draws + (size_t)g0 * row_elems, g0, n, PR, C, dv.as<int32_t>(), K, L, st.as<double>(), stream));
  }
  return amwg_autocov_collect(st.as<double>(), rows, C, D, K, L, where, acov, mean, between, stream);
}

AutocovArm *amwg_autocov_armed(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_acf_mu);
  auto it = g_acf.find(s);      // (pointers into an unordered_map stay valid while other entries come and go)
  return it == g_acf.end() || it->second.n_values < 1 ? nullptr : &it->second;
}

int amwg_autocov_begin(amwg_sampler *s, int64_t rows, AutocovArm **arm) {
  AutocovArm *a = amwg_autocov_armed(s);
  *arm = a;
  if (!a) return AMWG_OK;
  if (rows <= (int64_t)a->max_lag)
    return amwg_fail(AMWG_EINVAL, "amwg_sample_summarize: max_lag %d needs more than %d kept draws per chain (got %lld) -- the autocovariance armed with amwg_set_autocovariance", (int)a->max_lag, (int)a->max_lag, (long long)rows);
  HIP_TRY(hipMemsetAsync(a->d_state, 0, a->state_bytes, s->stream));      // (each summarising call starts afresh)
  a->folded = true;
  return AMWG_OK;
}

void amwg_autocov_forget(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_acf_mu);
  auto it = g_acf.find(s);
  if (it == g_acf.end()) return;
  free_arm(it->second);
  g_acf.erase(it);
}

extern "C" {

int amwg_set_autocovariance(amwg_sampler *s, const int32_t *values, int32_t n_values, int32_t max_lag) {
  const char *call = "amwg_set_autocovariance";
  if (!s) return amwg_fail(AMWG_EINVAL, "%s: null sampler", call);
  const bool disarm = !values && n_values == 0 && max_lag == 0;
  const int PR = s->P + s->D;
  size_t elems = 0;
  if (!disarm) {
    if (!values) return amwg_fail(AMWG_EINVAL, "%s: null values (NULL, 0, 0 disarms)", call);
    TRYB(amwg_covariance_values_check(call, values, n_values, PR));
    TRYB(amwg_autocov_lag_check(call, max_lag));
    if (!amwg_autocov_state_elems(n_values, s->C, max_lag, &elems)) return amwg_fail(AMWG_EINVAL, "%s: array too large (a byte count beyond size_t)", call);
  }
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));      // (a summarising call still in flight adds to the state that goes away)
  amwg_autocov_forget(s);
  if (disarm) return AMWG_OK;
  AutocovArm a;
  std::vector<int32_t> sorted;
  amwg_covariance_order(values, n_values, &sorted, &a.where);
  a.values.assign(values, values + n_values);
  const size_t list_bytes = (size_t)n_values * 4;
  a.state_bytes = elems * 8;
  if (hipMalloc(reinterpret_cast<void **>(&a.d_values), list_bytes) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&a.d_state), a.state_bytes) != hipSuccess ||
      hipMemcpy(a.d_values, sorted.data(), list_bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemset(a.d_state, 0, a.state_bytes) != hipSuccess) {
    const size_t want = a.state_bytes + list_bytes;
    free_arm(a);
    return amwg_fail(AMWG_EHIP, "%s: cannot place %zu bytes of lag sums, rows and values on the device", call, want);
  }
  a.n_values = n_values;
  a.max_lag = max_lag;
  a.bytes = a.state_bytes + list_bytes;
  std::lock_guard<std::mutex> lock(g_acf_mu);
  g_acf[s] = a;
  return AMWG_OK;
}

int amwg_autocovariance_info(const amwg_sampler *s, int32_t *n_values, int32_t *max_lag, size_t *bytes) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_autocovariance_info: null sampler");
  const AutocovArm *a = amwg_autocov_armed(s);
  if (n_values) *n_values = a ? a->n_values : 0;
  if (max_lag) *max_lag = a ? a->max_lag : 0;
  if (bytes) *bytes = a ? a->bytes : 0;
  return AMWG_OK;
}

int amwg_last_sample_dataset_autocovariance(amwg_sampler *s, const int32_t *values, int32_t n_values, int32_t max_lag, double *acov, double *mean, double *between) {
  const char *call = "amwg_last_sample_dataset_autocovariance";
  if (!s || !acov || !mean || !between) return amwg_fail(AMWG_EINVAL, "%s: null %s", call, !s ? "sampler" : !acov ? "acov" : !mean ? "mean" : "between");
  if (n_values < 1) return amwg_fail(AMWG_EINVAL, "%s: %d values (at least 1)", call, (int)n_values);
  TRYB(amwg_autocov_lag_check(call, max_lag));
  const int PR = s->P + s->D, D = s->n_datasets;
  if (amwg_summarised(s)) {      // the draws were not kept: only what was folded while they passed can be returned
    const AutocovArm *a = amwg_autocov_armed(s);
    if (values || !a || !a->folded || a->n_values != n_values || a->max_lag != max_lag)
      return amwg_fail(AMWG_EINVAL, "%s: the last sample call was amwg_sample_summarize, which kept no draw: %s", call,
                       values ? "values cannot be given afterwards -- arm them with amwg_set_autocovariance before the call, and pass NULL here"
                       : !a || !a->folded ? "no autocovariance was armed for it (amwg_set_autocovariance before the call)"
                                          : "the number of values or max_lag differs from what was armed with amwg_set_autocovariance");
    TRYB(amwg_autocov_shape(call, s->last_rows, PR, s->C, D, n_values, max_lag));
    HIP_TRY(hipSetDevice(s->device));
    return amwg_autocov_collect(a->d_state, s->last_rows, s->C, D, n_values, max_lag, a->where, acov, mean, between, s->stream);
  }
  if (!values) return amwg_fail(AMWG_EINVAL, "%s: null values (NULL asks for what a summarising call folded for the values of amwg_set_autocovariance; the last sample call was none)", call);
  TRYB(amwg_covariance_values_check(call, values, n_values, PR));
  if (!s->last_draws || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "%s: no sample() call yet", call);
  TRYB(amwg_autocov_shape(call, s->last_rows, PR, s->C, D, n_values, max_lag));
  HIP_TRY(hipSetDevice(s->device));
  return amwg_autocov_of_array(call, s->last_draws, s->last_rows, PR, s->C, D, values, n_values, max_lag, 0, acov, mean, between, s->stream);
}

}  // extern "C"
