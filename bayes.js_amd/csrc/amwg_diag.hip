// amwg_diag.hip -- what a caller can ask about a sampler and its draws (moments, R-hat / ESS, stepper state, launch geometry, kernel name), about the
// library (version, last error) and about the device (fp64 peak); the host build of the kernel arithmetic; the small kernels these need.  A summary has ONE
// launcher, over D datasets of C / D chains each: the pooled call of an ordinary sampler is its case D = 1.
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "amwg_build_id.h"
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_math.h"
#include "amwg_philox.h"

using namespace amwg;

namespace {
// per chain and recorded value: mean and (n-1) variance of each half of the chain's kept draws
// out[((h*2 + stat) * PR + p) * C + c], stat 0 = mean, 1 = variance; draws [row][PR][C] (coalesced over chains)
__global__ void chain_halves_kernel(const double *draws, int64_t rows, int PR, int64_t C, double *out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (c >= C) return;
  const int64_t half = rows / 2;
  for (int h = 0; h < 2; ++h) {
    const int64_t r0 = h * half, r1 = r0 + half;
    double m = 0, m2 = 0;   // Welford
    for (int64_t r = r0; r < r1; ++r) welford_add(draws[(r * PR + p) * C + c], r - r0 + 1, m, m2);
    out[((size_t)(h * 2 + 0) * PR + p) * C + c] = m;
    out[((size_t)(h * 2 + 1) * PR + p) * C + c] = half > 1 ? m2 / (double)(half - 1) : 0.0;
  }
}

// ---- summaries per dataset, one workgroup per (recorded value, dataset); dataset d owns the chains [d * cpd, (d + 1) * cpd).  An ordinary sampler is
// one dataset of all its chains (cpd = C).  Their sums go through block_sum (amwg_fold.h).
// mean and sd (n - 1 denominator) over the dataset's chains x kept draws, in a fixed order: thread t sums the values i = t, t + 1024, ... of the dataset's
// rows laid end to end, a halving tree adds the 1024 partial sums; a second pass for the squares about the mean.  out [D][PR] each
__global__ void __launch_bounds__(1024) dataset_moments_kernel(const double *draws, int64_t rows, int PR, int64_t C, int64_t cpd, double *mean, double *sd) {
  __shared__ double red[1024];
  const int p = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int64_t n = rows * cpd, c0 = (int64_t)d * cpd;
  double sum = 0;
  for (int64_t i = tid; i < n; i += nt) sum += draws[((i / cpd) * PR + p) * C + c0 + (i % cpd)];
  const double m = block_sum(sum, red) / (double)n;
  double ss = 0;
  for (int64_t i = tid; i < n; i += nt) { const double dlt = draws[((i / cpd) * PR + p) * C + c0 + (i % cpd)] - m; ss += dlt * dlt; }
  const double tot = block_sum(ss, red);
  if (tid == 0) { mean[(size_t)d * PR + p] = m; sd[(size_t)d * PR + p] = n > 1 ? sqrt(tot / (double)(n - 1)) : 0.0; }
}
// split-R-hat and ESS of one dataset from the per-chain halves (chain_halves_kernel's layout): the definition of amwg_last_sample_diagnostics over the
// dataset's cpd chains; out [D][PR] each
__global__ void __launch_bounds__(256) dataset_diagnostics_kernel(const double *hv, int64_t rows, int PR, int64_t C, int64_t cpd, double *rhat, double *ess) {
  __shared__ double red[256];
  const int p = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int64_t c0 = (int64_t)d * cpd;
  const double *m0 = hv + ((size_t)0 * PR + p) * C + c0, *v0 = hv + ((size_t)1 * PR + p) * C + c0, *m1 = hv + ((size_t)2 * PR + p) * C + c0, *v1 = hv + ((size_t)3 * PR + p) * C + c0;
  const double n = (double)(rows / 2), m = 2.0 * (double)cpd;      // 2 cpd half-chains of n draws
  double sm = 0, sw = 0, smc = 0;
  for (int64_t c = tid; c < cpd; c += nt) { sm += m0[c] + m1[c]; sw += v0[c] + v1[c]; smc += 0.5 * (m0[c] + m1[c]); }
  const double W = block_sum(sw, red) / m, gm = block_sum(sm, red) / m, gmc = block_sum(smc, red) / (double)cpd;
  double sb = 0, sbc = 0;
  for (int64_t c = tid; c < cpd; c += nt) {
    const double a = m0[c] - gm, b = m1[c] - gm, w = 0.5 * (m0[c] + m1[c]) - gmc;
    sb += a * a + b * b;
    sbc += w * w;
  }
  const double B_over_n = block_sum(sb, red) / (m - 1), var_chain_mean = block_sum(sbc, red) / ((double)cpd - 1);
  const double var_plus = (n - 1) / n * W + B_over_n;
  if (tid == 0) {
    rhat[(size_t)d * PR + p] = W > 0 ? sqrt(var_plus / W) : __builtin_nan("");
    ess[(size_t)d * PR + p] = var_chain_mean > 0 ? (double)cpd * var_plus / var_chain_mean : __builtin_nan("");
  }
}

// ---- summaries without stored draws (amwg_sample_summarize; amwg_fold.h).  One thread per (chain, recorded value), the chain the fastest index: a wavefront's 64
// loads of one row are one contiguous 512-byte run.  The accumulators are read once into registers and written once.  The Welford chains are serial per thread and
// carry an fp64 division, but the loads do not depend on them: kFoldAhead rows are fetched into registers ahead of the dependent updates, so a wavefront's time per
// row is the arithmetic and not a load's latency.  Which half a row belongs to is decided per row from its global index -- the same for every lane of a wavefront --,
// so a window may begin and end anywhere: a row crossing from the first half into the second, and the odd last row, need no special window.
constexpr int kFoldAhead = 8;
__global__ void __launch_bounds__(256) fold_window_kernel(const double *__restrict__ window, int64_t g0, int64_t nrows, int64_t half, int PR, int64_t C, double *__restrict__ acc) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (c >= C) return;
  const size_t stat = (size_t)PR * (size_t)C, at = (size_t)p * (size_t)C + (size_t)c;
  double m0 = acc[0 * stat + at], s0 = acc[1 * stat + at], m1 = acc[2 * stat + at], s1 = acc[3 * stat + at], ma = acc[4 * stat + at], sa = acc[5 * stat + at];
  const double *col = window + at;
  for (int64_t r = 0; r < nrows; r += kFoldAhead) {
    double x[kFoldAhead];
#pragma unroll
    for (int u = 0; u < kFoldAhead; ++u) x[u] = r + u < nrows ? col[(size_t)(r + u) * stat] : 0.0;
#pragma unroll
    for (int u = 0; u < kFoldAhead; ++u) {
      if (r + u >= nrows) break;
      const int64_t g = g0 + r + u;      // the row's index among the chain's kept draws
      if (g < half) welford_add(x[u], g + 1, m0, s0);
      else if (g < 2 * half) welford_add(x[u], g - half + 1, m1, s1);
      welford_add(x[u], g + 1, ma, sa);
    }
  }
  acc[0 * stat + at] = m0; acc[1 * stat + at] = s0; acc[2 * stat + at] = m1; acc[3 * stat + at] = s1; acc[4 * stat + at] = ma; acc[5 * stat + at] = sa;
}
// the accumulated halves in chain_halves_kernel's layout and with its last operation: out[((h*2 + stat) * PR + p) * C + c], the half M2 as (n-1) variances
__global__ void __launch_bounds__(256) fold_halves_kernel(const double *__restrict__ acc, int64_t rows, int PR, int64_t C, double *__restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (c >= C) return;
  const int64_t half = rows / 2;
  for (int h = 0; h < 2; ++h) {
    const double m = acc[((size_t)(h * 2 + 0) * PR + p) * C + c], m2 = acc[((size_t)(h * 2 + 1) * PR + p) * C + c];
    out[((size_t)(h * 2 + 0) * PR + p) * C + c] = m;
    out[((size_t)(h * 2 + 1) * PR + p) * C + c] = half > 1 ? m2 / (double)(half - 1) : 0.0;
  }
}
// mean and sd (n - 1 denominator) of a dataset's chains x kept draws from the whole-chain pairs (m_c, M2_c) of its cpd chains, every chain of `rows` draws, in a
// fixed order (thread t takes the chains t, t + 256, ...; block_sum's halving tree): mean = sum m_c / cpd, SS = sum M2_c + rows sum (m_c - mean)^2.  out [D][PR] each
__global__ void __launch_bounds__(256) fold_moments_kernel(const double *__restrict__ acc, int64_t rows, int PR, int64_t C, int64_t cpd, double *mean, double *sd) {
  __shared__ double red[256];
  const int p = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const double *mc = acc + ((size_t)4 * PR + p) * C + (size_t)d * cpd, *m2c = acc + ((size_t)5 * PR + p) * C + (size_t)d * cpd;
  double sm = 0, s2 = 0;
  for (int64_t c = tid; c < cpd; c += nt) { sm += mc[c]; s2 += m2c[c]; }
  const double m = block_sum(sm, red) / (double)cpd, within = block_sum(s2, red);
  double sb = 0;
  for (int64_t c = tid; c < cpd; c += nt) { const double dlt = mc[c] - m; sb += dlt * dlt; }
  const double ss = within + (double)rows * block_sum(sb, red);
  const double n = (double)rows * (double)cpd;
  if (tid == 0) { mean[(size_t)d * PR + p] = m; sd[(size_t)d * PR + p] = n > 1 ? sqrt(ss / (n - 1)) : 0.0; }
}

// 8 independent fma chains per lane, no memory traffic: the fp64 issue rate the chip sustains
__global__ void __launch_bounds__(1024) fp64_peak_kernel(double *out, int iters, double a, double b) {
  double x0 = threadIdx.x, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      x0 = __builtin_fma(x0, a, b); x1 = __builtin_fma(x1, a, b); x2 = __builtin_fma(x2, a, b); x3 = __builtin_fma(x3, a, b);
      x4 = __builtin_fma(x4, a, b); x5 = __builtin_fma(x5, a, b); x6 = __builtin_fma(x6, a, b); x7 = __builtin_fma(x7, a, b);
    }
  }
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7));
}

}  // namespace

thread_local std::string g_err;

int amwg_fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// a pooled summary over the chains of a dataset sampler would mix posteriors that have nothing to do with each other
int amwg_refuse_pooled(const amwg_sampler *s, const char *call) {
  if (s && s->n_datasets > 1)
    return amwg_fail(AMWG_EINVAL, "%s: this sampler runs %d datasets, a posterior each: pooled summaries are refused -- use amwg_last_sample_dataset_moments / amwg_last_sample_dataset_diagnostics / amwg_last_sample_dataset_quantiles", call, s->n_datasets);
  return AMWG_OK;
}

// ---- the launchers behind the summaries of the last sample call, over D datasets of C / D chains each (D = 1: pooled over all chains)
// mean and sd, [D][PR] each
static int last_sample_moments(amwg_sampler *s, int D, double *mean, double *sd) {
  HIP_TRY(hipSetDevice(s->device));
  const int PR = s->P + s->D;
  if (!amwg_summarised(s)) return amwg_moments_launch(s->last_draws, s->last_rows, PR, s->C, D, mean, sd, s->stream);
  const size_t n = (size_t)D * PR;
  DevBuf buf;
  HIP_TRY(buf.alloc(n * 16));
  double *dm = buf.as<double>();
  const FoldSummary *f = amwg_summary_of(s);      // (amwg_sample_summarize: from the whole-chain accumulators)
  if (!f || !f->acc) return amwg_fail(AMWG_EINVAL, "internal: a summarised sampler without accumulators");
  TRYB(amwg_fold_moments(f->acc, s->last_rows, PR, s->C, D, dm, dm + n, s->stream));
  HIP_TRY(hipMemcpyAsync(mean, dm, n * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(sd, dm + n, n * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMWG_OK;
}
// the halves of every chain (chain_halves_kernel's layout, 4 PR C doubles) in a scratch buffer, queued on the sampler's stream
static int last_sample_halves(amwg_sampler *s, DevBuf *halves) {
  HIP_TRY(hipSetDevice(s->device));
  const int PR = s->P + s->D;
  const size_t C = (size_t)s->C;
  HIP_TRY(halves->alloc(4 * (size_t)PR * C * 8));
  if (amwg_summarised(s)) {      // (amwg_sample_summarize: the halves were accumulated window by window, by the same recurrence)
    const FoldSummary *f = amwg_summary_of(s);
    if (!f || !f->acc) return amwg_fail(AMWG_EINVAL, "internal: a summarised sampler without accumulators");
    return amwg_fold_halves(f->acc, s->last_rows, PR, s->C, halves->as<double>(), s->stream);
  }
  return amwg_chain_halves(s->last_draws, s->last_rows, PR, s->C, halves->as<double>(), s->stream);
}

// ---- amwg_fold.h: the summaries over a device array (the sampler's calls above and below, and the selftest entry amwg_summaries_check)
int amwg_diagnostics_refusal(const char *call, bool have, int64_t rows, int64_t C, int D, bool per_dataset) {
  if (have && D >= 1 && rows >= 4 && C / D >= 2) return AMWG_OK;
  return amwg_fail(AMWG_EINVAL, "%s: needs a sample() of >= 4 kept draws on >= 2 chains%s", call, per_dataset ? " per dataset" : "");
}
int amwg_moments_launch(const double *draws, int64_t rows, int PR, int64_t C, int D, double *mean, double *sd, hipStream_t stream) {
  const size_t n = (size_t)D * PR;
  DevBuf buf;
  HIP_TRY(buf.alloc(n * 16));
  double *dm = buf.as<double>();
  hipLaunchKernelGGL(dataset_moments_kernel, dim3(PR, D), dim3(1024), 0, stream, draws, rows, PR, C, C / D, dm, dm + n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(mean, dm, n * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(sd, dm + n, n * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return AMWG_OK;
}
int amwg_dataset_diagnostics_launch(const double *halves, int64_t rows, int PR, int64_t C, int D, double *rhat, double *ess, hipStream_t stream) {
  const size_t n = (size_t)D * PR;
  DevBuf out;
  HIP_TRY(out.alloc(n * 16));
  double *dr = out.as<double>();
  hipLaunchKernelGGL(dataset_diagnostics_kernel, dim3(PR, D), dim3(256), 0, stream, halves, rows, PR, C, C / D, dr, dr + n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(rhat, dr, n * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(ess, dr + n, n * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return AMWG_OK;
}
int amwg_pooled_diagnostics(const double *halves, int64_t rows, int PR, int64_t Cn, double *rhat, double *ess, hipStream_t stream) {
  const size_t C = (size_t)Cn, n_out = 4 * (size_t)PR * C;
  std::vector<double> h(n_out);
  HIP_TRY(hipMemcpyAsync(h.data(), halves, n_out * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  const double n = (double)(rows / 2), m = 2.0 * (double)C;   // 2C half-chains of n draws
  for (int p = 0; p < PR; ++p) {
    // W = mean within-sequence variance; B/n = variance of the sequence means (over the 2C halves)
    long double sw = 0, sm = 0;
    for (int hf = 0; hf < 2; ++hf)
      for (size_t c = 0; c < C; ++c) { sm += h[((size_t)(hf * 2 + 0) * PR + p) * C + c]; sw += h[((size_t)(hf * 2 + 1) * PR + p) * C + c]; }
    const double W = (double)(sw / m), gm = (double)(sm / m);
    long double sb = 0, sbc = 0;
    for (int hf = 0; hf < 2; ++hf)
      for (size_t c = 0; c < C; ++c) { const double dlt = h[((size_t)(hf * 2 + 0) * PR + p) * C + c] - gm; sb += (long double)dlt * dlt; }
    const double B_over_n = (double)(sb / (m - 1));
    const double var_plus = (n - 1) / n * W + B_over_n;
    rhat[p] = W > 0 ? std::sqrt(var_plus / W) : (double)NAN;
    // whole-chain means: average of the two half means (equal lengths)
    long double smc = 0;
    for (size_t c = 0; c < C; ++c) smc += 0.5 * (h[((size_t)0 * PR + p) * C + c] + h[((size_t)2 * PR + p) * C + c]);
    const double gmc = (double)(smc / (double)C);
    for (size_t c = 0; c < C; ++c) { const double dlt = 0.5 * (h[((size_t)0 * PR + p) * C + c] + h[((size_t)2 * PR + p) * C + c]) - gmc; sbc += (long double)dlt * dlt; }
    const double var_chain_mean = (double)(sbc / ((double)C - 1));
    ess[p] = var_chain_mean > 0 ? (double)C * var_plus / var_chain_mean : (double)NAN;
  }
  return AMWG_OK;
}

// ---- amwg_fold.h: the launchers of the fold kernels (the sampler's summarising call and the selftest entry share them)
int amwg_fold_window(const double *window, int64_t g0, int64_t nrows, int64_t half, int PR, int64_t C, double *acc, hipStream_t stream) {
  if (!window || !acc || g0 < 0 || nrows < 1 || half < 0 || PR < 1 || PR > 65535 || C < 1) return amwg_fail(AMWG_EINVAL, "internal: fold of rows [%lld, +%lld) of %d values x %lld chains", (long long)g0, (long long)nrows, PR, (long long)C);
  hipLaunchKernelGGL(fold_window_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)PR), dim3(256), 0, stream, window, g0, nrows, half, PR, C, acc);
  HIP_TRY(hipGetLastError());
  return AMWG_OK;
}
int amwg_fold_halves(const double *acc, int64_t rows, int PR, int64_t C, double *halves, hipStream_t stream) {
  hipLaunchKernelGGL(fold_halves_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)PR), dim3(256), 0, stream, acc, rows, PR, C, halves);
  HIP_TRY(hipGetLastError());
  return AMWG_OK;
}
int amwg_fold_moments(const double *acc, int64_t rows, int PR, int64_t C, int D, double *mean, double *sd, hipStream_t stream) {
  hipLaunchKernelGGL(fold_moments_kernel, dim3((unsigned)PR, (unsigned)D), dim3(256), 0, stream, acc, rows, PR, C, C / D, mean, sd);
  HIP_TRY(hipGetLastError());
  return AMWG_OK;
}
// the selftest entry's other half: chain_halves_kernel on a stored array
int amwg_chain_halves(const double *draws, int64_t rows, int PR, int64_t C, double *halves, hipStream_t stream) {
  hipLaunchKernelGGL(chain_halves_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)PR), dim3(256), 0, stream, draws, rows, PR, C, halves);
  HIP_TRY(hipGetLastError());
  return AMWG_OK;
}

extern "C" {

const char *amwg_last_error(void) { return g_err.c_str(); }
// which sources this binary was built from (tools/build_id.py: a hash over every source of the library, and one over the device sources + compiler flags)
const char *amwg_version(void) { return "amwg-mi355x 0.4 (gfx950) build " AMWG_BUILD_ID " kernels " AMWG_KERNEL_ID; }

double amwg_exp(double x) { return exp_v8(x); }
double amwg_log(double x) { return log_v8(x); }
double amwg_uniform(uint64_t seed, uint64_t chain, uint64_t index) {
  ChainStream s;
  s.init(seed, chain, index);
  return s.next();
}

int amwg_num_datasets(const amwg_sampler *s) { return s ? s->n_datasets : 0; }
int amwg_dataset_n_obs(const amwg_sampler *s, int32_t *n_obs) {
  if (!s || !n_obs) return amwg_fail(AMWG_EINVAL, "amwg_dataset_n_obs: null argument");
  if (s->ds_n_obs.size() != (size_t)s->n_datasets) { n_obs[0] = s->d.n_obs; return AMWG_OK; }      // (a translated closure: one dataset, whose arrays carry their own lengths -- 0)
  for (int d = 0; d < s->n_datasets; ++d) n_obs[d] = s->ds_n_obs[d];
  return AMWG_OK;
}

int amwg_last_sample_dataset_moments(amwg_sampler *s, double *mean, double *sd) {
  if (!s || !mean || !sd) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_dataset_moments: null argument");
  if ((!s->last_draws && !amwg_summarised(s)) || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_dataset_moments: no sample() call yet");
  return last_sample_moments(s, s->n_datasets, mean, sd);
}

int amwg_last_sample_dataset_diagnostics(amwg_sampler *s, double *rhat, double *ess) {
  if (!s || !rhat || !ess) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_dataset_diagnostics: null argument");
  const int D = s->n_datasets;
  TRYB(amwg_diagnostics_refusal("amwg_last_sample_dataset_diagnostics", s->last_draws || amwg_summarised(s), s->last_rows, s->C, D, true));
  DevBuf halves;
  TRYB(last_sample_halves(s, &halves));
  return amwg_dataset_diagnostics_launch(halves.as<double>(), s->last_rows, s->P + s->D, s->C, D, rhat, ess, s->stream);
}

int amwg_last_sample_diagnostics(amwg_sampler *s, double *rhat, double *ess) {
  if (!s || !rhat || !ess) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_diagnostics: null argument");
  TRYB(amwg_refuse_pooled(s, "amwg_last_sample_diagnostics"));
  TRYB(amwg_diagnostics_refusal("amwg_last_sample_diagnostics", s->last_draws || amwg_summarised(s), s->last_rows, s->C, 1, false));
  DevBuf dout;
  TRYB(last_sample_halves(s, &dout));
  return amwg_pooled_diagnostics(dout.as<double>(), s->last_rows, s->P + s->D, s->C, rhat, ess, s->stream);
}

int amwg_info(amwg_sampler *s, double *pls, int32_t *ac, int32_t *it, int32_t *bc, int64_t *acc, int64_t *inb) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_info: null sampler");
  const size_t PC = (size_t)s->P * (size_t)s->C;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (pls) HIP_TRY(hipMemcpy(pls, s->ch.prop_log_scale, PC * 8, hipMemcpyDeviceToHost));
  if (ac) HIP_TRY(hipMemcpy(ac, s->ch.acceptance_count, PC * 4, hipMemcpyDeviceToHost));
  if (it) HIP_TRY(hipMemcpy(it, s->ch.iterations_since_adaption, PC * 4, hipMemcpyDeviceToHost));
  if (bc) HIP_TRY(hipMemcpy(bc, s->ch.batch_count, PC * 4, hipMemcpyDeviceToHost));
  std::vector<int32_t> tmp(PC);
  for (auto [out, dev] : {std::make_pair(acc, s->ch.accepts), std::make_pair(inb, s->ch.inbounds)}) {      // run totals: 32 bits on the device
    if (!out) continue;
    HIP_TRY(hipMemcpy(tmp.data(), dev, PC * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < PC; ++i) out[i] = tmp[i];
  }
  return AMWG_OK;
}

int amwg_chain_diag(amwg_sampler *s, uint64_t *uniforms, double *log_post_out, int32_t *named_order) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_chain_diag: null sampler");
  const size_t C = (size_t)s->C;
  HIP_TRY(hipSetDevice(s->device));
  // (log_post of the current state as the expression gives it: a 0-step launch computes it where it was never formed or where the stepper's cheaper value stands in)
  if (!s->lp_ready || !s->lp_is_expression) { int rc = launch_steps(s, 0, 1, nullptr, true); if (rc != AMWG_OK) return rc; }
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (uniforms) HIP_TRY(hipMemcpy(uniforms, s->ch.rng_n, C * 8, hipMemcpyDeviceToHost));
  if (log_post_out) HIP_TRY(hipMemcpy(log_post_out, s->ch.lp_curr, C * 8, hipMemcpyDeviceToHost));
  if (named_order && s->ch.perm16) {
    std::vector<uint16_t> p16((size_t)s->n_params * C);
    HIP_TRY(hipMemcpy(p16.data(), s->ch.perm16, p16.size() * 2, hipMemcpyDeviceToHost));
    for (size_t c = 0; c < C; ++c)
      for (int k = 0; k < s->n_params; ++k) named_order[c * s->n_params + k] = (int32_t)p16[(size_t)k * C + c];
  } else if (named_order) {
    std::vector<uint64_t> pv(C);
    HIP_TRY(hipMemcpy(pv.data(), s->ch.perm, C * 8, hipMemcpyDeviceToHost));
    for (size_t c = 0; c < C; ++c)
      for (int k = 0; k < s->n_params; ++k) named_order[c * s->n_params + k] = (int32_t)((pv[c] >> (4 * k)) & 0xF);
  }
  return AMWG_OK;
}

int amwg_last_sample_moments(amwg_sampler *s, double *mean, double *sd) {
  if (!s || !mean || !sd) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_moments: null argument");
  TRYB(amwg_refuse_pooled(s, "amwg_last_sample_moments"));
  if ((!s->last_draws && !amwg_summarised(s)) || s->last_rows < 1) return amwg_fail(AMWG_EINVAL, "amwg_last_sample_moments: no sample() call yet");
  return last_sample_moments(s, 1, mean, sd);      // (one dataset of all the chains: cpd = C)
}

int amwg_tuning(const amwg_sampler *s, int32_t *lanes, double *ms, int32_t cap) {
  if (!s) return 0;
  for (int32_t i = 0; i < cap && i < (int32_t)s->tuned.size(); ++i) {
    if (lanes) lanes[i] = s->tuned[i].first;
    if (ms) ms[i] = s->tuned[i].second;
  }
  return (int)s->tuned.size();
}

int amwg_num_components(const amwg_sampler *s) { return s ? s->P : 0; }
int amwg_num_recorded(const amwg_sampler *s) { return s ? s->P + s->D : 0; }
int64_t amwg_num_chains(const amwg_sampler *s) { return s ? s->C : 0; }

int amwg_launch_info(const amwg_sampler *s, int32_t *lanes, int32_t *block, int32_t *grid, int32_t *lds, int32_t *n_launches, double *kernel_ms) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_launch_info: null sampler");
  if (lanes) *lanes = s->plan.lanes;
  if (block) *block = s->plan.block;
  if (grid) *grid = s->plan.grid;
  if (lds) *lds = s->plan.lds;
  if (n_launches) *n_launches = s->n_launches;
  if (kernel_ms) *kernel_ms = s->kernel_ms;
  return AMWG_OK;
}

int amwg_summation_order(const amwg_sampler *s) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_summation_order: null sampler");
  // (the certified kernels evaluate the expression in the reference's order: amwg_kernel.h kRefOrder)
  return info(s->plan.variant).certified ? 1 : s->plan.lanes;
}

const char *amwg_kernel_name(const amwg_sampler *s) {
  if (!s) { (void)amwg_fail(AMWG_EINVAL, "amwg_kernel_name: null sampler"); return ""; }
  amwg_sampler *m = const_cast<amwg_sampler *>(s);
  if (m->kernel_name.empty()) {
    const LaunchPlan &p = s->plan;
    const int cls = p.block <= 256 ? 256 : (p.block <= 512 ? 512 : 1024);
    // (a dataset sampler launches the kernel's twin, amwg_dataset.h: the same name with the marker _ds)
    const std::string variant_name = std::string(info(p.variant).name) + (s->n_datasets > 1 ? "_ds" : "");
    const char *name = variant_name.c_str();
    static const char *const fam[] = {"NormalModel", "BetaBernModel", "HierNormalModel", "PoisGlmModel"};      // (AMWG_MODEL_* - 1)
    char buf[96];
    if (p.variant == Variant::Step || p.variant == Variant::StepCert)
      snprintf(buf, sizeof buf, "%s<%s,%d,%d>", name, fam[s->model - 1], p.lanes, p.lanes > 64 ? (p.lanes <= 256 ? 256 : (p.lanes <= 512 ? 512 : 1024)) : cls);
    else if (p.variant == Variant::GroupLocal || p.variant == Variant::HierSweep || p.variant == Variant::HierSweepCert)
      snprintf(buf, sizeof buf, "%s<%s,%d>", name, p.variant == Variant::GroupLocal ? "HierGlModel" : "HierNormalModel", cls);
    else snprintf(buf, sizeof buf, "%s", name);      // a translated closure: its hiprtc symbol
    m->kernel_name = buf;
  }
  return m->kernel_name.c_str();
}

int amwg_fp64_peak(int32_t device, double *lane_ops_per_s) {
  if (!lane_ops_per_s) return amwg_fail(AMWG_EINVAL, "amwg_fp64_peak: null argument");
  TRYB(use_device(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  const int blocks = (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256) * 2, threads = 1024, iters = 20000;
  DevBuf dout;
  HIP_TRY(dout.alloc((size_t)blocks * threads * 8));
  EventPair ev;
  HIP_TRY(hipEventCreate(&ev.e0));
  HIP_TRY(hipEventCreate(&ev.e1));
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {    // first repetition warms the clocks up
    HIP_TRY(hipEventRecord(ev.e0, 0));
    hipLaunchKernelGGL(fp64_peak_kernel, dim3(blocks), dim3(threads), 0, 0, dout.as<double>(), iters, 0.999999, 1e-7);
    HIP_TRY(hipEventRecord(ev.e1, 0));
    HIP_TRY(hipEventSynchronize(ev.e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (rep > 0 && ms < best) best = ms;
  }
  *lane_ops_per_s = (double)blocks * threads * (double)iters * 64.0 / (best * 1e-3);
  return AMWG_OK;
}

}  // extern "C"
