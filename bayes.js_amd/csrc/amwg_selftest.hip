// amwg_selftest.hip -- the test-only entry points of include/amwg_selftest.h: the building blocks one by one, for the test suite.  Linked into
// libamwg_selftest.so beside the product's own objects (csrc/Makefile, -DAMWG_SELFTEST); NOT part of libamwg.so.
#include <cstring>

#include "../../include/amwg_selftest.h"
#include "amwg_dataset_quantiles.h"
#include "amwg_autocov.h"
#include "amwg_covariance.h"
#include "amwg_fold.h"
#include "amwg_histogram.h"
#include "amwg_hpd.h"
#include "amwg_loo.h"
#include "amwg_waic.h"
#include "amwg_eval.h"      // device evaluation of the arithmetic building blocks
#include "amwg_host.h"
#include "amwg_kernel.h"
#include "amwg_kval.h"
#include "amwg_models.h"

using namespace amwg;
// tests only: thread j sums the same bit sequence from acc0[j] with addends l1[j], l0[j], once with two_valued_sum and
// once term by term
__global__ void two_valued_check_kernel(const uint32_t *tab, int N, int64_t m, const double *acc0, const double *l1, const double *l0,
                                        double *out_ff, double *out_seq) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const size_t W = BetaBernModel::words(N);
  BitData B{tab, tab + W, tab + 2 * W, tab + 3 * W, tab + 4 * W, tab + 5 * W, N};
  out_ff[j] = two_valued_sum(acc0[j], l1[j], l0[j], B);
  double acc = acc0[j];
  for (int i = 0; i < N; ++i) acc = acc + (((tab[i >> 5] >> (i & 31)) & 1u) ? l1[j] : l0[j]);
  out_seq[j] = acc;
}

// tests only: thread j sums the same sequence of value indices from acc0[j] with the K addends c[j][0 .. K - 1], once with k_valued_sum<K> on the caller's
// tables and once term by term; 64-thread workgroups, so that every wavefront holds 64 different cases (the divergence csrc/amwg_kval.h is shaped for)
template <int K>
__global__ void k_valued_check_kernel(const uint32_t *tab, const uint8_t *idx, int N, int64_t m, const double *acc0, const double *c, double *out_ff, double *out_seq) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  double cs[K];
#pragma unroll
  for (int k = 0; k < K; ++k) cs[k] = c[j * K + k];
  const KValData B{tab, idx, N};
  out_ff[j] = k_valued_sum<K>(acc0[j], cs, B);
  double acc = acc0[j];
  for (int i = 0; i < N; ++i) {
    const int v = (int)idx[i];
    double a = cs[0];
#pragma unroll
    for (int q = 1; q < K; ++q) a = v == q ? cs[q] : a;
    acc = acc + a;
  }
  out_seq[j] = acc;
}
template <int K>
static void k_valued_check_launch(const uint32_t *tab, const uint8_t *idx, int N, int64_t m, const double *acc0, const double *c, double *out_ff, double *out_seq) {
  hipLaunchKernelGGL(k_valued_check_kernel<K>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, 0, tab, idx, N, m, acc0, c, out_ff, out_seq);
}

// tests only (amwg_stream_check): the product's stream classes, drawn from one by one.  Chain c has id chain0 + c and starts at consumed0[c]; the lanes past the
// last chain of a wavefront shadow chain n_chains - 1, as the step kernels' dead lanes do, so that every cross-lane read has its 64 lanes.
__global__ void stream_chain_kernel(uint64_t seed, uint64_t chain0, int64_t n_chains, const uint64_t *consumed0, int64_t n_draws, double *out, uint64_t *consumed_out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chains) return;
  ChainStream s;
  s.init(seed, chain0 + (uint64_t)c, consumed0[c]);
  for (int64_t i = 0; i < n_draws; ++i) out[c * n_draws + i] = s.next();
  consumed_out[c] = s.n;
}

template <int G>
__global__ void stream_coop_kernel(uint64_t seed, uint64_t chain0, int64_t n_chains, const uint64_t *consumed0, int64_t n_draws, double *out, uint64_t *consumed_out) {
  constexpr int L = CoopStream<G>::L;
  const int tid = (int)threadIdx.x;      // (64-thread workgroups: one wavefront)
  int64_t c = (int64_t)blockIdx.x * (64 / L) + tid / L;
  const bool writer = c < n_chains && (tid & (L - 1)) == 0;
  if (c >= n_chains) c = n_chains - 1;
  CoopStream<G> s;
  s.init(seed, chain0 + (uint64_t)c, consumed0[c], tid);
  for (int64_t i = 0; i < n_draws; ++i) {
    const double u = s.next();
    if (writer) out[c * n_draws + i] = u;
  }
  if (writer) consumed_out[c] = s.consumed();
}

// the one-lane stream under a caller's sequence of next() and next_pair() calls (the same sequence for every chain; their starting parities differ)
__global__ void stream_pair_kernel(uint64_t seed, uint64_t chain0, int64_t n_chains, const uint64_t *consumed0, int64_t n_draws, const uint8_t *calls, int64_t n_calls,
                                   double *out, uint64_t *consumed_out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chains) return;
  CoopStream<1> s;
  s.init(seed, chain0 + (uint64_t)c, consumed0[c], (int)threadIdx.x);
  double *o = out + c * n_draws;
  int64_t k = 0;
  for (int64_t j = 0; j < n_calls; ++j) {
    if (calls[j]) {
      if (k + 2 > n_draws) break;      // (the host has checked that the calls add up to n_draws)
      double a, b;
      s.next_pair(a, b);
      o[k++] = a;
      o[k++] = b;
    } else {
      if (k + 1 > n_draws) break;
      o[k++] = s.next();
    }
  }
  consumed_out[c] = s.consumed();
}

// a chain per wavefront on the window stream; with_at: what a sweep does after its draws -- position(), ensure_b(), per-lane reads of the 128 uniforms ahead --, the
// flag words at each stage, and the whole window after a shift() and the next ensure_b()
__global__ void stream_window_kernel(uint64_t seed, uint64_t chain0, const uint64_t *consumed0, int64_t n_draws, int with_at, int64_t width, double *out,
                                     uint64_t *consumed_out, uint64_t *flags) {
  __shared__ double window[256];
  const int64_t c = (int64_t)blockIdx.x;
  const int lane = (int)threadIdx.x;
  WindowStream s;
  s.init(seed, chain0 + (uint64_t)c, consumed0[c], lane, window);
  __syncthreads();
  double *o = out + c * width;
  for (int64_t i = 0; i < n_draws; ++i) {
    const double u = s.next();
    if (lane == 0) o[i] = u;
  }
  if (lane == 0) consumed_out[c] = s.consumed();
  if (!with_at) return;
  uint64_t *f = flags + c * 12;
  const uint32_t p = s.position();
  s.ensure_b();
  if (lane == 0) { f[0] = s.EA; f[1] = s.OA; f[2] = s.EB; f[3] = s.OB; }
  o[n_draws + lane] = s.at(p + (uint32_t)lane);
  o[n_draws + 64 + lane] = s.at(p + 64u + (uint32_t)lane);
  s.shift();
  if (lane == 0) { f[4] = s.EA; f[5] = s.OA; f[6] = s.EB; f[7] = s.OB; }
  s.ensure_b();
  if (lane == 0) { f[8] = s.EA; f[9] = s.OA; f[10] = s.EB; f[11] = s.OB; }
  for (int k = 0; k < 4; ++k) o[n_draws + 128 + 64 * k + lane] = s.at((uint32_t)(64 * k + lane));
}

extern "C" {
double amwg_pow(double x, double y) { return pow_v8(x, y); }
double amwg_log1p(double x) { return log1p_v8(x); }
double amwg_expm1(double x) { return expm1_v8(x); }
double amwg_math1(int32_t fn, double x) { return math1_by_id(fn, x); }
double amwg_math2(int32_t fn, double x, double y) {
  switch (fn) {
    case 0: return atan2_v8(x, y);
    case 1: return hypot2_v8(x, y);
    case 2: return js_mod(x, y);                 // JavaScript's `%`
    case 3: return (double)js_toint32(x);        // `x | 0`
  }
  return __builtin_nan("");
}
double amwg_hypot3(double x, double y, double z) { return hypot3_v8(x, y, z); }
double amwg_ld_host(int32_t id, double x, double a, double b, double c) { return ld_by_id(id, x, a, b, c); }

// include/amwg_selftest.h: the host-side machinery that makes sample()'s destination resident ahead of the device-to-host copies (amwg_run.hip Prefaulter), run on a
// caller's buffer cut into `n_chunks` chunks with `threads` helpers: no byte may change, whatever the alignment and the sizes.  No GPU involved.
int amwg_prefault_selftest(char *buf, size_t bytes, int32_t n_chunks, int32_t threads) {
  if (!buf || n_chunks < 1 || threads < 0 || threads > 16) return amwg_fail(AMWG_EINVAL, "amwg_prefault_selftest: bad argument");
  Prefaulter pf((size_t)n_chunks);
  const size_t per = bytes / (size_t)n_chunks;
  for (int32_t j = 0; j < n_chunks; ++j) pf.add(buf + (size_t)j * per, j == n_chunks - 1 ? bytes - (size_t)j * per : per, (size_t)j);
  pf.start(threads);
  for (int32_t j = 0; j < n_chunks; ++j) pf.wait_chunk((size_t)j);
  return AMWG_OK;
}

int amwg_two_valued_sum_check(int32_t device, const double *x, int32_t n, int64_t m, const double *acc0, const double *l1, const double *l0,
                              double *out_fast_forward, double *out_term_by_term) {
  if (!x || !acc0 || !l1 || !l0 || !out_fast_forward || !out_term_by_term || n < 0 || m < 0) return amwg_fail(AMWG_EINVAL, "amwg_two_valued_sum_check: bad argument");
  TRYB(use_device(device));
  std::vector<uint8_t> xb((size_t)n);
  for (int i = 0; i < n; ++i) xb[i] = x[i] == 1 ? 1 : 0;
  const std::vector<uint32_t> tab = two_valued_tables(xb.data(), n);
  DevBuf dtab, d[5];
  HIP_TRY(dtab.alloc(tab.size() * 4));
  HIP_TRY(hipMemcpy(dtab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  const double *src[3] = {acc0, l1, l0};
  for (int k = 0; k < 5; ++k) {
    HIP_TRY(d[k].alloc((size_t)m * 8));
    if (k < 3 && m) HIP_TRY(hipMemcpy(d[k].p, src[k], (size_t)m * 8, hipMemcpyHostToDevice));
  }
  if (m) hipLaunchKernelGGL(two_valued_check_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, 0, dtab.as<uint32_t>(), n, m,
                            d[0].as<double>(), d[1].as<double>(), d[2].as<double>(), d[3].as<double>(), d[4].as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out_fast_forward, d[3].p, (size_t)m * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_term_by_term, d[4].p, (size_t)m * 8, hipMemcpyDeviceToHost));
  return AMWG_OK;
}

// the library's own copy of the table recipe (amwg_create.hip two_valued_tables), word for word as the samplers and the check above upload it.  No GPU involved.
int amwg_two_valued_tables(const uint8_t *x, int32_t n, uint32_t *out_words) {
  if ((!x && n > 0) || !out_words || n < 0) return amwg_fail(AMWG_EINVAL, "amwg_two_valued_tables: bad argument");
  const std::vector<uint32_t> tab = two_valued_tables(x, n);
  if (tab.size() != 6 * two_valued_words(n)) return amwg_fail(AMWG_EINVAL, "internal: two_valued_tables of %zu words, expected %zu", tab.size(), 6 * two_valued_words(n));
  memcpy(out_words, tab.data(), tab.size() * 4);
  return AMWG_OK;
}

int amwg_k_valued_sum_check(int32_t device, int32_t K, const uint8_t *idx, int32_t n, const uint32_t *tab, int64_t m, const double *acc0, const double *c,
                            double *out_fast_forward, double *out_term_by_term) {
  const char *call = "amwg_k_valued_sum_check";
  if (!idx || !tab || !acc0 || !c || !out_fast_forward || !out_term_by_term || n < 0 || m < 0 || m > ((int64_t)1 << 24)) return amwg_fail(AMWG_EINVAL, "%s: bad argument", call);
  if (!(K == 1 || K == 2 || K == 3 || K == 5 || K == 8 || K == 13 || K == 16)) return amwg_fail(AMWG_EINVAL, "%s: K = %d is not instantiated (1, 2, 3, 5, 8, 13, 16)", call, K);
  for (int i = 0; i < n; ++i) if ((int)idx[i] >= K) return amwg_fail(AMWG_EINVAL, "%s: idx[%d] = %d outside 0..%d", call, i, (int)idx[i], K - 1);
  if (m == 0) return AMWG_OK;
  TRYB(use_device(device));
  const size_t tab_bytes = 2 * (size_t)K * k_valued_words(n) * 4, lanes = (size_t)m;
  DevBuf dtab, didx, dacc, dc, dff, dseq;
  HIP_TRY(dtab.alloc(tab_bytes));
  HIP_TRY(didx.alloc(n ? (size_t)n : 1));      // (n = 0: a byte nobody reads, not a zero-sized buffer)
  HIP_TRY(dacc.alloc(lanes * 8));
  HIP_TRY(dc.alloc(lanes * (size_t)K * 8));
  HIP_TRY(dff.alloc(lanes * 8));
  HIP_TRY(dseq.alloc(lanes * 8));
  HIP_TRY(hipMemcpy(dtab.p, tab, tab_bytes, hipMemcpyHostToDevice));
  if (n) HIP_TRY(hipMemcpy(didx.p, idx, (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dacc.p, acc0, lanes * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dc.p, c, lanes * (size_t)K * 8, hipMemcpyHostToDevice));
  const uint32_t *t = dtab.as<uint32_t>();
  const uint8_t *ix = didx.as<uint8_t>();
  const double *a0 = dacc.as<double>(), *cc = dc.as<double>();
  double *ff = dff.as<double>(), *seq = dseq.as<double>();
  switch (K) {
    case 1: k_valued_check_launch<1>(t, ix, n, m, a0, cc, ff, seq); break;
    case 2: k_valued_check_launch<2>(t, ix, n, m, a0, cc, ff, seq); break;
    case 3: k_valued_check_launch<3>(t, ix, n, m, a0, cc, ff, seq); break;
    case 5: k_valued_check_launch<5>(t, ix, n, m, a0, cc, ff, seq); break;
    case 8: k_valued_check_launch<8>(t, ix, n, m, a0, cc, ff, seq); break;
    case 13: k_valued_check_launch<13>(t, ix, n, m, a0, cc, ff, seq); break;
    default: k_valued_check_launch<16>(t, ix, n, m, a0, cc, ff, seq); break;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out_fast_forward, dff.p, lanes * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_term_by_term, dseq.p, lanes * 8, hipMemcpyDeviceToHost));
  return AMWG_OK;
}

int amwg_stream_check(int32_t device, int32_t kind, uint64_t seed, uint64_t chain0, int64_t n_chains, const uint64_t *consumed0, int64_t n_draws,
                      const uint8_t *calls, int64_t n_calls, double *out, uint64_t *consumed_out, uint64_t *flags) {
  const bool coop = kind == 1 || kind == 2 || kind == 4 || kind == 8 || kind == 16 || kind == 32 || kind == 64;
  if (!(kind == 0 || coop || kind == 100 || kind == 200 || kind == 201)) return amwg_fail(AMWG_EINVAL, "amwg_stream_check: unknown kind %d", kind);
  if (!consumed0 || !out || !consumed_out || (kind == 201) != (flags != nullptr) || (kind == 100) != (calls != nullptr))
    return amwg_fail(AMWG_EINVAL, "amwg_stream_check: null argument, or flags / calls given to a kind that has none");
  const int64_t kMax = (int64_t)1 << 28;
  if (n_chains < 1 || n_draws < 0 || n_chains > kMax || n_draws > kMax || n_calls < 0 || n_calls > kMax) return amwg_fail(AMWG_EINVAL, "amwg_stream_check: bad shape");
  const int64_t width = n_draws + (kind == 201 ? 384 : 0);
  if (width > kMax / n_chains) return amwg_fail(AMWG_EINVAL, "amwg_stream_check: bad shape");
  if (kind == 100) {
    int64_t total = 0;
    for (int64_t j = 0; j < n_calls; ++j) total += calls[j] ? 2 : 1;
    if (total != n_draws) return amwg_fail(AMWG_EINVAL, "amwg_stream_check: the calls draw %lld uniforms, not n_draws = %lld", (long long)total, (long long)n_draws);
  }
  TRYB(use_device(device));
  DevBuf dc0, dout, dcons, dflags, dcalls;
  const size_t C = (size_t)n_chains;
  HIP_TRY(dc0.alloc(C * 8));
  HIP_TRY(dout.alloc(C * (size_t)width * 8));
  HIP_TRY(dcons.alloc(C * 8));
  HIP_TRY(hipMemcpy(dc0.p, consumed0, C * 8, hipMemcpyHostToDevice));
  if (flags) HIP_TRY(dflags.alloc(C * 12 * 8));
  if (calls) {
    HIP_TRY(dcalls.alloc((size_t)n_calls));
    if (n_calls) HIP_TRY(hipMemcpy(dcalls.p, calls, (size_t)n_calls, hipMemcpyHostToDevice));
  }
  const uint64_t *c0 = dc0.as<uint64_t>();
  double *o = dout.as<double>();
  uint64_t *co = dcons.as<uint64_t>();
  const dim3 wave(64);
  auto per_wave = [&](int chains_per_wave) { return dim3((unsigned)((n_chains + chains_per_wave - 1) / chains_per_wave)); };
  switch (kind) {
    case 0: hipLaunchKernelGGL(stream_chain_kernel, per_wave(64), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, o, co); break;
    case 1: hipLaunchKernelGGL(stream_coop_kernel<1>, per_wave(64), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, o, co); break;
    case 2: hipLaunchKernelGGL(stream_coop_kernel<2>, per_wave(32), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, o, co); break;
    case 4: hipLaunchKernelGGL(stream_coop_kernel<4>, per_wave(16), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, o, co); break;
    case 8: hipLaunchKernelGGL(stream_coop_kernel<8>, per_wave(8), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, o, co); break;
    case 16: hipLaunchKernelGGL(stream_coop_kernel<16>, per_wave(4), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, o, co); break;
    case 32: hipLaunchKernelGGL(stream_coop_kernel<32>, per_wave(2), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, o, co); break;
    case 64: hipLaunchKernelGGL(stream_coop_kernel<64>, per_wave(1), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, o, co); break;
    case 100: hipLaunchKernelGGL(stream_pair_kernel, per_wave(64), wave, 0, 0, seed, chain0, n_chains, c0, n_draws, dcalls.as<uint8_t>(), n_calls, o, co); break;
    default: hipLaunchKernelGGL(stream_window_kernel, per_wave(1), wave, 0, 0, seed, chain0, c0, n_draws, (int)(kind == 201), width, o, co, dflags.as<uint64_t>()); break;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.p, C * (size_t)width * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(consumed_out, dcons.p, C * 8, hipMemcpyDeviceToHost));
  if (flags) HIP_TRY(hipMemcpy(flags, dflags.p, C * 12 * 8, hipMemcpyDeviceToHost));
  return AMWG_OK;
}

int amwg_ld_device(int32_t device, int64_t n, const double *records, double *out) {
  if (!records || !out || n < 0) return amwg_fail(AMWG_EINVAL, "amwg_ld_device: bad argument");
  TRYB(use_device(device));
  DevBuf dr, dout;
  HIP_TRY(dr.alloc((size_t)n * 40));
  HIP_TRY(dout.alloc((size_t)n * 8));
  HIP_TRY(hipMemcpy(dr.p, records, (size_t)n * 40, hipMemcpyHostToDevice));
  if (n) hipLaunchKernelGGL(amwg_ld_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, dr.as<double>(), dout.as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return AMWG_OK;
}

int amwg_device_eval(int32_t device, int32_t op, int64_t n, const double *a, const double *b, const double *c, double *out) {
  if (!a || !out || n < 0) return amwg_fail(AMWG_EINVAL, "amwg_device_eval: bad argument");
  TRYB(use_device(device));
  DevBuf da, db, dc, dout;
  const size_t bytes = (size_t)n * 8;
  HIP_TRY(da.alloc(bytes));
  HIP_TRY(dout.alloc(bytes));
  HIP_TRY(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice));
  if (b) { HIP_TRY(db.alloc(bytes)); HIP_TRY(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice)); }
  if (c) { HIP_TRY(dc.alloc(bytes)); HIP_TRY(hipMemcpy(dc.p, c, bytes, hipMemcpyHostToDevice)); }
  if (n) hipLaunchKernelGGL(amwg_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, n, da.as<double>(), db.as<double>(), dc.as<double>(), dout.as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
  return AMWG_OK;
}

int amwg_dataset_quantiles_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const double *probs, int32_t n_probs, double *out) {
  if (!draws || !probs || !out) return amwg_fail(AMWG_EINVAL, "amwg_dataset_quantiles_check: null argument");
  TRYB(amwg_dataset_quantiles_shape("amwg_dataset_quantiles_check", rows, PR, C, D, n_probs));      // (bounds rows * C / D, and with it the bytes below unless PR * D is absurd)
  if (rows > INT64_MAX / 8 / PR / C) return amwg_fail(AMWG_EINVAL, "amwg_dataset_quantiles_check: array too large");
  TRYB(use_device(device));
  const size_t bytes = (size_t)rows * (size_t)PR * (size_t)C * 8;
  DevBuf dd;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  return amwg_dataset_quantiles_launch("amwg_dataset_quantiles_check", dd.as<double>(), rows, PR, C, D, probs, n_probs, out, nullptr);
}

int amwg_hpd_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const double *probs, int32_t n_probs, double *out) {
  if (!draws || !probs || !out) return amwg_fail(AMWG_EINVAL, "amwg_hpd_check: null argument");
  TRYB(amwg_hpd_shape("amwg_hpd_check", rows, PR, C, D, n_probs));
  if (rows > INT64_MAX / 8 / PR / C) return amwg_fail(AMWG_EINVAL, "amwg_hpd_check: array too large");
  TRYB(use_device(device));
  const size_t bytes = (size_t)rows * (size_t)PR * (size_t)C * 8;
  DevBuf dd;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  return amwg_hpd_launch("amwg_hpd_check", dd.as<double>(), rows, PR, C, D, probs, n_probs, out, nullptr);
}

int amwg_hpd_limits(int32_t device, int64_t scratch_bytes, int64_t *lds_keys, int64_t *scratch_before) {
  if (scratch_bytes < 0) return amwg_fail(AMWG_EINVAL, "amwg_hpd_limits: bad argument (scratch_bytes %lld)", (long long)scratch_bytes);
  if (lds_keys) { TRYB(use_device(device)); TRYB(amwg_hpd_lds_keys(lds_keys)); }
  const size_t before = amwg_hpd_set_budget((size_t)scratch_bytes);
  if (scratch_before) *scratch_before = (int64_t)before;
  return AMWG_OK;
}

}  // extern "C"
// one array of every dataset, the copies back to back on 256-byte boundaries as amwg_create.hip lays them (upload_datasets); off[d] in elements
template <class T, class Len, class Fill>
static int waic_pack(int D, Len len, Fill fill, std::vector<int64_t> &off, DevBuf &dev) {
  constexpr size_t align = 256 / sizeof(T);
  size_t total = 0;
  off.assign((size_t)D, 0);
  for (int d = 0; d < D; ++d) { off[(size_t)d] = (int64_t)total; total += (len(d) + align - 1) / align * align; }
  std::vector<T> packed(total ? total : 1, T(0));
  for (int d = 0; d < D; ++d) fill(d, packed.data() + off[(size_t)d]);
  HIP_TRY(dev.alloc(packed.size() * sizeof(T)));
  HIP_TRY(hipMemcpy(dev.p, packed.data(), packed.size() * sizeof(T), hipMemcpyHostToDevice));
  return AMWG_OK;
}
// amwg_waic_check and amwg_loo_check: the arguments checked, the draws and the family's data on the device as the sampler lays them, then the launcher of either
// (extra: WAIC's loglik, or LOO's tails)
static int pointwise_check(const char *call, bool loo, int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const amwg_model_desc *models,
                           int64_t scratch_bytes, double *summary, int32_t *high, double *pointwise, double *extra) {
  double *loglik = loo ? nullptr : extra;
  if (!draws || !models || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (scratch_bytes < 0) return amwg_fail(AMWG_EINVAL, "%s: bad argument (scratch_bytes %lld)", call, (long long)scratch_bytes);
  TRYB(loo ? amwg_loo_shape(call, rows, PR, C, D) : amwg_waic_shape(call, rows, PR, C, D));
  if (rows > INT64_MAX / 8 / PR / C) return amwg_fail(AMWG_EINVAL, "%s: array too large", call);
  const int model = models[0].model;
  if (model < AMWG_MODEL_NORMAL || model > AMWG_MODEL_POIS_GLM) return amwg_fail(AMWG_EINVAL, "%s: unknown model %d", call, model);
  if (model == AMWG_MODEL_HIER_NORMAL && D != 1) return amwg_fail(AMWG_EINVAL, "%s: the hierarchical family runs on one dataset", call);
  int64_t n_max = 0;
  for (int d = 0; d < D; ++d) {
    const amwg_model_desc &m = models[d];
    if (m.model != model) return amwg_fail(AMWG_EINVAL, "%s: dataset %d is of model %d, dataset 0 of %d", call, d, m.model, model);
    if (m.n_obs < 1 || !m.x) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: n_obs %d (at least 1) or a null x", call, d, m.n_obs);
    if (model == AMWG_MODEL_POIS_GLM && (!m.y || m.K != 7)) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: the Poisson family needs y and K = 7", call, d);
    if (model == AMWG_MODEL_HIER_NORMAL) {
      if (!m.g || m.G < 1 || m.G > 255) return amwg_fail(AMWG_EINVAL, "%s: the hierarchical family needs g and 1 <= G <= 255", call);
      for (int i = 0; i < m.n_obs; ++i) if (m.g[i] < 0 || m.g[i] >= m.G) return amwg_fail(AMWG_EINVAL, "%s: g[%d] = %d outside 0..%d", call, i, m.g[i], m.G - 1);
    }
    n_max = m.n_obs > n_max ? m.n_obs : n_max;
  }
  const int need = model == AMWG_MODEL_NORMAL ? 2 : model == AMWG_MODEL_BETA_BERN ? 1 : model == AMWG_MODEL_HIER_NORMAL ? models[0].G + 2 : 9;
  if (PR < need) return amwg_fail(AMWG_EINVAL, "%s: the family reads %d components of a draw, the draws hold %d", call, need, PR);
  if (loglik && (double)D * (double)rows * (double)(C / D) * (double)n_max > 16777216.0) return amwg_fail(AMWG_EINVAL, "%s: loglik of more than 2^24 doubles", call);
  if (loo && extra && (double)D * (double)(loo_tail_len(rows * (C / D)) + 1) * (double)n_max > 16777216.0) return amwg_fail(AMWG_EINVAL, "%s: tails of more than 2^24 doubles", call);
  TRYB(use_device(device));
  const size_t bytes = (size_t)rows * (size_t)PR * (size_t)C * 8;
  DevBuf dd, dx, dy, dlf, dxb, dbad;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  std::vector<WaicDataset> sets((size_t)D);
  std::vector<int64_t> off;
  WaicModel wm{};
  wm.model = model; wm.G = models[0].G; wm.exact_division = 0;
  wm.neg_half_log_2pi = -0.5 * log_v8(2 * kPi);
  for (int d = 0; d < D; ++d) sets[(size_t)d] = WaicDataset{models[d].n_obs, 1, 0, 0, 0, 0};
  if (model == AMWG_MODEL_NORMAL || model == AMWG_MODEL_HIER_NORMAL) {
    TRYB((waic_pack<double>(D, [&](int d) { return (size_t)models[d].n_obs; }, [&](int d, double *dst) { for (int i = 0; i < models[d].n_obs; ++i) dst[i] = models[d].x[i]; }, off, dx)));
    for (int d = 0; d < D; ++d) {
      sets[(size_t)d].off_x = off[(size_t)d];
      bool mid = true;
      for (int i = 0; i < models[d].n_obs; ++i) mid = mid && (models[d].x[i] == 0.0 || mid_range(std::fabs(models[d].x[i])));
      sets[(size_t)d].data_mid_range = mid ? 1 : 0;
    }
    wm.x = dx.as<double>();
    if (model == AMWG_MODEL_HIER_NORMAL) {
      TRYB((waic_pack<uint8_t>(D, [&](int d) { return (size_t)models[d].n_obs; }, [&](int d, uint8_t *dst) { for (int i = 0; i < models[d].n_obs; ++i) dst[i] = (uint8_t)models[d].g[i]; }, off, dxb)));
      wm.xb = dxb.as<uint8_t>();
    }
  } else if (model == AMWG_MODEL_BETA_BERN) {
    TRYB((waic_pack<uint8_t>(D, [&](int d) { return (size_t)models[d].n_obs; }, [&](int d, uint8_t *dst) { for (int i = 0; i < models[d].n_obs; ++i) dst[i] = models[d].x[i] == 1 ? 1 : 0; }, off, dxb)));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_xb = off[(size_t)d];
    wm.xb = dxb.as<uint8_t>();
    bool any = false;
    for (int d = 0; d < D; ++d) for (int i = 0; i < models[d].n_obs; ++i) any = any || !(models[d].x[i] == 1 || models[d].x[i] == 0);
    if (any) {
      TRYB((waic_pack<uint8_t>(D, [&](int d) { return (size_t)models[d].n_obs; }, [&](int d, uint8_t *dst) { for (int i = 0; i < models[d].n_obs; ++i) dst[i] = !(models[d].x[i] == 1 || models[d].x[i] == 0); }, off, dbad)));
      wm.invalid = dbad.as<uint8_t>();
    }
  } else {      // the Poisson family: X column-major [7][n_d], the counts, lfactorial of the counts (+inf for a negative one) -- amwg_create.hip upload_poisson_data
    TRYB((waic_pack<double>(D, [&](int d) { return (size_t)models[d].n_obs * 7; }, [&](int d, double *dst) { const int N = models[d].n_obs; for (int i = 0; i < N; ++i) for (int k = 0; k < 7; ++k) dst[(size_t)k * N + i] = models[d].x[(size_t)i * 7 + k]; }, off, dx)));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_x = off[(size_t)d];
    TRYB((waic_pack<double>(D, [&](int d) { return (size_t)models[d].n_obs; }, [&](int d, double *dst) { for (int i = 0; i < models[d].n_obs; ++i) dst[i] = models[d].y[i]; }, off, dy)));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_y = off[(size_t)d];
    TRYB((waic_pack<double>(D, [&](int d) { return (size_t)models[d].n_obs; }, [&](int d, double *dst) { for (int i = 0; i < models[d].n_obs; ++i) dst[i] = models[d].y[i] < 0 ? (double)INFINITY : lfactorial_js(models[d].y[i]); }, off, dlf)));
    for (int d = 0; d < D; ++d) sets[(size_t)d].off_lfact = off[(size_t)d];
    wm.x = dx.as<double>(); wm.y = dy.as<double>(); wm.lfact = dlf.as<double>();
  }
  if (loo) {
    const size_t before = amwg_loo_set_budget((size_t)scratch_bytes);
    const int rc = amwg_loo_launch(call, dd.as<double>(), rows, PR, C, D, wm, sets.data(), summary, high, pointwise, extra, nullptr);
    amwg_loo_set_budget(before);
    return rc;
  }
  const size_t before = amwg_waic_set_budget((size_t)scratch_bytes);
  const int rc = amwg_waic_launch(call, dd.as<double>(), rows, PR, C, D, wm, sets.data(), summary, high, pointwise, loglik, nullptr);
  amwg_waic_set_budget(before);
  return rc;
}
extern "C" {

int amwg_waic_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const amwg_model_desc *models, int64_t scratch_bytes, double *summary,
                    int32_t *high, double *pointwise, double *loglik) {
  return pointwise_check("amwg_waic_check", false, device, draws, rows, PR, C, D, models, scratch_bytes, summary, high, pointwise, loglik);
}

int amwg_loo_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const amwg_model_desc *models, int64_t scratch_bytes, double *summary,
                   int32_t *high, double *pointwise, double *tails) {
  return pointwise_check("amwg_loo_check", true, device, draws, rows, PR, C, D, models, scratch_bytes, summary, high, pointwise, tails);
}

// amwg_user_waic_check and amwg_user_loo_check: a closure's source and pointwise text, its arrays per dataset as amwg_create_user_datasets takes them, on a handle
// that holds nothing but those (no chains, no step kernel): the arrays uploaded as a sampler's, the code object compiled and loaded as its first WAIC / LOO call does
static int user_pointwise_check(const char *call, bool loo, int32_t device, const amwg_user_model *models, int32_t D, int32_t P, const char *terms, const double *draws, int64_t rows,
                                int32_t PR, int64_t C, int64_t scratch_bytes, double *summary, int32_t *high, double *pointwise, double *extra) {
  if (!models || !terms || !draws || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (scratch_bytes < 0) return amwg_fail(AMWG_EINVAL, "%s: bad argument (scratch_bytes %lld)", call, (long long)scratch_bytes);
  TRYB(loo ? amwg_loo_shape(call, rows, PR, C, D) : amwg_waic_shape(call, rows, PR, C, D));
  if (rows > INT64_MAX / 8 / PR / C) return amwg_fail(AMWG_EINVAL, "%s: array too large", call);
  if (P < 1 || PR < P) return amwg_fail(AMWG_EINVAL, "%s: the closure reads %d components of a draw, the draws hold %d", call, P, PR);
  for (int d = 0; d < D; ++d) {
    if (!models[d].source || strcmp(models[d].source, models[0].source) != 0 || models[d].n_arrays != models[0].n_arrays) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: another source or n_arrays than dataset 0's", call, d);
    for (int j = 0; j < models[d].n_arrays; ++j) if (models[d].array_len[j] != models[0].array_len[j]) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: array %d of another length than dataset 0's", call, d, j);
  }
  TRYB(use_device(device));
  struct Handle { amwg_sampler *s = new amwg_sampler(); ~Handle() { amwg_destroy(s); } } h;
  amwg_sampler *s = h.s;
  s->device = device; s->user = true; s->P = P; s->n_datasets = D; s->C = C;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  s->user_source = models[0].source;
  s->user_arch = prop.gcnArchName;
  TRYB(upload_user_arrays(s, models, D));
  TRYB(amwg_set_pointwise(s, terms));
  const int64_t S = rows * (C / D), n = s->pw_n_obs;
  if (!loo && extra && (double)D * (double)S * (double)n > 16777216.0) return amwg_fail(AMWG_EINVAL, "%s: loglik of more than 2^24 doubles", call);
  if (loo && extra && (double)D * (double)(loo_tail_len(S) + 1) * (double)n > 16777216.0) return amwg_fail(AMWG_EINVAL, "%s: tails of more than 2^24 doubles", call);
  const size_t bytes = (size_t)rows * (size_t)PR * (size_t)C * 8;
  DevBuf dd;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  std::vector<WaicDataset> sets;
  UserPointwise u;
  TRYB(amwg_pointwise_describe_user(s, sets, u));
  PointwiseLaunch K;
  amwg_pointwise_user_kernels(K, u);
  const size_t before = loo ? amwg_loo_set_budget((size_t)scratch_bytes) : amwg_waic_set_budget((size_t)scratch_bytes);
  const int rc = loo ? amwg_loo_run(call, dd.as<double>(), rows, PR, C, D, K, sets.data(), summary, high, pointwise, extra, nullptr)
                     : amwg_waic_run(call, dd.as<double>(), rows, PR, C, D, K, sets.data(), summary, high, pointwise, extra, nullptr);
  if (loo) amwg_loo_set_budget(before); else amwg_waic_set_budget(before);
  return rc;
}

int amwg_user_waic_check(int32_t device, const amwg_user_model *models, int32_t n_datasets, int32_t P, const char *terms_source, const double *draws, int64_t rows, int32_t PR, int64_t C,
                         int64_t scratch_bytes, double *summary, int32_t *high, double *pointwise, double *loglik) {
  return user_pointwise_check("amwg_user_waic_check", false, device, models, n_datasets, P, terms_source, draws, rows, PR, C, scratch_bytes, summary, high, pointwise, loglik);
}

int amwg_user_loo_check(int32_t device, const amwg_user_model *models, int32_t n_datasets, int32_t P, const char *terms_source, const double *draws, int64_t rows, int32_t PR, int64_t C,
                        int64_t scratch_bytes, double *summary, int32_t *high, double *pointwise, double *tails) {
  return user_pointwise_check("amwg_user_loo_check", true, device, models, n_datasets, P, terms_source, draws, rows, PR, C, scratch_bytes, summary, high, pointwise, tails);
}

int amwg_loo_stats(int32_t timing, int32_t *passes, double *ms) {
  const LooStats st = amwg_loo_last_stats();
  if (passes) *passes = st.passes;
  if (ms) { ms[0] = st.timed ? st.ms_lppd : -1.0; ms[1] = st.timed ? st.ms_select : -1.0; ms[2] = st.timed ? st.ms_compact : -1.0; ms[3] = st.timed ? st.ms_fit : -1.0; }
  amwg_loo_set_timing(timing);
  return AMWG_OK;
}

int amwg_fold_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, int64_t window_rows,
                    double *halves_folded, double *halves_direct, double *mean, double *sd) {
  if (!draws || !halves_folded || !halves_direct || !mean || !sd) return amwg_fail(AMWG_EINVAL, "amwg_fold_check: null argument");
  if (rows < 1 || PR < 1 || PR > 65535 || C < 1 || D < 1 || D > 65535 || C % D != 0 || window_rows < 1)
    return amwg_fail(AMWG_EINVAL, "amwg_fold_check: bad shape (rows %lld, values %d, chains %lld, datasets %d -- dividing the chains --, window_rows %lld)", (long long)rows, PR, (long long)C, D, (long long)window_rows);
  if (rows > INT64_MAX / 8 / PR / C) return amwg_fail(AMWG_EINVAL, "amwg_fold_check: array too large");
  TRYB(use_device(device));
  const size_t row_elems = (size_t)PR * (size_t)C, bytes = (size_t)rows * row_elems * 8, n_mom = (size_t)D * (size_t)PR;
  DevBuf dd, acc, hf, hd, mom;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(acc.alloc(kFoldStats * row_elems * 8));
  HIP_TRY(hf.alloc(4 * row_elems * 8));
  HIP_TRY(hd.alloc(4 * row_elems * 8));
  HIP_TRY(mom.alloc(2 * n_mom * 8));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(acc.p, 0, kFoldStats * row_elems * 8, nullptr));
  for (int64_t g0 = 0; g0 < rows; g0 += window_rows)      // (window after window, as launch_steps folds them)
    TRYB(amwg_fold_window(dd.as<double>() + (size_t)g0 * row_elems, g0, rows - g0 < window_rows ? rows - g0 : window_rows, rows / 2, PR, C, acc.as<double>(), nullptr));
  TRYB(amwg_fold_halves(acc.as<double>(), rows, PR, C, hf.as<double>(), nullptr));
  TRYB(amwg_fold_moments(acc.as<double>(), rows, PR, C, D, mom.as<double>(), mom.as<double>() + n_mom, nullptr));
  TRYB(amwg_chain_halves(dd.as<double>(), rows, PR, C, hd.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(halves_folded, hf.p, 4 * row_elems * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(halves_direct, hd.p, 4 * row_elems * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(mean, mom.p, n_mom * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sd, mom.as<double>() + n_mom, n_mom * 8, hipMemcpyDeviceToHost));
  return AMWG_OK;
}

int amwg_histogram_check(const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const double *edges, int32_t bins, int64_t window_rows,
                         uint64_t *counts, int32_t device) {
  if (!draws || !edges || !counts) return amwg_fail(AMWG_EINVAL, "amwg_histogram_check: null argument");
  if (window_rows < 0) return amwg_fail(AMWG_EINVAL, "amwg_histogram_check: bad shape (window_rows %lld)", (long long)window_rows);
  TRYB(amwg_histogram_shape("amwg_histogram_check", rows, PR, C, D, bins));
  TRYB(amwg_histogram_edges_check("amwg_histogram_check", edges, PR, bins));
  TRYB(use_device(device));
  const size_t row_elems = (size_t)PR * (size_t)C, bytes = (size_t)rows * row_elems * 8;
  const size_t edge_bytes = (size_t)PR * (size_t)(bins + 1) * 8, count_bytes = (size_t)D * (size_t)PR * (size_t)(bins + 3) * 8;
  DevBuf dd, de, dc;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(de.alloc(edge_bytes));
  HIP_TRY(dc.alloc(count_bytes));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(de.p, edges, edge_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dc.p, counts, count_bytes, hipMemcpyHostToDevice));
  const int64_t w = window_rows > 0 ? window_rows : rows;
  for (int64_t g0 = 0; g0 < rows; g0 += w)      // (window after window, as launch_steps counts them)
    TRYB(amwg_histogram_launch("amwg_histogram_check", dd.as<double>() + (size_t)g0 * row_elems, rows - g0 < w ? rows - g0 : w, PR, C, D, de.as<double>(), bins, amwg_histogram_uniform(edges, PR, bins), dc.as<uint64_t>(), nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(counts, dc.p, count_bytes, hipMemcpyDeviceToHost));
  return AMWG_OK;
}

int amwg_covariance_check(const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const int32_t *values, int32_t n_values, int64_t window_rows,
                          double *cov, int32_t device) {
  const char *call = "amwg_covariance_check";
  if (!draws || !values || !cov) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (window_rows < 0) return amwg_fail(AMWG_EINVAL, "%s: bad shape (window_rows %lld)", call, (long long)window_rows);
  TRYB(amwg_covariance_shape(call, rows, PR, C, D, n_values));
  TRYB(amwg_covariance_values_check(call, values, n_values, PR));
  TRYB(use_device(device));
  const size_t bytes = (size_t)rows * (size_t)PR * (size_t)C * 8;
  DevBuf dd;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  return amwg_covariance_of_array(call, dd.as<double>(), rows, PR, C, D, values, n_values, window_rows, cov, nullptr);
}

int amwg_autocovariance_check(const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const int32_t *values, int32_t n_values, int32_t max_lag,
                              int64_t window_rows, double *acov, double *mean, double *between, int32_t device) {
  const char *call = "amwg_autocovariance_check";
  if (!draws || !values || !acov || !mean || !between) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (window_rows < 0) return amwg_fail(AMWG_EINVAL, "%s: bad shape (window_rows %lld)", call, (long long)window_rows);
  TRYB(amwg_autocov_shape(call, rows, PR, C, D, n_values, max_lag));
  TRYB(amwg_covariance_values_check(call, values, n_values, PR));
  TRYB(use_device(device));
  const size_t bytes = (size_t)rows * (size_t)PR * (size_t)C * 8;
  DevBuf dd;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  return amwg_autocov_of_array(call, dd.as<double>(), rows, PR, C, D, values, n_values, max_lag, window_rows, acov, mean, between, nullptr);
}

int amwg_summaries_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, int64_t window_rows,
                         double *mean, double *sd, double *rhat_ds, double *ess_ds, double *rhat_pooled, double *ess_pooled) {
  if (!draws || !mean || !sd || !rhat_ds || !ess_ds || !rhat_pooled || !ess_pooled) return amwg_fail(AMWG_EINVAL, "amwg_summaries_check: null argument");
  if (rows < 1 || PR < 1 || PR > 65535 || C < 1 || D < 1 || D > 65535 || C % D != 0 || window_rows < 0)
    return amwg_fail(AMWG_EINVAL, "amwg_summaries_check: bad shape (rows %lld, values %d, chains %lld, datasets %d -- dividing the chains --, window_rows %lld)", (long long)rows, PR, (long long)C, D, (long long)window_rows);
  TRYB(amwg_diagnostics_refusal("amwg_summaries_check", true, rows, C, D, true));
  if (rows > INT64_MAX / 8 / PR / C) return amwg_fail(AMWG_EINVAL, "amwg_summaries_check: array too large");
  TRYB(use_device(device));
  const size_t row_elems = (size_t)PR * (size_t)C, bytes = (size_t)rows * row_elems * 8;
  DevBuf dd, acc, hv;
  HIP_TRY(dd.alloc(bytes));
  HIP_TRY(hv.alloc(4 * row_elems * 8));
  HIP_TRY(hipMemcpy(dd.p, draws, bytes, hipMemcpyHostToDevice));
  if (window_rows > 0) {      // (the summarised path: window after window, as launch_steps folds them)
    HIP_TRY(acc.alloc(kFoldStats * row_elems * 8));
    HIP_TRY(hipMemsetAsync(acc.p, 0, kFoldStats * row_elems * 8, nullptr));
    for (int64_t g0 = 0; g0 < rows; g0 += window_rows)
      TRYB(amwg_fold_window(dd.as<double>() + (size_t)g0 * row_elems, g0, rows - g0 < window_rows ? rows - g0 : window_rows, rows / 2, PR, C, acc.as<double>(), nullptr));
    TRYB(amwg_fold_halves(acc.as<double>(), rows, PR, C, hv.as<double>(), nullptr));
  } else {
    TRYB(amwg_chain_halves(dd.as<double>(), rows, PR, C, hv.as<double>(), nullptr));
  }
  TRYB(amwg_moments_launch(dd.as<double>(), rows, PR, C, D, mean, sd, nullptr));
  TRYB(amwg_dataset_diagnostics_launch(hv.as<double>(), rows, PR, C, D, rhat_ds, ess_ds, nullptr));
  return amwg_pooled_diagnostics(hv.as<double>(), rows, PR, C, rhat_pooled, ess_pooled, nullptr);
}

}  // extern "C"
