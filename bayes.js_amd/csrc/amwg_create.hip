// amwg_create.hip -- building a sampler: the checks of a call, the parameter layout, the device, the data of a built-in family or of a translated closure, the
// chains' state; then the launch plan and its kernel (amwg_plan.hip, amwg_rtc.hip).  amwg_destroy takes a sampler back, however far its constructor got.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>

#include "amwg_autocov.h"
#include "amwg_covariance.h"
#include "amwg_fold.h"
#include "amwg_histogram.h"
#include "amwg_host.h"
#include "amwg_dataset.h"
#include "amwg_kernel.h"
#include "amwg_models.h"

using namespace amwg;

// The data-only tables of two_valued_sum (amwg_models.h), back to back: the observations as bits (w), the ones before every
// word (pre), and for each symbol the marks of the occurrences whose immediately preceding run of the OTHER symbol has odd
// length (om1 / om0) with their per-word prefix counts (po1 / po0).
std::vector<uint32_t> two_valued_tables(const uint8_t *xb, int N) {
  const size_t W = two_valued_words(N);
  std::vector<uint32_t> tab(6 * W, 0u);
  for (int i = 0; i < N; ++i) if (xb[i]) tab[(size_t)i >> 5] |= 1u << (i & 31);
  for (size_t k = 1; k < W; ++k) tab[W + k] = tab[W + k - 1] + (uint32_t)__builtin_popcount(tab[k - 1]);
  for (int sym = 1; sym >= 0; --sym) {
    uint32_t *om = tab.data() + (sym ? 2 : 4) * W, *po = om + W;
    int run = 0;   // length of the current run of the other symbol
    for (int i = 0; i < N; ++i) {
      const int v = xb[i] ? 1 : 0;
      if (v == sym) { if (run & 1) om[(size_t)i >> 5] |= 1u << (i & 31); run = 0; } else ++run;
    }
    for (size_t k = 1; k < W; ++k) po[k] = po[k - 1] + (uint32_t)__builtin_popcount(om[k - 1]);
  }
  return tab;
}

// ---- pieces of construction shared by the built-in and the translated models
static int check_options(const amwg_options *options, int max_threads) {
  if (options->chains < 1) return amwg_fail(AMWG_EINVAL, "amwg_create: chains must be >= 1");
  // a launch counts its accepted / evaluated proposals in 16-bit fields: longer launches are not silently shortened (launch_info and the
  // bench's per-launch figures assume the requested size)
  if (options->steps_per_launch < 0 || options->steps_per_launch > 65535)
    return amwg_fail(AMWG_EINVAL, "steps_per_launch must be 0 (auto) or 1..65535, got %d", options->steps_per_launch);
  const int G_opt = options->lanes_per_chain;
  if (G_opt && G_opt != AMWG_LANES_FASTEST && G_opt != AMWG_LANES_AUTOTUNE && (G_opt < 1 || G_opt > 1024 || (G_opt & (G_opt - 1))))
    return amwg_fail(AMWG_EINVAL, "lanes_per_chain must be a power of two in 1..1024 (or 0 = auto, AMWG_LANES_FASTEST = -1, AMWG_LANES_AUTOTUNE = -2)");
  if (G_opt > 64 && options->block_threads && options->block_threads != G_opt)
    return amwg_fail(AMWG_EINVAL, "a chain on %d lanes is one workgroup of %d threads: block_threads must be 0 or %d", G_opt, G_opt, G_opt);
  if (G_opt > max_threads) return amwg_fail(AMWG_EINVAL, "lanes_per_chain %d exceeds this model's workgroup limit %d", G_opt, max_threads);
  if (options->block_threads && (options->block_threads % 64 || options->block_threads > 1024 || options->block_threads < 64))
    return amwg_fail(AMWG_EINVAL, "block_threads must be a multiple of 64 in 64..1024");
  if (options->block_threads > max_threads)
    return amwg_fail(AMWG_EINVAL, "block_threads %d exceeds this model's workgroup limit %d", options->block_threads, max_threads);
#if defined(AMWG_AUDIT)      // (the audit build also SHRINKS the bounds -- the converse experiment of tools/bound_audit.py: how far before a chain differs)
  if (options->test_bound_shift < -60 || options->test_bound_shift > 40) return amwg_fail(AMWG_EINVAL, "test_bound_shift must be -60..40 in the audit build, got %d", options->test_bound_shift);
#else
  if (options->test_bound_shift < 0 || options->test_bound_shift > 40) return amwg_fail(AMWG_EINVAL, "test_bound_shift must be 0..40, got %d", options->test_bound_shift);
#endif
  if (options->sufficient_statistics != 0 && options->sufficient_statistics != 1) return amwg_fail(AMWG_EINVAL, "sufficient_statistics must be 0 or 1, got %d", options->sufficient_statistics);
  if (options->sufficient_statistics && (options->full_evaluation != 0 || options->exact_division)) return amwg_fail(AMWG_EINVAL, "sufficient_statistics decides from certified values: not with full_evaluation or exact_division");
  if (options->full_evaluation < 0 || options->full_evaluation > 2)
    return amwg_fail(AMWG_EINVAL, "full_evaluation must be 0 (default), 1 (every evaluation passes over all the data) or 2 (sweeps decided update by update), got %d", options->full_evaluation);
  return AMWG_OK;
}

// completed params (mcmc.js:357-403) -> flat layout.  Stepped parameters first (s->n_params of them, any number up to kMaxIndex);
// trailing AMWG_FIXED entries only add state slots.  The per-parameter table goes to the device (upload_layout).
static int build_layout(amwg_sampler *s, const amwg_param_desc *params, int n_params, bool allow_fixed) {
  ParamLayout &pl = s->pl;
  pl.max_top = 1;
  int P = 0, n_stepped = 0;
  std::vector<int32_t> base, len, top, multidim;
  bool fixed_seen = false;
  for (int p = 0; p < n_params; ++p) {
    const amwg_param_desc &q = params[p];
    if (q.type == AMWG_FIXED) {
      if (!allow_fixed) return amwg_fail(AMWG_EINVAL, "parameter %d: AMWG_FIXED entries are only supported by amwg_create_user", p);
      if (q.len < 1) return amwg_fail(AMWG_EINVAL, "parameter %d: bad len %d", p, q.len);
      fixed_seen = true;
      P += q.len;
      continue;
    }
    if (fixed_seen) return amwg_fail(AMWG_EINVAL, "parameter %d: stepped parameters must come before the AMWG_FIXED entries", p);
    if (q.type != AMWG_REAL && q.type != AMWG_INT && q.type != AMWG_BINARY)
      return amwg_fail(AMWG_EINVAL, "AmwgStepper can't handle parameter %d with type %d", p, q.type);   // mcmc.js:867
    // the built-in families' kernels are compiled without the BinaryStepper branch (none of them has a binary parameter): a binary
    // parameter there would silently be stepped by the Metropolis stepper instead of mcmc.js:753-767 -- refuse it
    if (q.type == AMWG_BINARY && !allow_fixed)
      return amwg_fail(AMWG_EINVAL, "parameter %d: the built-in model families have no binary parameters (BinaryStepper runs for translated closures, amwg_create_user)", p);
    if (n_stepped >= kMaxIndex) return amwg_fail(AMWG_EINVAL, "more than %d stepped parameters", kMaxIndex);
    if (q.len < 1 || q.top < 1 || q.len % q.top) return amwg_fail(AMWG_EINVAL, "parameter %d: bad dim (len %d, top %d)", p, q.len, q.top);
    if (q.top > kMaxIndex) return amwg_fail(AMWG_EINVAL, "parameter %d: leading dimension %d > %d", p, q.top, kMaxIndex);
    if (!q.multidim && q.len != 1) return amwg_fail(AMWG_EINVAL, "parameter %d: dim [1] but len %d", p, q.len);
    base.push_back(P); len.push_back(q.len); top.push_back(q.top); multidim.push_back(q.multidim ? 1 : 0);
    if (q.multidim && q.top > pl.max_top) pl.max_top = q.top;
    P += q.len;
    ++n_stepped;
    pl.P_stepped = P;
  }
  if (n_stepped < 1) return amwg_fail(AMWG_EINVAL, "no parameter to step");
  pl.n_params = n_stepped;
  pl.P = P;
  s->P = P;
  s->n_params = n_stepped;
  s->h_layout.clear();
  for (const std::vector<int32_t> *v : {&base, &len, &top, &multidim}) s->h_layout.insert(s->h_layout.end(), v->begin(), v->end());
  return AMWG_OK;
}

// AMWG_TIMING=1: the constructor's phases on stderr (development aid; the end-to-end bench reports the constructor as a whole)
namespace {
struct PhaseClock {
  bool on;
  std::chrono::steady_clock::time_point t0;
  explicit PhaseClock(bool enabled = true) : on(enabled && getenv("AMWG_TIMING") && getenv("AMWG_TIMING")[0] == '1'), t0(std::chrono::steady_clock::now()) {}
  void mark(const char *what) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[amwg timing] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};
// owns the half-built sampler: every early exit of a constructor is a plain return, and destroys it
struct SamplerGuard {
  amwg_sampler *s;
  SamplerGuard(const amwg_options *options, int model) : s(new amwg_sampler()) { s->opt = *options; s->model = model; s->C = options->chains; s->device = options->device; }
  ~SamplerGuard() { amwg_destroy(s); }
  amwg_sampler *release() { amwg_sampler *r = s; s = nullptr; return r; }
};
}  // namespace

static int open_device(amwg_sampler *s, hipDeviceProp_t *prop) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1) return amwg_fail(AMWG_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (s->device < 0 || s->device >= ndev) return amwg_fail(AMWG_EINVAL, "device %d out of range (%d visible)", s->device, ndev);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipGetDeviceProperties(prop, s->device));
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&s->ev0));
  HIP_TRY(hipEventCreate(&s->ev1));
  return AMWG_OK;
}

// a host array on the device, for as long as the sampler lives
template <class T>
static int upload(amwg_sampler *s, const T *host, size_t n, T **dev) {
  TRYB(dev_alloc(s, dev, n));
  if (n) HIP_TRY(hipMemcpy(*dev, host, n * sizeof(T), hipMemcpyHostToDevice));
  return AMWG_OK;
}
template <class T>
static int dev_zeros(amwg_sampler *s, T **dev, size_t n) {
  TRYB(dev_alloc(s, dev, n));
  HIP_TRY(hipMemset(*dev, 0, n * sizeof(T)));
  return AMWG_OK;
}

// per-component constants and per-chain state (every chain starts at the same init, mcmc.js:954-957)
static int alloc_chain_state(amwg_sampler *s, const amwg_param_desc *params, int n_params, const double *init,
                             const amwg_comp_opt *comp_opts) {
  const int P = s->P;
  std::vector<CompConst> hcc((size_t)P);
  s->h_adapt.resize((size_t)P);
  for (int p = 0, ci = 0; p < n_params; ++p)
    for (int e2 = 0; e2 < params[p].len; ++e2, ++ci) {
      const amwg_comp_opt &o = comp_opts[ci];
      hcc[ci] = CompConst{params[p].lower, params[p].upper, o.max_adaptation, o.initial_adaptation, o.target_accept_rate,
                          o.batch_size, params[p].type};
      s->h_adapt[ci] = o.is_adapting ? 1 : 0;
    }
  TRYB(upload(s, hcc.data(), (size_t)P, &s->d_cc));
  TRYB(upload(s, s->h_adapt.data(), (size_t)P, &s->d_adapt));
  int32_t *d_tab = nullptr;
  TRYB(upload(s, s->h_layout.data(), s->h_layout.size(), &d_tab));
  s->pl.tab = d_tab;

  const size_t PC = (size_t)P * (size_t)s->C, C = (size_t)s->C;
  ChainArrays &ch = s->ch;
  TRYB(dev_alloc(s, &ch.state, PC));
  TRYB(dev_alloc(s, &ch.prop_log_scale, PC));
  TRYB(dev_zeros(s, &ch.acceptance_count, PC));
  TRYB(dev_zeros(s, &ch.iterations_since_adaption, PC));
  TRYB(dev_zeros(s, &ch.batch_count, PC));
  TRYB(dev_zeros(s, &ch.accepts, PC));
  TRYB(dev_zeros(s, &ch.inbounds, PC));
  const bool wide_perm = s->n_params > kPackedNamed;
  TRYB(dev_alloc(s, &ch.perm, C));
  ch.perm16 = nullptr;
  if (wide_perm) TRYB(dev_alloc(s, &ch.perm16, (size_t)s->n_params * C));
  TRYB(dev_zeros(s, &ch.rng_n, C));
  TRYB(dev_zeros(s, &ch.lp_curr, C));
  TRYB(dev_zeros(s, &ch.lp_eps, C));
  // (64 doubles per wavefront of a one-lane-per-chain launch: where the certified pass of the Normal family / a closure's certified tail leaves the wavefront's means for the
  // scalar memory path, amwg_pass.h norm_sq_pass_wave.  Allocated once the geometry is known: size_wave_scratch)
  s->d.wave_scratch = nullptr;
  TRYB(dev_zeros(s, &ch.error, (size_t)1));
  ch.audit = nullptr;
  ch.audit_hist = nullptr;
#if defined(AMWG_AUDIT) || defined(AMWG_X_PHASES)      // (libamwg_audit.so: the bound audit's per-chain maxima and histograms, amwg_kernel.h "BOUND AUDIT"; the phase-clock development build)
  TRYB(dev_zeros(s, &ch.audit, 4 * C));
  TRYB(dev_zeros(s, &ch.audit_hist, (size_t)128));
#endif
  {
    std::vector<double> tmp(PC);
    for (int p = 0; p < P; ++p) for (size_t c = 0; c < C; ++c) tmp[(size_t)p * C + c] = init[p];
    HIP_TRY(hipMemcpy(ch.state, tmp.data(), PC * 8, hipMemcpyHostToDevice));
    for (int p = 0; p < P; ++p) for (size_t c = 0; c < C; ++c) tmp[(size_t)p * C + c] = comp_opts[p].prop_log_scale;
    HIP_TRY(hipMemcpy(ch.prop_log_scale, tmp.data(), PC * 8, hipMemcpyHostToDevice));
    uint64_t ident = 0;
    for (int i = 0; i < kPackedNamed; ++i) ident |= (uint64_t)i << (4 * i);
    std::vector<uint64_t> pv(C, ident);
    HIP_TRY(hipMemcpy(ch.perm, pv.data(), C * 8, hipMemcpyHostToDevice));
    if (wide_perm) {   // initial order = Object.keys(params) (mcmc.js:839)
      std::vector<uint16_t> p16((size_t)s->n_params * C);
      for (int k = 0; k < s->n_params; ++k) for (size_t c = 0; c < C; ++c) p16[(size_t)k * C + c] = (uint16_t)k;
      HIP_TRY(hipMemcpy(ch.perm16, p16.data(), p16.size() * 2, hipMemcpyHostToDevice));
    }
  }
  return AMWG_OK;
}

// ---- amwg_create, step by step.  The order of the steps is the order of the checks: it decides which error a bad call reports.
static int check_family_args(const amwg_model_desc *m, const amwg_param_desc *params, int n_params, int P) {
  const int N = m->n_obs;
  switch (m->model) {
    case AMWG_MODEL_NORMAL:
      if (P != 2 || n_params != 2) return amwg_fail(AMWG_EINVAL, "normal model expects params {mu, sigma}");
      if (!m->x && N) return amwg_fail(AMWG_EINVAL, "normal model: x is null");
      return AMWG_OK;
    case AMWG_MODEL_BETA_BERN:
      if (P != 1) return amwg_fail(AMWG_EINVAL, "beta_bern model expects params {theta}");
      if (!m->x && N) return amwg_fail(AMWG_EINVAL, "beta_bern model: x is null");
      return AMWG_OK;
    case AMWG_MODEL_HIER_NORMAL:
      if (n_params != 3 || m->G < 1 || m->G > 256 || params[0].len != m->G || P != m->G + 2)   // group ids are bytes in LDS
        return amwg_fail(AMWG_EINVAL, "hier_normal model expects params {theta[G], mu, sigma}, 1 <= G <= 256 (more groups: write the closure, it is translated)");
      if ((!m->x || !m->g) && N) return amwg_fail(AMWG_EINVAL, "hier_normal model: y or g is null");
      return AMWG_OK;
    case AMWG_MODEL_POIS_GLM:
      if (n_params != 2 || params[0].len != 8 || P != 9 || m->K != 7) return amwg_fail(AMWG_EINVAL, "pois_glm model expects params {beta[8], cp} and K = 7");
      if ((!m->x || !m->y) && N) return amwg_fail(AMWG_EINVAL, "pois_glm model: X or y is null");
      if (N > (1 << 28)) return amwg_fail(AMWG_EINVAL, "pois_glm model: %d observations (supported: up to 2^28; the kernel addresses a column with 32-bit byte offsets)", N);
      return AMWG_OK;
  }
  return amwg_fail(AMWG_EINVAL, "unknown model id %d", m->model);
}

// the constants that depend on a dataset's SIZE alone: the Poisson family's prior ld.unif(cp, 0, n - 1)
static void size_constants(int n_obs, DatasetConsts &k) {
  k.n_obs = n_obs;
  k.cp_upper = (double)(n_obs - 1);
  k.lunif_cp = log_v8(1 / (k.cp_upper - 0.0));
}
// the model constants that follow from the hyper-parameters and the options, with the kernel's own log (same roundings as the reference expression trees).
// What follows from a dataset's data or size is not formed here: DatasetConsts (create_builtin).
static void model_constants(const amwg_model_desc *m, const amwg_options *options, ModelConsts &mc) {
  mc.neg_half_log_2pi = -0.5 * log_v8(2 * kPi);
  const double *h = m->hyper;
  if (m->model == AMWG_MODEL_NORMAL || m->model == AMWG_MODEL_HIER_NORMAL || m->model == AMWG_MODEL_POIS_GLM) {
    mc.m0 = h[0];
    mc.c0 = mc.neg_half_log_2pi - log_v8(h[1]);     // ld.norm's  -0.5*log(2*pi) - log(sd)
    mc.den0 = 2 * h[1] * h[1];                      //            (2*sd)*sd
  }
  if (m->model == AMWG_MODEL_NORMAL || m->model == AMWG_MODEL_HIER_NORMAL) {
    mc.ua = h[2]; mc.ub = h[3];
    mc.lunif = log_v8(1 / (h[3] - h[2]));           // ld.unif's log(1/(max-min))
  }
  if (m->model == AMWG_MODEL_HIER_NORMAL) {
    mc.c1 = mc.neg_half_log_2pi - log_v8(h[4]);
    mc.den1 = 2 * h[4] * h[4];
  }
  if (m->model == AMWG_MODEL_BETA_BERN) {
    mc.ba = h[0]; mc.bb = h[1];
    mc.lbeta_ab = lbeta_js(h[0], h[1]);
  }
  // reciprocals of the constant prior divisors, as the kernel's own make_reciprocal computes them
  const Reciprocal y0 = make_reciprocal(mc.den0), y1 = make_reciprocal(mc.den1);
  mc.y0_hi = y0.hi; mc.y0_lo = y0.lo; mc.den0_ok = (!options->exact_division && mid_range(mc.den0)) ? 1 : 0;
  mc.y1_hi = y1.hi; mc.y1_lo = y1.lo; mc.den1_ok = (!options->exact_division && mid_range(mc.den1)) ? 1 : 0;
  mc.exact_division = options->exact_division ? 1 : 0;
  mc.group_local = 0, mc.sufficient = 0;
}

// amwg_options::sufficient_statistics: the two sufficient statistics of the Normal likelihood, in quad precision -- xbar as a double-double (its error must stay
// far below an ulp of xbar - mu when mu sits next to the data: 2^-106 |xbar|), SS = sum (x_i - xbar)^2 rounded once
static void sufficient_statistics(const double *x, int N, DatasetConsts &k) {
  __float128 sum = 0;
  for (int i = 0; i < N; ++i) sum += (__float128)x[i];
  const __float128 xbar = N > 0 ? sum / (__float128)N : (__float128)0;
  __float128 ss = 0;
  for (int i = 0; i < N; ++i) { const __float128 t = (__float128)x[i] - xbar; ss += t * t; }
  k.suff_xbar_hi = (double)xbar;
  k.suff_xbar_lo = (double)(xbar - (__float128)k.suff_xbar_hi);
  k.suff_ss = (double)ss;
}
// what the option asks of the call, and what it sets for the sampler: the one-lane certified kernel, told to read the statistics
static int use_sufficient_statistics(amwg_sampler *s, const amwg_model_desc *m, const amwg_options *options) {
  if (m->model != AMWG_MODEL_NORMAL) return amwg_fail(AMWG_EINVAL, "sufficient_statistics: only the Normal family has a pass-free certified value");
  // (AMWG_LANES_AUTOTUNE would time -- and could keep -- a multi-lane kernel, which never reads mc.sufficient; AMWG_LANES_FASTEST is taken as 1 below)
  if (options->lanes_per_chain > 1 || options->lanes_per_chain == AMWG_LANES_AUTOTUNE)
    return amwg_fail(AMWG_EINVAL, "sufficient_statistics decides from the one-lane certified kernel: lanes_per_chain must be 0, 1 or AMWG_LANES_FASTEST, got %d", options->lanes_per_chain);
  s->mc.sufficient = 1;
  s->opt.lanes_per_chain = 1;
  return AMWG_OK;
}

// group-local evaluation (include/amwg.h, amwg_options::group_local; amwg_gl.h): the hierarchical family with a chain on one whole
// wavefront, every lane serving one group -- which is what lets one pass evaluate all the proposals of a sweep over theta
static int group_local_setup(amwg_sampler *s, const amwg_model_desc *m, const amwg_param_desc *params, int n_params, const amwg_options *options, GlLayoutHost *gl) {
  if (m->model != AMWG_MODEL_HIER_NORMAL) return amwg_fail(AMWG_EINVAL, "group_local: only the hierarchical Normal family has a group-local evaluation");
  if (n_params != 3 || !params[0].multidim || params[0].len != m->G || params[0].top != m->G)
    return amwg_fail(AMWG_EINVAL, "group_local: parameters must be theta (dim [G]), mu, sigma");
  if (options->lanes_per_chain != 0 && options->lanes_per_chain != 64) return amwg_fail(AMWG_EINVAL, "group_local runs a chain on one wavefront: lanes_per_chain must be 0 or 64");
  TRYB(gl_layout(m->x, m->g, m->n_obs, m->G, gl));
  s->opt.lanes_per_chain = 64;
  s->mc.group_local = 1;
  return AMWG_OK;
}

// A dataset sampler (amwg_create_datasets, amwg_create_datasets_ragged) keeps the copies of its D datasets back to back, one allocation per array: dataset d's
// len(d) elements begin at the element offset this records in consts[d].*off, every copy on a 256-byte boundary like an allocation of its own (the sizes may
// differ, so these are running sums, not multiples of a stride).  D == 1: the ordinary sampler's allocation.  get(d): dataset d's elements on the host.
template <class T, class Len, class Get>
static int upload_datasets(amwg_sampler *s, int D, Len len, Get get, std::vector<DatasetConsts> &consts, int64_t DatasetConsts::*off, T **dev) {
  if (D == 1) return upload(s, get(0), len(0), dev);
  constexpr size_t align = 256 / sizeof(T);
  size_t total = 0;
  for (int d = 0; d < D; ++d) { consts[d].*off = (int64_t)total; total += (len(d) + align - 1) / align * align; }
  std::vector<T> packed(total, T(0));
  for (int d = 0; d < D; ++d) { const T *src = get(d); const size_t n = len(d); T *dst = packed.data() + (size_t)(consts[d].*off); for (size_t i = 0; i < n; ++i) dst[i] = src[i]; }
  return upload(s, packed.data(), packed.size(), dev);
}

// Normal and hierarchical families: the observations; the hierarchical family's group labels as bytes; with group_local the lane-major tile and the
// lane table instead of the observations (amwg_gl.h).  (D > 1 datasets: the Normal family only; data_mid_range is a per-dataset constant)
static int upload_normal_data(amwg_sampler *s, const amwg_model_desc *models, int D, const GlLayoutHost &gl, std::vector<DatasetConsts> &consts) {
  const amwg_model_desc *m = &models[0];
  const int N = m->n_obs;
  DataRef &d = s->d;
  for (int k = 0; k < D; ++k) {
    bool mid = true;
    for (int i = 0; i < models[k].n_obs; ++i) mid = mid && (models[k].x[i] == 0.0 || mid_range(std::fabs(models[k].x[i])));
    consts[k].data_mid_range = mid ? 1 : 0;
  }
  double *dx = nullptr;
  TRYB(upload_datasets(s, D, [&](int k) { return (size_t)models[k].n_obs; }, [&](int k) { return models[k].x; }, consts, &DatasetConsts::off_x, &dx));
  d.x = dx;
  if (m->model != AMWG_MODEL_HIER_NORMAL) return AMWG_OK;
  std::vector<uint8_t> gb((size_t)N);
  for (int i = 0; i < N; ++i) {
    if (m->g[i] < 0 || m->g[i] >= m->G) return amwg_fail(AMWG_EINVAL, "hier_normal: g[%d] = %d outside 0..%d", i, m->g[i], m->G - 1);
    gb[i] = (uint8_t)m->g[i];
  }
  uint8_t *dg = nullptr;
  TRYB(upload(s, gb.data(), (size_t)N, &dg));
  d.xb = dg;
  if (!s->mc.group_local) return AMWG_OK;
  double *dt = nullptr;
  GlLane *dl = nullptr;
  TRYB(upload(s, gl.tile.data(), gl.tile.size(), &dt));
  TRYB(upload(s, gl.lane.data(), gl.lane.size(), &dl));
  d.x = dt;
  d.arr[0] = dl;
  s->gl_rounds = gl.rounds;
  d.K = gl.n_min;
  return AMWG_OK;
}
// Bernoulli family: the observations as bytes and as bits, and the tables of two_valued_sum -- per dataset, in that dataset's own sizes, as is has_invalid
static int upload_bernoulli_data(amwg_sampler *s, const amwg_model_desc *models, int D, std::vector<DatasetConsts> &consts) {
  std::vector<std::vector<uint8_t>> xb((size_t)D);
  std::vector<std::vector<uint32_t>> xw((size_t)D), tab((size_t)D);
  for (int k = 0; k < D; ++k) {
    const int N = models[k].n_obs;
    xb[k].assign((size_t)N, 0);
    xw[k].assign(BetaBernModel::words(N), 0u);
    bool invalid = false;
    for (int i = 0; i < N; ++i) {
      const bool one = models[k].x[i] == 1;
      invalid = invalid || !(one || models[k].x[i] == 0);
      xb[k][i] = one ? 1 : 0;
      if (one) xw[k][(size_t)i >> 5] |= 1u << (i & 31);
    }
    consts[k].has_invalid = invalid ? 1 : 0;
    tab[k] = two_valued_tables(xb[k].data(), N);
    if (tab[k].size() != 6 * two_valued_words(N)) return amwg_fail(AMWG_EINVAL, "internal: two_valued_tables of %zu words, expected %zu", tab[k].size(), 6 * two_valued_words(N));
  }
  uint8_t *dxb = nullptr;
  uint32_t *dxw = nullptr, *dtab = nullptr;
  TRYB(upload_datasets(s, D, [&](int k) { return tab[k].size(); }, [&](int k) { return tab[k].data(); }, consts, &DatasetConsts::off_arr0, &dtab));
  s->d.arr[0] = dtab;
  TRYB(upload_datasets(s, D, [&](int k) { return xb[k].size(); }, [&](int k) { return xb[k].data(); }, consts, &DatasetConsts::off_xb, &dxb));
  TRYB(upload_datasets(s, D, [&](int k) { return xw[k].size(); }, [&](int k) { return xw[k].data(); }, consts, &DatasetConsts::off_xw, &dxw));
  s->d.xb = dxb;
  s->d.xw = dxw;
  // which observations are neither 0 nor 1 (xb holds 0 there): no step kernel asks -- has_invalid settles their sum --, the pointwise terms of
  // amwg_last_sample_dataset_waic do.  Bytes laid out like xb (the same lengths, so off_xb serves both), behind arr[1]; absent while every value is valid
  bool any_invalid = false;
  for (int k = 0; k < D; ++k) any_invalid = any_invalid || consts[k].has_invalid;
  if (any_invalid) {
    std::vector<std::vector<uint8_t>> bad((size_t)D);
    for (int k = 0; k < D; ++k) {
      bad[k].assign((size_t)models[k].n_obs, 0);
      for (int i = 0; i < models[k].n_obs; ++i) bad[k][i] = !(models[k].x[i] == 1 || models[k].x[i] == 0);
    }
    std::vector<DatasetConsts> same(consts);      // (the offsets come out as off_xb's)
    uint8_t *dbad = nullptr;
    TRYB(upload_datasets(s, D, [&](int k) { return bad[k].size(); }, [&](int k) { return bad[k].data(); }, same, &DatasetConsts::off_xb, &dbad));
    s->d.arr[1] = dbad;
  }
  return AMWG_OK;
}
// Poisson family: the design matrix column-major [7][n_d] (a dataset's column stride is its own size), the counts, log(y_i!), and what the bounds of the certified
// pass are made of (PoisGlmModel::log_post_approx) -- per dataset
static int upload_poisson_data(amwg_sampler *s, const amwg_model_desc *models, int D, std::vector<DatasetConsts> &consts) {
  std::vector<std::vector<double>> lf((size_t)D), Xt((size_t)D);
  for (int d = 0; d < D; ++d) {
    const amwg_model_desc *m = &models[d];
    const int N = m->n_obs;
    DatasetConsts &mc = consts[d];
    lf[d].assign((size_t)N, 0.0);
    Xt[d].assign((size_t)N * 7, 0.0);
    for (int i = 0; i < N; ++i) lf[d][i] = m->y[i] < 0 ? (double)INFINITY : lfactorial_js(m->y[i]);
    for (int i = 0; i < N; ++i) for (int k = 0; k < 7; ++k) Xt[d][(size_t)k * N + i] = m->x[(size_t)i * 7 + k];   // row-major [N][7] -> column-major [7][N]
    for (int k = 0; k < 7; ++k) { double mx = 0; for (int i = 0; i < N; ++i) { const double v = std::fabs(m->x[(size_t)i * 7 + k]); mx = (v > mx || v != v) ? v : mx; } mc.glm_xmax[k] = mx; }
    mc.glm_sum_y = 0; mc.glm_sum_lf = 0;
    for (int i = 0; i < N; ++i) { mc.glm_sum_y += std::fabs(m->y[i]); mc.glm_sum_lf += std::fabs(lf[d][i]); }
  }
  double *dX = nullptr, *dy = nullptr, *dlf = nullptr;
  TRYB(upload_datasets(s, D, [&](int d) { return Xt[d].size(); }, [&](int d) { return Xt[d].data(); }, consts, &DatasetConsts::off_x, &dX));
  TRYB(upload_datasets(s, D, [&](int d) { return (size_t)models[d].n_obs; }, [&](int d) { return models[d].y; }, consts, &DatasetConsts::off_y, &dy));
  TRYB(upload_datasets(s, D, [&](int d) { return lf[d].size(); }, [&](int d) { return lf[d].data(); }, consts, &DatasetConsts::off_lfact, &dlf));
  s->d.x = dX; s->d.y = dy; s->d.lfact = dlf;
  return AMWG_OK;
}

// hierarchical family: for which lane counts 2^j do the group labels repeat with the lane stride (bit j: g[i] == g[i mod 2^j])?
static uint32_t periodic_label_mask(const amwg_model_desc *m) {
  uint32_t mask = 0;
  for (int j = 0; j <= 10; ++j) {
    const int Gj = 1 << j;
    bool periodic = m->n_obs > 0;
    for (int i = Gj; i < m->n_obs && periodic; ++i) periodic = m->g[i] == m->g[i % Gj];
    if (periodic) mask |= 1u << j;
  }
  return mask;
}

// ---- What both constructors end with, once the data and the chains' state are on the device: the device's limits, the plan (measured or priced), the kernel
// (`prepare`, once a plan is adopted), a sync.  The constructor's warm-up log_post (mcmc.js:961-963) is folded into the first launch
// (StepArgs.init_lp); amwg_chain_diag forces it with a 0-step launch if asked earlier.
static int plan_and_prepare(amwg_sampler *s, const hipDeviceProp_t &prop, PhaseClock &clk, const std::function<int()> &prepare) {
  const size_t max_lds = prop.sharedMemPerBlock ? prop.sharedMemPerBlock : 65536;
  const int n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (s->opt.lanes_per_chain == AMWG_LANES_AUTOTUNE) TRYB(autotune_geometry(s, n_cus, max_lds, prepare));
  else { LaunchPlan plan; TRYB(choose_geometry(s, s->opt.lanes_per_chain, n_cus, max_lds, &plan)); TRYB(adopt_plan(s, plan)); }
  clk.mark("geometry");
  TRYB(prepare());
  clk.mark("kernel attribute (module load)");
  HIP_TRY(hipStreamSynchronize(s->stream));
  clk.mark("sync");
  return AMWG_OK;
}

// ---- amwg_create_user, step by step.  The model struct, and the row plan as far as the GENERATED SOURCE states it: the source is what gets compiled, and a caller built against an older
// amwg_user_model -- a shorter struct: the rows_* fields are then whatever follows it in memory -- must not switch a layout on that the model has
// no code for (round-5 advisor finding).  The certified tails are read from the source alone: no struct field carries them.
static int adopt_user_model(amwg_sampler *s, const amwg_user_model *m, int max_threads) {
  s->user = true;
  s->D = m->n_derived;
  s->user_lds = (m->lds_bytes + 15) & ~15;
  s->user_lds_one_lane = m->lds_bytes_one_lane > 0 ? ((m->lds_bytes_one_lane + 15) & ~15) : s->user_lds;
  s->user_parallel = m->parallel ? 1 : 0;
  s->user_max_threads = max_threads;
  s->user_work = m->work_per_eval;
  s->user_work_one_lane = m->work_one_lane;
  if (m->rows_n_obs < 0 || m->rows_groups < 0) return amwg_fail(AMWG_EINVAL, "amwg_create_user: negative row plan");
  const SourceTraits t = source_traits(m->source);
  const bool rows_ok = m->rows_n_obs > 0 && t.row_n == (long)m->rows_n_obs && t.row_groups == (long)m->rows_groups;
  if (m->rows_n_obs > 0 && !rows_ok && t.row_n >= 0)
    return amwg_fail(AMWG_EINVAL, "amwg_create_user: row plan (%d observations, %d groups) does not match the generated source (kRowN = %ld, kRowGroups = %ld)", m->rows_n_obs, m->rows_groups, t.row_n, t.row_groups);
  s->user_rows_n = rows_ok ? m->rows_n_obs : 0;
  s->user_rows_groups = rows_ok ? m->rows_groups : 0;
  s->user_rows_sweep = (rows_ok && m->rows_sweep && t.row_sweep) ? 1 : 0;
  s->user_rows_cert = s->user_rows_sweep && t.row_cert;
  s->user_cert_tail_n = t.cert_tail_n;
  s->user_pois_tail_n = t.pois_tail_n;
  s->user_logit_tail_n = t.logit_tail_n;
  return AMWG_OK;
}

// array j of a closure stored as the type T (the doubles themselves, or an integer type: elements that it cannot hold are refused), with `pad` spare elements behind
// it.  D > 1 (amwg_create_user_datasets): the D copies back to back in ONE allocation, each starting on a 256-byte boundary like an allocation of its own and followed by
// its own spare elements; dev[d] = dataset d's copy.
template <class T>
static int upload_user_array(amwg_sampler *s, const amwg_user_model *models, int D, int j, const char *type_name, size_t pad, const void **dev) {
  const size_t n = (size_t)models[0].array_len[j];
  constexpr size_t align = 256 / sizeof(T);
  const size_t stride = D == 1 ? n + pad : (n + pad + align - 1) / align * align;
  std::vector<T> tmp(stride * (size_t)D, T(0));
  for (int d = 0; d < D; ++d)
    for (size_t i = 0; i < n; ++i) {
      const double v = models[d].arrays[j][i];
      if constexpr (!std::is_same<T, double>::value) {
        if (!(v >= (double)std::numeric_limits<T>::min() && v <= (double)std::numeric_limits<T>::max() && v == (double)(T)v)) {
          if (D == 1) return amwg_fail(AMWG_EINVAL, "amwg_create_user: array %d element %lld (%g) does not fit %s", j, (long long)i, v, type_name);
          return amwg_fail(AMWG_EINVAL, "amwg_create_user_datasets: dataset %d: array %d element %lld (%g) does not fit %s", d, j, (long long)i, v, type_name);
        }
      }
      tmp[(size_t)d * stride + i] = (T)v;
    }
  T *p = nullptr;
  TRYB(dev_alloc(s, &p, tmp.size()));
  if (D == 1 ? n > 0 : !tmp.empty()) HIP_TRY(hipMemcpy(p, tmp.data(), (D == 1 ? n : tmp.size()) * sizeof(T), hipMemcpyHostToDevice));
  for (int d = 0; d < D; ++d) dev[d] = p + (size_t)d * stride;
  return AMWG_OK;
}

// every array the closure reads, row-major, in the storage type the translator chose.  D > 1: of every dataset, and the device table [D][row_stride] of their
// places (amwg_user_dataset.h); the sampler's own DataRef then holds dataset 0's, as an ordinary sampler's would.
int upload_user_arrays(amwg_sampler *s, const amwg_user_model *models, int D) {
  const amwg_user_model *m = &models[0];
  s->d.n_obs = 0;
  const int row_stride = m->n_arrays > kInlineUserArrays ? m->n_arrays : kInlineUserArrays;
  std::vector<const void *> table((size_t)D * row_stride, nullptr), at((size_t)D);
  for (int j = 0; j < m->n_arrays; ++j) {
    for (int d = 0; d < D; ++d)
      if (models[d].array_len[j] < 0 || (models[d].array_len[j] && !models[d].arrays[j])) return amwg_fail(AMWG_EINVAL, "amwg_create_user: array %d is null or has a negative length", j);
    const int ty = m->array_type ? m->array_type[j] : AMWG_F64;
    if (ty == AMWG_F64 && D == 1) { double *pd = nullptr; TRYB(upload(s, m->arrays[j], (size_t)m->array_len[j], &pd)); at[0] = pd; }      // (as they lie: no packing)
    else if (ty == AMWG_F64) TRYB(upload_user_array<double>(s, models, D, j, "f64", 0, at.data()));
    else if (ty == AMWG_U8) TRYB(upload_user_array<uint8_t>(s, models, D, j, "u8", 16, at.data()));
    else if (ty == AMWG_I32) TRYB(upload_user_array<int32_t>(s, models, D, j, "i32", 4, at.data()));
    else return amwg_fail(AMWG_EINVAL, "amwg_create_user: array %d has unknown storage type %d", j, ty);
    for (int d = 0; d < D; ++d) table[(size_t)d * row_stride + j] = at[d];
  }
  for (int j = 0; j < m->n_arrays && j < kInlineUserArrays; ++j) s->d.arr[j] = table[j];
  if (m->n_arrays > kInlineUserArrays || D > 1) {      // (one table serves both: row d's entries from kInlineUserArrays on are dataset d's arr_ext)
    const void **d_table = nullptr;
    TRYB(upload(s, table.data(), table.size(), &d_table));
    s->d.arr_ext = d_table + kInlineUserArrays;
    if (D > 1) { s->d_user_ds_table = d_table; s->user_ds_row_stride = row_stride; s->user_ds_n_arrays = m->n_arrays; }
  }
  return AMWG_OK;
}

// ---- amwg_create, amwg_create_datasets and amwg_create_datasets_ragged from here on: D datasets of one built-in family, of any sizes (D == 1: the ordinary
// sampler; equal sizes: the special case the second entry insists on).  What depends on ONE dataset's data or size is written into that dataset's DatasetConsts and
// nowhere else.  From there it goes one way: dataset 0's into the sampler's own ModelConsts (dataset_constants, amwg_dataset.h -- what an ordinary sampler's kernel
// reads), and for D > 1 the whole table to the device, beside the arrays laid back to back, where every workgroup takes its dataset's row (dataset_view).
static int create_builtin(const amwg_model_desc *models, int D, const amwg_param_desc *params, int32_t n_params, const double *init,
                          const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out) {
  const amwg_model_desc *m = &models[0];
  if (n_params < 1 || n_params > kMaxIndex) return amwg_fail(AMWG_EINVAL, "amwg_create: %d named parameters (supported: 1..%d)", n_params, kMaxIndex);
  for (int d = 0; d < D; ++d) if (models[d].n_obs < 0) return amwg_fail(AMWG_EINVAL, "amwg_create: n_obs < 0");
  const FamilyRow *family = family_of(m->model);      // (an unknown model is reported by check_family_args, after the options and the layout)
  TRYB(check_options(options, family ? family->max_threads : 64));
  SamplerGuard guard(options, m->model);
  amwg_sampler *s = guard.s;
  PhaseClock clk;
  TRYB(build_layout(s, params, n_params, false));
  for (int d = 0; d < D; ++d) TRYB(check_family_args(&models[d], params, n_params, s->P));
  hipDeviceProp_t prop;
  clk.mark("layout + checks");
  TRYB(open_device(s, &prop));
  clk.mark("open device (HIP runtime)");
  model_constants(m, options, s->mc);
  std::vector<DatasetConsts> consts((size_t)D, DatasetConsts{});
  s->ds_n_obs.resize((size_t)D);
  int n_max = 0;
  for (int d = 0; d < D; ++d) {
    consts[d].data_mid_range = 1;      // (the Normal and hierarchical families look at their observations: upload_normal_data)
    size_constants(models[d].n_obs, consts[d]);
    s->ds_n_obs[d] = models[d].n_obs;
    n_max = models[d].n_obs > n_max ? models[d].n_obs : n_max;
  }
  if (options->sufficient_statistics) {
    TRYB(use_sufficient_statistics(s, m, options));
    for (int d = 0; d < D; ++d) sufficient_statistics(models[d].x, models[d].n_obs, consts[d]);
  }
  GlLayoutHost gl;
  if (options->group_local) TRYB(group_local_setup(s, m, params, n_params, options, &gl));
  s->d.n_obs = n_max; s->d.G = m->G; s->d.K = m->K;      // (D > 1: the LARGEST dataset's size -- a workgroup's own arrives through the table, amwg_dataset.h; the plan reads ds_n_obs)
  if (m->model == AMWG_MODEL_NORMAL || m->model == AMWG_MODEL_HIER_NORMAL) TRYB(upload_normal_data(s, models, D, gl, consts));
  else if (m->model == AMWG_MODEL_BETA_BERN) TRYB(upload_bernoulli_data(s, models, D, consts));
  else TRYB(upload_poisson_data(s, models, D, consts));
  dataset_constants(s->mc, consts[0]);
  if (D > 1) {
    TRYB(upload(s, consts.data(), consts.size(), &s->d_ds_consts));
    s->n_datasets = D;
  }
  clk.mark("device + data upload");
  TRYB(alloc_chain_state(s, params, n_params, init, comp_opts));
  clk.mark("chain state");
  if (m->model == AMWG_MODEL_HIER_NORMAL && !options->exact_division) s->hier_periodic_mask = periodic_label_mask(m);
  TRYB(plan_and_prepare(s, prop, clk, [s]() -> int {      // once the plan is adopted
    const void *kernel = s->n_datasets > 1 ? reinterpret_cast<const void *>(s->ds_kernel) : reinterpret_cast<const void *>(s->kernel);
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, s->plan.lds);
    return e == hipSuccess ? AMWG_OK : amwg_fail(AMWG_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
  }));
  *out = guard.release();
  return AMWG_OK;
}

extern "C" {

int amwg_create(const amwg_model_desc *m, const amwg_param_desc *params, int32_t n_params, const double *init,
                const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out) {
  if (!m || !params || !init || !comp_opts || !options || !out) return amwg_fail(AMWG_EINVAL, "amwg_create: null argument");
  return create_builtin(m, 1, params, n_params, init, comp_opts, options, out);
}

// what both dataset entries check before a device is opened; `ragged`: the sizes may differ
static int create_datasets(const char *entry, bool ragged, const amwg_model_desc *models, int32_t n_datasets, const amwg_param_desc *params, int32_t n_params, const double *init,
                           const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out) {
  if (!models || !params || !init || !comp_opts || !options || !out) return amwg_fail(AMWG_EINVAL, "%s: null argument", entry);
  if (n_datasets < 1) return amwg_fail(AMWG_EINVAL, "%s: n_datasets must be >= 1, got %d", entry, n_datasets);
  if (n_datasets == 1) return amwg_create(models, params, n_params, init, comp_opts, options, out);
  if (options->chains % n_datasets != 0)
    return amwg_fail(AMWG_EINVAL, "%s: chains (%lld, the total) must be a multiple of n_datasets (%d)", entry, (long long)options->chains, n_datasets);
  for (int d = 1; d < n_datasets; ++d) {
    if (models[d].model != models[0].model) return amwg_fail(AMWG_EINVAL, "%s: dataset %d is of model %d, dataset 0 of model %d (one family per sampler)", entry, d, models[d].model, models[0].model);
    if (!ragged && models[d].n_obs != models[0].n_obs)
      return amwg_fail(AMWG_EINVAL, "%s: dataset %d has n_obs = %d, dataset 0 has %d (ragged datasets are not supported); datasets of unequal sizes: amwg_create_datasets_ragged", entry, d, models[d].n_obs, models[0].n_obs);
    if (models[d].K != models[0].K || models[d].G != models[0].G) return amwg_fail(AMWG_EINVAL, "%s: dataset %d has K = %d, G = %d, dataset 0 has K = %d, G = %d", entry, d, models[d].K, models[d].G, models[0].K, models[0].G);
    for (int k = 0; k < 8; ++k)
      if (memcmp(&models[d].hyper[k], &models[0].hyper[k], sizeof(double)) != 0)
        return amwg_fail(AMWG_EINVAL, "%s: dataset %d has hyper[%d] = %g, dataset 0 has %g (the hyper-parameters are shared)", entry, d, k, models[d].hyper[k], models[0].hyper[k]);
  }
  if (models[0].model == AMWG_MODEL_HIER_NORMAL)
    return amwg_fail(AMWG_EINVAL, "%s: the hierarchical family is not supported (its launch plan depends on properties of the group labels, which differ between datasets)", entry);
  if (options->group_local) return amwg_fail(AMWG_EINVAL, "%s: group_local is an evaluation of the hierarchical family, which dataset samplers do not support", entry);
  if (options->lanes_per_chain == AMWG_LANES_AUTOTUNE)
    return amwg_fail(AMWG_EINVAL, "%s: AMWG_LANES_AUTOTUNE is not supported (the timing runs would have to search the geometries that serve whole datasets); give lanes_per_chain or leave it 0", entry);
  return create_builtin(models, n_datasets, params, n_params, init, comp_opts, options, out);
}

int amwg_create_datasets(const amwg_model_desc *models, int32_t n_datasets, const amwg_param_desc *params, int32_t n_params, const double *init,
                         const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out) {
  return create_datasets("amwg_create_datasets", false, models, n_datasets, params, n_params, init, comp_opts, options, out);
}

int amwg_create_datasets_ragged(const amwg_model_desc *models, int32_t n_datasets, const amwg_param_desc *params, int32_t n_params, const double *init,
                                const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out) {
  return create_datasets("amwg_create_datasets_ragged", true, models, n_datasets, params, n_params, init, comp_opts, options, out);
}

// amwg_create_user and amwg_create_user_datasets from here on: one translated closure on D datasets (D == 1: the ordinary sampler).  `entry`: the name in the messages.
static int create_user(const char *entry, const amwg_user_model *models, int D, const amwg_param_desc *params, int32_t n_params, const double *init,
                       const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out);

int amwg_create_user(const amwg_user_model *m, const amwg_param_desc *params, int32_t n_params, const double *init,
                     const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out) {
  if (!m || !m->source || !params || !init || !comp_opts || !options || !out) return amwg_fail(AMWG_EINVAL, "amwg_create_user: null argument");
  return create_user("amwg_create_user", m, 1, params, n_params, init, comp_opts, options, out);
}

// What the dataset entry of a closure checks before a device is opened: ONE source, ONE layout of the arrays, nothing in the source that is formed from one dataset's
// values (the row plan's layout, the sums of the certified Poisson / logistic tails).
int amwg_create_user_datasets(const amwg_user_model *models, int32_t n_datasets, const amwg_param_desc *params, int32_t n_params, const double *init,
                              const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out) {
  const char *entry = "amwg_create_user_datasets";
  if (!models || !params || !init || !comp_opts || !options || !out) return amwg_fail(AMWG_EINVAL, "%s: null argument", entry);
  if (n_datasets < 1) return amwg_fail(AMWG_EINVAL, "%s: n_datasets must be >= 1, got %d", entry, n_datasets);
  for (int d = 0; d < n_datasets; ++d) if (!models[d].source) return amwg_fail(AMWG_EINVAL, "%s: null argument (dataset %d: source)", entry, d);
  if (n_datasets == 1) return amwg_create_user(models, params, n_params, init, comp_opts, options, out);
  if (options->chains % n_datasets != 0)
    return amwg_fail(AMWG_EINVAL, "%s: chains (%lld, the total) must be a multiple of n_datasets (%d)", entry, (long long)options->chains, n_datasets);
  const amwg_user_model &m0 = models[0];
  for (int d = 1; d < n_datasets; ++d) {
    const amwg_user_model &m = models[d];
    if (strcmp(m.source, m0.source) != 0)
      return amwg_fail(AMWG_EINVAL, "%s: dataset %d: source differs from dataset 0's (one generated source serves all datasets: translate.js translate_datasets)", entry, d);
    if (m.n_arrays != m0.n_arrays) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: n_arrays = %d, dataset 0 has %d", entry, d, m.n_arrays, m0.n_arrays);
    if (m.n_arrays > 0 && (!m.arrays || !m.array_len || !m0.arrays || !m0.array_len)) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: arrays is null", entry, d);
    for (int j = 0; j < m.n_arrays; ++j) {
      if (m.array_len[j] != m0.array_len[j])
        return amwg_fail(AMWG_EINVAL, "%s: dataset %d: array_len[%d] = %lld, dataset 0 has %lld (the datasets of a closure are of equal shape; ragged ones are not supported)", entry, d, j,
                         (long long)m.array_len[j], (long long)m0.array_len[j]);
      const int t = m.array_type ? m.array_type[j] : AMWG_F64, t0 = m0.array_type ? m0.array_type[j] : AMWG_F64;
      if (t != t0) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: array_type[%d] = %d, dataset 0 has %d (one storage type per array: the widest over the datasets)", entry, d, j, t, t0);
    }
#define AMWG_SAME(field) if (m.field != m0.field) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: " #field " = %d, dataset 0 has %d", entry, d, (int)m.field, (int)m0.field)
    AMWG_SAME(n_derived); AMWG_SAME(lds_bytes); AMWG_SAME(lds_bytes_one_lane); AMWG_SAME(parallel); AMWG_SAME(max_threads); AMWG_SAME(rows_n_obs); AMWG_SAME(rows_groups); AMWG_SAME(rows_sweep);
#undef AMWG_SAME
  }
  const SourceTraits t = source_traits(m0.source);
  if (t.row_n >= 0 || m0.rows_n_obs > 0)
    return amwg_fail(AMWG_EINVAL, "%s: the source has a row plan (kRowN): its layout is formed from one dataset's labels; translate with no_row_plan (translate_datasets does)", entry);
  // (a certified Poisson / logistic tail: accepted when its sums and column maxima are slots of each dataset's own constants array -- kTailPerDataset --, refused when
  // they are literals of the text, formed from ONE dataset's values)
  if ((t.pois_tail_n > 0 || t.logit_tail_n > 0) && !t.tail_per_dataset)
    return amwg_fail(AMWG_EINVAL, "%s: the source has a certified %s tail (%s): its bound holds sums over one dataset's values; translate with no_pois_tail / no_logit_tail (translate_datasets does)", entry,
                     t.pois_tail_n > 0 ? "Poisson" : "logistic", t.pois_tail_n > 0 ? "kPoisTail" : "kLogitTail");
  if (options->lanes_per_chain == AMWG_LANES_AUTOTUNE)
    return amwg_fail(AMWG_EINVAL, "%s: AMWG_LANES_AUTOTUNE is not supported (the timing runs would have to search the geometries that serve whole datasets); give lanes_per_chain or leave it 0", entry);
  return create_user(entry, models, n_datasets, params, n_params, init, comp_opts, options, out);
}

static int create_user(const char *entry, const amwg_user_model *models, int D, const amwg_param_desc *params, int32_t n_params, const double *init,
                       const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out) {
  const amwg_user_model *m = &models[0];
  (void)entry;
  if (n_params < 1 || n_params > (1 << 20)) return amwg_fail(AMWG_EINVAL, "amwg_create_user: %d parameter entries (supported: 1..%d, of which at most %d stepped)", n_params, 1 << 20, kMaxIndex);
  if (m->n_arrays < 0) return amwg_fail(AMWG_EINVAL, "amwg_create_user: %d data arrays", m->n_arrays);
  if (m->n_arrays && (!m->arrays || !m->array_len)) return amwg_fail(AMWG_EINVAL, "amwg_create_user: arrays is null");
  if (m->n_derived < 0 || m->lds_bytes < 0) return amwg_fail(AMWG_EINVAL, "amwg_create_user: negative size");
  const int max_threads = m->max_threads > 0 ? (m->max_threads / 64) * 64 : 1024;
  if (max_threads < 64 || max_threads > 1024) return amwg_fail(AMWG_EINVAL, "amwg_create_user: max_threads must be in 64..1024");
  TRYB(check_options(options, max_threads));
  if (options->sufficient_statistics) return amwg_fail(AMWG_EINVAL, "sufficient_statistics: only the built-in Normal family has a pass-free certified value (translated closures: the certified tail's pass)");
  SamplerGuard guard(options, 0);
  amwg_sampler *s = guard.s;
  PhaseClock clk(false);
  TRYB(adopt_user_model(s, m, max_threads));
  TRYB(build_layout(s, params, n_params, true));
  for (int p = 0; p < n_params; ++p) s->user_has_binary = s->user_has_binary || params[p].type == AMWG_BINARY;
  hipDeviceProp_t prop;
  if (D > 1) { s->n_datasets = D; s->ds_n_obs.assign((size_t)D, 0); }      // (before the plan: only geometries that serve whole datasets are searched, amwg_plan.hip)
  TRYB(open_device(s, &prop));
  TRYB(upload_user_arrays(s, models, D));
  TRYB(alloc_chain_state(s, params, n_params, init, comp_opts));
  TRYB(plan_and_prepare(s, prop, clk, [&]() { return load_user_kernel(s, m->source, prop.gcnArchName); }));
  s->user_source = m->source;      // (amwg_set_pointwise: the program of the pointwise terms begins with it)
  s->user_arch = prop.gcnArchName;
  *out = guard.release();
  return AMWG_OK;
}

int amwg_destroy(amwg_sampler *s) {
  if (!s) return AMWG_OK;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (void *p : s->dev_allocs) (void)hipFree(p);
  amwg_summary_forget(s);      // (amwg_fold.h: the accumulators of a summarising call were among dev_allocs)
  amwg_histogram_forget(s);    // (amwg_histogram.h: the edges and counts of an armed histogram)
  amwg_covariance_forget(s);   // (amwg_covariance.h: the co-moments and values of an armed covariance)
  amwg_autocov_forget(s);      // (amwg_autocov.h: the lag sums, rows and values of an armed autocovariance)
  if (s->d_draws) (void)hipFree(s->d_draws);
  if (s->user_module) (void)hipModuleUnload(s->user_module);
  if (s->pw_module) (void)hipModuleUnload(s->pw_module);
  for (hipEvent_t e : s->chunk_ev) (void)hipEventDestroy(e);
  if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
  return AMWG_OK;
}

}  // extern "C"
