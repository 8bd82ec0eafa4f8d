/* amwg_selftest.h -- TEST BUILD ONLY (libamwg_selftest.so = libamwg.so's sources compiled with -DAMWG_SELFTEST): the arithmetic building
 * blocks of the kernel exported one by one, so that each can be pinned against V8 / the reference's distributions.js on the host and on
 * the device.  None of this is in the product library. */
#ifndef AMWG_SELFTEST_H
#define AMWG_SELFTEST_H
#include "amwg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Device evaluation: op in {0:exp,1:log,2:sqrt,3:lgamma,4:a/b via hoisted reciprocal,5:ld_norm(a,b,c),...};
 * a,b,c host arrays of n doubles (b,c may be NULL), out host array of n doubles. */
int amwg_device_eval(int32_t device, int32_t op, int64_t n, const double *a, const double *b, const double *c, double *out);
double amwg_pow(double x, double y);   /* bit-identical to V8 Math.pow */
double amwg_log1p(double x);           /* bit-identical to V8 Math.log1p */
double amwg_expm1(double x);           /* bit-identical to V8 Math.expm1 */
double amwg_math1(int32_t fn, double x); /* fn 0 tanh, 1 atan, 2 log10, 3 sin, 4 cos, 5 tan, 6 asin, 7 acos, 8 sinh, 9 cosh, 10 asinh, 11 acosh, 12 atanh, 13 cbrt, 14 log2:
                                            bit-identical to V8's Math.* (host build of the kernel source, csrc/amwg_math.h + amwg_trig.h) */
double amwg_math2(int32_t fn, double x, double y); /* fn 0: Math.atan2(x, y), 1: Math.hypot(x, y), 2: x % y (JavaScript), 3: x | 0 (ToInt32; y ignored) */
double amwg_hypot3(double x, double y, double z);   /* Math.hypot(x, y, z) */
/* Every scalar ld.* density and helper of distributions.js by id (0 norm 1 unif 2 beta 3 bern 4 pois 5 cauchy
 * 6 laplace 7 gamma 8 invgamma 9 lnorm 10 pareto 11 t 12 weibull 13 logis 14 exp 15 binom 16 nbinom 17 hyper
 * 18 lgamma 19 lfactorial 20 lchoose 21 lbeta): host evaluation of the kernel's own source, and the same on
 * the device for n records of {id, x, a, b, c}. */
double amwg_ld_host(int32_t id, double x, double a, double b, double c);
int amwg_ld_device(int32_t device, int64_t n, const double *records, double *out);
/* out_fast_forward[j] = the two-valued sequential sum of csrc/amwg_twoval.h (exact fast-forward over binades) and
 * out_term_by_term[j] = the plain loop, both on the device, over the n observations x (0/1) from acc0[j] with addends
 * l1[j] (x_i = 1) and l0[j] (x_i = 0); j < m.  Lane j is thread j of 64-thread workgroups: every wavefront holds 64 different cases (tests/test_gpu_twoval.py
 * relies on it).  The six tables are built here, by the library's own two_valued_tables. */
int amwg_two_valued_sum_check(int32_t device, const double *x, int32_t n, int64_t m, const double *acc0, const double *l1, const double *l0,
                              double *out_fast_forward, double *out_term_by_term);
/* Those tables themselves (csrc/amwg_create.hip two_valued_tables, the copy of the recipe that the samplers and the check above upload) for the n observations
 * x (host bytes, non-zero = 1): out_words[6 * (n / 32 + 2)] = w, pre, om1, po1, om0, po0 back to back.  Host only: no device is opened. */
int amwg_two_valued_tables(const uint8_t *x, int32_t n, uint32_t *out_words);
/* The same for the K-valued sequential sum of csrc/amwg_kval.h, K in {1, 2, 3, 5, 8, 13, 16}: idx[n] (host bytes) is the value index of every observation, shared
 * by all lanes; tab the 2 K k_valued_words(n) table words AS THE CALLER BUILT THEM (per block of 32 observations pre[K] then mask[K]; they are not rebuilt here, so
 * that a translator's tables can be put to the test); lane j < m starts from acc0[j] with the addends c[j * K + k].  Lane j is thread j of 64-thread workgroups:
 * every wavefront holds 64 different cases.  out_fast_forward[j] = k_valued_sum<K>, out_term_by_term[j] = acc = acc + c[idx[i]], both on the device.
 * Refused before any device call: null pointers, n < 0, m < 0 or above 2^24, any other K, idx[i] >= K.  n = 0 and m = 0 are legal (m = 0 opens no device). */
int amwg_k_valued_sum_check(int32_t device, int32_t K, const uint8_t *idx, int32_t n, const uint32_t *tab, int64_t m, const double *acc0, const double *c,
                            double *out_fast_forward, double *out_term_by_term);

/* The product's own uniform-stream classes (csrc/amwg_philox.h ChainStream, csrc/amwg_kernel.h CoopStream<G>, csrc/amwg_window.h WindowStream) driven one by one
 * on the device: chain i < n_chains has id chain0 + i under `seed` and starts with consumed0[i] uniforms consumed (host array), so that the chains sharing a
 * wavefront stand at different positions and parities.  kind:
 *     0                          ChainStream::next, a chain per thread
 *     1, 2, 4, 8, 16, 32, 64     CoopStream<kind>::next, `kind` lanes per chain and 64 / kind chains per wavefront (64: the readlane path)
 *     100                        CoopStream<1> under calls[n_calls] (host bytes; 0: next(), 1: next_pair()), which must add up to n_draws uniforms
 *     200                        WindowStream::next, a chain per wavefront
 *     201                        the same, then position() = p, ensure_b(), at(p + i) for i < 128, shift(), ensure_b(), at(q) for q < 256
 * out[n_chains][width] (host): the n_draws uniforms in the order drawn; width = n_draws, for kind 201 n_draws + 128 + 256 (the two runs of at()).
 * consumed_out[n_chains]: consumed() after the n_draws draws.  flags[n_chains][12] (kind 201 only, else NULL): EA, OA, EB, OB after the first ensure_b(), after
 * shift(), and after the second ensure_b().  calls is NULL unless kind is 100.
 * Refused before a device is opened: null pointers, an unknown kind, n_chains < 1, n_draws < 0, sizes beyond 2^28 doubles, calls that do not add up. */
int amwg_stream_check(int32_t device, int32_t kind, uint64_t seed, uint64_t chain0, int64_t n_chains, const uint64_t *consumed0, int64_t n_draws,
                      const uint8_t *calls, int64_t n_calls, double *out, uint64_t *consumed_out, uint64_t *flags);

/* the kernel of amwg_last_sample_dataset_quantiles on a caller's array draws[rows][PR][C] (host), D datasets of C / D chains each: out[D][PR][n_probs] (host).
 * The arguments are checked before a device is opened. */
int amwg_dataset_quantiles_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D,
                                 const double *probs, int32_t n_probs, double *out);

/* the kernels of amwg_last_sample_dataset_hpd on a caller's array draws[rows][PR][C] (host), D datasets of C / D chains each: out[D][PR][n_probs][2] (host),
 * through the launcher the sampler uses.  The arguments are checked before a device is opened. */
int amwg_hpd_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const double *probs, int32_t n_probs, double *out);
/* the two sizes at which that launcher changes route, so that tests can stand on them: lds_keys (NULL: not asked, and no device is opened) = the keys one
 * workgroup sorts in LDS on `device`, a power of two; the scratch budget of later calls in this process is set to scratch_bytes (0: the default of csrc/amwg_hpd.h)
 * and the one in force before goes to scratch_before (may be NULL). */
int amwg_hpd_limits(int32_t device, int64_t scratch_bytes, int64_t *lds_keys, int64_t *scratch_before);

/* the kernels of amwg_last_sample_dataset_waic on a caller's draws[rows][PR][C] (host) and the data of D model descriptions of one family (ragged sizes allowed; the
 * hyper-parameters are not read: priors are not part of the terms), through the launcher the sampler uses: summary[D][4], high[D] (or NULL), pointwise (NULL, or
 * [D][n_max][2]) as that call returns them.  loglik (NULL, or [D][S][n_max], S = rows * (C / D), NaN beyond n_d): the terms l_si themselves from the same device
 * functions, in draw order s = row * (C / D) + chain -- for small shapes, more than 2^24 doubles are refused.  scratch_bytes: the scratch budget of this call
 * (0: the default of csrc/amwg_waic.h).  The arguments are checked before a device is opened. */
int amwg_waic_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const amwg_model_desc *models, int64_t scratch_bytes, double *summary,
                    int32_t *high, double *pointwise, double *loglik);
/* the kernels of amwg_last_sample_dataset_loo likewise: summary[D][4], high[D] (or NULL), pointwise (NULL, or [D][n_max][3]) as that call returns them.  tails (NULL,
 * or [D][n_max][M + 1], M the tail length of S = rows * (C / D)): the M + 1 smallest terms of each observation, sorted, as the fit read them; NaN beyond n_d and for an
 * observation with a non-finite term -- more than 2^24 doubles are refused.  scratch_bytes: the scratch budget of this call (0: the default of csrc/amwg_loo.h). */
int amwg_loo_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const amwg_model_desc *models, int64_t scratch_bytes, double *summary,
                   int32_t *high, double *pointwise, double *tails);
/* the same two for a TRANSLATED CLOSURE (amwg_set_pointwise): models[n_datasets] as amwg_create_user_datasets takes them (one source, arrays of equal shape), P the
 * components of its state, terms_source the pointwise text of translate.js (options.pointwise).  No sampler is made: the arrays are uploaded as a sampler's, the
 * code object is compiled and loaded as a sampler's first WAIC / LOO call does, and the same launchers run on draws[rows][PR][C].  Every dataset has kTermN
 * observations; pointwise, loglik and tails are laid out as above with n_max = kTermN. */
int amwg_user_waic_check(int32_t device, const amwg_user_model *models, int32_t n_datasets, int32_t P, const char *terms_source, const double *draws, int64_t rows, int32_t PR,
                         int64_t C, int64_t scratch_bytes, double *summary, int32_t *high, double *pointwise, double *loglik);
int amwg_user_loo_check(int32_t device, const amwg_user_model *models, int32_t n_datasets, int32_t P, const char *terms_source, const double *draws, int64_t rows, int32_t PR,
                        int64_t C, int64_t scratch_bytes, double *summary, int32_t *high, double *pointwise, double *tails);
/* what the last LOO call of this process did, for the measurement: *passes = the select passes over the terms; ms[4] = milliseconds of the lppd pass, the select,
 * the compaction, the sort and fit (-1 unless timing was on).  Then timing of later calls is switched on (1) or off (0).  Either pointer may be NULL. */
int amwg_loo_stats(int32_t timing, int32_t *passes, double *ms);

/* The fold of amwg_sample_summarize on a caller's array draws[rows][PR][C] (host): the array is folded in windows of window_rows rows through the kernels and the
 * launcher the sampler uses (halves_folded, 4 * PR * C doubles in chain_halves_kernel's layout [half][mean | variance][PR][C]), chain_halves_kernel runs on the whole
 * array (halves_direct, the same size), and the moments of D datasets of C / D chains each come from the folded whole-chain pairs (mean, sd: [D][PR]).
 * Refused before a device is opened: null pointers, non-positive shapes, C % D != 0, window_rows < 1. */
int amwg_fold_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, int64_t window_rows,
                    double *halves_folded, double *halves_direct, double *mean, double *sd);

/* The summaries of stored draws on a caller's array draws[rows][PR][C] (host), D datasets of C / D chains each, through the launchers the sampler's calls use:
 *   mean, sd             [D][PR]  dataset_moments_kernel (amwg_last_sample_moments / _dataset_moments on stored draws)
 *   rhat_ds, ess_ds      [D][PR]  the halves of every chain + dataset_diagnostics_kernel (amwg_last_sample_dataset_diagnostics)
 *   rhat_pooled, ess_pooled [PR]  the same halves + the host reduction of amwg_last_sample_diagnostics over all C chains
 * window_rows = 0: the halves come from chain_halves_kernel (stored draws); window_rows > 0: from the fold of amwg_sample_summarize in windows of window_rows rows.
 * Refused before a device is opened, with the product's words: a null pointer, a bad shape (non-positive sizes, C % D != 0, window_rows < 0), and what split-R-hat
 * refuses ("needs a sample() of >= 4 kept draws on >= 2 chains per dataset": rows < 4 or C / D < 2). */
int amwg_summaries_check(int32_t device, const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, int64_t window_rows,
                         double *mean, double *sd, double *rhat_ds, double *ess_ds, double *rhat_pooled, double *ess_pooled);

/* The histogram kernel of amwg_last_sample_dataset_histogram / amwg_set_histogram on a caller's array draws[rows][PR][C] (host), D datasets of C / D chains each, under
 * edges[PR][bins + 1] (host): the array is uploaded and the product's launcher runs over it in windows of window_rows rows (0 = all at once), as a summarising call
 * runs it window after window.  counts[D][PR][bins + 3] (host) is IN and OUT: the kernel adds to what the caller passes.
 * Refused before a device is opened, with the product's words: null pointers, a bad shape (non-positive sizes, C % D != 0, window_rows < 0), bins outside 1 .. 4096,
 * edges that are not finite or not strictly ascending. */
int amwg_histogram_check(const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const double *edges, int32_t bins, int64_t window_rows,
                         uint64_t *counts, int32_t device);

/* The covariance kernels of amwg_last_sample_dataset_covariance / amwg_set_covariance on a caller's array draws[rows][PR][C] (host), D datasets of C / D chains each,
 * over values[n_values]: the array is uploaded and the product's launchers run over it from zeroed per-chain scratch -- window_rows = 0: the stored path, the whole
 * array as one window; window_rows > 0: window after window through the co-moment kernel and the fold, as a summarising call enqueues them.  cov[D][n_values][n_values]
 * (host) in the order of `values`.  Refused before a device is opened, with the product's words: null pointers, a bad shape (non-positive sizes, C % D != 0,
 * window_rows < 0), n_values outside 1 .. PR, an index outside [0, PR), a repeated index, rows x C / D < 2, a byte count beyond size_t. */
int amwg_covariance_check(const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const int32_t *values, int32_t n_values, int64_t window_rows,
                          double *cov, int32_t device);

/* The autocovariance kernels of amwg_last_sample_dataset_autocovariance / amwg_set_autocovariance on a caller's array draws[rows][PR][C] (host), D datasets of C / D
 * chains each, over values[n_values] at lags 0 .. max_lag: the array is uploaded and the product's launchers run over it from a zeroed state -- window_rows = 0: the
 * stored path, the whole array as one window; window_rows > 0: window after window through the lag-sum and the carry kernel, as a summarising call enqueues them.
 * acov[D][n_values][max_lag + 1], mean and between [D][n_values] (host) in the order of `values`.  Refused before a device is opened, with the product's words: null
 * pointers, a bad shape (non-positive sizes, C % D != 0, window_rows < 0), n_values outside 1 .. PR, an index outside [0, PR), a repeated index, max_lag outside
 * 1 .. 1024, max_lag >= rows, a byte count beyond size_t. */
int amwg_autocovariance_check(const double *draws, int64_t rows, int32_t PR, int64_t C, int32_t D, const int32_t *values, int32_t n_values, int32_t max_lag,
                              int64_t window_rows, double *acov, double *mean, double *between, int32_t device);

/* The host machinery behind sample()'s copy-out (csrc/amwg_run.hip Prefaulter: huge pages, MADV_POPULATE_WRITE, helper threads that touch the destination ahead of
 * the device-to-host copies) on a caller's buffer, cut into n_chunks chunks, with `threads` helpers (0 = the calling thread alone).  Changes no byte.  No GPU. */
int amwg_prefault_selftest(char *buf, size_t bytes, int32_t n_chunks, int32_t threads);

/* BOUND AUDIT build only (libamwg_audit.so = the library's sources compiled with -DAMWG_AUDIT; tools/bound_audit.py, tests/test_gpu_bound_audit.py).  The kernels that
 * decide accept tests from a cheaper value A of log_post and a bound eps (csrc/amwg_kernel.h "certified decisions") evaluate the reference's expression E in EVERY
 * update there as well and record how far apart the two really are:
 *   per_chain [4][chains]: max |A - E| / eps,  max |dA - dE| / eta,  audited decisions,  certified verdicts that contradict exp(dE) > u (must be 0)
 *   hist      [2][64]:     counts of the two ratios by binary exponent, bin b >= 1 holding [2^(b-40), 2^(b-39)) -- bins >= 40 are violated bounds; bin 0: exactly equal
 * reset != 0 clears both afterwards.  amwg_options::test_bound_shift may be negative (down to -60) in this build.  Not in the product library. */
#if defined(AMWG_AUDIT) || defined(AMWG_X_PHASES)
int amwg_audit_fetch(amwg_sampler *s, double *per_chain, uint64_t *hist, int32_t reset);
#endif

#ifdef __cplusplus
}
#endif
#endif
