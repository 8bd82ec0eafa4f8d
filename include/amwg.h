/*
 * amwg.h -- C ABI of libamwg.so: many-chain Adaptive-Metropolis-within-Gibbs on MI355X.
 *
 * This is the drop-in boundary for ONE path of rasmusab/bayes.js:
 *
 *     new mcmc.AmwgSampler(params, log_post, data, options)      mcmc.js:1090-1099 (Sampler ctor :940-966)
 *     sampler.burn(n)                                            mcmc.js:1035-1039
 *     sampler.sample(n)                                          mcmc.js:1005-1030
 *     sampler.thin(k) / .monitor(names)                          mcmc.js:1053-1055 / :1045-1047  (host side; see thin arg)
 *     sampler.start_adaptation() / .stop_adaptation()            mcmc.js:1060-1073
 *     sampler.info()                                             mcmc.js:977-980 -> :906-912 -> :563-571
 *     sampler.state                                              mcmc.js:964
 *
 * Each entry point below names the reference method it replaces.  The reference has no
 * FFI of its own (it is two plain-JS files); the binding a maintainer adds is the N-API
 * shim bayes.js_amd/csrc/amwg_napi.c, described in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * negative AMWG_E* code, with text available from amwg_last_error() (thread-local).  The
 * caller owns every host buffer it passes; the library owns all device memory it allocates.
 * Calls on one sampler must be serialised by the caller (the reference is single-threaded).
 * Many independent chains run per sampler; chain c (global id chain_offset + c) uses the
 * Philox4x32-10 stream keyed by (seed, global id), so results do not depend on how chains
 * are sharded over GPUs.
 */
#ifndef AMWG_H
#define AMWG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMWG_OK 0
#define AMWG_EINVAL (-1)   /* bad argument / unsupported model description */
#define AMWG_EHIP (-2)     /* HIP runtime error (no device, launch failure, out of memory) */
#define AMWG_ESIZE (-3)    /* caller buffer too small */

/* Built-in model registry: the user's `log_post(state, data)` closure (mcmc.js:958-960),
 * restricted to the BASELINE.json model families.  Each is the README pattern
 * (README.md:149-164): priors, then a loop over the data adding one ld.* term per observation. */
enum {
  AMWG_MODEL_NORMAL = 1,      /* mu ~ norm(0,100); sigma ~ unif(0,100); x_i ~ norm(mu, sigma)            (README.md:22-36) */
  AMWG_MODEL_BETA_BERN = 2,   /* theta ~ beta(2,2); x_i ~ bern(theta)                                    (README.md:149-164) */
  AMWG_MODEL_HIER_NORMAL = 3, /* mu ~ norm(0,100); sigma ~ unif(0,100); theta_g ~ norm(mu,10); y_i ~ norm(theta[g_i], sigma) */
  AMWG_MODEL_POIS_GLM = 4     /* beta_k ~ norm(0,10); cp ~ unif(0,N-1); y_i ~ pois(exp(X_i.beta[0:K] + [i>=cp] beta[7])) */
};

enum { AMWG_REAL = 0, AMWG_INT = 1, AMWG_BINARY = 2, AMWG_FIXED = 3 };

/* One named parameter AFTER complete_params() (mcmc.js:357-403), flattened row-major.
 * The order of the array is Object.keys(params) order (mcmc.js:839). */
typedef struct {
  int32_t type;      /* AMWG_REAL | AMWG_INT (Metropolis steppers, mcmc.js:517-553) | AMWG_BINARY (BinaryStepper, mcmc.js:753-767) |
                        AMWG_FIXED: a state entry log_post reads but this sampler never steps -- the rest of the shared state
                        object of a stand-alone stepper (mcmc.js:424-431, 1109-1115: every stepper class takes the whole state and
                        moves one parameter of it).  Fixed entries come after all stepped ones; amwg_create_user only. */
  int32_t len;       /* prod(dim) */
  int32_t top;       /* dim[0]: the only dimension whose visiting order is shuffled (mcmc.js:244-258) */
  int32_t multidim;  /* 0 iff dim equals [1]  (stepper dispatch rule, mcmc.js:846-857) */
  double lower, upper;
} amwg_param_desc;

/* Stepper options of one scalar component, already merged the way AmwgStepper merges them
 * (mcmc.js:869-878) and defaulted (mcmc.js:500-505). */
typedef struct {
  double prop_log_scale;      /* default 0    */
  double max_adaptation;      /* default 0.33 */
  double initial_adaptation;  /* default 1.0  */
  double target_accept_rate;  /* default 0.44 */
  double batch_size;          /* default 50; a JS number: compared and divided as such (mcmc.js:538, 543), so 50.5 or 0 behave as in the reference */
  int32_t is_adapting;        /* default 1    */
} amwg_comp_opt;

/* The `data` argument (mcmc.js:942): host arrays, copied to the device by amwg_create. */
typedef struct {
  int32_t model;     /* AMWG_MODEL_* */
  int32_t n_obs;
  const double *x;   /* NORMAL: x[N]; BETA_BERN: x[N]; HIER_NORMAL: y[N]; POIS_GLM: X[N][K] row-major */
  const double *y;   /* POIS_GLM: counts y[N]; otherwise NULL */
  const int32_t *g;  /* HIER_NORMAL: group index of observation i, 0 <= g_i < G; otherwise NULL */
  int32_t G;         /* HIER_NORMAL: number of groups (= len of the first param) */
  int32_t K;         /* POIS_GLM: number of real columns (7) */
  /* Prior hyper-parameters (the numeric literals of the user's closure):
   *   NORMAL      {m0, s0, a, b}        mu ~ norm(m0,s0); sigma ~ unif(a,b)              default {0,100,0,100}
   *   BETA_BERN   {a, b}                theta ~ beta(a,b)                                default {2,2}
   *   HIER_NORMAL {m0, s0, a, b, tau}   mu ~ norm(m0,s0); sigma ~ unif(a,b); theta_g ~ norm(mu,tau)   default {0,100,0,100,10}
   *   POIS_GLM    {m, s}                beta_k ~ norm(m,s); cp ~ unif(0,N-1)             default {0,10} */
  double hyper[8];
} amwg_model_desc;

#define AMWG_LANES_FASTEST (-1)
#define AMWG_LANES_AUTOTUNE (-2)
typedef struct {
  int64_t chains;          /* independent chains on this sampler (>= 1) */
  uint64_t seed;           /* Philox key */
  uint64_t chain_offset;   /* global id of local chain 0 (multi-GPU sharding) */
  int32_t device;          /* HIP device ordinal */
  int32_t lanes_per_chain; /* lanes that split one chain's observation loop: a power of two 1..1024 (above 64 the chain is one workgroup of
                              several wavefronts, each a replica of the scalar logic; few chains, long data loops), or
                              0 = auto, REFERENCE ORDER FIRST: one lane per chain -- the reference's own sequential `lp += term`, every draw of a
                                  seeded run bit-identical to the reference -- whenever the cost model prices it within 12 % of the cheapest
                                  geometry, else the cheapest (decisions identical to the reference, doubles in the G-lane order);
                              AMWG_LANES_FASTEST (-1) = the cheapest geometry regardless of summation order;
                              AMWG_LANES_AUTOTUNE (-2) = measured instead of modelled: at construction every lane count that fits runs a few
                                  steps on the device (the chain state is saved and restored, tuning leaves no trace) and the fastest is kept --
                                  one lane per chain whenever it measures within 12 % of the fastest.  The pick may differ between machines,
                                  and with it the summation order (decisions stay the reference's); amwg_tuning reports the timings */
  int32_t block_threads;   /* 0 = auto; else multiple of 64, <= 1024.  (Hierarchical family at 64 lanes per chain: its sweep kernel runs in workgroups of
                              at most 512 threads; asking for more selects the kernel that evaluates everything, as full_evaluation = 1 does.) */
  int32_t steps_per_launch;/* 0 = auto: one launch per burn call (up to 65535 steps); a sample call that will be fetched is cut into launches of ~32 MB
                            * of recorded rows, so that the rows of one launch are copied out while the next ones run.  Results never depend on it. */
  int32_t exact_division;  /* 0 = default: result-preserving shortcuts (hoisted-reciprocal division, fast-forward of two-valued sums), bit-identical
                              to the plain schedule and tested against it; 1 = the reference's operation schedule: IEEE '/', term-by-term sums */
  int32_t group_local;     /* 0 = default.  1 = GROUP-LOCAL evaluation of the hierarchical family (AMWG_MODEL_HIER_NORMAL, any labels g_i in [0, G), G <= 64
                              -- since round 4: the library deals the 64 lanes of a chain's wavefront to the groups in aligned power-of-two blocks and
                              lays the data out lane-major, csrc/amwg_gl.h; forces 64 lanes per chain; anything else is AMWG_EINVAL): a proposal for theta_g is decided on the
                              difference of ITS group's terms only -- and the G proposals of a sweep are evaluated in ONE pass over the data, every lane
                              with the proposed mean of its own group -- instead of on two full sums (mcmc.js:524-526 evaluates the whole log_post twice
                              per update).  NOT the reference's operation schedule: the doubles follow the order restated in oracle/amwg_oracle.c (gl_*),
                              bit for bit; accept decisions, adaptation and uniforms consumed equal the reference's on every golden and over the
                              1e10-decision campaign of tools/flip_rate.py (a decision can differ only when the accept uniform falls inside the ~1e-12-relative
                              sliver between the two summation orders).  Opt-in, reported separately by bench.py */
  int32_t full_evaluation; /* How accept tests get their log_post values (mcmc.js:524-528).  All three settings give the same draws; they differ in what is evaluated
                              how often, and in the summation order the rare close call is decided in.
                              0 = default: CERTIFIED DECISIONS where the library has them (csrc/amwg_kernel.h; the kernels amwg_step_kernel_cert / amwg_sweep_kernel_cert):
                              the Normal family at one lane per chain, the Poisson family at 16 lanes, the hierarchical family on a wavefront per chain in its row
                              layout (the proposals of a whole sweep over theta drawn ahead -- in stream order: nothing an update draws depends on an earlier decision --
                              and all its accept tests decided at once).  The test is decided from a cheaper value of log_post with a rigorous bound on its distance from
                              the reference's expression summed in the REFERENCE's order (one running sum); a uniform inside the bound (1e-7 .. 1e-6 of the updates)
                              gets that expression itself.  Decisions, draws and the cached log_post are the reference's at every one of those lane counts
                              (amwg_summation_order() == 1).  Every other geometry, and translated closures: the expression in every update, summed in lane order; a
                              closure with a row plan (amwg_user_model::rows_*) keeps the per-lane sums an update cannot have changed and prepares a sweep's
                              sums in one pass.
                              1 = every evaluation is the expression, with its full pass over the data, summed in the geometry's lane order (amwg_step_kernel).
                              2 = the hierarchical family's row layout without certified decisions (amwg_sweep_kernel): per-lane sums kept while an update cannot
                              have changed them (csrc/amwg_models.h lane_sum_rows), a sweep's proposed sums formed in one pass (prefetch_rows), its accept tests
                              one after the other from butterflies of those sums -- bit for bit what 1 computes.  A verification switch */
  int32_t test_bound_shift; /* TEST HOOK, 0 in production: the rounding bounds of the certified decisions (csrc/amwg_kernel.h: accept tests decided from a cheaper value
                               of log_post, from the local differences of a sweep) are multiplied by 2^shift, 0..40.  A wider bound sends more
                               updates down the path that evaluates the reference's expression; the results must not change by a bit (tests run 0 against 14 and 40) */
  int32_t sufficient_statistics; /* OPT-IN, 0 by default; the Normal family at one lane per chain only (AMWG_EINVAL elsewhere).  A THIRD TIER next to full_evaluation = 1
                               (the expression in every update, 8 operations per observation) and the default (the certified pass, 2 per observation): the cheaper
                               value of log_post the accept test is decided from (csrc/amwg_kernel.h "certified decisions") needs NO pass over the data for this
                               likelihood -- sum (x_i - mu)^2 = SS + n (xbar - mu)^2, with xbar (a double-double) and SS formed once on the host in quad precision --, so
                               an update costs the stepper alone, whatever n is.  Same bound, same fallback to the reference's expression, hence the same draws bit for
                               bit (tests/test_gpu_parity.py; tools/bound_audit.py audits it); what changes is that mcmc.js:524-526's pass over the observations is
                               made only where a uniform falls inside the bound.  Reported separately by bench.py, never as the headline */
} amwg_options;

typedef struct amwg_sampler amwg_sampler;

/* Replaces `new mcmc.AmwgSampler(params, log_post, data, options)` (mcmc.js:1090, 940-966).
 * init: P = sum(len) initial values (completed params' init, mcmc.js:954-957), the same for every chain. */
int amwg_create(const amwg_model_desc *model, const amwg_param_desc *params, int32_t n_params, const double *init,
                const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out);

/* MANY DATASETS IN ONE SAMPLER: the same built-in model on n_datasets datasets, a posterior per dataset, one launch (what the reference's users loop over
 * in JavaScript: one A/B test per segment, one fit per bootstrap replicate, per sensor, per simulated dataset of a calibration study).
 * options->chains is the TOTAL and must be a multiple of n_datasets; with cpd = chains / n_datasets, dataset d owns the local chains [d * cpd, (d + 1) * cpd)
 * and everywhere else chain c means dataset c / cpd: amwg_burn, amwg_sample*, amwg_fetch_draws*, amwg_get/set_state, amwg_info, amwg_chain_diag and the
 * gathers of draws work unchanged.  Chain c draws from the stream of global id chain_offset + c as ever, so dataset d's chains are bit for bit the chains
 * of an amwg_create sampler on models[d] with chain_offset + d * cpd at the same lanes_per_chain and block_threads -- and a shard of a larger job is a dataset
 * sampler over a contiguous slice of the datasets with chain_offset = first dataset * cpd.
 * A workgroup serves one dataset: the launch geometry is chosen among those whose chains per workgroup (block_threads / lanes_per_chain; 1 for a chain on
 * several wavefronts) divide cpd -- small cpd means more lanes per chain or smaller workgroups --, and a fixed lanes_per_chain / block_threads pair that does
 * not divide cpd is AMWG_EINVAL.  The kernel is the twin of the ordinary one (amwg_kernel_name: "amwg_step_kernel_ds<...>", "amwg_step_kernel_cert_ds<...>").
 * All descriptions must agree in model, n_obs, K, G and hyper: RAGGED DATASETS ARE NOT SUPPORTED BY THIS ENTRY -- a caller who relies on it to catch a wrong
 * slice keeps that check; datasets of unequal sizes go through amwg_create_datasets_ragged below.  Refused with AMWG_EINVAL, before a device is opened:
 * AMWG_MODEL_HIER_NORMAL (its launch plan depends on properties of the group labels), options->group_local, AMWG_LANES_AUTOTUNE.  Supported:
 * AMWG_MODEL_NORMAL, AMWG_MODEL_BETA_BERN, AMWG_MODEL_POIS_GLM with every other option.  n_datasets == 1 is amwg_create(models, ...).
 * The pooled summaries (amwg_last_sample_moments / _diagnostics / _quantiles, amwg_group_moments / _diagnostics / _quantiles, amwg_comm_moments) return
 * AMWG_EINVAL on such a sampler -- a pooled mean over unrelated posteriors is a bug the caller did not mean to write --; the per-dataset ones are below.
 * Per-dataset quantiles are a radix select over each dataset's draws where they lie (amwg_last_sample_dataset_quantiles). */
int amwg_create_datasets(const amwg_model_desc *models, int32_t n_datasets, const amwg_param_desc *params, int32_t n_params, const double *init,
                         const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out);
/* RAGGED DATASETS: amwg_create_datasets with models[d].n_obs free to differ between datasets (one A/B test per segment, one fit per sensor: real segments are
 * never of one size, and a likelihood cannot be padded).  Everything else in the contract above holds: the descriptions still agree in model, K, G and hyper,
 * the same three refusals apply, chains % n_datasets == 0, n_datasets == 1 is amwg_create; each dataset's n_obs passes the check amwg_create makes for an
 * ordinary sampler of the family.  Equal sizes are the special case: both entries build the same sampler then.  The parity statement is unchanged -- dataset
 * d's chains are bit for bit those of an amwg_create sampler on models[d] with the same params, chain_offset + d * cpd, lanes_per_chain and block_threads.
 * `params` is ONE array for the whole sampler: the bounds of a parameter are shared by all datasets (the Poisson family's change point cp has one `upper`;
 * its prior ld.unif(cp, 0, n_d - 1) is per dataset).  Per-dataset parameter bounds are not supported.
 * One launch geometry serves all datasets: its LDS is that of the dataset that needs most (so small datasets run at the occupancy the largest allows), its
 * lane count is priced with the mean size.  A largest dataset that fits no admissible geometry is AMWG_EINVAL, with a message that names it.
 * Workgroups are dispatched in the caller's order of the datasets.  PASS THE LARGEST DATASETS FIRST when the launch has more workgroups than the device holds
 * at once: measured at 2048 datasets x 256 chains, sizes 10^2..10^4, largest first took 1.06 times the time of equal sizes with the same
 * sum, smallest first 1.17, a shuffled order 1.53.  With one workgroup per CU or fewer the order does not matter: the launch lasts as long as the largest dataset. */
int amwg_create_datasets_ragged(const amwg_model_desc *models, int32_t n_datasets, const amwg_param_desc *params, int32_t n_params, const double *init,
                                const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out);
/* Datasets of a sampler: 1 for every sampler not made by amwg_create_datasets / amwg_create_datasets_ragged / amwg_create_user_datasets with n_datasets > 1. */
int amwg_num_datasets(const amwg_sampler *s);
/* n_obs of every dataset, n_obs[amwg_num_datasets(s)] (an ordinary sampler: its one size; a translated closure, whose arrays carry their own lengths: 0, one per dataset). */
int amwg_dataset_n_obs(const amwg_sampler *s, int32_t *n_obs);
/* amwg_last_sample_moments per dataset, computed on the device over the dataset's chains x kept draws: mean[D][P], sd[D][P]. */
int amwg_last_sample_dataset_moments(amwg_sampler *s, double *mean, double *sd);
/* amwg_last_sample_diagnostics per dataset (the same definitions over the dataset's chains; one workgroup per recorded value and dataset):
 * rhat[D][P], ess[D][P].  Needs >= 2 chains per dataset and >= 4 kept draws. */
int amwg_last_sample_dataset_diagnostics(amwg_sampler *s, double *rhat, double *ess);
/* amwg_last_sample_quantiles per dataset: out[D][P + derived][n_probs].  R's default (type 7) rule over the dataset's chains x kept draws: h = (n - 1) q,
 * x[floor h] + (h - floor h) (x[floor h + 1] - x[floor h]); a q outside [0, 1] or NaN gives NaN.  Nothing is gathered or sorted: one workgroup per (recorded
 * value, dataset) selects the order statistics by radix, most significant digit first, and the result comes to the host in one copy.  Any n_probs >= 1 (the
 * kernel runs once per 24 probabilities).  Works on an ordinary sampler too (D = 1: the pooled call's result).  AMWG_EINVAL: a null argument or n_probs < 1
 * (before any device call), no sample() yet, more than 2^31 - 1 values per dataset and component, more than 65535 datasets. */
int amwg_last_sample_dataset_quantiles(amwg_sampler *s, const double *probs, int32_t n_probs, double *out);
/* HIGHEST-DENSITY INTERVALS per dataset: out[D][P + derived][n_probs][2], (lower, upper) per probability.  amwg_last_sample_dataset_quantiles at (0.025, 0.975)
 * is the equal-tailed interval; for a skewed posterior the shortest interval of the same content is the one to report.
 * THE RULE applies per dataset d, recorded value v (the P parameters plus the derived quantities) and probability p.  The N = rows * (C / D) draws of (d, v) in the
 * last stored sample() are ordered by the key order of the doubles: the order of the doubles, with -0 before +0.  Write the sorted draws as x_(0) <= ... <= x_(N-1).
 *   g = floor(p * (double)N), one IEEE fp64 multiply then floor, clamped to [1, N - 1].  Set k = N - g.
 *   w_i = x_(i+g) - x_(i) in fp64, for i = 0 ... k - 1.
 *   i* is the smallest i whose w_i is minimal, with widths compared as doubles.
 *   The result is (x_(i*), x_(i*+g)): the shortest interval spanning g + 1 sorted draws (the Kruschke / ArviZ rule).  Its bytes are those of two draws.
 *   A p that is NaN or outside the open interval (0, 1) gives (NaN, NaN) for that probability (as amwg_last_sample_dataset_quantiles does with a bad q).
 *   A NaN or +-inf anywhere among the N draws of (d, v) gives (NaN, NaN) for every probability of that (d, v), and nowhere else (the autocovariance's convention).
 * (0.29 * 100 floors to 28, not 29: the rule is what the fp64 product says.)
 * The draws do not leave the device and no slice is gathered or sorted whole: per probability a radix select finds t_lo = x_(k-1) and t_hi = x_(g) where the draws
 * lie, the k draws up to t_lo and the k draws from t_hi go into scratch, the two tails are sorted (in LDS where a tail fits, else by global passes) and the k
 * widths are scanned for the first smallest.  Scratch is 2 x k keys per (d, v), rounded up to a power of two, allocated per call on the sampler's device and freed
 * before the call returns; the (d, v) go in batches under a budget of 256 MiB, and a single (d, v) whose two tails exceed the budget runs alone.  Any p in
 * (0, 1) is served; AS p -> 0 THE TAILS APPROACH THE WHOLE SLICE, twice over: the call is meant for the probabilities people report (0.5 .. 0.99).
 * Works on an ordinary sampler too (D = 1).  AMWG_EINVAL: a null argument or n_probs < 1 (before any device call), no sample() yet, after a summarising call,
 * fewer than 2 values per dataset and value, and the shape limits of amwg_last_sample_dataset_quantiles.  A failed scratch allocation is AMWG_EHIP. */
int amwg_last_sample_dataset_hpd(amwg_sampler *s, const double *probs, int32_t n_probs, double *out);   /* out[D][P + derived][n_probs][2] */
/* WAIC per dataset (Watanabe; Vehtari, Gelman & Gabry 2017): how well the model predicts each dataset, from the stored draws, on the device.
 *   summary[D][4] = elpd_waic, se, p_waic, lppd;  high[D] (or NULL) = the number of observations with p_i > 0.4, the usual warning that WAIC is unreliable there;
 *   pointwise (NULL, or [D][n_max][2] = lppd_i, p_i; NaN beyond n_d), n_max the largest value amwg_dataset_n_obs reports.
 * THE RULE applies per dataset d with n_d observations; the S = rows * (C / D) draws of d in the last stored sample() are numbered s = row * (C / D) + chain.
 *   l_si is the double the reference's expression adds for observation i under draw s, the family's own term, BIT FOR BIT:
 *     AMWG_MODEL_NORMAL       ld_norm(x_i, mu, sigma)
 *     AMWG_MODEL_BETA_BERN    ld_bern(x_i, theta)              (-inf for an x_i that is neither 0 nor 1)
 *     AMWG_MODEL_HIER_NORMAL  ld_norm(y_i, theta[g_i], sigma)
 *     AMWG_MODEL_POIS_GLM     log(lambda) * y_i - lambda - lfactorial(y_i), lambda = exp(eta), eta = X[i][0] * beta[0] + ... + X[i][6] * beta[6] by products and
 *                             additions in that order (no fused operation), + beta[7] from i >= cp on; exp and log are V8's, lfactorial(y_i) the stored one
 *     (the quotient of ld_norm is IEEE's; where the step kernels form it by the reciprocal of csrc/amwg_div.h, which reproduces it, so does this call.)  Priors are
 *     not part of l.
 *   lppd_i = m_i + log(sum_s exp(l_si - m_i)) - log S, with m_i = max_s l_si.
 *   p_i    = sum_s (l_si - mean_i)^2 / (S - 1).
 *   These two ACCUMULATIONS ARE NOT FIXED TO THE BIT; they are deterministic (no floating-point atomics: a fixed split of the draws, merged in a fixed order: (m, sum)
 *   by rescaling, (count, mean, M2) by Chan's formula), and a dataset's result bytes depend only on its own draws, its own data and (rows, C / D) -- not on D, the other
 *   datasets or the scratch budget.  The exponential is exp_v8 (V8's: fdlibm's, below 1 ulp); the logarithm log_v8.  With u = 2^-53 and E = 8 (S + 16) u:
 *     |lppd_i - exact| <= E + 4 u |exact|,     |p_i - exact| <= E sqrt(V (V + mean_i^2)) + (E max_s |l_si|)^2, V the exact p_i
 *   (a sum of S non-negative terms of relative error 2 u is within (S + 3) u in any order; the variance term is Chan, Golub & LeVeque's bound for updating and
 *   two-pass schemes; the factor 8 covers any merge tree).  tests/README.waic.md has the derivation and the largest ratio observed.
 *   NON-FINITE VALUES: if any l_si of (d, i) is NaN or +-inf, lppd_i and p_i are NaN for that (d, i) only; the totals of d are then NaN, and no other dataset's are
 *   (the convention of the autocovariance and of the HPD).  Terms whose squared distance from their mean overflows (beyond 1e154) count as non-finite.
 *   THE FINISH runs on the host inside the library from the pointwise pairs, in index order, so its bytes are a function of the pointwise bytes:
 *     elpd_i = lppd_i - p_i;  lppd, p_waic and elpd_waic are running sums from 0.0 over i = 0 ... n_d - 1;
 *     se = sqrt(n_d * sum_i (elpd_i - elpd_waic / n_d)^2 / (n_d - 1)), the sum again from 0.0 in index order; NaN for n_d = 1;  high[d] counts p_i > 0.4.
 * Works on ordinary samplers (D = 1), dataset samplers and ragged dataset samplers; the hierarchical family on an ordinary sampler (amwg_create_datasets refuses it).
 * The Bernoulli family's pairs take two values per dataset (x_i = 1, x_i = 0): those two are computed, not n_d.
 * AMWG_EINVAL with a message that names the call: a null s or summary (before any device call); no sample() yet; after a summarising call (the message names
 * amwg_sample_summarize); fewer than 2 draws per dataset; a translated closure (amwg_create_user*): "the pointwise terms of a closure are not known to the library;
 * built-in families only"; a group_local sampler (its observations lie as a lane-major tile).  Scratch -- the partials of the split, 32 bytes per observation and
 * run of draws -- is allocated per call on the sampler's device and freed before the call returns; the datasets go in batches under a budget of 256 MiB (a dataset
 * beyond it runs alone).  A failed allocation is AMWG_EHIP.
 * A TRANSLATED CLOSURE WHOSE POINTWISE TEXT IS SET (amwg_set_pointwise below) is served like a family, with [D][kTermN] where the families have n_d; every other
 * rule, bound, refusal and scratch budget is as stated.  THE OBSERVATIONS OF A CLOSURE are the iterations of its FINAL LOOP -- the last statement before `return acc`,
 * a counted loop at the top level of log_post that ends in `acc += term` --, and l_si is the double that statement adds in iteration i under draw s: V8's value, bit
 * for bit, formed by the same generated expressions the step kernel evaluates.  Everything before the loop counts as prior and is no part of l: a closure with
 * likelihood terms outside its final loop gets the WAIC of the final loop's observations only.  The draws of a run are staged kStage = 256 at a time wherever 256 of
 * the closure's Draw (what an evaluation keeps of a draw) fit in 48 KiB of LDS, otherwise the largest multiple of 4 that fits -- a function of sizeof(Draw) alone, so
 * a dataset's bytes depend on its own draws and data, on (rows, C / D) and on the closure's text; a Draw of which fewer than 4 fit is refused when the text is compiled.
 * OUT OF SCOPE: WAIC after amwg_sample_summarize (per-observation accumulators could be folded; not built), a public pointwise log-likelihood matrix,
 * likelihood terms of a closure outside its final loop, a pooled WAIC across devices (no amwg_group_* / amwg_comm_* twin). */
int amwg_last_sample_dataset_waic(amwg_sampler *s, double *summary /* [D][4]: elpd_waic, se, p_waic, lppd */, int32_t *high /* [D] or NULL */,
                                  double *pointwise /* NULL or [D][n_max][2]: lppd_i, p_i; NaN beyond n_d */);
/* PSIS-LOO per dataset (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024): leave-one-out predictive accuracy by Pareto-smoothed importance
 * sampling from the stored draws, on the device -- what to use where WAIC's high[d] is not zero.
 *   summary[D][4] = elpd_loo, se, p_loo, lppd;  high[D] (or NULL) = the number of observations with khat_i > 0.7, where the estimate is unreliable;
 *   pointwise (NULL, or [D][n_max][3] = elpd_loo_i, lppd_i, khat_i; NaN beyond n_d).
 * THE RULE applies per dataset d and observation i; S and the terms l_s = l_si are those of amwg_last_sample_dataset_waic, the same doubles.
 *   Sorted ascending by the key order of doubles (-0 before +0): a_0 <= ... <= a_{S-1}; a small term is a large importance ratio.
 *   TAIL LENGTH M = min(floor(S / 5), m3), m3 the smallest integer with m3^2 >= 9 S (integer arithmetic).
 *   lppd_i is WAIC's, the same bytes.
 *   RAW ROUTE, if M < 5: khat_i = +inf, elpd_loo_i = a_0 + log S - log sum_t exp(a_0 - a_t).
 *   SMOOTHED ROUTE otherwise: ec = exp_v8(a_0 - a_M); THE EXCESSES ARE PINNED TO THE BIT: x_r = exp_v8(a_0 - a_{M-r}) - ec for r = 1 ... M, ascending.
 *   FIT (Zhang & Stephens 2009, as the loo package's gpdfit): mm = 30 + floor(sqrt(M)); x* = x_{floor(M / 4 + 0.5)};
 *     theta_j = 1 / x_M + (1 - sqrt(mm / (j - 0.5))) / (3 x*) for j = 1 ... mm;  k_j = mean_r log1p(-theta_j x_r);  L_j = M (log(-theta_j / k_j) - k_j - 1);
 *     w_j = 1 / sum_i exp(L_i - L_j);  theta^ = sum_j theta_j w_j;  k' = mean_r log1p(-theta^ x_r);  sigma = -k' / theta^;  khat_i = (M k' + 5) / (M + 10).
 *     If x* <= 0, or x_M <= 0, or khat is not finite: the raw route, khat_i = +inf (the loo package's behaviour for a degenerate tail).
 *   SMOOTHING: p_r = (r - 0.5) / M;  q_r = sigma expm1(-khat log1p(-p_r)) / khat, and -sigma log1p(-p_r) when khat == 0;  lw~_r = min(log(q_r + ec), 0), paired by
 *     rank with the raw lw_r = a_0 - a_{M-r}.
 *   elpd_loo_i = a_0 + log((S - M) + sum_r exp(lw~_r - lw_r)) - log(B + sum_r exp(lw~_r)), with B = sum_{t >= M} exp(a_0 - a_t).
 *   Only the sorted multiset of the M + 1 smallest terms and B enter: no draw indices, and ties at the cutoff cannot change the result.
 *   exp, log, log1p and expm1 are V8's (exp_v8, log_v8, log1p_v8, expm1_v8).  THE ACCUMULATIONS ARE NOT PINNED TO THE BIT; they are deterministic: no floating-point
 *   atomics (the only atomics count and place terms: integers), a split of the draws that is a function of (S, n_d) alone merged in a fixed order, a fixed order of
 *   every sum over the tail; a dataset's result bytes depend only on its own draws, its own data and (rows, C / D) -- not on D, the other datasets or the scratch budget.
 *   With u = 2^-53, E = 8 (S + 16) u and E_k = M (M + mm) u (1 + |khat|):
 *     |khat_i - exact| <= E_k,     |elpd_loo_i - exact| <= E (1 + |exact|) + 4 ln(2 M) E_k
 *   (measured, not proven: tests/README.loo.md has the measurement and the largest ratios observed).
 *   NON-FINITE VALUES: if any l_s of (d, i) is NaN or +-inf, elpd_loo_i, lppd_i and khat_i are NaN for that (d, i) only; the totals of d are then NaN, and no other
 *   dataset's are.  Where WAIC's lppd_i is NaN for terms beyond 1e154 (its rule), so is the triple.
 *   THE FINISH runs on the host inside the library from the pointwise triples, in index order, running sums from 0.0:
 *     elpd_loo = sum_i elpd_loo_i;  lppd = sum_i lppd_i;  p_loo = lppd - elpd_loo;
 *     se = sqrt(n_d * sum_i (elpd_loo_i - elpd_loo / n_d)^2 / (n_d - 1)); NaN for n_d = 1;  high[d] counts khat_i > 0.7, +inf included.
 * The samplers served are WAIC's; the Bernoulli family's two values (x_i = 1, x_i = 0) are computed and expanded, as there.
 * AMWG_EINVAL with a message that names the call: a null s or summary (before any device call); no sample() yet; after a summarising call (the message names
 * amwg_sample_summarize); fewer than 2 draws per dataset; a translated closure: "the pointwise terms of a closure are not known to the library; built-in families
 * only"; a group_local sampler; and, from the shape alone, M + 1 > 8192 (about 7.4e6 draws per dataset): one workgroup sorts and fits a tail in LDS, 8192 doubles (64 KB) of it at most.
 * Scratch -- per observation the tail (M + 1 padded to a power of two, at least 64 doubles), 512 bytes of counters, a double per run of draws -- is allocated per call
 * and freed before the call returns; the datasets go in batches under a budget of 256 MiB (a dataset beyond it runs alone).  A failed allocation is AMWG_EHIP.
 * OUT OF SCOPE: LOO after amwg_sample_summarize, moment matching or exact refits for observations of high khat, a relative-efficiency (r_eff) correction of the tail
 * length, likelihood terms of a closure outside its final loop, a pooled LOO across devices, tails beyond the LDS cap.
 * A translated closure whose pointwise text is set is served as by amwg_last_sample_dataset_waic: the same observations, the same doubles, the same kStage rule. */
int amwg_last_sample_dataset_loo(amwg_sampler *s, double *summary /* [D][4]: elpd_loo, se, p_loo, lppd */, int32_t *high /* [D] or NULL: observations with khat_i > 0.7 */,
                                 double *pointwise /* NULL or [D][n_max][3]: elpd_loo_i, lppd_i, khat_i; NaN beyond n_d */);

/* A user-written `log_post(state, data)` closure (mcmc.js:958-960) translated to HIP by
 * bayes.js_amd/translate.js.  `source` defines `struct amwg::UserModel` (interface: csrc/amwg_kernel.h,
 * "translated closure"); amwg_create_user compiles it with hiprtc for the device's gfx target,
 * together with the same step kernel the built-in models use.  Arrays are the numeric arrays of
 * the closure's `data` argument that the body reads, flattened row-major. */
enum { AMWG_F64 = 0, AMWG_U8 = 1, AMWG_I32 = 2 };
typedef struct {
  const char *source;            /* HIP C++ text (NUL-terminated) */
  int32_t n_arrays;              /* any number (the first 16 pointers travel in the kernel arguments, the rest in a device table) */
  const double *const *arrays;   /* host pointers; copied to the device by amwg_create_user */
  const int64_t *array_len;      /* elements per array */
  const int32_t *array_type;     /* device storage per array: AMWG_F64 | AMWG_U8 | AMWG_I32 (values must be exactly representable);
                                    NULL = all AMWG_F64.  Host arrays are always doubles. */
  int32_t n_derived;             /* derived quantities (`state.key = expr`, mcmc.js:961-963, 990-995) recorded after the P components */
  int32_t lds_bytes;             /* bytes of data the generated stage() keeps in LDS (lanes_per_chain > 1) */
  int32_t lds_bytes_one_lane;    /* the same for lanes_per_chain == 1 (the generated code may stage other arrays then); 0 = same as lds_bytes */
  int32_t parallel;              /* 1 = the body has lane-split loops, lanes_per_chain > 1 is allowed */
  int32_t max_threads;           /* workgroup-size cap the translator suggests (0 = 1024) */
  double work_per_eval;          /* rough instruction count of one log_post evaluation (0 = unknown); only steers lanes_per_chain */
  double work_one_lane;          /* the same with ONE lane per chain, when the generated code then fast-forwards a two-valued sum (0 = no) */
  /* Row plan (csrc/amwg_rows.h): the closure ENDS in `lp += ld.norm(y[i], state.theta[g[i]], sd)` over all rows_n_obs observations, labels that repeat
   * with a stride of 64 and rows_groups <= 64 group means.  With 64 lanes per chain the library then lays the observations out in rows (one per lane)
   * and re-forms only the per-lane sums an update can have changed -- the same bits as evaluating everything (amwg_options::full_evaluation = 1
   * switches it off).  rows_sweep: the translator PROVED that a lane's sum depends on one entry of theta only, which allows the proposals of a whole
   * sweep over theta to be evaluated in one pass (UserModel::kRowSweep in the source says the same).  0 / 0 / 0 = no row plan.
   * The struct carries no size or version field: amwg_create_user therefore honours these three only as far as the GENERATED SOURCE states the same
   * (kRowN, kRowGroups, kRowSweep) and refuses a mismatch -- a caller built against an older, shorter struct cannot switch a layout on that the source has
   * no code for.  Everything the translator added since is read from the source alone: kRowCert (certified decisions in the row layout: amwg_user_sweep_cert),
   * kCertifiedTail / kTailN (certified decisions for a closure ending in a constant-mean normal loop: amwg_user_step_cert at one lane per chain), kPoisTail / kTailN
   * and kLogitTail / kTailN (the same for a closure ending in a log-link Poisson loop or in a logistic-regression loop: amwg_user_step_cert at 16 lanes per chain),
   * kTailPerDataset / kTailConsts (those two tails read the data-dependent constants of their bound -- sum y, sum lfactorial(y) and the column maxima of the linear
   * predictor; sum |y| -- from the f64 array kTailConsts of the model, `#tail:consts`, instead of from literals of the text: translate.js tail_consts_array). */
  int32_t rows_n_obs, rows_groups, rows_sweep;
} amwg_user_model;

/* Replaces `new mcmc.AmwgSampler(params, log_post, data, options)` for an arbitrary (translated) closure. */
int amwg_create_user(const amwg_user_model *model, const amwg_param_desc *params, int32_t n_params, const double *init,
                     const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out);

/* MANY DATASETS IN ONE SAMPLER FOR A TRANSLATED CLOSURE: amwg_create_datasets for amwg_create_user.  models[0..n_datasets) describe the SAME closure on n_datasets
 * datasets OF EQUAL SHAPE -- every array has the same length and storage type in every dataset, the values are free -- and carry the SAME source: bayes.js_amd/translate.js
 * translate_datasets translates every dataset under the union of what the values decide (the widest storage type, the hull of the index ranges, scalar fields that differ
 * read from one-element arrays) and insists that all texts come out identical.  Chains, cpd, the geometries that serve whole datasets, the pooled summaries' refusal and
 * the per-dataset summaries are those of amwg_create_datasets above; derived quantities are recorded and summarised per dataset like the components.  Dataset d's chains are
 * bit for bit the chains of an amwg_create_user sampler compiled from the same source on models[d]'s arrays with chain_offset + d * cpd at the same lanes_per_chain and
 * block_threads.  The kernel is the twin of the ordinary one (amwg_kernel_name: "amwg_user_step_ds", "amwg_user_step_cert_ds"; csrc/amwg_user_dataset.h): a workgroup takes
 * its dataset's arrays from a device table of pointers [n_datasets][n_arrays]; per array the copies lie back to back in one allocation, each on a 256-byte boundary.
 * n_datasets == 1 is amwg_create_user(models, ...).  amwg_dataset_n_obs fills n_datasets zeros (a closure's arrays carry their own lengths).
 * Refused with AMWG_EINVAL before a device is opened, with a message that names the dataset and the field: a null argument, n_datasets < 1, chains % n_datasets != 0,
 * models[d].source not string-equal to models[0].source, a difference in n_arrays, any array_len or array_type, n_derived, lds_bytes, lds_bytes_one_lane, parallel,
 * max_threads or rows_*; a source with a row plan (kRowN) -- its layout is formed from one dataset's labels --; a source with a certified Poisson / logistic tail
 * (kPoisTail / kLogitTail) whose bound holds LITERALS, i.e. sums over one dataset's values; AMWG_LANES_AUTOTUNE; sufficient_statistics.
 * A Poisson / logistic tail IS accepted when the source states kTailPerDataset = true: the constants of its bound are then the slots of models[d]'s own array
 * kTailConsts (the last one, `#tail:consts`), which translate_datasets forms from dataset d's values by the code that forms the literals of an ordinary translation --
 * the library takes them as data and checks nothing about them.  Such a sampler runs "amwg_user_step_cert_ds" at 16 lanes per chain (block_threads / 16 must divide cpd;
 * lanes_per_chain = 0 finds such a geometry where it is priced cheapest) with amwg_summation_order 1: every dataset's chains are the reference's, bit for bit.
 * amwg_create_user takes a marked source too: the constants are its one dataset's array.
 * NOT SUPPORTED: ragged closure datasets (the generated loops and LDS copies carry the lengths as constants), autotune, the stand-alone steppers. */
int amwg_create_user_datasets(const amwg_user_model *models, int32_t n_datasets, const amwg_param_desc *params, int32_t n_params, const double *init,
                              const amwg_comp_opt *comp_opts, const amwg_options *options, amwg_sampler **out);

/* hiprtc compilation of a translated closure without a device (build-time / CPU-test check).
 * arch e.g. "gfx950".  On failure returns AMWG_EINVAL and amwg_last_error() carries the compiler log. */
/* THE POINTWISE TERMS OF A TRANSLATED CLOSURE (translate.js, options.pointwise: `struct amwg::UserTerms`, a second text beside `source`).  amwg_set_pointwise stores the
 * text on an amwg_create_user* sampler -- any other sampler: AMWG_EINVAL, a built-in family needs no text --; it is compiled (hiprtc; the options and the on-disk cache
 * of amwg_compile_user) at the first amwg_last_sample_dataset_waic / _loo call, where a text that does not compile gives AMWG_EINVAL with the hiprtc log.
 * amwg_pointwise_n_obs: kTermN of the stored text, 0 without one (amwg_dataset_n_obs keeps reporting zeros for closures).  amwg_compile_pointwise: the device-less
 * twin of amwg_compile_user -- compiles the program of (source, terms_source) for `arch`, *code_bytes (may be NULL) the size of the code object. */
int amwg_set_pointwise(amwg_sampler *s, const char *terms_source);
int64_t amwg_pointwise_n_obs(const amwg_sampler *s);
int amwg_compile_pointwise(const char *source, const char *terms_source, const char *arch, size_t *code_bytes);
int amwg_compile_user(const char *source, int32_t lanes_per_chain, int32_t block_threads, const char *arch, size_t *code_bytes);
/* The same with the dataset twins compiled in (amwg_user_step_ds, amwg_user_step_cert_ds): the code object of an amwg_create_user_datasets sampler. */
int amwg_compile_user_datasets(const char *source, int32_t lanes_per_chain, int32_t block_threads, const char *arch, size_t *code_bytes);

/* Compiled closures are kept on disk ($AMWG_CACHE_DIR, else $XDG_CACHE_HOME/amwg, else $HOME/.cache/amwg; AMWG_CACHE_DIR="" disables), keyed by
 * program text + kernel headers + compile options + target + hiprtc version: a second process constructing the same sampler loads the
 * code object instead of compiling it (README.md:41-42: a script that is simply run again).  This process's hits / misses so far; `dir`
 * (may be null) receives the directory in use, empty when the cache is off. */
int amwg_code_cache_stats(int64_t *hits, int64_t *misses, char *dir, size_t dir_capacity);

/* Replaces sampler.burn(n) (mcmc.js:1035-1039).  amwg_burn blocks until the steps are done;
 * amwg_burn_async only enqueues them on the sampler's stream (pair with amwg_sync), which is how
 * one host thread keeps several GPUs busy. */
int amwg_burn(amwg_sampler *s, int64_t n);
int amwg_burn_async(amwg_sampler *s, int64_t n);

/* Replaces sampler.sample(n) with thinning interval `thin` (mcmc.js:1005-1030, 1053-1055):
 * draw k is the state BEFORE step k*thin.  out_draws (host) receives ceil(n/thin) * P * chains
 * doubles laid out [draw][component][chain]; out_bytes is its capacity.  (P here and below means
 * amwg_num_recorded(): the parameters followed by a translated closure's derived quantities.) */
int amwg_sample(amwg_sampler *s, int64_t n, int64_t thin, double *out_draws, size_t out_bytes);

/* Two-phase form of amwg_sample for multi-GPU hosts: enqueue the steps into a library-owned
 * device buffer, then (after doing the same on the other devices) copy the draws out. */
int amwg_sample_async(amwg_sampler *s, int64_t n, int64_t thin);
int amwg_fetch_draws(amwg_sampler *s, double *out_draws, size_t out_bytes);
/* The same, delivered the way sampler.sample() returns it (mcmc.js:1009-1029: one array per monitored parameter): slice k receives the
 * recorded values base[k] .. base[k] + len[k] - 1 of every kept draw, laid out [draw][len[k]][chain], into out[k] (capacity out_bytes[k]).
 * Both forms copy the rows of each launch as soon as that launch has finished, while the later launches of the call still run.  The output
 * buffers must be writable and must not be touched by another thread during the call: their pages are made resident ahead of the copy by
 * rewriting one byte per page with its own value. */
int amwg_fetch_draws_slices(amwg_sampler *s, int32_t n_slices, const int32_t *base, const int32_t *len, double *const *out, const size_t *out_bytes);

/* Same, but the destination is DEVICE memory owned by the caller (e.g. a buffer that is then
 * gathered across GPUs with RCCL); no host copy is made.  Asynchronous on the sampler's stream
 * until amwg_sync(). */
int amwg_sample_device(amwg_sampler *s, int64_t n, int64_t thin, double *out_draws_dev, size_t out_bytes);

/* SUMMARIES WITHOUT STORED DRAWS.  Runs the n steps of amwg_sample_async(s, n, thin) -- the same draws, Philox stream, adaptation and launches cut by
 * steps_per_launch and the 65 535-step limit: afterwards the chains' state, amwg_info and amwg_chain_diag are those of that call, every byte -- but keeps no draw:
 * the recorded rows go into a device window of window_rows rows, and each time the window is full, and again at the end of the call, a fold kernel adds its rows to
 * per-chain accumulators (per recorded value and chain the Welford pair (mean, M2) of the first half of the kept draws, of the second half and of the whole chain:
 * 6 x 8 bytes) and the window is reused.  Everything is enqueued on the sampler's stream, without a host synchronisation between windows; a launch never records past
 * the end of the window (its steps are capped).  window_rows = 0: the rows that fit into 64 MiB; never more rows than the call keeps, never fewer than 1.  The device
 * memory of a call is therefore the window and the accumulators, whatever n -- amwg_sample_async needs ceil(n/thin) rows.
 * Afterwards amwg_last_sample_moments, amwg_last_sample_diagnostics, amwg_last_sample_dataset_moments and amwg_last_sample_dataset_diagnostics answer from the
 * accumulators: the halves are accumulated by the recurrence of the stored path in the same row order, so split-R-hat and ESS equal those of the stored run BIT FOR BIT
 * (same refusals: < 4 kept draws, < 2 chains); mean and sd come from the whole-chain pairs (mean = sum m_c / chains, SS = sum M2_c + kept * sum (m_c - mean)^2) and
 * agree with the stored path's to rounding.  Calls that need the draws themselves -- amwg_last_sample_quantiles, amwg_last_sample_dataset_quantiles, amwg_last_sample_dataset_hpd, amwg_last_sample_dataset_waic, amwg_last_sample_dataset_loo, amwg_fetch_draws*,
 * amwg_group_*, amwg_comm_gather_draws, amwg_comm_moments -- return AMWG_EINVAL with a message that names amwg_sample_summarize; so do
 * amwg_last_sample_dataset_histogram, amwg_last_sample_dataset_covariance and amwg_last_sample_dataset_autocovariance unless they were armed before the call
 * (amwg_set_histogram, amwg_set_covariance, amwg_set_autocovariance) and are asked for what was folded while the draws passed (edges = NULL, values = NULL).  An
 * armed autocovariance whose max_lag is not below the kept draws makes the summarising call itself AMWG_EINVAL, before its first launch.  A later amwg_sample* call replaces
 * the summary, amwg_burn leaves it alone, and every summarising call starts its accumulators afresh.  n = 0 succeeds and leaves nothing to summarise.
 * amwg_launch_info's n_launches (step-kernel launches) and kernel_ms (which includes the folds) cover the whole call.
 * amwg_sample_summarize = the _async form + amwg_sync.  Refused before a device is opened: null sampler, n < 0, thin < 1, window_rows < 0.
 * amwg_summary_info: the kept rows, the rows of the window, the number of folds, and the bytes of window and accumulators held by the last summarising call
 * (any pointer may be NULL); AMWG_EINVAL when the sampler's last sample call was not a summarising one. */
int amwg_sample_summarize_async(amwg_sampler *s, int64_t n, int64_t thin, int64_t window_rows);
int amwg_sample_summarize(amwg_sampler *s, int64_t n, int64_t thin, int64_t window_rows);
int amwg_summary_info(const amwg_sampler *s, int64_t *rows, int64_t *window_rows, int64_t *windows, size_t *window_bytes, size_t *accumulator_bytes);

/* POSTERIOR HISTOGRAMS over caller-given edges, counted on the device.  Per recorded value p (components, then derived quantities: PR = amwg_num_recorded) the caller
 * gives edges[p][0 .. bins]: finite, strictly ascending, 1 <= bins <= 4096.  THE BIN RULE is comparisons with the edges and no arithmetic on the draws: x is in bin i
 * iff edges[i] <= x < edges[i + 1]; x < edges[0] counts as UNDER, x >= edges[bins] as OVER (+inf is over, -inf under), a NaN as NAN; -0 equals +0 -- numpy's
 * searchsorted(edges, x, side="right") - 1.  counts[dataset][p][bins + 3]: the bins, then under, over, nan; a dataset's counts are over its chains x kept draws, and an
 * ordinary sampler is one dataset (as for amwg_last_sample_dataset_quantiles).  Counts are integers and do not depend on the order of the draws: the histogram of a
 * summarising call EQUALS that of the stored run, count for count, whatever the window.
 *   amwg_last_sample_dataset_histogram -- after amwg_sample*: the histogram of the kept draws under any valid edges.  After amwg_sample_summarize*: pass edges = NULL and
 *     the armed number of bins, and receive the counts folded under the edges armed before the call; edges given afterwards, another number of bins, or a call for which
 *     nothing was armed is AMWG_EINVAL with a message that names amwg_set_histogram.
 *   amwg_set_histogram -- arms a histogram for every later amwg_sample_summarize[_async] of this sampler (the edges are copied; NULL, 0 disarms): the counts are zeroed
 *     when a summarising call starts, and after each fold of a window the histogram kernel counts the same window on the same stream.  The edges stay fixed for the
 *     whole of a call.  Moments, R-hat, ESS, the chains' state, n_launches and amwg_summary_info are those of the unarmed call.
 *   amwg_histogram_info -- the armed number of bins (0: none) and the device bytes of its edges and counts (either pointer may be NULL).
 * Refused with AMWG_EINVAL and the call's name, before any device call: null pointers, bins outside 1 .. 4096, an edge that is not finite, edges that are not strictly
 * ascending, no sample call yet. */
int amwg_last_sample_dataset_histogram(amwg_sampler *s, const double *edges, int32_t bins, uint64_t *counts);
int amwg_set_histogram(amwg_sampler *s, const double *edges, int32_t bins);
int amwg_histogram_info(const amwg_sampler *s, int32_t *bins, size_t *bytes);

/* POSTERIOR COVARIANCE over a caller-chosen subset of the recorded values, per dataset, on the device.  values[0 .. n_values) are DISTINCT indices into the recorded
 * values (components, then derived quantities: PR = amwg_num_recorded); cov[dataset][n_values][n_values] is the full symmetric matrix in the order of `values`, with
 * the n - 1 denominator over the dataset's n = kept draws x chains; an ordinary sampler is one dataset.  A pair is computed once and written to both places.
 * THE ARITHMETIC is fixed (compiled with -ffp-contract=off, every operation rounds once).  Per chain c, in row order, for the k-th kept draw (1-based, over all kept
 * draws): dx_i = x_i - m_i; m_i += dx_i / k -- the mean line of the fold's Welford update, so m_i is bit for bit the whole-chain mean the fold keeps --; then for every
 * pair C_ij += dx_i * (x_j - m_j) with m_j already advanced to row k.  Of a pair, i is the value with the SMALLER index among the recorded values, wherever the two
 * stand in `values`: permuting `values` permutes rows and columns, every byte.  Per (dataset, pair), over the dataset's cpd chains of `rows` kept draws each, in the
 * order of the moments of a summarising call (256 threads, thread t takes chains t, t + 256, ...; a halving tree): gm_i = sum m_ic / cpd; within = sum C_ijc;
 * between = sum (m_ic - gm_i)(m_jc - gm_j); cov_ij = (within + rows between) / (n - 1).  The diagonal is that call's own SS / (n - 1) from the whole-chain M2: after
 * a summarising call sqrt(cov_ii) equals the sd of amwg_last_sample_dataset_moments as bytes.  The stored path runs the same kernels over the stored array from
 * zeroed per-chain scratch, so the matrix of a summarising call EQUALS the stored run's byte for byte, whatever the window.  Non-finite draws give what IEEE gives: a
 * NaN or infinity among a value's draws makes that value's row and column NaN in that dataset, and every other entry keeps its bytes.
 *   amwg_last_sample_dataset_covariance -- after amwg_sample*: the matrices of the kept draws over any valid `values`.  After amwg_sample_summarize*: pass values = NULL
 *     and the armed n_values, and receive the folded matrices; values given afterwards, another n_values, or a call for which nothing was armed is AMWG_EINVAL with a
 *     message that names amwg_set_covariance.
 *   amwg_set_covariance -- arms the covariance of `values` for every later amwg_sample_summarize[_async] of this sampler (the list is copied; NULL, 0 disarms): the
 *     co-moments are zeroed when a summarising call starts, and before each fold of a window the co-moment kernel adds the same window on the same stream, starting
 *     from the running means the fold has reached.  Moments, R-hat, ESS, the chains' state, n_launches and amwg_summary_info are those of the unarmed call.
 *   amwg_covariance_info -- the armed n_values (0: none) and the device bytes it holds: n_values (n_values - 1) / 2 x chains doubles of co-moments plus the list of
 *     values (either pointer may be NULL).
 * There is no cap on n_values other than PR.  Refused with AMWG_EINVAL and the call's name, before any device call: null pointers, n_values < 1 or > PR, an index
 * outside [0, PR), a repeated index, no sample call yet, kept draws x chains per dataset < 2, a byte count beyond size_t.  One device only: the amwg_group_* and
 * amwg_comm_* calls have no covariance. */
int amwg_last_sample_dataset_covariance(amwg_sampler *s, const int32_t *values, int32_t n_values, double *cov);
int amwg_set_covariance(amwg_sampler *s, const int32_t *values, int32_t n_values);
int amwg_covariance_info(const amwg_sampler *s, int32_t *n_values, size_t *bytes);

/* AUTOCOVARIANCE ALONG THE CHAINS at lags 0 .. max_lag over a caller-chosen subset of the recorded values, per dataset, on the device: what an autocorrelation, an
 * integrated autocorrelation time and an effective sample size that needs no second chain are formed from (the host function autocorrelation_ess of the front ends
 * does that: Geyer's initial monotone sequence, BDA3 section 11.5, without rank normalisation).  values[0 .. n_values) are DISTINCT indices into the recorded values;
 * acov[dataset][n_values][max_lag + 1], mean[dataset][n_values] and between[dataset][n_values] are in the order of `values`; an ordinary sampler is one dataset,
 * and one chain per dataset is allowed.
 * THE ARITHMETIC is fixed (compiled with -ffp-contract=off, every operation rounds once).  Per chain c and value, x_0 .. x_(n-1) its kept draws in row order, n = kept
 * draws: the pilot a = x_0 and y_t = x_t - a; in row order Y += y_t and, for every lag l = 0 .. min(t, L), S_l += y_t * y_(t-l), each S_l one running sum in
 * ascending t.  At the end ybar = Y / n; H_0 = T_0 = 0, H_(l+1) = H_l + y_l, T_(l+1) = T_l + y_(n-1-l) (the sums of the first and of the last l deviations);
 *   gamma_l = ((S_l - ybar * ((Y - H_l) + (Y - T_l))) + (double)(n - l) * (ybar * ybar)) / (double)n
 * -- in exact arithmetic (1 / n) sum_(t >= l) (x_t - xbar)(x_(t-l) - xbar), the estimator an FFT-based ACF computes; centring on the pilot removes a large offset --
 * and the chain mean m_c = a + ybar.  Per (dataset, value), over the dataset's cpd chains in the order of the moments of a summarising call (256 threads, thread t
 * takes chains t, t + 256, ...; a halving tree): acov_l = (sum_c gamma_lc) / cpd; gm = (sum_c m_c) / cpd, returned as mean; between = sum_c (m_c - gm)^2 / (cpd - 1),
 * 0.0 when cpd = 1.  A NaN or an infinity among a value's draws in a dataset -- and sums that overflow: whatever leaves acov_0 not finite -- makes that (dataset,
 * value)'s acov, mean and between NaN; every other output keeps its bytes.  The stored path runs the kernels of the folded path over the stored array from a zeroed
 * state, so the result of a summarising call EQUALS the stored run's byte for byte, whatever the window.
 *   amwg_last_sample_dataset_autocovariance -- after amwg_sample*: over any valid `values` and max_lag.  After amwg_sample_summarize*: pass values = NULL with the
 *     armed n_values and max_lag and receive what was folded; values given afterwards, another n_values or max_lag, or a call for which nothing was armed is
 *     AMWG_EINVAL with a message that names amwg_set_autocovariance.
 *   amwg_set_autocovariance -- arms `values` and max_lag for every later amwg_sample_summarize[_async] of this sampler (the list is copied; NULL, 0, 0 disarms): the
 *     state is zeroed when a summarising call starts; after the fold (and the histogram) of each window a kernel adds the window's lagged sums on the same stream,
 *     reading draws older than the window from a ring of the last max_lag kept rows, and a second kernel then moves the ring on.  A summarising call that would keep
 *     <= max_lag draws is itself refused (AMWG_EINVAL) before its first launch, the chains' state untouched.  Moments, R-hat, ESS, the chains' state, n_launches and
 *     amwg_summary_info are those of the unarmed call.
 *   amwg_autocovariance_info -- the armed n_values (0: none) and max_lag and the device bytes held: (3 max_lag + 2) x n_values x chains doubles (the lagged sums,
 *     the sum of deviations, the ring and the first max_lag rows) plus the list of values (any pointer may be NULL).
 * max_lag is at most 1024, a chosen cap: the state grows with it.  Refused with AMWG_EINVAL and the call's name, before any device call: null pointers, n_values < 1 or
 * > PR, an index outside [0, PR), a repeated index, max_lag outside 1 .. 1024, no sample call yet, max_lag >= kept draws, a byte count beyond size_t.  One device
 * only: the amwg_group_* and amwg_comm_* calls have no autocovariance. */
int amwg_last_sample_dataset_autocovariance(amwg_sampler *s, const int32_t *values, int32_t n_values, int32_t max_lag, double *acov, double *mean, double *between);
int amwg_set_autocovariance(amwg_sampler *s, const int32_t *values, int32_t n_values, int32_t max_lag);
int amwg_autocovariance_info(const amwg_sampler *s, int32_t *n_values, int32_t *max_lag, size_t *bytes);

/* Replaces sampler.start_adaptation() / .stop_adaptation() (mcmc.js:1060-1073). */
int amwg_set_adapting(amwg_sampler *s, int32_t flag);

/* Replaces reading sampler.state (mcmc.js:964): out[component][chain], P*chains doubles. */
int amwg_get_state(amwg_sampler *s, double *out, size_t out_bytes);

/* Per-chain starting points (the reference starts every chain of a run at the same completed `init`,
 * mcmc.js:954-957; with many chains over-dispersed starts are what R-hat needs): state[component][chain],
 * P*chains doubles.  Invalidates the cached log_post, which is recomputed by the next launch. */
int amwg_set_state(amwg_sampler *s, const double *state, size_t state_bytes);

/* Replaces sampler.info() (mcmc.js:977-980 -> 906-912 -> 563-571).  Every array is
 * [component][chain]; any pointer may be NULL.  `accepts`/`inbounds` are run totals the
 * reference does not keep (accept decisions and in-bounds proposals), used by parity tests. */
int amwg_info(amwg_sampler *s, double *prop_log_scale, int32_t *acceptance_count, int32_t *iterations_since_adaption,
              int32_t *batch_count, int64_t *accepts, int64_t *inbounds);

/* Per chain: uniforms consumed so far, cached log_post(state), and the current order of the
 * named sub-steppers (mcmc.js:887), order[chain * n_params + k]. */
int amwg_chain_diag(amwg_sampler *s, uint64_t *uniforms, double *log_post, int32_t *named_order);

/* Posterior summaries computed on the device over the draws of the LAST amwg_sample* call:
 * mean[P], sd[P] (n-1 denominator) over all chains x kept draws. */
int amwg_last_sample_moments(amwg_sampler *s, double *mean, double *sd);

/* Convergence diagnostics over the draws of the LAST amwg_sample* call, computed on the device per recorded value
 * (what the reference's users do in R on the returned arrays, tests/test_mcmc_js.R): split-R-hat (every chain cut in
 * two halves; Gelman et al., BDA3 section 11.4) and the effective sample size from the variance of the chain means,
 * ess = chains * var_plus / Var(chain mean).  Needs >= 2 chains and >= 4 kept draws.  rhat[P], ess[P].
 * Degenerate columns: rhat is NaN when W = 0 (every half-chain constant) or when any used draw is not finite; ess is NaN when the chain means do not
 * vary (Var(chain mean) = 0) or a used draw is not finite.  With an odd number of kept draws the last one is ignored (half = kept / 2, rounded down). */
int amwg_last_sample_diagnostics(amwg_sampler *s, double *rhat, double *ess);

/* Posterior quantiles over the draws of the LAST amwg_sample* call (all chains x kept draws pooled), per recorded value:
 * radix sort on the device, R's default interpolation (type 7).  probs[n_probs] in [0,1]; out[P][n_probs]. */
int amwg_last_sample_quantiles(amwg_sampler *s, const double *probs, int32_t n_probs, double *out);

/* The same three summaries over SEVERAL samplers that are the shards of one logical job (chains split over the devices of a node
 * with amwg_options.chain_offset; `options.devices` of the JavaScript front-end): every device reduces its own draws and the
 * partial results are combined with an RCCL all-reduce over xGMI (quantiles: grouped ncclSend/ncclRecv of one component's
 * values to the first shard's device, sorted there) -- SURVEY.md section 8(e) "all-gather of per-chain moment summaries".
 * One process, ncclCommInitAll over the shards' devices (cached); RCCL is loaded on first use.  Shards may share a device
 * (they are summed on the device before the collective).  All shards must hold a sample() of the same number of kept draws.
 * Output sizes as for the single-sampler calls. */
int amwg_group_moments(amwg_sampler *const *shards, int32_t n_shards, double *mean, double *sd);
int amwg_group_diagnostics(amwg_sampler *const *shards, int32_t n_shards, double *rhat, double *ess);
int amwg_group_quantiles(amwg_sampler *const *shards, int32_t n_shards, const double *probs, int32_t n_probs, double *out);

/* The gather at sample collection (BASELINE.json north_star: "chains shard across the GPUs of one node with an RCCL-over-xGMI gather only at
 * sample collection").  The reference has one chain and nothing to gather: this is where `sampler.sample(n)`'s return
 * value (mcmc.js:1005-1030) is put together for a job whose chains live on several devices.
 *   amwg_group_gather_draws -- ONE process, one sampler per device: every shard's block of recorded draws [kept][P + derived][chains_i] of the
 *     last sample call travels to the device of shard `root_index` (grouped ncclSend / ncclRecv over the shards' communicator; shards on the
 *     root's own device are copied), where the blocks stand back to back in shard order -- in dst_device (on the root's device; may be null:
 *     a scratch buffer is used) and, if dst_host is given, in ONE copy to the host.  offsets[i] (optional) = first element of shard i's block.
 *   amwg_group_comm_info -- what the communicator says about itself: ranks (ncclCommCount) and the device of every rank. */
int amwg_group_gather_draws(amwg_sampler *const *shards, int32_t n_shards, int32_t root_index, double *dst_device, double *dst_host,
                            size_t capacity_bytes, int64_t *offsets);
int amwg_group_comm_info(amwg_sampler *const *shards, int32_t n_shards, int32_t *n_ranks, int32_t *devices, int32_t capacity);

/* The same exchanges for hosts that run ONE PROCESS PER DEVICE (torch.distributed.run, MPI, a process pool of Node workers): a communicator is
 * built from a shared 128-byte id -- amwg_comm_unique_id on one rank, the bytes travel by whatever the host has, amwg_comm_create on every
 * rank (collective) -- and then, all collective:
 *   amwg_comm_gather_draws -- the block [kept][P + derived][chains] of this rank's last sample call travels to rank `root`, where the blocks stand
 *     back to back in rank order in dst_device (root only).  Blocks may differ in size (uneven shards): the counts are exchanged first;
 *     counts (optional, one entry per rank, filled on every rank) = the elements each rank contributed.
 *   amwg_comm_moments -- mean and sd over the recorded draws of all ranks (two all-reduces of a few doubles), on every rank.
 *   amwg_comm_info -- ranks, own rank and device AS RCCL REPORTS THEM (ncclCommCount / ncclCommUserRank / ncclCommCuDevice). */
typedef struct amwg_comm amwg_comm;
#define AMWG_COMM_ID_BYTES 128
int amwg_comm_unique_id(char *id, size_t capacity);
int amwg_comm_create(const char *id, size_t id_bytes, int32_t n_ranks, int32_t rank, int32_t device, amwg_comm **out);
int amwg_comm_info(amwg_comm *c, int32_t *n_ranks, int32_t *rank, int32_t *device);
int amwg_comm_gather_draws(amwg_sampler *s, amwg_comm *c, int32_t root, double *dst_device, size_t capacity_bytes, int64_t *counts);
int amwg_comm_moments(amwg_sampler *s, amwg_comm *c, double *mean, double *sd);
int amwg_comm_destroy(amwg_comm *c);

/* AMWG_LANES_AUTOTUNE: the candidates that were timed at construction -- lanes[i] lanes per chain took ms[i] milliseconds PER STEP (the
 * fastest of several launches long enough to take >= 1 ms, after an untimed warm-up launch).  Returns the number of candidates (0 if the sampler was not autotuned); fills at most `cap` entries. */
int amwg_tuning(const amwg_sampler *s, int32_t *lanes, double *ms, int32_t cap);

int amwg_sync(amwg_sampler *s);
int amwg_num_components(const amwg_sampler *s);   /* P: scalar parameter components */
int amwg_num_recorded(const amwg_sampler *s);     /* values per draw row: P + derived quantities */
int64_t amwg_num_chains(const amwg_sampler *s);
/* Launch geometry actually used and HIP-event time of the step kernels of the last burn/sample call. */
int amwg_launch_info(const amwg_sampler *s, int32_t *lanes_per_chain, int32_t *block_threads, int32_t *grid_blocks,
                     int32_t *lds_bytes, int32_t *n_launches, double *kernel_ms);
/* Name of the step kernel this sampler launches, as a profiler lists it (without the amwg:: qualifiers): "amwg_step_kernel<HierNormalModel,64,512>",
 * "amwg_sweep_kernel<HierNormalModel,512>" (the hierarchical family's row layout: lane-local re-evaluation + sweep prefetch), "amwg_step_kernel_cert<NormalModel,1,256>" /
 * "amwg_sweep_kernel_cert<HierNormalModel,512>" (the kernels that decide from certified values: options.full_evaluation = 0 where a family has them),
 * "amwg_gl_kernel<HierGlModel,512>" (options.group_local), "amwg_user_step" (a translated closure).  The last number is the workgroup size
 * class the kernel was compiled for (256 / 512 / 1024).  Valid until the sampler is destroyed. */
const char *amwg_kernel_name(const amwg_sampler *s);
/* The summation order this sampler's decisions and its cached log_post follow: the number of per-lane partial sums log_post is formed from.
 * 1 = the REFERENCE's own order (one running sum over the closure's terms, mcmc.js:524-526 calling the model's log_post): accept counts and draws are
 * the reference's bit for bit -- every sampler at one lane per chain, and at any lane count the kernels that decide from certified values against the
 * expression in that order (round 5: the hierarchical family's sweep kernel at 64 lanes, the Poisson family at 16 lanes; options.full_evaluation = 0).
 * Otherwise lanes_per_chain: the expression is summed per lane and the lanes' sums by a butterfly (the oracle's lane order; a decision can differ from
 * the reference's where a uniform falls between the two orders' values, ~1e-10 of the decisions).  Negative: an error code. */
int amwg_summation_order(const amwg_sampler *s);
int amwg_destroy(amwg_sampler *s);
const char *amwg_last_error(void);
const char *amwg_version(void);

/* Host evaluations of the exact source the kernel compiles (csrc/amwg_math.h, amwg_philox.h): what the JavaScript front-end's host-side
 * log_post() and the data generators of the harnesses use.  (The remaining building blocks are exported one by one by the test build
 * only: include/amwg_selftest.h, libamwg_selftest.so.) */
double amwg_exp(double x);   /* bit-identical to V8 Math.exp */
double amwg_log(double x);   /* bit-identical to V8 Math.log */
double amwg_uniform(uint64_t seed, uint64_t chain, uint64_t index);
/* Measured fp64 vector issue ceiling of the device: a register-only kernel of independent v_fma_f64 chains on every SIMD
 * (what the chip sustains under fp64 load at its own clocks), in lane-operations per second.  bench.py prices the step
 * kernel against this next to the datasheet number. */
int amwg_fp64_peak(int32_t device, double *lane_ops_per_s);

#ifdef __cplusplus
}
#endif
#endif
