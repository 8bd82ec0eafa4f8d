// amwg_plan.hip -- the launch plan of a sampler: which kernel (variant_for), in which geometry (choose_geometry: priced; autotune_geometry: measured) and
// what goes with it (adopt_plan: the built-in kernel, DataRef::pad, the wave scratch); and the group-local layout a plan of that kind runs on (gl_layout).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "amwg_host.h"
#include "amwg_kernel.h"
#include "amwg_models.h"

using namespace amwg;

const FamilyRow *family_of(int model) {
  static const FamilyRow rows[4] = {amwg_family_row<0>(), amwg_family_row<1>(), amwg_family_row<2>(), amwg_family_row<3>()};      // (AMWG_MODEL_* - 1)
  return model >= AMWG_MODEL_NORMAL && model <= AMWG_MODEL_POIS_GLM ? &rows[model - 1] : nullptr;
}

// Group-local evaluation (amwg_gl.h): deals the 64 lanes of a chain's wavefront to the groups and lays the observations out lane-major.
//   * lanes: every group one lane to begin with (Gn <= 64); then, while lanes are left, the group with the most observations per lane
//     (ceil(n_k / L_k); ties: the smaller index) has its lane count doubled -- it stops when that group cannot be doubled any more, since
//     doubling others would not shorten the longest lane;
//   * placement: blocks in order of decreasing size (ties: group index), so that every block of 2^j lanes starts at a multiple of 2^j;
//   * observations: lane m of block k takes the group's observations (in index order) number m, m + L_k, m + 2 L_k, ...;
//   * tile[r * 64 + lane] = the r-th observation of that lane, rows padded with 0 up to the longest lane.
// Restated in oracle/amwg_oracle.c (gl_layout) -- the order of additions of the group-local mode follows from it.
int gl_layout(const double *y, const int32_t *g, int N, int Gn, GlLayoutHost *out) {
  if (Gn < 1 || Gn > 64) return amwg_fail(AMWG_EINVAL, "group_local: 1 to 64 groups (a chain runs on one wavefront, a lane serves one group), got %d", Gn);
  std::vector<int> n(Gn, 0), L(Gn, 1), first(Gn, 0);
  for (int i = 0; i < N; ++i) {
    if (g[i] < 0 || g[i] >= Gn) return amwg_fail(AMWG_EINVAL, "group_local: g[%d] = %d outside 0..%d", i, g[i], Gn - 1);
    n[g[i]]++;
  }
  int total = Gn;
  for (;;) {
    int best = 0;
    long load_best = -1;
    for (int k = 0; k < Gn; ++k) { const long load = (n[k] + L[k] - 1) / L[k]; if (load > load_best) { load_best = load; best = k; } }
    if (load_best <= 1 || total + L[best] > 64) break;
    total += L[best];
    L[best] *= 2;
  }
  std::vector<int> order(Gn);
  for (int k = 0; k < Gn; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return L[a] > L[b]; });
  out->lane.assign(64, GlLane{0, -1, 1, 0, 0});
  int at = 0;
  for (int k : order) {
    first[k] = at;
    for (int m = 0; m < L[k]; ++m) {
      GlLane &q = out->lane[at + m];
      q.grp = (int8_t)k; q.blk = (int8_t)L[k]; q.first = m == 0 ? 1 : 0;
      q.cnt = (n[k] - m + L[k] - 1) / L[k];
      if (q.cnt < 0) q.cnt = 0;
    }
    at += L[k];
  }
  for (int c = 0; c < Gn; ++c) out->lane[c].first_of = (int8_t)first[c];
  int rounds = 0, n_min = -1;
  for (int j = 0; j < 64; ++j) {
    if (out->lane[j].cnt > rounds) rounds = out->lane[j].cnt;
    if (out->lane[j].cnt > 0 && (n_min < 0 || out->lane[j].cnt < n_min)) n_min = out->lane[j].cnt;
  }
  if (rounds < 1) rounds = 1;
  if (n_min < 0) n_min = 0;
  out->rounds = rounds;
  out->n_min = n_min;
  out->tile.assign((size_t)rounds * 64, 0.0);
  std::vector<int> seen(Gn, 0);
  for (int i = 0; i < N; ++i) {
    const int k = g[i], m = seen[k] % L[k], r = seen[k] / L[k];
    out->tile[(size_t)r * 64 + first[k] + m] = y[i];
    seen[k]++;
  }
  return AMWG_OK;
}

// ---- The launch plan: variant_for decides the kernel of a geometry, choose_geometry picks the geometry, adopt_plan sets what goes with it.
// Per variant: the kernel's name (a translated closure's: its hiprtc symbol, amwg_user_kernels.h) and whether it decides accept tests from certified values
// (amwg_kernel.h kCert).  The certified kernels evaluate the expression in the reference's order: their summation order is 1.
static const VariantInfo kVariants[] = {
    {"amwg_step_kernel", false}, {"amwg_step_kernel_cert", true}, {"amwg_sweep_kernel", false}, {"amwg_sweep_kernel_cert", true}, {"amwg_gl_kernel", false},
    {"amwg_user_step", false}, {"amwg_user_step_cert", true}, {"amwg_user_sweep", false}, {"amwg_user_sweep_cert", true}};
const VariantInfo &info(Variant v) { return kVariants[(int)v]; }

// A dataset sampler (amwg_create_datasets; amwg_dataset.h): chains per dataset, 0 for every other sampler; and the chains a workgroup of a geometry serves
static int64_t chains_per_dataset(const amwg_sampler *s) { return s->n_datasets > 1 ? s->C / s->n_datasets : 0; }
static int chains_per_workgroup(int lanes, int block) { return lanes > 64 ? 1 : block / lanes; }

// The kernel G lanes per chain in workgroups of bt threads with max_lds bytes of LDS run, and its DataRef::pad: the plan's lanes, block, variant and pad.
//   * certified decisions unless full_evaluation or exact_division ask for the expression: the Normal family at one lane per chain, the Poisson family at
//     16, the hierarchical family's sweep kernel; a closure without binary parameters with a certified tail (amwg_user.h norm_tail_approx: one lane;
//     amwg_gtail.h glm_tail_approx<PoisLink | LogitLink>: 16 lanes, four chains sharing every row they read) or a row plan marked kRowCert
//     (amwg_rows.h);
//   * the row layout (lane-local re-evaluation) of the hierarchical family and of a closure's row plan (amwg_rows.h): a chain on one wavefront, not
//     switched off, the tile, the label bytes and the per-wavefront term rows beside the stepper state.  Its sweep kernels are compiled for at most 512
//     threads: a caller who ASKS for 1024 gets the kernel that evaluates everything, not a "no launch geometry fits" that names the wrong cause.  A
//     closure sweeps when a lane's sum depends on one entry of the swept vector (rows_sweep), no parameter is binary (BinaryStepper draws differently)
//     and every parameter vector fits the lanes of a wavefront;
//   * the Normal family at one lane per chain stages its observations in LDS for the certified pass (NormalModel::lds_bytes_of: pad = 1) in workgroups
//     of at most 512 threads, unless sufficient statistics replace the pass.
static LaunchPlan variant_for(const amwg_sampler *s, int G, int bt, size_t max_lds) {
  const amwg_options &o = s->opt;
  LaunchPlan p;
  p.lanes = G, p.block = bt;
  const bool decide_certified = o.full_evaluation == 0 && !o.exact_division;
  const bool rows_wanted = G == 64 && o.full_evaluation != 1 && !(o.block_threads > 512);
  auto rows_fit = [&](int pitch, int groups) {
    return lds_layout(HierNormalModel::rows_lds_bytes(pitch, bt / 64, groups), s->P, bt / 64, s->pl.max_top, s->n_params).total <= max_lds;
  };
  if (s->user) {
    const bool rows = rows_wanted && s->user_rows_n >= 64 && s->user_rows_groups >= 1 && s->user_rows_groups <= 64 && bt <= 512 &&
                      rows_fit(HierNormalModel::row_pitch(s->user_rows_n), s->user_rows_groups);
    const bool cert = decide_certified && !s->user_has_binary;
    p.pad = rows ? HierNormalModel::row_pitch(s->user_rows_n) : 0;
    if (rows && s->user_rows_sweep && !s->user_has_binary && s->pl.max_top <= 64)
      p.variant = cert && s->user_rows_cert ? Variant::UserSweepCert : Variant::UserSweep;
    else
      p.variant = cert && ((s->user_cert_tail_n > 0 && G == 1) || ((s->user_pois_tail_n > 0 || s->user_logit_tail_n > 0) && G == 16)) ? Variant::UserStepCert : Variant::UserStep;
    return p;
  }
  if (s->mc.group_local) { p.variant = Variant::GroupLocal, p.pad = s->gl_rounds; return p; }
  const bool rows = s->model == AMWG_MODEL_HIER_NORMAL && rows_wanted && ((s->hier_periodic_mask >> 6) & 1u) && s->d.G <= 64 && s->d.n_obs >= 64 &&
                    rows_fit(HierNormalModel::row_pitch(s->d.n_obs), s->d.G);
  const bool cert = decide_certified && ((s->model == AMWG_MODEL_NORMAL && G == 1) || (s->model == AMWG_MODEL_POIS_GLM && G == 16) || rows) &&
                    family_of(s->model)->certified(G, bt).plain != nullptr;
  p.variant = rows ? (cert ? Variant::HierSweepCert : Variant::HierSweep) : (cert ? Variant::StepCert : Variant::Step);
  p.pad = rows ? HierNormalModel::row_pitch(s->d.n_obs) : ((cert && s->model == AMWG_MODEL_NORMAL && bt <= 512 && !o.sufficient_statistics) ? 1 : 0);
  return p;
}

// does the plan use the row layout (the hierarchical family's sweep kernels; a closure's row plan)?
static bool row_layout(const amwg_sampler *s, const LaunchPlan &p) {
  return p.variant == Variant::HierSweep || p.variant == Variant::HierSweepCert || (s->user && p.pad > 0);
}

// LDS bytes of a workgroup of the plan on data of n_obs observations: the data its variant stages, then the stepper state of `cpb` chains (0: block / lanes).  cpb < block / lanes
// (one-wavefront workgroups only) is the fallback for models whose per-chain state is so large that 64 / G copies do not fit: the spare lane groups
// replicate the last chain.
static uint32_t lds_of_size(const amwg_sampler *s, const LaunchPlan &p, int cpb, int n_obs) {
  const int G = p.lanes, bt = p.block;
  size_t data = 0;
  switch (p.variant) {
    case Variant::GroupLocal: data = HierGlModel::gl_lds_bytes(p.pad, bt / 64); break;
    case Variant::HierSweep: case Variant::HierSweepCert: data = HierNormalModel::rows_lds_bytes(p.pad, bt / 64, s->d.G); break;
    case Variant::Step: case Variant::StepCert:
      data = (s->model == AMWG_MODEL_NORMAL && G == 1) ? (p.pad ? NormalModel::one_lane_tile_bytes(n_obs) : 0) : family_of(s->model)->lds_bytes(n_obs, s->d.G, G);
      break;
    default:      // a translated closure: its row plan, else the translator's figure
      data = p.pad ? HierNormalModel::rows_lds_bytes(p.pad, bt / 64, s->user_rows_groups) : (size_t)(G == 1 ? s->user_lds_one_lane : s->user_lds);
  }
  return G > 64 ? lds_layout(data, s->P, G / 64, s->pl.max_top, s->n_params, true).total : lds_layout(data, s->P, cpb ? cpb : bt / G, s->pl.max_top, s->n_params).total;
}

// A dataset sampler whose sizes differ (amwg_create_datasets_ragged): every workgroup lays its LDS out for ITS dataset (amwg_kernel.h DataBytesOf), the launch's
// dynamic LDS has to cover the largest of those layouts -- the maximum over the sizes, not the layout of the largest size: the one-lane tiles of the Normal and
// the Bernoulli family are dropped beyond a limit, so the bytes are not monotone in n_obs.
static uint32_t lds_of(const amwg_sampler *s, const LaunchPlan &p, int cpb = 0) {
  if (s->n_datasets <= 1) return lds_of_size(s, p, cpb, s->d.n_obs);
  uint32_t most = 0;
  int last = -1;
  for (int n : s->ds_n_obs) {      // (a run of equal sizes is priced once: the common case is all of them equal)
    if (n == last) continue;
    most = std::max(most, lds_of_size(s, p, cpb, n));
    last = n;
  }
  return most;
}

// Geometry.  For every lanes-per-chain G take the largest workgroup that still gives every CU a workgroup (more waves
// share one LDS copy of the data) and price it with a two-term model of one parameter update:
//     cost(G) = rounds * [ S(G) * max(w_res, 1.8) + (W / G) * max(w_res, 1.15) * (1 + 0.3 / w_res) ]
// S(G) = the replicated stepper (Philox, proposal, exp, accept, adaptation), W/G the wave's share of the log-likelihood
// work, w_res the number of waves a SIMD holds at once (limited by LDS and by the number of chains), rounds the number of
// such batches; the floors are the occupancies below which each part is latency- rather than issue-bound.  The cheapest
// G wins, ties go to the smaller G.  The choice depends only on the model, the data size and the chain count, so a
// given sampler configuration always gets the same G (the lane count fixes the summation order, hence the draws).
// W is priced for the kernel G lanes would run in 256-thread workgroups with 160 KB of LDS, whatever the device.
// A dataset sampler has ONE geometry (the lanes fix the summation order); LDS is fitted with its largest dataset (lds_of), the work priced with the mean size
// ceil(sum n_d / D): the launch's work is the sum over the datasets.  Still a function of (model, sizes, chains) alone.
static int priced_n_obs(const amwg_sampler *s) {
  if (s->n_datasets <= 1) return s->d.n_obs;
  int64_t sum = 0;
  for (int n : s->ds_n_obs) sum += n;
  return (int)((sum + s->n_datasets - 1) / s->n_datasets);
}
static int log2_of(int lanes) { int lg = 0; for (int g = lanes; g > 1; g >>= 1) ++lg; return lg; }      // (lane counts are powers of two)
static double model_work(const amwg_sampler *s, int G) {
  const LaunchPlan q = variant_for(s, G, 256, (size_t)160 * 1024);
  const double N = (double)priced_n_obs(s);
  switch (s->model) {
    // (one lane per chain: accept tests are decided from the certified pass -- two operations per observation -- unless the caller asked for the expression in every update)
    case AMWG_MODEL_NORMAL: return q.variant == Variant::StepCert ? (s->opt.sufficient_statistics ? 40.0 : 2.6 * N) : 9.0 * N;
    case AMWG_MODEL_BETA_BERN:   // one lane: exact fast-forward over ~log2(N) binades (or the scalar jump-table pass, one add per observation)
      return G == 1 ? (s->mc.exact_division ? 1.8 * N : 400.0 * (1.0 + std::log2(N + 2.0))) : 6.0 * N;
    case AMWG_MODEL_HIER_NORMAL: {
      // group labels that repeat with the lane stride: a lane reads its one mean once (constant-mean pass, 8.1 VALU and 1 LDS read per
      // observation); otherwise the gathered pass (9.4 VALU, 2.5 LDS reads: the LDS pipe, not the VALU, then sets the pace)
      const bool periodic = ((s->hier_periodic_mask >> log2_of(G)) & 1u) != 0;
      double w = (periodic ? 8.6 : 12.0) * N + 12.0 * s->d.G;
      // lane-local re-evaluation (row layout): of the G + 2 updates of a step only two make the full pass, the others re-form the sums of
      // the lanes of one group (~0.3 of a pass in time: a dependent chain on one lane)
      if (row_layout(s, q)) w *= (2.0 + 0.35 * s->d.G) / (2.0 + s->d.G);
      return w;
    }
    case AMWG_MODEL_POIS_GLM: return q.variant == Variant::StepCert ? 36.0 * N : 90.0 * N;      // (16 lanes per chain: the certified pass, four chains sharing every row they read)
  }
  if (q.variant == Variant::UserStepCert && s->user_pois_tail_n > 0) {      // exp + log per observation (~70 of the term's operations) become exp_bounded's 19, and a row is read once for four chains
    const double n = (double)s->user_pois_tail_n, w = s->user_work > 0 ? s->user_work : 1e6;
    return (w - 70.0 * n > 0.4 * w) ? w - 70.0 * n : 0.4 * w;
  }
  if (q.variant == Variant::UserStepCert && s->user_logit_tail_n > 0) {
    // exp, log1p and two quotients per observation (130 vector instructions per observation and chain in the lane-split loop) become softplus_bounded's 52, and a row is
    // read once for four chains.  0.36 of the translator's estimate: the ratio of the rates MEASURED on logit_n10k at 8 192 chains, 16 lanes, 512 threads -- 2.13e7
    // updates/s for the lane-order kernel, 5.95e7 for this one
    return 0.36 * (s->user_work > 0 ? s->user_work : 1e6);
  }
  if (q.variant == Variant::UserStepCert) {      // the tail loop's ~16 instructions per observation become the certified pass's 2.6
    const double w1 = s->user_work_one_lane > 0 ? s->user_work_one_lane : s->user_work, n = (double)s->user_cert_tail_n;
    return (w1 - 16.0 * n > 0 ? w1 - 16.0 * n : 0.0) + 2.6 * n;
  }
  if (G == 1 && s->user_work_one_lane > 0) return s->user_work_one_lane;   // translated closure with a two-valued sum: fast-forwarded
  double w = s->user_work > 0 ? s->user_work : 1e6;   // translated closure: the translator's estimate
  // row plan (lane-local re-evaluation, like the hierarchical family's): of the groups + 2 updates of a step only a few make the full pass
  if (row_layout(s, q)) w *= (2.0 + 0.35 * s->user_rows_groups) / (2.0 + s->user_rows_groups);
  return w;
}

// DataRef::wave_scratch for the geometry in s->plan: one line of 64 doubles per wavefront of the launch (amwg_pass.h wave_scratch_of indexes it by
// blockIdx.x * (blockDim.x / 64) + wavefront).  Only one-lane-per-chain kernels read it (the certified pass of the Normal family, a closure's certified tail); with the
// replica fallback (cpb < 64 chains in a one-wavefront workgroup) that is C / cpb lines, not C / 64.  Grows, never shrinks: an autotune candidate's launch and the
// adopted geometry find it large enough.  AMWG_WAVE_SCRATCH=0 (read while the sampler is constructed): none, the pass broadcasts with v_readlane.
// Its size is the allocation's own (hipMemGetAddressRange); launch_steps checks the invariant.
size_t wave_scratch_lines(const amwg_sampler *s) {
  if (!s->d.wave_scratch) return 0;
  hipDeviceptr_t base = nullptr;
  size_t bytes = 0;
  if (hipMemGetAddressRange(&base, &bytes, s->d.wave_scratch) != hipSuccess || base != s->d.wave_scratch) return 0;
  return bytes / (64 * sizeof(double));
}
static int size_wave_scratch(amwg_sampler *s) {
  const char *env = getenv("AMWG_WAVE_SCRATCH");
  if ((env && env[0] == '0') || s->plan.lanes != 1) return AMWG_OK;
  const size_t lines = (size_t)s->plan.grid * (size_t)(s->plan.block / 64);
  if (s->d.wave_scratch && lines <= wave_scratch_lines(s)) return AMWG_OK;
  double *p = nullptr;
  TRYB(dev_alloc(s, &p, lines * 64));
  if (s->d.wave_scratch) {
    for (auto it = s->dev_allocs.begin(); it != s->dev_allocs.end(); ++it)
      if (*it == s->d.wave_scratch) { (void)hipFree(*it); s->dev_allocs.erase(it); break; }
  }
  s->d.wave_scratch = p;
  return AMWG_OK;
}

// The plan for lanes_per_chain `lanes` (0 = auto, AMWG_LANES_FASTEST, or one lane count: autotune_geometry asks for each in turn).  No HIP calls, no writes
// to the sampler: adopt_plan does the rest.
int choose_geometry(const amwg_sampler *s, int lanes, int n_cus, size_t max_lds, LaunchPlan *out) {
  const amwg_options &o = s->opt;
  const int max_bt = s->user ? s->user_max_threads : family_of(s->model)->max_threads;
  // a dataset sampler: a workgroup serves ONE dataset, so the chains per workgroup divide the chains per dataset -- only such geometries are searched
  // (a closure with a certified Poisson / logistic tail in its per-dataset form -- kTailPerDataset -- is searched like any other: G = 16 is among those geometries when
  // block / 16 divides cpd, variant_for gives it UserStepCert and model_work prices it with the tail terms; a fixed (16, block) that does not divide cpd is the EINVAL below)
  const int64_t cpd = chains_per_dataset(s);
  bool lds_short = false;      // (a dataset sampler: some geometry that serves whole datasets was given up for LDS alone)
  auto fits = [&](int bt, int G) {
    if (bt > max_bt || bt % G != 0) return false;
    if (cpd && cpd % chains_per_workgroup(G, bt) != 0) return false;
    const LaunchPlan p = variant_for(s, G, bt, max_lds);
    if (cpd && lds_of(s, p) > max_lds) lds_short = true;
    // (the sweep kernels -- row layout, 64 lanes per chain -- keep the window stream and the sweep's per-lane values in registers: compiled for at most 512 threads,
    // where a lane has 256 of them; with the 128 of a 1024-thread workgroup the hierarchical family's ran from scratch memory, five times slower)
    if (lds_of(s, p) > max_lds || (bt > 512 && row_layout(s, variant_for(s, G, 512, max_lds)))) return false;
    // (one lane per chain with certified decisions -- the Normal family, a closure with a certified tail --: the wavefront's pass keeps 64 partial sums per lane: the 512
    // registers of a 256-thread workgroup with blocks of 16 observations, the 256 of a 512-thread one with blocks of 8 (round 6, last day: 9 spilled registers; 1.58e9 against
    // the 256-thread class's 1.55e9 at >= 131 072 chains, where 512-thread workgroups still fill every CU).  The 1024-thread class keeps the scalar-path pass (7.2e8) and is not
    // picked unless asked for; a closure's certified tail is compiled for the 256-thread class only)
    return !(G == 1 && info(p.variant).certified && !o.block_threads && bt > (p.variant == Variant::UserStepCert ? 256 : 512));
  };
  // (a closure's certified row plan -- amwg_user_sweep_cert -- ran in 256-thread workgroups for a day of round 6: in 512-thread ones it spilled 520 registers.  With the
  // S2 pass out of line -- amwg_rows.h rows_sq -- it spills 40 and the 512-thread class, two wavefronts per SIMD, is the faster one again: 2.82e9 against 1.90e9)
  if (s->user && !s->user_parallel && lanes > 1)
    return amwg_fail(AMWG_EINVAL, "this closure has no loop that can be split over lanes: lanes_per_chain must be 1 (or 0 = auto), got %d", lanes);
  const int bts[5] = {1024, 512, 256, 128, 64};
  LaunchPlan best, one;      // the cheapest plan, and the one with one lane per chain
  double best_cost = -1.0, cost1 = -1.0;
  const bool fixed_lanes = lanes > 0;
  for (int G = 1; G <= 1024; G <<= 1) {
    if (fixed_lanes && G != lanes) continue;
    if (s->user && !s->user_parallel && G > 1) break;   // nothing to split: one lane per chain
    // translated closures: with one lane per chain every data index is wave-uniform and the compiler moves the
    // per-observation integer logic to the scalar unit, which issues 4x slower than the vector lanes (measured 2.5x on
    // the beta-Bernoulli closure); two lanes per chain keep it on the vector path at no measurable cost elsewhere
    if (s->user && s->user_parallel && !fixed_lanes && G == 1 && !(s->user_work_one_lane > 0) && variant_for(s, 1, 256, max_lds).variant != Variant::UserStepCert) continue;
    int pick = 0;
    for (int bi = 0; bi < 5; ++bi) {   // largest workgroup with >= one workgroup per CU, else the smallest that fits
      const int bt = bts[bi];
      if (o.block_threads && bt != o.block_threads) continue;
      if (G > 64 && bt != G) continue;              // a multi-wave chain is exactly one workgroup
      if (!fits(bt, G)) continue;
      pick = bt;
      if ((s->C + bt / G - 1) / (bt / G) >= n_cus) break;
    }
    int cpb = 0;
    // (the replica fallback is refused for dataset samplers rather than reasoned about: none of their three families can reach it)
    if (!pick && !cpd && G < 64 && max_bt >= 64 && (!o.block_threads || o.block_threads == 64)) {
      for (int c = 32 / G; c >= 1; c >>= 1)      // fewer chains than lane groups in a one-wavefront workgroup
        if (lds_of(s, variant_for(s, G, 64, max_lds), c) <= max_lds) { pick = 64; cpb = c; break; }
    }
    if (!pick) continue;
    LaunchPlan p = variant_for(s, G, pick, max_lds);
    p.cpb = cpb;
    const int CPB = cpb ? cpb : pick / G;
    const int64_t blocks = (s->C + CPB - 1) / CPB;
    const uint32_t lds = lds_of(s, p, cpb);
    int64_t per_cu = 2048 / pick;                                  // 32 waves per CU
    if (lds > 0 && (int64_t)(max_lds / lds) < per_cu) per_cu = (int64_t)(max_lds / lds);
    if (per_cu < 1) per_cu = 1;
    const int64_t resident = blocks < per_cu * n_cus ? blocks : per_cu * n_cus;
    const double w_res = (double)resident * (pick / 64) / (4.0 * n_cus);          // waves a SIMD holds at once
    const double w_total = (double)blocks * (pick / 64) / (4.0 * n_cus);            // waves a SIMD has to run in all
    // stepper: 394 VALU instructions per update measured at G = 64 (rocprofv3, empty data), ~980 at G = 1, where the rnorm
    // rejection loops of the 64/G chains sharing a wave diverge (the expected maximum of 64/G geometric counts grows with
    // its logarithm); serial dependency chains, so it needs ~1.8 waves per SIMD to stay issue-bound.  Data loop: eight
    // independent terms in flight per lane, issue-bound already with one wave per SIMD.
    const double S = 400.0 + 97.0 * (G < 64 ? 6 - log2_of(G) : 0);
    const double Wl = model_work(s, G) / G + (G > 64 ? 150.0 : 0.0);   // + the workgroup barrier of every evaluation
    // (round 2, hand-pipelined data loops: one wave per SIMD already issues back to back; what a lone wave loses is the issue slots
    // of its own non-arithmetic instructions, 10 % at cfg2 with one lane per chain vs four waves -- measured 3.64e8 vs 4.03e8)
    const double w1 = w_res > 1.0 ? w_res : 1.0;
    const double cost = (w_total / w_res) * (S * (w_res > 1.8 ? w_res : 1.8) + Wl * w1 * (1.0 + 0.14 / w1));
    if (G == 1) { cost1 = cost; one = p; }
    if (best_cost < 0 || cost < best_cost * (1.0 - 1e-9)) { best_cost = cost; best = p; }
  }
  // Reference order first: with ONE lane per chain a chain's log_post is summed exactly as the reference sums it (`lp += term`,
  // mcmc.js:958-960), so every draw of a seeded run is the reference's bit for bit; with more lanes only the decisions are
  // (tested), the doubles are those of the G-lane order.  Unless the caller asked for a lane count (or for AMWG_LANES_FASTEST),
  // take one lane per chain whenever the model prices it within 12 % of the cheapest geometry.
  if (lanes == 0 && best.lanes > 1 && cost1 > 0 && cost1 <= 1.12 * best_cost) best = one;
  if (!best.lanes && cpd && lds_short) {      // (s->d.n_obs is the largest size: name the dataset that has it)
    int d_max = 0;
    for (int d = 1; d < s->n_datasets; ++d) if (s->ds_n_obs[d] > s->ds_n_obs[d_max]) d_max = d;
    return amwg_fail(AMWG_EINVAL, "no launch geometry fits dataset %d, the largest (n_obs = %d): every workgroup is given the LDS of the largest dataset, and with lanes %d (0 = any), block %d (0 = any) "
                     "that is more than %zu bytes", d_max, s->ds_n_obs[d_max], lanes, o.block_threads, max_lds);
  }
  if (!best.lanes && cpd)
    return amwg_fail(AMWG_EINVAL, "no launch geometry serves whole datasets: the chains of a workgroup (block_threads / lanes_per_chain, or 1 for a chain on several wavefronts) must divide "
                     "cpd = %lld chains per dataset; asked for lanes %d (0 = any), block %d (0 = any), %zu bytes of LDS", (long long)cpd, lanes, o.block_threads, max_lds);
  if (!best.lanes) return amwg_fail(AMWG_EINVAL, "no launch geometry fits: the model needs more than %zu bytes of LDS", max_lds);
  const int CPB = best.lanes > 64 ? 1 : (best.cpb ? best.cpb : best.block / best.lanes);
  best.grid = (int)((s->C + CPB - 1) / CPB);
  best.lds = (int)lds_of(s, best, best.cpb);
  *out = best;
  return AMWG_OK;
}

// Everything that goes with a plan: the sampler's geometry, DataRef::pad, the constant-mean pass of the hierarchical family (HierNormalModel::pass_fast:
// the labels repeat with the lane stride), the built-in kernel with its dataset twin (the family's row is asked once: KernelPair) and the wave scratch.
// A translated closure's kernel is compiled and loaded afterwards (amwg_create_user, prepare).
int adopt_plan(amwg_sampler *s, const LaunchPlan &p) {
  s->plan = p;
  s->d.pad = p.pad;
  if (s->user) {
    if (s->n_datasets > 1) {      // a closure on many datasets launches the twin (amwg_user_dataset.h); how many workgroups serve one dataset
      const int cpw = chains_per_workgroup(p.lanes, p.block);
      const int64_t cpd = chains_per_dataset(s);
      if (p.cpb || p.pad || (p.variant != Variant::UserStep && p.variant != Variant::UserStepCert) || cpd % cpw != 0)
        return amwg_fail(AMWG_EINVAL, "internal: a plan of %d lanes in workgroups of %d (cpb %d, pad %d) for a closure on datasets of %lld chains", p.lanes, p.block, p.cpb, p.pad, (long long)cpd);
      s->ds_blocks_per_dataset = (int)(cpd / cpw);
    }
    return size_wave_scratch(s);
  }
  if (s->model == AMWG_MODEL_HIER_NORMAL) s->mc.group_lane_const = (int32_t)((s->hier_periodic_mask >> log2_of(p.lanes)) & 1u);
  KernelPair k;
  switch (p.variant) {
    case Variant::StepCert: case Variant::HierSweepCert: k = family_of(s->model)->certified(p.lanes, p.block); break;
    case Variant::HierSweep: k.plain = amwg_kernel_hier_sweep(p.block); break;
    case Variant::GroupLocal: k.plain = amwg_kernel_hier_gl(p.block); break;
    default: k = family_of(s->model)->kernel(p.lanes, p.block);
  }
  s->kernel = k.plain;
  s->ds_kernel = k.ds;
  if (s->n_datasets > 1) {      // a dataset sampler launches the twin (amwg_dataset.h); how many workgroups serve one dataset
    const int cpw = chains_per_workgroup(p.lanes, p.block);
    const int64_t cpd = chains_per_dataset(s);
    if (p.cpb || (p.variant != Variant::Step && p.variant != Variant::StepCert) || cpd % cpw != 0)
      return amwg_fail(AMWG_EINVAL, "internal: a plan of %d lanes in workgroups of %d (cpb %d) for datasets of %lld chains", p.lanes, p.block, p.cpb, (long long)cpd);
    s->ds_blocks_per_dataset = (int)(cpd / cpw);
    if (!s->ds_kernel) return amwg_fail(AMWG_EINVAL, "no dataset kernel for model %d with %d lanes per chain in workgroups of %d", s->model, p.lanes, p.block);
  }
  if (s->n_datasets <= 1 && !s->kernel) return amwg_fail(AMWG_EINVAL, "no kernel for model %d with %d lanes per chain in workgroups of %d", s->model, p.lanes, p.block);
  return size_wave_scratch(s);
}
// ---- AMWG_LANES_AUTOTUNE: measure instead of model.  Every lane count whose geometry fits is adopted (adopt_plan) and prepared (`prepare`: kernel
// attribute, or hiprtc compile + load), run for a few steps on the real chain state -- which is saved
// before and restored after, so tuning leaves no trace in the chains -- and timed with HIP events.  The fastest wins, except that one
// lane per chain (the reference's summation order) is kept whenever it MEASURES within 12 % of the fastest.
struct TuneCandidate { LaunchPlan plan; hipModule_t module; hipFunction_t fn; float ms; };

int autotune_geometry(amwg_sampler *s, int n_cus, size_t max_lds, const std::function<int()> &prepare) {
  // the chain state the timing runs touch
  const size_t PC = (size_t)s->P * (size_t)s->C, C = (size_t)s->C;
  std::vector<std::pair<void *, size_t>> parts = {
      {s->ch.state, PC * 8}, {s->ch.prop_log_scale, PC * 8}, {s->ch.acceptance_count, PC * 4}, {s->ch.iterations_since_adaption, PC * 4},
      {s->ch.batch_count, PC * 4}, {s->ch.accepts, PC * 4}, {s->ch.inbounds, PC * 4}, {s->ch.perm, C * 8}, {s->ch.rng_n, C * 8}, {s->ch.lp_curr, C * 8}, {s->ch.lp_eps, C * 8}};
  if (s->ch.perm16) parts.push_back({s->ch.perm16, (size_t)s->n_params * C * 2});
  size_t total = 0;
  for (auto &p : parts) total += (p.second + 255) & ~(size_t)255;
  DevBuf save;
  HIP_TRY(save.alloc(total));
  auto copy_all = [&](bool restore) -> hipError_t {
    size_t off = 0;
    for (auto &p : parts) {
      char *sv = save.as<char>() + off;
      hipError_t e = restore ? hipMemcpyAsync(p.first, sv, p.second, hipMemcpyDeviceToDevice, s->stream) : hipMemcpyAsync(sv, p.first, p.second, hipMemcpyDeviceToDevice, s->stream);
      if (e != hipSuccess) return e;
      off += (p.second + 255) & ~(size_t)255;
    }
    return hipStreamSynchronize(s->stream);
  };
  HIP_TRY(copy_all(false));
  std::vector<TuneCandidate> cand;
  std::string first_error;
  for (int G = 1; G <= 1024; G <<= 1) {
    LaunchPlan plan;
    if (choose_geometry(s, G, n_cus, max_lds, &plan) != AMWG_OK || adopt_plan(s, plan) != AMWG_OK || prepare() != AMWG_OK) { if (first_error.empty()) first_error = g_err; continue; }
    TuneCandidate c{plan, s->user_module, s->user_fn, 0.f};
    // One untimed launch first (it evaluates log_post(init), stages the data for the first time and warms the instruction cache); then the
    // run length is scaled until a launch takes >= 1 ms -- short data loops would otherwise be ranked by launch overhead and noise -- and the
    // candidate's figure is the FASTEST of three such launches, per step.  The runs continue the chains from one another (a valid lp_curr,
    // no init evaluation inside a timed launch); the saved state is put back once the candidate is done.
    bool ok = true;
    s->lp_ready = false;
    ok = launch_steps(s, 1, 1, nullptr) == AMWG_OK && finish_timing(s) == AMWG_OK;
    int n_tune = 3, kept = 0;
    float best = -1.f;
    for (int rep = 0; rep < 10 && ok && kept < 3; ++rep) {
      ok = launch_steps(s, n_tune, 1, nullptr) == AMWG_OK && finish_timing(s) == AMWG_OK;
      if (!ok) break;
      const float ms = (float)s->kernel_ms;
      if (ms < 1.0f && n_tune < 192) { n_tune *= 4; continue; }      // too short to rank: a longer run
      const float per_step = ms / (float)n_tune;
      if (best < 0 || per_step < best) best = per_step;
      ++kept;
    }
    if (copy_all(true) != hipSuccess) ok = false;
    c.ms = best;
    ok = ok && best >= 0;
    s->lp_ready = false;
    if (ok) cand.push_back(c);
    else if (c.module) { (void)hipModuleUnload(c.module); }
    s->user_module = nullptr;
    s->user_fn = nullptr;
  }
  if (cand.empty()) return amwg_fail(AMWG_EINVAL, "autotune: no lane count could be run (%s)", first_error.c_str());
  size_t best = 0;
  for (size_t i = 1; i < cand.size(); ++i) if (cand[i].ms < cand[best].ms) best = i;
  if (cand[0].plan.lanes == 1 && cand[0].ms <= 1.12f * cand[best].ms) best = 0;      // reference order first
  for (size_t i = 0; i < cand.size(); ++i) if (i != best && cand[i].module) (void)hipModuleUnload(cand[i].module);
  const TuneCandidate &c = cand[best];
  s->user_module = c.module;
  s->user_fn = c.fn;
  TRYB(adopt_plan(s, c.plan));
  s->tuned.clear();
  for (auto &q : cand) s->tuned.push_back({q.plan.lanes, q.ms});
  s->n_launches = 0;
  s->kernel_ms = 0;
  return AMWG_OK;
}
