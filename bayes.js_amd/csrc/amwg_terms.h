// amwg_terms.h -- the pointwise terms l_si of the four built-in families over stored draws: what the WAIC (amwg_waic.hip) and the PSIS-LOO (amwg_loo.hip) kernels
// share, so that both see the same doubles.  The kernels that evaluate them, and the split of a dataset's draws over workgroups, are amwg_pointwise.h's.  Device code; internal to those two translation units, and
// not a source of the step kernels (tools/build_id.py).  The terms are the reference's, bit for bit (amwg_ld.h, amwg_div.h, exp_log_v8).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "amwg_div.h"
#include "amwg_ld.h"
#include "amwg_pointwise.h"
#include "amwg_waic.h"

namespace amwg {

// ---- the families: what an evaluation needs of a draw (staged in LDS), what it needs of an observation (registers), and the term
template <int MODEL> struct Family;

template <> struct Family<AMWG_MODEL_NORMAL> {
  struct Draw { double mu, c, den, yhi, ylo; int32_t fast, pad; };
  struct Obs { double x; };
  __device__ static int64_t n_eff(const WaicDataset &ds) { return ds.n_obs; }
  __device__ static Draw make_draw(const double *at, int64_t C, const WaicModel &M, const WaicDataset &ds) {      // at: component 0 of the draw
    Draw w;
    w.mu = at[0];
    const double sigma = at[C];
    w.c = norm_c(M.neg_half_log_2pi, sigma);
    w.den = norm_den(sigma);
    const Reciprocal y = make_reciprocal(w.den);
    w.yhi = y.hi; w.ylo = y.lo;
    w.fast = !M.exact_division && ds.data_mid_range && mid_range(w.den) && (w.mu == 0 || mid_range(__builtin_fabs(w.mu)));      // NormalModel::begin's condition
    w.pad = 0;
    return w;
  }
  __device__ static void set_base(Draw &, int64_t) {}
  __device__ static Obs load_obs(const WaicModel &M, const WaicDataset &ds, int64_t i) { return Obs{M.x[ds.off_x + i]}; }
  __device__ __forceinline__ static double term(const WaicModel &, const Obs &o, const Draw &w, int64_t, const double *, int64_t) {
    const double t = o.x - w.mu;
    const double tt = t * t;
    return w.c - (w.fast ? div_by_invariant(tt, w.den, Reciprocal{w.yhi, w.ylo}) : tt / w.den);
  }
};

template <> struct Family<AMWG_MODEL_HIER_NORMAL> {      // theta[0 .. G - 1], mu, sigma.  The group's mean is read where the draws lie; IEEE division throughout
  struct Draw { double c, den; int64_t base; };
  struct Obs { double x; int64_t g_off; };
  __device__ static int64_t n_eff(const WaicDataset &ds) { return ds.n_obs; }
  __device__ static Draw make_draw(const double *at, int64_t C, const WaicModel &M, const WaicDataset &) {
    Draw w;
    const double sigma = at[(int64_t)(M.G + 1) * C];
    w.c = norm_c(M.neg_half_log_2pi, sigma);
    w.den = norm_den(sigma);
    w.base = 0;
    return w;
  }
  __device__ static void set_base(Draw &w, int64_t base) { w.base = base; }      // where the draw's component 0 lies
  __device__ static Obs load_obs(const WaicModel &M, const WaicDataset &ds, int64_t i) { return Obs{M.x[ds.off_x + i], (int64_t)M.xb[ds.off_xb + i]}; }
  __device__ __forceinline__ static double term(const WaicModel &, const Obs &o, const Draw &w, int64_t, const double *draws, int64_t C) {
    const double t = o.x - draws[w.base + o.g_off * C];
    return w.c - (t * t) / w.den;
  }
};

template <> struct Family<AMWG_MODEL_BETA_BERN> {      // two observations: x = 1 and x = 0
  struct Draw { double l1, l0; };
  struct Obs { int one; };
  __device__ static int64_t n_eff(const WaicDataset &ds) { return ds.n_obs > 0 ? 2 : 0; }
  __device__ static Draw make_draw(const double *at, int64_t, const WaicModel &, const WaicDataset &) {
    const double th = at[0];
    return Draw{log_v8(th), log_v8(1 - th)};      // BetaBernModel::begin: ld.bern(1, th), ld.bern(0, th)
  }
  __device__ static void set_base(Draw &, int64_t) {}
  __device__ static Obs load_obs(const WaicModel &, const WaicDataset &, int64_t i) { return Obs{i == 0}; }
  __device__ __forceinline__ static double term(const WaicModel &, const Obs &o, const Draw &w, int64_t, const double *, int64_t) { return o.one ? w.l1 : w.l0; }
};

template <> struct Family<AMWG_MODEL_POIS_GLM> {      // beta[0 .. 7], cp
  struct Draw { double b[8]; int32_t icp, pad; };
  struct Obs { double v[9]; };
  __device__ static int64_t n_eff(const WaicDataset &ds) { return ds.n_obs; }
  __device__ static Draw make_draw(const double *at, int64_t C, const WaicModel &, const WaicDataset &) {
    Draw w;
#pragma unroll
    for (int k = 0; k < 8; ++k) w.b[k] = at[(int64_t)k * C];
    const double cp = at[8 * C];
    w.icp = !(cp < 536870912.0) ? 536870912 : (cp <= 0.0 ? 0 : (int)__builtin_ceil(cp));      // PoisGlmModel::begin: i >= cp as an integer comparison
    w.pad = 0;
    return w;
  }
  __device__ static void set_base(Draw &, int64_t) {}
  __device__ static Obs load_obs(const WaicModel &M, const WaicDataset &ds, int64_t i) {
    Obs o;
#pragma unroll
    for (int k = 0; k < 7; ++k) o.v[k] = M.x[ds.off_x + (int64_t)k * ds.n_obs + i];
    o.v[7] = M.y[ds.off_y + i];
    o.v[8] = M.lfact[ds.off_lfact + i];
    return o;
  }
  __device__ __forceinline__ static double term(const WaicModel &, const Obs &o, const Draw &w, int64_t i, const double *, int64_t) {      // PoisGlmModel::eta_of, term_of
    double eta = o.v[0] * w.b[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) eta += o.v[k] * w.b[k];
    if (i >= (int64_t)w.icp) eta += w.b[7];
    double lam;
    const double lg = exp_log_v8(eta, lam, ExpLogLiterals{});
    return lg * o.v[7] - lam - o.v[8];
  }
};

}  // namespace amwg
