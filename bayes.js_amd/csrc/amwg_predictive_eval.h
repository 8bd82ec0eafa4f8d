// amwg_predictive_eval.h -- what one (draw, observation) contributes to the predictive calls, per built-in family: the evaluation of THE RULE of
// amwg_last_sample_dataset_predictive (include/amwg.h), shared by its kernels (amwg_predictive.hip) and by the PSIS-LOO weighted ones (amwg_loo_predictive.hip) so
// that both form F, Fm, mean and var by the same device functions.  Device code; not a source of the step kernels (tools/build_id.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "amwg_cdf.h"
#include "amwg_ld.h"
#include "amwg_pointwise.h"
#include "amwg_waic.h"

namespace amwg {

struct Eval { double F, Fm, mean, var; };                 // one (draw, observation) of THE RULE

// ---- the families: what a predictive evaluation needs of a draw (staged in LDS), of an observation (registers), and THE RULE's row.  R: the register block
template <int MODEL> struct Pred;

template <> struct Pred<AMWG_MODEL_NORMAL> {
  static constexpr int R = 4;
  struct Draw { double mu, sigma; };
  struct Obs { double x; };
  __device__ static Draw make_draw(const double *at, int64_t C, const WaicModel &, int64_t) { return Draw{at[0], at[C]}; }
  __device__ static Obs load_obs(const WaicModel &M, const WaicDataset &ds, int64_t j) { return Obs{M.x[ds.off_x + j]}; }
  __device__ static double y_of(const Obs &o) { return o.x; }
  __device__ __forceinline__ static Eval eval(const Obs &o, const Draw &w, int64_t, const double *, int64_t) {
    const double F = normal_cdf((o.x - w.mu) / w.sigma);
    return Eval{F, F, w.mu, w.sigma * w.sigma};
  }
};

template <> struct Pred<AMWG_MODEL_HIER_NORMAL> {      // theta[0 .. G - 1], mu, sigma: the group's mean is read where the draws lie
  static constexpr int R = 4;
  struct Draw { double sigma; int64_t base; };
  struct Obs { double x; int64_t g_off; };
  __device__ static Draw make_draw(const double *at, int64_t C, const WaicModel &M, int64_t base) { return Draw{at[(int64_t)(M.G + 1) * C], base}; }
  __device__ static Obs load_obs(const WaicModel &M, const WaicDataset &ds, int64_t j) { return Obs{M.x[ds.off_x + j], (int64_t)M.xb[ds.off_xb + j]}; }
  __device__ static double y_of(const Obs &o) { return o.x; }
  __device__ __forceinline__ static Eval eval(const Obs &o, const Draw &w, int64_t, const double *draws, int64_t C) {
    const double th = draws[w.base + o.g_off * C];
    const double F = normal_cdf((o.x - th) / w.sigma);
    return Eval{F, F, th, w.sigma * w.sigma};
  }
};

template <> struct Pred<AMWG_MODEL_BETA_BERN> {      // every x_j served directly; an x that is neither 0 nor 1: NaN
  static constexpr int R = 4;
  struct Draw { double th; };
  struct Obs { int one, invalid; };
  __device__ static Draw make_draw(const double *at, int64_t, const WaicModel &, int64_t) { return Draw{at[0]}; }
  __device__ static Obs load_obs(const WaicModel &M, const WaicDataset &ds, int64_t j) { return Obs{M.xb[ds.off_xb + j] ? 1 : 0, M.invalid && M.invalid[ds.off_xb + j] ? 1 : 0}; }
  __device__ static double y_of(const Obs &o) { return o.invalid ? __builtin_nan("") : (double)o.one; }
  __device__ __forceinline__ static Eval eval(const Obs &o, const Draw &w, int64_t, const double *, int64_t) {
    const double q = 1.0 - w.th, nan = __builtin_nan("");
    if (o.invalid) return Eval{nan, nan, nan, nan};
    return Eval{o.one ? 1.0 : q, o.one ? q : 0.0, w.th, w.th * q};
  }
};

template <> struct Pred<AMWG_MODEL_POIS_GLM> {      // beta[0 .. 7], cp.  eta: the double Family<POIS_GLM>::term forms (amwg_terms.h), the position rule included
  static constexpr int R = 2;
  struct Draw { double b[8]; int32_t icp, pad; };
  struct Obs { double v[7], y, lfact; };
  __device__ static Draw make_draw(const double *at, int64_t C, const WaicModel &, int64_t) {
    Draw w;
#pragma unroll
    for (int k = 0; k < 8; ++k) w.b[k] = at[(int64_t)k * C];
    const double cp = at[8 * C];
    w.icp = !(cp < 536870912.0) ? 536870912 : (cp <= 0.0 ? 0 : (int)__builtin_ceil(cp));
    w.pad = 0;
    return w;
  }
  __device__ static Obs load_obs(const WaicModel &M, const WaicDataset &ds, int64_t j) {
    Obs o;
#pragma unroll
    for (int k = 0; k < 7; ++k) o.v[k] = M.x[ds.off_x + (int64_t)k * ds.n_obs + j];
    o.y = M.y[ds.off_y + j];
    o.lfact = M.lfact[ds.off_lfact + j];
    return o;
  }
  __device__ static double y_of(const Obs &o) { return o.y; }
  __device__ __forceinline__ static Eval eval(const Obs &o, const Draw &w, int64_t pos, const double *, int64_t) {
    double eta = o.v[0] * w.b[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) eta += o.v[k] * w.b[k];
    if (pos >= (int64_t)w.icp) eta += w.b[7];
    double lam, F, Fm, Q;
    const double lg = exp_log_v8(eta, lam, ExpLogLiterals{});
    poisson_cdf_pair(o.y, o.lfact, lam, lg, F, Fm, Q);
    return Eval{F, Fm, lam, lam};
  }
};

}  // namespace amwg
