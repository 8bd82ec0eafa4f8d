// amwg_waic_fold.hip -- WAIC without stored draws (amwg_set_waic, amwg_waic_info; part of libamwg.so): the records a summarising call folds its windows' pointwise
// terms into, the launcher of the fold kernel (waic_fold_body, amwg_pointwise.h; the families' instantiations are amwg_waic.hip's, a closure's its code object's),
// the finish kernel, and the fold armed per sampler.  amwg_waic.h states the route, include/amwg.h the rule.  Deterministic: every record has one writer per window,
// the windows follow each other on one stream, and the splits are merged in ascending order.  Not a source of the step kernels (tools/build_id.py).
#include <hip/hip_runtime.h>

#include <mutex>
#include <unordered_map>
#include <vector>

#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_pointwise.h"
#include "amwg_sampler.h"
#include "amwg_waic.h"

using namespace amwg;

namespace {

int64_t n_eff(const PointwiseLaunch &K, const WaicDataset &ds) { return K.bern ? (ds.n_obs > 0 ? 2 : 0) : ds.n_obs; }

// out[(d * out_stride + i) * 2 + (0 | 1)] = lppd_i | p_i for i < n: the records of observation i merged over the splits in ascending order, a record's count from
// the indices -- `windows` full windows of Sw draws and a last one of Sl (model-free: bern = the family of two observations per dataset)
__global__ void __launch_bounds__(kThreads) waic_fold_finish_kernel(int64_t Sw, int64_t windows, int64_t Sl, const WaicDataset *__restrict__ sets, int bern,
                                                                    const int64_t *__restrict__ state_off, const Part *__restrict__ state, double *__restrict__ out, int64_t out_stride) {
  const int d = (int)blockIdx.y;
  const WaicDataset ds = sets[d];
  const int64_t n = bern ? (ds.n_obs > 0 ? 2 : 0) : ds.n_obs, splits = fold_splits(Sw, n);
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const Part *p = state + state_off[d] + i;
  Part a{-kInf, 0.0, 0.0, 0.0};
  double cnt = 0.0;
  for (int64_t k = 0; k < splits; ++k) merge_parts(a, cnt, p[k * n], fold_count(Sw, windows, Sl, splits, k));      // (a split that never held a draw counts 0: skipped)
  const double Sd = (double)(windows * Sw + Sl);
  double lppd = a.m + log_v8(a.sum) - log_v8(Sd), pv = a.M2 / (Sd - 1.0);
  if (!(__builtin_fabs(a.M2) < kInf) || !(__builtin_fabs(lppd) < kInf)) { lppd = __builtin_nan(""); pv = __builtin_nan(""); }
  out[(d * out_stride + i) * 2] = lppd;
  out[(d * out_stride + i) * 2 + 1] = pv;
}

void drop(DevBuf &b) { if (b.p) { (void)hipFree(b.p); b.p = nullptr; } }

// ---- the fold armed per sampler.  Beside the handle, not in it: amwg_sampler.h is one of the sources the step kernels' id is formed from
std::mutex g_waic_mu;
std::unordered_map<const amwg_sampler *, WaicFold> g_waic;

}  // namespace

size_t amwg_waic_fold_bytes(const PointwiseLaunch &K, const WaicDataset *sets, int D, int64_t window_rows, int64_t cpd) {
  size_t records = 0;
  for (int d = 0; d < D; ++d) { const int64_t n = n_eff(K, sets[d]); records += (size_t)(fold_splits(window_rows * cpd, n) * n); }
  return records * sizeof(Part);
}

int amwg_waic_fold_begin(const char *call, const PointwiseLaunch &K, const WaicDataset *sets, int D, int PR, int64_t C, int64_t window_rows, int64_t total_rows,
                         hipStream_t stream, WaicFold &f) {
  TRYB(amwg_waic_shape(call, total_rows, PR, C, D));
  if (window_rows < 1 || window_rows > 2147483647 / (C / D)) return amwg_fail(AMWG_EINVAL, "%s: a window of %lld rows (at least 1, fewer than 2^31 draws per dataset)", call, (long long)window_rows);
  for (int d = 0; d < D; ++d) if (sets[d].n_obs < 0) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: n_obs < 0", call, d);
  f.K = K;
  f.sets.assign(sets, sets + D);
  f.off.assign((size_t)D, 0);
  f.D = D; f.PR = PR; f.C = C; f.window_rows = window_rows; f.total_rows = total_rows;
  f.tiles = f.splits = f.n_most = 0;
  f.folded = false;
  const int64_t Sw = window_rows * (C / D);
  int64_t records = 0;
  for (int d = 0; d < D; ++d) {
    const int64_t n = n_eff(K, sets[d]), t = (n + kTile - 1) / kTile, sp = fold_splits(Sw, n);
    f.off[(size_t)d] = records;
    records += sp * n;
    f.tiles = t > f.tiles ? t : f.tiles; f.splits = sp > f.splits ? sp : f.splits; f.n_most = n > f.n_most ? n : f.n_most;
  }
  drop(f.d_sets); drop(f.d_off); drop(f.d_state);
  f.state_bytes = (size_t)records * sizeof(Part);
  HIP_TRY(f.d_sets.alloc((size_t)D * sizeof(WaicDataset)));
  HIP_TRY(f.d_off.alloc((size_t)D * 8));
  HIP_TRY(f.d_state.alloc(f.state_bytes));
  HIP_TRY(hipMemcpyAsync(f.d_sets.p, f.sets.data(), (size_t)D * sizeof(WaicDataset), hipMemcpyHostToDevice, stream));      // (from f's own vectors: they outlive the copies)
  HIP_TRY(hipMemcpyAsync(f.d_off.p, f.off.data(), (size_t)D * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(f.d_state.p, 0, f.state_bytes ? f.state_bytes : 8, stream));      // (each call starts afresh)
  f.folded = true;
  return AMWG_OK;
}

int amwg_waic_fold_window(const WaicFold &f, const double *window, int64_t g0, int64_t nrows, hipStream_t stream) {
  if (!window || !f.d_state.p || nrows < 0 || nrows > f.window_rows || g0 < 0 || g0 % f.window_rows != 0 || g0 + nrows > f.total_rows)
    return amwg_fail(AMWG_EINVAL, "internal: a WAIC fold of rows [%lld, %lld) in windows of %lld of %lld rows", (long long)g0, (long long)(g0 + nrows), (long long)f.window_rows, (long long)f.total_rows);
  if (nrows == 0 || f.tiles == 0) return AMWG_OK;
  int64_t cpd = f.C / f.D, window_rows = f.window_rows, C = f.C;      // (not const: the args[] list points at them)
  int PR = f.PR;
  const WaicDataset *d_sets = f.d_sets.as<WaicDataset>();
  const int64_t *d_off = f.d_off.as<int64_t>();
  Part *d_state = f.d_state.as<Part>();
  void *args[] = {&window, &nrows, &g0, &window_rows, &PR, &C, &cpd, f.K.model_arg(), &d_sets, &d_off, &d_state};
  HIP_TRY(amwg_pointwise_go(f.K, kPwWaicFold, dim3((unsigned)f.tiles, (unsigned)f.splits, (unsigned)f.D), stream, args));
  return AMWG_OK;
}

int amwg_waic_fold_finish(const char *call, const WaicFold &f, double *summary, int32_t *high, double *pointwise, hipStream_t stream) {
  if (!summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  const int D = f.D;
  PointwiseOut o;
  TRYB(amwg_pointwise_begin(call, f.sets.data(), D, 0, stream, o));
  DevBuf two;
  if (f.K.bern) HIP_TRY(two.alloc((size_t)D * 4 * 8));
  const int64_t Sw = f.window_rows * (f.C / D), windows = f.total_rows / f.window_rows, Sl = f.total_rows % f.window_rows * (f.C / D);
  if (f.n_most > 0) {
    hipLaunchKernelGGL(waic_fold_finish_kernel, dim3((unsigned)((f.n_most + kThreads - 1) / kThreads), (unsigned)D), dim3(kThreads), 0, stream, Sw, windows, Sl,
                       f.d_sets.as<WaicDataset>(), f.K.bern ? 1 : 0, f.d_off.as<int64_t>(), f.d_state.as<Part>(), f.K.bern ? two.as<double>() : o.pw.as<double>(),
                       f.K.bern ? (int64_t)2 : o.n_max);
    HIP_TRY(hipGetLastError());
  }
  if (f.K.bern) HIP_TRY(amwg_pointwise_bern_expand(f.K, o.sets.as<WaicDataset>(), D, two.as<double>(), o.pw.as<double>(), o.n_max, 2, stream));
  HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is freed on return)
  std::vector<double> own;
  double *pw = pointwise;
  if (!pw) { own.resize(o.pw_count ? o.pw_count : 1); pw = own.data(); }
  TRYB(amwg_pointwise_fetch(o, pw, nullptr));
  for (int d = 0; d < D; ++d) amwg_waic_totals(pw + (size_t)d * (size_t)o.n_max * 2, f.sets[(size_t)d].n_obs, summary + (size_t)d * 4, high ? high + d : nullptr);
  return AMWG_OK;
}

WaicFold *amwg_waic_armed(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_waic_mu);
  auto it = g_waic.find(s);      // (pointers into an unordered_map stay valid while other entries come and go)
  return it == g_waic.end() || !it->second.armed ? nullptr : &it->second;
}

int amwg_waic_begin(amwg_sampler *s, int64_t window_rows, int64_t rows, WaicFold **arm) {
  static const char *call = "amwg_sample_summarize";
  WaicFold *f = amwg_waic_armed(s);
  *arm = f;
  if (!f) return AMWG_OK;
  const int D = s->n_datasets, PR = s->P + s->D;
  TRYB(amwg_waic_shape(call, rows, PR, s->C, D));      // (before the code object of a closure is compiled or anything is allocated)
  std::vector<WaicDataset> sets;
  PointwiseLaunch K;
  if (s->user) {
    TRYB(amwg_pointwise_describe_user(s, sets, K));
  } else {
    WaicModel m{};
    TRYB(amwg_waic_describe(s, sets, m));
    TRYB(amwg_pointwise_family(call, m, PR, D, K));
  }
  return amwg_waic_fold_begin(call, K, sets.data(), D, PR, s->C, window_rows, rows, s->stream, *f);
}

void amwg_waic_forget(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_waic_mu);
  g_waic.erase(s);      // (the records go with it: DevBuf)
}

extern "C" {

int amwg_set_waic(amwg_sampler *s, int32_t on) {
  static const char *call = "amwg_set_waic";
  if (!s) return amwg_fail(AMWG_EINVAL, "%s: null sampler", call);
  if (on) {
    if (s->mc.group_local) return amwg_fail(AMWG_EINVAL, "%s: a group_local sampler keeps its observations as a lane-major tile; the pointwise terms need them in index order", call);
    if (s->user && s->pw_terms.empty()) return amwg_fail(AMWG_EINVAL, "%s: the pointwise terms of a closure are not known to the library (options.pointwise; amwg_set_pointwise)", call);
    if (s->model == AMWG_MODEL_HIER_NORMAL && !s->user && s->n_datasets != 1) return amwg_fail(AMWG_EINVAL, "%s: the hierarchical family runs on one dataset", call);
  }
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));      // (a summarising call still in flight writes to the records that go away)
  amwg_waic_forget(s);
  if (!on) return AMWG_OK;
  std::lock_guard<std::mutex> lock(g_waic_mu);
  g_waic[s].armed = true;
  return AMWG_OK;
}

int amwg_waic_info(const amwg_sampler *s, int32_t *armed, size_t *bytes) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_waic_info: null sampler");
  const WaicFold *f = amwg_waic_armed(s);
  if (armed) *armed = f ? 1 : 0;
  if (bytes) *bytes = f && f->folded ? f->state_bytes : 0;
  return AMWG_OK;
}

}  // extern "C"
