// amwg_pointwise_host.hip -- the host path that WAIC (amwg_waic.hip) and PSIS-LOO (amwg_loo.hip) share, declared in amwg_waic.h: how a call launches the kernels that
// evaluate the model, the two model-free kernels both need (NaN fill, the Bernoulli family's expand), the batches under the scratch budget, the device outputs of a
// call, the sampler's datasets and model as the launchers take them, and the one body of the two amwg_last_sample_dataset_* entries.  The statistics' own kernels and
// totals are in their files.  Part of libamwg.so; not a source of the step kernels (tools/build_id.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "amwg_dataset.h"
#include "amwg_fold.h"
#include "amwg_host.h"
#include "amwg_pointwise.h"
#include "amwg_sampler.h"
#include "amwg_waic.h"

using namespace amwg;

namespace {

__global__ void __launch_bounds__(kThreads) pointwise_fill_nan_kernel(double *out, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < count) out[k] = __builtin_nan("");
}

// the Bernoulli family: observation i takes the values of its x (two[d][0] for x = 1, two[d][1] for x = 0), `width` doubles each; an invalid x_i has the term -inf in
// every draw: NaN
__global__ void __launch_bounds__(kThreads) pointwise_bern_expand_kernel(const WaicModel M, const WaicDataset *__restrict__ sets, const double *__restrict__ two, double *__restrict__ out,
                                                                         int64_t n_max, int64_t width) {
  const int d = blockIdx.y;
  const WaicDataset ds = sets[d];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= ds.n_obs) return;
  const bool invalid = M.invalid && M.invalid[ds.off_xb + i];
  const int k = M.xb[ds.off_xb + i] ? 0 : 1;
  for (int64_t t = 0; t < width; ++t) out[(d * n_max + i) * width + t] = invalid ? __builtin_nan("") : two[(d * 2 + k) * width + t];
}

}  // namespace

int amwg_pointwise_family(const char *call, const WaicModel &model, int PR, int D, PointwiseLaunch &K) {
  const int need = model.model == AMWG_MODEL_NORMAL ? 2 : model.model == AMWG_MODEL_BETA_BERN ? 1 : model.model == AMWG_MODEL_HIER_NORMAL ? model.G + 2 : model.model == AMWG_MODEL_POIS_GLM ? 9 : -1;
  if (need < 0) return amwg_fail(AMWG_EINVAL, "%s: unknown model %d", call, model.model);
  if (PR < need) return amwg_fail(AMWG_EINVAL, "%s: the family reads %d components of a draw, the draws hold %d", call, need, PR);
  if (model.model == AMWG_MODEL_HIER_NORMAL && D != 1) return amwg_fail(AMWG_EINVAL, "%s: the hierarchical family runs on one dataset", call);
  K = PointwiseLaunch{};
  K.bern = model.model == AMWG_MODEL_BETA_BERN;
  K.builtin = true;
  K.family = model;
  for (int k = 0; k < 2; ++k) { K.fn[kPwWaicPartial + k] = amwg_waic_family_fn(model.model, k); K.fn[kPwLooHist + k] = amwg_loo_family_fn(model.model, k); }
  K.fn[kPwWaicFold] = amwg_waic_family_fn(model.model, 2);
  for (int k = 0; k < 4; ++k) K.fn[kPwGrouped + k] = amwg_grouped_family_fn(model.model, k);
  return AMWG_OK;
}

int32_t amwg_group_csr(const int32_t *labels, int32_t n, std::vector<int32_t> &start, std::vector<int32_t> &member, std::vector<int32_t> &deal) {
  member.resize((size_t)n);
  std::iota(member.begin(), member.end(), 0);
  std::stable_sort(member.begin(), member.end(), [&](int32_t a, int32_t b) { return labels[a] < labels[b]; });
  start.clear();
  for (int32_t m = 0; m < n; ++m) if (m == 0 || labels[member[(size_t)m]] != labels[member[(size_t)m - 1]]) start.push_back(m);
  const int32_t G = (int32_t)start.size();
  start.push_back(n);
  deal.resize((size_t)G);
  std::iota(deal.begin(), deal.end(), 0);
  std::stable_sort(deal.begin(), deal.end(), [&](int32_t a, int32_t b) { return start[(size_t)a + 1] - start[(size_t)a] > start[(size_t)b + 1] - start[(size_t)b]; });
  return G;
}

int amwg_pointwise_labels(const char *call, const int32_t *labels) {
  return labels ? AMWG_OK : amwg_fail(AMWG_EINVAL, "%s: NULL labels: a grouped call needs a label per observation", call);
}

int amwg_pointwise_groups(const char *call, PointwiseLaunch &K, const WaicDataset *sets, int D, const int32_t *labels, hipStream_t stream, PointwiseGroups &g) {
  if (K.bern)
    return amwg_fail(AMWG_EINVAL, "%s: the Bernoulli family is served through the two values an observation can take, which does not carry over to sums over groups: "
                     "not served by the grouped calls", call);
  g.by_group.assign(sets, sets + D);
  g.gsets.assign((size_t)D, GroupSet{});
  g.csr.clear();
  std::vector<int32_t> start, member, deal;
  for (int d = 0; d < D; ++d) {
    const int32_t n = sets[d].n_obs;
    if (n < 0) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: n_obs < 0", call, d);
    const int32_t G = amwg_group_csr(labels, n, start, member, deal);
    GroupSet &gs = g.gsets[(size_t)d];
    gs.G = G;
    gs.at_start = (int64_t)g.csr.size(); g.csr.insert(g.csr.end(), start.begin(), start.end());
    gs.at_member = (int64_t)g.csr.size(); g.csr.insert(g.csr.end(), member.begin(), member.end());
    gs.at_deal = (int64_t)g.csr.size(); g.csr.insert(g.csr.end(), deal.begin(), deal.end());
    g.by_group[(size_t)d].n_obs = G;
    labels += n;
  }
  HIP_TRY(g.d_sets.alloc((size_t)D * sizeof(WaicDataset)));
  HIP_TRY(g.d_gsets.alloc((size_t)D * sizeof(GroupSet)));
  HIP_TRY(g.d_csr.alloc(g.csr.size() * 4));
  HIP_TRY(hipMemcpyAsync(g.d_sets.p, sets, (size_t)D * sizeof(WaicDataset), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(g.d_gsets.p, g.gsets.data(), (size_t)D * sizeof(GroupSet), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(g.d_csr.p, g.csr.data(), g.csr.size() * 4, hipMemcpyHostToDevice, stream));
  K.groups = &g;
  return AMWG_OK;
}

hipError_t amwg_pointwise_go(const PointwiseLaunch &K, int k, dim3 grid, hipStream_t stream, void **args) {
  if (K.builtin) { (void)hipLaunchKernel(K.fn[k], grid, dim3(kThreads), args, 0, stream); return hipGetLastError(); }      // (what hipLaunchKernelGGL comes to)
  return hipModuleLaunchKernel((hipFunction_t)K.fn[k], grid.x, grid.y, grid.z, kThreads, 1, 1, 0, stream, args, nullptr);
}

hipError_t amwg_pointwise_fill_nan(double *out, int64_t count, hipStream_t stream) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(pointwise_fill_nan_kernel,dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, out, count);
  return hipGetLastError();
}

hipError_t amwg_pointwise_bern_expand(const PointwiseLaunch &K, const WaicDataset *d_sets, int D, const double *two, double *out, int64_t n_max, int64_t width, hipStream_t stream) {
  hipLaunchKernelGGL(pointwise_bern_expand_kernel, dim3((unsigned)((n_max + kThreads - 1) / kThreads), (unsigned)D), dim3(kThreads), 0, stream, K.family, d_sets, two, out, n_max, width);
  return hipGetLastError();
}

PointwisePlan amwg_pointwise_plan(const PointwiseLaunch &K, const WaicDataset *sets, int D, int64_t S, size_t obs_bytes, size_t part_bytes, size_t scratch_bytes) {
  const size_t budget = scratch_bytes ? scratch_bytes : kPointwiseScratchBytes;
  PointwisePlan p;
  p.off.assign((size_t)D * 2, 0);
  PointwiseBatch b{0, 0, 0, 0, 0, 0};
  size_t in_batch = 0;
  int64_t prt = 0;
  for (int d = 0; d < D; ++d) {
    const int64_t n = K.bern ? (sets[d].n_obs > 0 ? 2 : 0) : sets[d].n_obs, t = (n + kTile - 1) / kTile, sp = waic_splits(S, n), np = sp * n;
    const size_t bytes = (size_t)n * obs_bytes + (size_t)np * part_bytes;
    if (in_batch && in_batch + bytes > budget) { b.d1 = d; p.batches.push_back(b); b = PointwiseBatch{d, d, 0, 0, 0, 0}; in_batch = 0; prt = 0; }
    p.off[(size_t)d] = b.obs; p.off[(size_t)D + (size_t)d] = prt;
    in_batch += bytes; b.obs += n; prt += np;
    b.tiles = t > b.tiles ? t : b.tiles; b.splits = sp > b.splits ? sp : b.splits; b.n_most = n > b.n_most ? n : b.n_most;
    p.most_obs = b.obs > p.most_obs ? b.obs : p.most_obs; p.most_parts = prt > p.most_parts ? prt : p.most_parts;
  }
  b.d1 = D;
  p.batches.push_back(b);
  return p;
}

int amwg_pointwise_begin(const char *call, const WaicDataset *sets, int D, int64_t extra_per_obs, hipStream_t stream, PointwiseOut &o) {
  for (int d = 0; d < D; ++d) {
    if (sets[d].n_obs < 0) return amwg_fail(AMWG_EINVAL, "%s: dataset %d: n_obs < 0", call, d);
    o.n_max = sets[d].n_obs > o.n_max ? sets[d].n_obs : o.n_max;
  }
  o.pw_count = (size_t)D * (size_t)o.n_max * 2;
  o.extra_count = (size_t)D * (size_t)o.n_max * (size_t)extra_per_obs;
  HIP_TRY(o.sets.alloc((size_t)D * sizeof(WaicDataset)));
  HIP_TRY(hipMemcpyAsync(o.sets.p, sets, (size_t)D * sizeof(WaicDataset), hipMemcpyHostToDevice, stream));
  HIP_TRY(o.pw.alloc(o.pw_count * 8));
  HIP_TRY(amwg_pointwise_fill_nan(o.pw.as<double>(), (int64_t)o.pw_count, stream));
  if (extra_per_obs) {
    HIP_TRY(o.extra.alloc(o.extra_count * 8));
    HIP_TRY(amwg_pointwise_fill_nan(o.extra.as<double>(), (int64_t)o.extra_count, stream));
  }
  return AMWG_OK;
}

int amwg_pointwise_fetch(const PointwiseOut &o, double *pw, double *extra) {
  if (o.pw_count) HIP_TRY(hipMemcpy(pw, o.pw.p, o.pw_count * 8, hipMemcpyDeviceToHost));
  if (o.extra_count) HIP_TRY(hipMemcpy(extra, o.extra.p, o.extra_count * 8, hipMemcpyDeviceToHost));
  return AMWG_OK;
}

// the sampler's datasets and family as the launchers take them; the sampler's device is current
int amwg_waic_describe(amwg_sampler *s, std::vector<WaicDataset> &sets, WaicModel &m) {
  const int D = s->n_datasets;
  sets.assign((size_t)D, WaicDataset{});
  if (D == 1) {
    sets[0] = WaicDataset{s->ds_n_obs.empty() ? s->d.n_obs : s->ds_n_obs[0], s->mc.data_mid_range, 0, 0, 0, 0};
  } else {
    std::vector<DatasetConsts> consts((size_t)D);
    HIP_TRY(hipMemcpy(consts.data(), s->d_ds_consts, (size_t)D * sizeof(DatasetConsts), hipMemcpyDeviceToHost));
    for (int d = 0; d < D; ++d) sets[(size_t)d] = WaicDataset{consts[(size_t)d].n_obs, consts[(size_t)d].data_mid_range, consts[(size_t)d].off_x, consts[(size_t)d].off_y, consts[(size_t)d].off_lfact, consts[(size_t)d].off_xb};
  }
  m.model = s->model; m.G = s->d.G; m.exact_division = s->mc.exact_division;
  m.neg_half_log_2pi = s->mc.neg_half_log_2pi;
  m.x = s->d.x; m.y = s->d.y; m.lfact = s->d.lfact; m.xb = s->d.xb;
  m.invalid = s->model == AMWG_MODEL_BETA_BERN ? static_cast<const uint8_t *>(s->d.arr[1]) : nullptr;      // (amwg_create.hip upload_bernoulli_data)
  return AMWG_OK;
}

// ... and of a closure whose pointwise text is set (amwg_set_pointwise): the code object compiled and loaded on first use (amwg_rtc.hip load_pointwise), its
// entries and its model argument; every dataset with kTermN observations
int amwg_pointwise_describe_user(amwg_sampler *s, std::vector<WaicDataset> &sets, PointwiseLaunch &K) {
  TRYB(load_pointwise(s, s->user_arch.c_str()));
  K = PointwiseLaunch{};
  for (int k = 0; k < kPwWaicFold; ++k) K.fn[k] = s->pw_fn[k];
  hipFunction_t fold = nullptr;      // (the fifth entry is looked up where it is asked for: the handle's layout stays as it is)
  HIP_TRY(hipModuleGetFunction(&fold, s->pw_module, "amwg_pw_waic_fold"));
  K.fn[kPwWaicFold] = fold;
  static const char *const kGrouped[4] = {"amwg_pw_waic_partial_grouped", "amwg_pw_waic_loglik_grouped", "amwg_pw_loo_hist_grouped", "amwg_pw_loo_compact_grouped"};
  for (int k = 0; k < 4; ++k) {
    hipFunction_t f = nullptr;
    HIP_TRY(hipModuleGetFunction(&f, s->pw_module, kGrouped[k]));
    K.fn[kPwGrouped + k] = f;
  }
  K.user.d = s->d;
  K.user.table = s->n_datasets > 1 ? s->d_user_ds_table : nullptr;
  K.user.row_stride = s->user_ds_row_stride;
  K.user.reserved = 0;
  sets.assign((size_t)s->n_datasets, WaicDataset{s->pw_n_obs, 0, 0, 0, 0, 0});
  return AMWG_OK;
}

extern "C" int amwg_set_pointwise(amwg_sampler *s, const char *terms_source) {
  static const char *call = "amwg_set_pointwise";
  if (!s || !terms_source) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (!s->user) return amwg_fail(AMWG_EINVAL, "%s: the pointwise terms of a built-in family are known to the library; the text is for amwg_create_user* samplers only", call);
  auto int_after = [&](const char *key) -> long {
    const char *q = strstr(terms_source, key);
    return q ? strtol(q + strlen(key), nullptr, 10) : -1;
  };
  const long n = int_after("kTermN = "), p = int_after("kStateN = ");
  if (!strstr(terms_source, "struct UserTerms") || n < 1 || n >= (1l << 31)) return amwg_fail(AMWG_EINVAL, "%s: the text does not define struct amwg::UserTerms with kTermN >= 1 (translate.js, options.pointwise)", call);
  if (p != s->P) return amwg_fail(AMWG_EINVAL, "%s: the text was made for a state of %ld components, the sampler's has %d", call, p, s->P);
  HIP_TRY(hipSetDevice(s->device));
  if (s->pw_module) { (void)hipModuleUnload(s->pw_module); s->pw_module = nullptr; }
  s->pw_terms = terms_source;
  s->pw_n_obs = (int)n; s->pw_state_n = (int)p;
  return AMWG_OK;
}

extern "C" int64_t amwg_pointwise_n_obs(const amwg_sampler *s) { return s && s->user && !s->pw_terms.empty() ? s->pw_n_obs : 0; }

int amwg_pointwise_entry(const char *call, amwg_sampler *s, double *summary, int32_t *high, double *pointwise, PointwiseShapeFn shape, PointwiseRunFn run, bool grouped,
                         const int32_t *labels, int32_t *n_groups_out) {
  if (!s || !summary) return amwg_fail(AMWG_EINVAL, "%s: null argument", call);
  if (grouped) TRYB(amwg_pointwise_labels(call, labels));
  if (s->user && s->pw_terms.empty()) return amwg_fail(AMWG_EINVAL, "%s: the pointwise terms of a closure are not known to the library; built-in families only", call);
  TRYB(amwg_need_stored_draws(s, call));
  const int D = s->n_datasets, PR = s->P + s->D;
  TRYB(shape(call, s->last_rows, PR, s->C, D));
  if (s->mc.group_local) return amwg_fail(AMWG_EINVAL, "%s: a group_local sampler keeps its observations as a lane-major tile; the pointwise terms need them in index order", call);
  HIP_TRY(hipSetDevice(s->device));
  std::vector<WaicDataset> sets;
  PointwiseLaunch K;
  if (s->user) {
    TRYB(amwg_pointwise_describe_user(s, sets, K));
  } else {
    WaicModel m{};
    TRYB(amwg_waic_describe(s, sets, m));
    TRYB(amwg_pointwise_family(call, m, PR, D, K));
  }
  if (!grouped) return run(call, s->last_draws, s->last_rows, PR, s->C, D, K, sets.data(), summary, high, pointwise, nullptr, 0, s->stream);
  PointwiseGroups groups;
  TRYB(amwg_pointwise_groups(call, K, sets.data(), D, labels, s->stream, groups));
  if (n_groups_out) for (int d = 0; d < D; ++d) n_groups_out[d] = groups.gsets[(size_t)d].G;
  return run(call, s->last_draws, s->last_rows, PR, s->C, D, K, groups.by_group.data(), summary, high, pointwise, nullptr, 0, s->stream);
}
