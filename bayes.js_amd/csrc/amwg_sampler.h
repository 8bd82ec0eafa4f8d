// amwg_sampler.h -- the sampler handle behind the C ABI (internal to libamwg.so; shared by the host units -- amwg_host.h --,
// amwg_summaries.hip and amwg_group.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/amwg.h"
#include "amwg_types.h"

typedef void (*step_kernel_t)(const amwg::StepArgs);
namespace amwg { struct DatasetArgs; struct DatasetConsts; }
typedef void (*dataset_kernel_t)(const amwg::StepArgs, const amwg::DatasetArgs);      // a dataset twin (amwg_dataset.h)

// The step kernel a sampler launches.  The variant fixes the LDS data layout, DataRef::pad, the kernel's name and whether it decides from certified
// values (amwg_plan.hip: variant_for decides it, kVariants describes it).
enum class Variant : uint8_t {
  Step, StepCert, HierSweep, HierSweepCert, GroupLocal,              // built-in families (amwg_kernels.hip)
  UserStep, UserStepCert, UserSweep, UserSweepCert                   // translated closures (amwg_user_kernels.h)
};
// One launch geometry and the kernel that runs it.  cpb: chains per workgroup if fewer than block / lanes (StepArgs::cpb); pad: DataRef::pad for this
// variant (the group-local row count, the Normal family's one-lane tile flag, or the row pitch of the row layout; 0 = none)
struct LaunchPlan {
  int lanes = 0, block = 0, grid = 0, lds = 0, cpb = 0;
  Variant variant = Variant::Step;
  int pad = 0;
};

struct amwg_sampler {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int model = 0, P = 0, n_params = 0;
  int64_t C = 0;
  amwg_options opt{};
  amwg::ParamLayout pl{};
  amwg::ModelConsts mc{};
  amwg::DataRef d{};
  amwg::ChainArrays ch{};
  std::vector<void *> dev_allocs;
  amwg::CompConst *d_cc = nullptr;
  uint8_t *d_adapt = nullptr;
  std::vector<uint8_t> h_adapt;
  std::vector<int32_t> h_layout;   // [4][n_params] base | len | top | multidim (ParamLayout::tab on the device)
  LaunchPlan plan;                  // geometry and kernel (adopt_plan)
  step_kernel_t kernel = nullptr;   // the built-in kernel of plan.variant
  // many datasets in one sampler (amwg_create_datasets; amwg_dataset.h): D > 1 datasets of cpd = C / D chains each, the kernel's second argument as far as it
  // is fixed at construction (blocks_per_dataset follows the plan: adopt_plan), and the twin that takes it
  int n_datasets = 1;
  std::vector<int32_t> ds_n_obs;                  // n_obs of every dataset (a built-in family; D == 1: the one size).  With D > 1, d.n_obs is the LARGEST of them
  amwg::DatasetConsts *d_ds_consts = nullptr;
  int ds_blocks_per_dataset = 0;
  dataset_kernel_t ds_kernel = nullptr;
  // ... of a translated closure (amwg_create_user_datasets; amwg_user_dataset.h): the device table [n_datasets][row_stride] of the datasets' arrays
  const void *const *d_user_ds_table = nullptr;
  int user_ds_row_stride = 0, user_ds_n_arrays = 0;
  int gl_rounds = 0;                // group_local: rows of the lane-major tile (GlLayoutHost::rounds; the group-local kernel's DataRef::pad)
  std::string kernel_name;          // amwg_kernel_name(): filled on first request
  uint32_t hier_periodic_mask = 0;   // HIER: bit j set = the group labels repeat with a lane stride of 2^j (g[i] == g[i mod 2^j])
  bool lp_ready = false;
  bool lp_is_expression = true;      // ch.lp_curr holds the expression's value for every chain (false after steps of a kernel with certified decisions, until a finalize launch)
  std::vector<std::pair<int, float>> tuned;   // AMWG_LANES_AUTOTUNE: (lanes per chain, ms of the timing run) of every candidate
  // translated closure (amwg_create_user): hiprtc module function instead of a built-in kernel
  bool user = false;
  int D = 0;                       // derived quantities recorded after the P components
  int user_lds = 0, user_lds_one_lane = 0, user_parallel = 0, user_max_threads = 1024;
  int user_rows_n = 0, user_rows_groups = 0, user_rows_sweep = 0;   // row plan of a translated closure (amwg_rows.h): observations and groups of its final likelihood loop; 0 = none
  bool user_rows_cert = false;     // the row plan has certified values (kRowCert of the generated source: amwg_rows.h log_post_approx / sweep_approx / reference_order)
  int user_cert_tail_n = 0;        // certified tail of a translated closure (amwg_user.h norm_tail_approx): observations of its final constant-mean normal loop (kTailN of the generated source); 0 = none
  int user_pois_tail_n = 0;        // certified Poisson tail of a translated closure (amwg_gtail.h glm_tail_approx<PoisLink>): observations of its final log-link Poisson loop (kPoisTail / kTailN of the generated source); 0 = none
  int user_logit_tail_n = 0;       // certified logistic tail of a translated closure (amwg_gtail.h glm_tail_approx<LogitLink>): observations of its final logistic-regression loop (kLogitTail / kTailN of the generated source); 0 = none
  bool user_has_binary = false;    // the model has binary parameters
  double user_work = 0;            // translator's estimate of the instructions of one log_post evaluation
  double user_work_one_lane = 0;   // the same with one lane per chain when that enables a fast-forwarded sum (0 = n/a)
  hipFunction_t user_fn = nullptr;
  hipModule_t user_module = nullptr;
  // ... its pointwise terms (amwg_set_pointwise; amwg_pointwise.h): the closure's source and the terms text as given, the architecture of the device, and the code
  // object of the four kernels that evaluate them, compiled and loaded at the first call that needs it (amwg_rtc.hip load_pointwise)
  std::string user_source, user_arch, pw_terms;
  int pw_n_obs = 0, pw_state_n = 0;      // kTermN, kStateN of the terms text
  hipModule_t pw_module = nullptr;
  hipFunction_t pw_fn[4] = {nullptr, nullptr, nullptr, nullptr};      // the entries of amwg_pointwise.h, in its order
  // last call
  int n_launches = 0;
  double kernel_ms = 0.0;
  double *d_draws = nullptr;       // library-owned draw buffer of the last amwg_sample
  size_t d_draws_cap = 0;
  const double *last_draws = nullptr;  // device pointer (library- or caller-owned) of the last sample call
  int64_t last_rows = 0;
  // rows of the last sample call become final launch by launch: an event after each launch and the row count up to it, so that
  // amwg_fetch_draws* copies the rows of launch j on copy_stream while launches j + 1, ... still run
  std::vector<hipEvent_t> chunk_ev;
  std::vector<int64_t> chunk_rows;     // cumulative rows after launch j of the last sample call
  hipStream_t copy_stream = nullptr;
};

// shared helper (amwg_diag.hip): records an error message for amwg_last_error() and returns `code`
int amwg_fail(int code, const char *fmt, ...);
// shared helper (amwg_diag.hip): AMWG_EINVAL with a message that points to the per-dataset calls when `s` is a dataset sampler (amwg_create_datasets), else AMWG_OK
int amwg_refuse_pooled(const amwg_sampler *s, const char *call);
