// amwg_host.h -- what the host units of libamwg.so share (amwg_plan.hip, amwg_rtc.hip, amwg_create.hip, amwg_run.hip, amwg_diag.hip and, in the
// test library, amwg_selftest.hip).  Host only and free of the device headers: a unit that needs amwg_kernel.h / amwg_models.h includes them itself.
// Nothing declared here leaves the shared object (hidden visibility); the C ABI is include/amwg.h.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/amwg.h"
#include "amwg_sampler.h"

// the hierarchical family's two kernels beside its row (amwg_kernels.hip)
step_kernel_t amwg_kernel_hier_gl(int block);      // the group-local kernel (amwg_gl.h)
step_kernel_t amwg_kernel_hier_sweep(int block);   // the kernel with the sweep prefetch (row layout, 64 lanes per chain)

#pragma GCC visibility push(hidden)

// ---- errors: amwg_fail (amwg_sampler.h) records the message of amwg_last_error() in g_err and returns the code
extern thread_local std::string g_err;
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return amwg_fail(AMWG_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
#define TRYB(x) do { int rc_ = (x); if (rc_ != AMWG_OK) return rc_; } while (0)
// scratch device buffer of the helper entry points: freed on every exit path
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
  template <class T> T *as() const { return static_cast<T *>(p); }
};
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
// device memory that lives as long as the sampler (amwg_destroy frees dev_allocs)
template <class T>
int dev_alloc(amwg_sampler *s, T **p, size_t n) {
  void *q = nullptr;
  HIP_TRY(hipMalloc(&q, n * sizeof(T) ? n * sizeof(T) : 1));
  s->dev_allocs.push_back(q);
  *p = static_cast<T *>(q);
  return AMWG_OK;
}

// ---- amwg_kernels.hip: a built-in family is one row of facts, exported by the family's own translation unit (AMWG_FAMILY = AMWG_MODEL_* - 1)
struct KernelPair { step_kernel_t plain = nullptr; dataset_kernel_t ds = nullptr; };      // a kernel and its dataset twin (amwg_dataset.h); nullptr: none
struct FamilyRow {
  KernelPair (*kernel)(int lanes, int block), (*certified)(int lanes, int block);      // the step kernel of a geometry, and the one that decides from certified values (kCert)
  size_t (*lds_bytes)(int n_obs, int groups, int lanes);      // LDS bytes of the data the family stages
  int max_threads;                                            // the family's largest workgroup
};
template <int Family> FamilyRow amwg_family_row();

// ---- amwg_plan.hip: the launch plan
const FamilyRow *family_of(int model);      // the row of AMWG_MODEL_*; nullptr: no such family
struct VariantInfo { const char *name; bool certified; };
const VariantInfo &info(Variant v);
namespace amwg { struct GlLane; }
struct GlLayoutHost {      // group-local evaluation (amwg_gl.h): the lane-major tile and the table of the wavefront's 64 lanes
  std::vector<double> tile;
  std::vector<amwg::GlLane> lane;
  int rounds = 0, n_min = 0;
};
int gl_layout(const double *y, const int32_t *g, int N, int Gn, GlLayoutHost *out);
size_t wave_scratch_lines(const amwg_sampler *s);
int choose_geometry(const amwg_sampler *s, int lanes, int n_cus, size_t max_lds, LaunchPlan *out);
int adopt_plan(amwg_sampler *s, const LaunchPlan &p);
int autotune_geometry(amwg_sampler *s, int n_cus, size_t max_lds, const std::function<int()> &prepare);

// ---- amwg_rtc.hip: what the generated source of a translated closure states about itself; compile (hiprtc, cached) and load of the kernel of s->plan
struct SourceTraits { long row_n, row_groups; bool row_sweep, row_cert; int cert_tail_n, pois_tail_n, logit_tail_n; bool tail_per_dataset; };
SourceTraits source_traits(const char *src);
int load_user_kernel(amwg_sampler *s, const char *source, const char *arch);
int load_pointwise(amwg_sampler *s, const char *arch);      // the code object of amwg_set_pointwise's text on the sampler's device (once)

// ---- amwg_create.hip: every array a closure reads on the sampler's device, in its storage type, and the table of a dataset sampler (also the check library's)
int upload_user_arrays(amwg_sampler *s, const amwg_user_model *models, int D);
// ---- amwg_create.hip (the tables of two_valued_sum), amwg_run.hip
std::vector<uint32_t> two_valued_tables(const uint8_t *xb, int N);
int use_device(int device);      // hipSetDevice for the helper entry points that take a device number; AMWG_EHIP where there is none
struct FoldWindow;      // (amwg_fold.h: the rows are folded window by window instead of kept -- amwg_sample_summarize)
int launch_steps(amwg_sampler *s, int64_t n, int64_t thin, double *d_draws, bool finalize = false, FoldWindow *win = nullptr);
int finish_timing(amwg_sampler *s);
// Makes the destination of a sample call resident ahead of the device-to-host copies: helper threads walk it in copy order (amwg_run.hip)
struct Prefaulter {
  struct Piece { char *p; size_t bytes; size_t chunk; };
  std::vector<Piece> pieces;              // in copy order
  std::vector<std::thread> workers;
  std::atomic<size_t> next{0};
  std::vector<std::atomic<int>> done;     // pieces finished per chunk
  std::vector<int> per_chunk;
  explicit Prefaulter(size_t n_chunks);
  void add(char *p, size_t bytes, size_t chunk);
  void start(int n_threads);
  void wait_chunk(size_t j);      // (the caller helps instead of idling: it takes pieces too)
  ~Prefaulter();
};
#pragma GCC visibility pop
