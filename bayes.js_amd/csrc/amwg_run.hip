// amwg_run.hip -- running a sampler: the launch loop (launch_steps) and what a call leaves behind (finish_timing), burn / sample / sync, the
// overlapped fetch of the recorded draws with its prefaulter, the chains' state in and out.
#include <dlfcn.h>
#include <sys/mman.h>

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <mutex>
#include <unordered_map>

#include "../../include/amwg_selftest.h"      // (amwg_audit_fetch: the audit build)
#include "amwg_autocov.h"
#include "amwg_covariance.h"
#include "amwg_fold.h"
#include "amwg_histogram.h"
#include "amwg_host.h"
#include "amwg_kernel.h"      // (StepArgs, and the kErr* bits the step kernels report)
#include "amwg_dataset.h"     // (DatasetArgs: the second argument of a dataset sampler's kernel)
#include "amwg_user_dataset.h"      // (UserDatasetArgs: the same for a translated closure)

using namespace amwg;

int use_device(int device) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1) return amwg_fail(AMWG_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
  HIP_TRY(hipSetDevice(device));
  return AMWG_OK;
}

// Optional tracing: roctx ranges around every burn/sample call, visible to `rocprofv3 --marker-trace`.
// the roctx library is looked up at run time; without it (or with AMWG_ROCTX=0) these are no-ops.
namespace {
struct Roctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char *env = getenv("AMWG_ROCTX");
    if (env && env[0] == '0') return;
    void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_GLOBAL);   // ROCm 7
    if (!h) h = dlopen("libroctx64.so", RTLD_LAZY | RTLD_GLOBAL);               // older ROCm
    if (h) {
      push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
      pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (!push || !pop) push = nullptr, pop = nullptr;
    }
  }
};
Roctx &roctx() { static Roctx r; return r; }
}  // namespace

// `win` (amwg_sample_summarize): d_draws holds win->window_rows rows only.  A launch never records past the end of the window -- its steps are capped to the rows
// left x thin, step0 / row0 as ever --, and each time the window is full, and again at the end of the call, its rows are folded into win->acc (amwg_fold.h) on the
// same stream and the window is reused: no host synchronisation in between, and the call's launch count and event pair span all of it.
int launch_steps(amwg_sampler *s, int64_t n, int64_t thin, double *d_draws, bool finalize, FoldWindow *win) {
  Roctx &rx = roctx();
  if (rx.push) rx.push(d_draws ? "amwg_sample" : "amwg_burn");
  struct PopOnExit { Roctx &r; ~PopOnExit() { if (r.pop) r.pop(); } } pop_on_exit{rx};
  // a launch counts its accepted / evaluated proposals in 16-bit fields (amwg_kernel.h, TOTme): at most 65535 steps per launch
  int64_t chunk = (s->opt.steps_per_launch > 0 && s->opt.steps_per_launch < 65535) ? s->opt.steps_per_launch : 65535;
  if (win && (!d_draws || win->window_rows < 1 || !win->acc)) return amwg_fail(AMWG_EINVAL, "internal: a fold window of %lld rows", (long long)win->window_rows);
  if (d_draws && d_draws == s->d_draws && s->opt.steps_per_launch <= 0 && !win) {
    // draws that will be fetched (amwg_sample / amwg_sample_async): launches of ~32 MB of recorded rows each, so that the rows of one launch
    // leave the device while the next launches run (amwg_fetch_draws_slices); results do not depend on how a call is cut into launches
    const double per_step = (double)(s->P + s->D) * (double)s->C * 8.0 / (double)thin;
    const double steps = 33554432.0 / (per_step > 0 ? per_step : 1.0);
    if (steps < (double)chunk) chunk = steps < 16.0 ? 16 : (int64_t)steps;
  }
  // the invariants the kernel relies on, enforced where the launch is made (the kernel's own guards -- device_error -- are the backstop)
  const LaunchPlan &p = s->plan;
  if (p.cpb > 0 && p.block != 64) return amwg_fail(AMWG_EINVAL, "internal: %d chains per workgroup of %d threads (replicated chains need one-wavefront workgroups)", p.cpb, p.block);
  if (p.lanes == 1 && s->d.wave_scratch && wave_scratch_lines(s) < (size_t)p.grid * (size_t)(p.block / 64))
    return amwg_fail(AMWG_EINVAL, "internal: a wave scratch of %zu lines for %d workgroups of %d threads (one line per wavefront)", wave_scratch_lines(s), p.grid, p.block);
  if (chunk > 65535) return amwg_fail(AMWG_EINVAL, "internal: launches of %lld steps (at most 65535)", (long long)chunk);
  StepArgs a{};
  a.C = s->C;
  a.seed = s->opt.seed;
  a.chain_offset = s->opt.chain_offset;
  a.thin = (int32_t)thin;
  a.draws = d_draws;
  a.cc = s->d_cc;
  a.is_adapting = s->d_adapt;
  a.pl = s->pl;
  a.cpb = p.cpb;
  a.sweep_update_by_update = s->opt.full_evaluation == 2 ? 1 : 0;
  a.certified = info(p.variant).certified ? 1 : 0;      // (informational: certified decisions are the kernel's, not a switch inside it)
  a.bound_scale = std::ldexp(1.0, s->opt.test_bound_shift);
  a.audit_adversarial = 0;
#if defined(AMWG_AUDIT)
  { const char *e = getenv("AMWG_AUDIT_ADVERSARIAL"); a.audit_adversarial = (e && e[0] == '1') ? 1 : 0; }
#endif
  a.mc = s->mc;
  a.d = s->d;
  if (p.lanes != 1) a.d.wave_scratch = nullptr;      // (sized for one-lane geometries only; no other kernel reads it)
  a.ch = s->ch;
  DatasetArgs ds{};      // (a dataset sampler: which workgroups serve which dataset, and where its data and constants lie)
  if (s->n_datasets > 1 && !s->user) {
    if (!s->ds_kernel || s->ds_blocks_per_dataset < 1 || (int64_t)s->ds_blocks_per_dataset * s->n_datasets != p.grid)
      return amwg_fail(AMWG_EINVAL, "internal: %d workgroups for %d datasets of %d workgroups each", p.grid, s->n_datasets, s->ds_blocks_per_dataset);
    ds.blocks_per_dataset = s->ds_blocks_per_dataset;
    ds.n_datasets = s->n_datasets;
    ds.consts = s->d_ds_consts;
  }
  // (a closure on many datasets: StepArgs and UserDatasetArgs, in that order, are the twin's argument buffer)
  struct { StepArgs a; UserDatasetArgs ds; } ua{};
  static_assert(offsetof(decltype(ua), ds) == sizeof(StepArgs) && sizeof(StepArgs) % alignof(UserDatasetArgs) == 0, "the second kernel argument follows the first without padding");
  if (s->n_datasets > 1 && s->user) {
    if (!s->d_user_ds_table || s->ds_blocks_per_dataset < 1 || (int64_t)s->ds_blocks_per_dataset * s->n_datasets != p.grid || s->user_ds_row_stride < kInlineUserArrays)
      return amwg_fail(AMWG_EINVAL, "internal: %d workgroups for %d datasets of %d workgroups each (closure; table rows of %d entries)", p.grid, s->n_datasets, s->ds_blocks_per_dataset, s->user_ds_row_stride);
    ua.ds.blocks_per_dataset = s->ds_blocks_per_dataset;
    ua.ds.n_datasets = s->n_datasets;
    ua.ds.row_stride = s->user_ds_row_stride;
    ua.ds.n_arrays = s->user_ds_n_arrays;
    ua.ds.table = s->d_user_ds_table;
  }
  // (a 0-step finalize launch on chains that have stepped -- amwg_chain_diag asking for the expression's value after a certified kernel ran -- is not "the latest call":
  // the sample call's launch count, its per-launch marks and its event pair stay, so that a diag() between sample_async and fetch_draws neither loses the copy overlap
  // nor replaces the call's kernel time with its own; round-5 advisor finding)
  const bool quiet = finalize && n == 0 && s->lp_ready;
  if (!quiet) {
    s->n_launches = 0;
    s->chunk_rows.clear();
    HIP_TRY(hipEventRecord(s->ev0, s->stream));
  }
  int64_t done = 0, row = 0, folded = 0;      // (with a window: `row` counts the rows in the window, `folded` those of the windows before it)
  do {
    int64_t m = (n - done < chunk) ? n - done : chunk;
    a.init_lp = s->lp_ready ? 0 : 1;
    a.finalize_lp = finalize ? 1 : 0;
    // steps until the first recorded step of this launch: smallest t >= 0 with (done + t) % thin == 0
    a.step0 = (thin - (done % thin)) % thin;
    a.row0 = row;
    if (win && m > a.step0 + (win->window_rows - row) * thin) m = a.step0 + (win->window_rows - row) * thin;      // (the window has room for >= 1 row: m >= 1)
    a.n_steps = (int32_t)m;
    if (s->user) {
      size_t arg_bytes = sizeof a;
      void *arg_buf = &a;
      if (s->n_datasets > 1) { ua.a = a; arg_buf = &ua; arg_bytes = sizeof ua; }
      void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, arg_buf, HIP_LAUNCH_PARAM_BUFFER_SIZE, &arg_bytes, HIP_LAUNCH_PARAM_END};
      HIP_TRY(hipModuleLaunchKernel(s->user_fn, (unsigned)p.grid, 1, 1, (unsigned)p.block, 1, 1, (unsigned)p.lds, s->stream, nullptr, extra));
    } else if (s->n_datasets > 1) {
      hipLaunchKernelGGL(s->ds_kernel, dim3(p.grid), dim3(p.block), (size_t)p.lds, s->stream, a, ds);
      HIP_TRY(hipGetLastError());
    } else {
      hipLaunchKernelGGL(s->kernel, dim3(p.grid), dim3(p.block), (size_t)p.lds, s->stream, a);
      HIP_TRY(hipGetLastError());
    }
    s->lp_ready = true;
    if (finalize || a.init_lp) s->lp_is_expression = true;                        // (the launch began / ends with the expression)
    if (m > 0 && !finalize && info(p.variant).certified) s->lp_is_expression = false;      // (it may have left the stepper's cheaper value and its bound behind)
    if (!quiet) s->n_launches++;
    if (d_draws) row += (m > a.step0) ? (m - a.step0 + thin - 1) / thin : 0;
    // a mark for amwg_fetch_draws*: only for the library's own buffer, and only once >= 8 MB of new rows (or the end of the call) stand
    // behind it -- a caller who asks for one-step launches gets a handful of events, not one per launch
    const int64_t marked = s->chunk_rows.empty() ? 0 : s->chunk_rows.back();
    if (!win && d_draws && d_draws == s->d_draws && row > marked &&
        (done + m >= n || (double)(row - marked) * (double)(s->P + s->D) * (double)s->C * 8.0 >= 8388608.0)) {
      const size_t j = s->chunk_rows.size();
      if (j >= s->chunk_ev.size()) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        s->chunk_ev.push_back(e);
      }
      HIP_TRY(hipEventRecord(s->chunk_ev[j], s->stream));
      s->chunk_rows.push_back(row);
    }
    done += m;
    if (win && row > 0 && (row == win->window_rows || done >= n)) {
      if (row > win->window_rows || folded + row > win->total_rows) return amwg_fail(AMWG_EINVAL, "internal: %lld rows in a window of %lld (%lld of %lld folded)", (long long)row, (long long)win->window_rows, (long long)folded, (long long)win->total_rows);
      if (win->cov)      // (reads acc[4] as the fold of the window before left it: the running means its rows start from)
        TRYB(amwg_comoment_window(d_draws, folded, row, s->P + s->D, s->C, win->cov->d_values, win->cov->n_values, win->acc, win->cov->d_co, s->stream));
      TRYB(amwg_fold_window(d_draws, folded, row, win->total_rows / 2, s->P + s->D, s->C, win->acc, s->stream));
      if (win->hist)      // (the same rows once more, on the same stream: the counts add up over the windows)
        TRYB(amwg_histogram_launch("amwg_sample_summarize", d_draws, row, s->P + s->D, s->C, s->n_datasets, win->hist->d_edges, win->hist->bins, win->hist->uniform, win->hist->d_counts, s->stream));
      if (win->acf)       // (the lag sums read the ring as the windows before left it; the carry kernel behind them, on the same stream, moves it on)
        TRYB(amwg_autocov_window(d_draws, folded, row, s->P + s->D, s->C, win->acf->d_values, win->acf->n_values, win->acf->max_lag, win->acf->d_state, s->stream));
      win->windows++;
      folded += row;
      row = 0;
    }
  } while (done < n);
  if (!quiet) HIP_TRY(hipEventRecord(s->ev1, s->stream));
  return AMWG_OK;
}

int finish_timing(amwg_sampler *s) {
  HIP_TRY(hipEventSynchronize(s->ev1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
  s->kernel_ms = ms;
  // what the step kernels had to say (amwg_kernel.h device_error): a launch that refused itself, or a register mirror that no longer
  // equals the state it mirrors, is an error of this call -- not a successful no-op
  if (s->ch.error) {
    int32_t bits = 0;
    HIP_TRY(hipMemcpy(&bits, s->ch.error, sizeof bits, hipMemcpyDeviceToHost));
    if (bits) {
      HIP_TRY(hipMemset(s->ch.error, 0, sizeof bits));
      return amwg_fail(AMWG_EHIP, "the step kernel reported an internal error (bits %d:%s%s%s%s%s%s): the chains' state is not to be trusted", bits,
                       (bits & kErrReplicasNeedOneWave) ? " replicated chains in a workgroup of more than one wavefront" : "",
                       (bits & kErrLaunchTooLong) ? " more than 65535 steps in one launch" : "",
                       (bits & kErrMirrorOutOfSync) ? " the register mirror of the state is out of sync with the state" : "",
                       (bits & kErrSweepNeedsOrderInRegisters) ? " the sweep kernel was launched for a parameter vector of more than 64 entries" : "",
                       (bits & kErrNoKernelBody) ? " the launched kernel has no body for this closure at this geometry" : "",
                       (bits & kErrLeanShape) ? " the Normal family's one-lane stepper was launched for something other than two scalar parameters of real or int type" : "");
    }
  }
  return AMWG_OK;
}

// Makes the pages of [p, p + bytes) resident without changing a byte.  A freshly allocated typed array / numpy array is untouched virtual memory, and a copy from the
// device into it runs at the speed the pages can be faulted in, not at the link's: measured on the GPU box (tools/ubench/pinned_copy.hip, 1 GiB) 9.8 GB/s into
// untouched pageable memory against 56 GB/s into the same memory once resident (pinning it first buys nothing more: 57 GB/s, and hipHostRegister / hipHostMalloc
// of a gigabyte cost 55-170 ms themselves).  Round 5 touched the pages with ONE thread -- ~6 GB/s, slower than the kernels produce rows at cfg2 (10 GB/s): sample()
// took three times its kernels' time.  Now: transparent huge pages are asked for (512 times fewer faults where the host grants them), the kernel is asked to populate
// the range in one call (MADV_POPULATE_WRITE, Linux 5.14), and where that is not available the pages are touched -- a write of the value just read.
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
static void prefault(char *p, size_t bytes) {
  if (!p || !bytes) return;
  const size_t page = 4096;
  const uintptr_t a0 = ((uintptr_t)p + page - 1) & ~(uintptr_t)(page - 1), a1 = ((uintptr_t)p + bytes) & ~(uintptr_t)(page - 1);
  if (a1 > a0 && madvise(reinterpret_cast<void *>(a0), a1 - a0, MADV_POPULATE_WRITE) == 0) {
    volatile char *q = p;
    q[0] = q[0];
    q[bytes - 1] = q[bytes - 1];      // (the partial pages at either end)
    return;
  }
  volatile char *q = p;
  for (size_t o = 0; o < bytes; o += page) q[o] = q[o];
  q[bytes - 1] = q[bytes - 1];
}
// ... by a few helper threads that run AHEAD of the copies: the rows of a sample call leave the device launch by launch (below), and the destination of launch j's rows must
// be resident when its kernel ends.  The helpers walk the destination in the order the copies will (chunk by chunk, slice by slice) and publish how far they are.
Prefaulter::Prefaulter(size_t n_chunks) : done(n_chunks), per_chunk(n_chunks, 0) { for (auto &d : done) d.store(0); }
void Prefaulter::add(char *p, size_t bytes, size_t chunk) {
  const size_t step = (size_t)8 << 20;      // 8 MB pieces: several helpers share one chunk's range
  for (size_t o = 0; o < bytes; o += step) { pieces.push_back({p + o, bytes - o < step ? bytes - o : step, chunk}); per_chunk[chunk]++; }
}
void Prefaulter::start(int n_threads) {
  for (int t = 0; t < n_threads; ++t)
    workers.emplace_back([this] {
      for (;;) {
        const size_t i = next.fetch_add(1);
        if (i >= pieces.size()) return;
        prefault(pieces[i].p, pieces[i].bytes);
        done[pieces[i].chunk].fetch_add(1, std::memory_order_release);
      }
    });
}
void Prefaulter::wait_chunk(size_t j) {
  while (done[j].load(std::memory_order_acquire) < per_chunk[j]) {
    const size_t i = next.fetch_add(1);
    if (i < pieces.size()) { prefault(pieces[i].p, pieces[i].bytes); done[pieces[i].chunk].fetch_add(1, std::memory_order_release); }
    else std::this_thread::yield();
  }
}
Prefaulter::~Prefaulter() { for (auto &w : workers) w.join(); }

// ---- amwg_fold.h: what a summarising call left behind, per sampler.  Kept beside the handle, not in it: amwg_sampler.h is one of the sources the step kernels'
// id is formed from (tools/build_id.py), and this feature changes no step kernel.  The accumulators themselves are the sampler's (dev_allocs); amwg_destroy forgets the entry.
namespace {
std::mutex g_summaries_mu;
std::unordered_map<const amwg_sampler *, FoldSummary> g_summaries;
FoldSummary &summary_slot(const amwg_sampler *s) {      // (references into an unordered_map stay valid while other entries come and go)
  std::lock_guard<std::mutex> lock(g_summaries_mu);
  return g_summaries[s];
}
}  // namespace
bool amwg_summarised(const amwg_sampler *s) { return s && !s->last_draws && s->last_rows > 0; }
const FoldSummary *amwg_summary_of(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_summaries_mu);
  auto it = g_summaries.find(s);
  return it == g_summaries.end() ? nullptr : &it->second;
}
void amwg_summary_forget(const amwg_sampler *s) {
  std::lock_guard<std::mutex> lock(g_summaries_mu);
  g_summaries.erase(s);
}
int amwg_refuse_summarised(const amwg_sampler *s, const char *call) {
  if (amwg_summarised(s))
    return amwg_fail(AMWG_EINVAL, "%s: the last sample call was amwg_sample_summarize: its draws were folded into per-chain accumulators and not kept (moments and diagnostics answer from those; this call needs the draws of amwg_sample*)", call);
  return AMWG_OK;
}

// The rows of a sample call are final launch by launch (launch_steps records an event after each): the rows of launch j leave the
// device on copy_stream while launches j + 1, ... run on the sampler's stream -- a pageable destination (a JavaScript typed array, a numpy
// array) makes each copy block THIS thread, not the GPU.  65 536 chains x 1000 draws x 2 components are 1.05 GB: with the destination resident
// in time (Prefaulter) they leave at the link's rate behind the kernels that produce them.
extern "C" {

int amwg_burn_async(amwg_sampler *s, int64_t n) {
  if (!s || n < 0) return amwg_fail(AMWG_EINVAL, "amwg_burn: bad argument");
  HIP_TRY(hipSetDevice(s->device));
  return launch_steps(s, n, 1, nullptr);
}

int amwg_burn(amwg_sampler *s, int64_t n) {
  TRYB(amwg_burn_async(s, n));
  return finish_timing(s);
}

int amwg_sample_device(amwg_sampler *s, int64_t n, int64_t thin, double *out_dev, size_t out_bytes) {
  if (!s || n < 0 || thin < 1 || (!out_dev && n > 0)) return amwg_fail(AMWG_EINVAL, "amwg_sample_device: bad argument");
  const int64_t rows = (n + thin - 1) / thin;
  const size_t need = (size_t)rows * (size_t)(s->P + s->D) * (size_t)s->C * 8;
  if (out_bytes < need) return amwg_fail(AMWG_ESIZE, "amwg_sample: output needs %zu bytes, got %zu", need, out_bytes);
  HIP_TRY(hipSetDevice(s->device));
  TRYB(launch_steps(s, n, thin, out_dev));
  s->last_draws = out_dev;
  s->last_rows = rows;
  return AMWG_OK;
}

int amwg_sample_async(amwg_sampler *s, int64_t n, int64_t thin) {
  if (!s || n < 0 || thin < 1) return amwg_fail(AMWG_EINVAL, "amwg_sample: bad argument");
  const int64_t rows = (n + thin - 1) / thin;
  const size_t need = (size_t)rows * (size_t)(s->P + s->D) * (size_t)s->C * 8;
  HIP_TRY(hipSetDevice(s->device));
  if (need > s->d_draws_cap) {
    if (s->d_draws) {
      if (s->last_draws == s->d_draws) { s->last_draws = nullptr; s->last_rows = 0; }
      (void)hipFree(s->d_draws); s->d_draws = nullptr; s->d_draws_cap = 0;
    }
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_draws), need ? need : 8));
    s->d_draws_cap = need;
  }
  if (!s->d_draws) {  // n == 0 before any allocation
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_draws), 8));
    s->d_draws_cap = 8;
  }
  return amwg_sample_device(s, n, thin, s->d_draws, need);
}

// Summaries without stored draws: the steps of amwg_sample_async(n, thin), the recorded rows folded window by window into per-chain accumulators (amwg_fold.h)
// instead of kept.  The window is the library's own draw buffer, grown only when too small: its size does not depend on n.
int amwg_sample_summarize_async(amwg_sampler *s, int64_t n, int64_t thin, int64_t window_rows) {
  if (!s || n < 0 || thin < 1 || window_rows < 0) return amwg_fail(AMWG_EINVAL, "amwg_sample_summarize: bad argument (%s)", !s ? "null sampler" : n < 0 ? "n < 0" : thin < 1 ? "thin < 1" : "window_rows < 0");
  const int64_t rows = (n + thin - 1) / thin;
  const int PR = s->P + s->D;
  const size_t row_bytes = (size_t)PR * (size_t)s->C * 8;
  int64_t W = window_rows > 0 ? window_rows : (int64_t)(kFoldWindowBytes / row_bytes);
  if (W > rows) W = rows;      // (no run needs a window longer than itself)
  if (W < 1) W = 1;
  const size_t need = (size_t)W * row_bytes, acc_bytes = (size_t)kFoldStats * row_bytes;
  HIP_TRY(hipSetDevice(s->device));
  AutocovArm *acf = nullptr;
  TRYB(amwg_autocov_begin(s, rows, &acf));      // (amwg_set_autocovariance: refuses a call of too few kept rows before anything is touched; its state starts afresh too)
  if (need > s->d_draws_cap) {
    if (s->d_draws) { (void)hipFree(s->d_draws); s->d_draws = nullptr; s->d_draws_cap = 0; }
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_draws), need));
    s->d_draws_cap = need;
  }
  s->last_draws = nullptr;      // (whatever stood in the buffer is overwritten)
  s->last_rows = 0;
  FoldSummary &f = summary_slot(s);
  if (!f.acc) { TRYB(dev_alloc(s, &f.acc, (size_t)kFoldStats * (size_t)PR * (size_t)s->C)); f.acc_bytes = acc_bytes; }
  f.rows = f.window_rows = f.windows = 0;
  f.window_bytes = 0;
  HIP_TRY(hipMemsetAsync(f.acc, 0, acc_bytes, s->stream));      // (each call starts afresh)
  FoldWindow win;
  win.window_rows = W;
  win.total_rows = rows;
  win.acc = f.acc;
  HistArm *arm = nullptr;
  TRYB(amwg_histogram_begin(s, &arm));      // (amwg_set_histogram: its counts start afresh too)
  win.hist = arm;
  CovArm *cov = nullptr;
  TRYB(amwg_covariance_begin(s, &cov));      // (amwg_set_covariance: its co-moments start afresh too)
  win.cov = cov;
  win.acf = acf;
  TRYB(launch_steps(s, n, thin, s->d_draws, false, &win));
  f.rows = rows; f.window_rows = W; f.windows = win.windows; f.window_bytes = need;
  s->last_rows = rows;      // (rows > 0 without last_draws: the mark of a summary -- amwg_summarised)
  return AMWG_OK;
}

int amwg_sample_summarize(amwg_sampler *s, int64_t n, int64_t thin, int64_t window_rows) {
  TRYB(amwg_sample_summarize_async(s, n, thin, window_rows));
  return amwg_sync(s);
}

int amwg_summary_info(const amwg_sampler *s, int64_t *rows, int64_t *window_rows, int64_t *windows, size_t *window_bytes, size_t *accumulator_bytes) {
  const FoldSummary *f = (s && amwg_summarised(s)) ? amwg_summary_of(s) : nullptr;
  if (!f) return amwg_fail(AMWG_EINVAL, "amwg_summary_info: %s", s ? "the last sample call of this sampler was not amwg_sample_summarize (or kept no draw)" : "null sampler");
  if (rows) *rows = f->rows;
  if (window_rows) *window_rows = f->window_rows;
  if (windows) *windows = f->windows;
  if (window_bytes) *window_bytes = f->window_bytes;
  if (accumulator_bytes) *accumulator_bytes = f->acc_bytes;
  return AMWG_OK;
}

int amwg_fetch_draws_slices(amwg_sampler *s, int32_t n_slices, const int32_t *base, const int32_t *len, double *const *out, const size_t *out_bytes) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_fetch_draws: null sampler");
  TRYB(amwg_refuse_summarised(s, "amwg_fetch_draws"));
  if (s->last_draws != s->d_draws) return amwg_fail(AMWG_EINVAL, "amwg_fetch_draws: no amwg_sample_async pending");
  if (n_slices < 0 || (n_slices > 0 && (!base || !len || !out || !out_bytes))) return amwg_fail(AMWG_EINVAL, "amwg_fetch_draws_slices: bad argument");
  const int PR = s->P + s->D;
  const size_t C = (size_t)s->C;
  size_t total_bytes = 0;
  for (int k = 0; k < n_slices; ++k) {
    if (base[k] < 0 || len[k] < 0 || base[k] > PR || len[k] > PR - base[k]) return amwg_fail(AMWG_EINVAL, "amwg_fetch_draws_slices: slice %d = [%d, %d) outside the %d recorded values", k, base[k], base[k] + len[k], PR);
    const size_t need = (size_t)s->last_rows * (size_t)len[k] * C * 8;
    if (need && !out[k]) return amwg_fail(AMWG_EINVAL, "amwg_fetch_draws: null output");
    if (out_bytes[k] < need) return amwg_fail(AMWG_ESIZE, "amwg_sample: output needs %zu bytes, got %zu", need, out_bytes[k]);
    total_bytes += need;
  }
  HIP_TRY(hipSetDevice(s->device));
  if (!s->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
  // (launches since the sample call -- a burn in between -- have reset the per-launch marks: then everything is final once the stream is idle)
  const bool marks = !s->chunk_rows.empty() && s->chunk_rows.back() == s->last_rows;
  const size_t n_chunks = marks ? s->chunk_rows.size() : 1;
  // the destination becomes resident ahead of the copies, in their order.  Helpers only where there is something to win (>= 16 MB): small results are touched inline
  Prefaulter pf(n_chunks);
  {
    int64_t r0 = 0;
    for (size_t j = 0; j < n_chunks; ++j) {
      const int64_t r1 = marks ? s->chunk_rows[j] : s->last_rows;
      if (r1 > r0)
        for (int k = 0; k < n_slices; ++k) {
          if (!len[k]) continue;
          const size_t width = (size_t)len[k] * C * 8;
          pf.add(reinterpret_cast<char *>(out[k]) + (size_t)r0 * width, (size_t)(r1 - r0) * width, j);
        }
      r0 = r1;
    }
    for (int k = 0; k < n_slices; ++k) {      // transparent huge pages for the whole destination, where the host grants them on request
      const size_t need = (size_t)s->last_rows * (size_t)len[k] * C * 8;
      const uintptr_t a0 = ((uintptr_t)out[k] + 4095) & ~(uintptr_t)4095, a1 = ((uintptr_t)out[k] + need) & ~(uintptr_t)4095;
      if (need >= ((size_t)4 << 20) && a1 > a0) (void)madvise(reinterpret_cast<void *>(a0), a1 - a0, MADV_HUGEPAGE);
    }
    unsigned hw = std::thread::hardware_concurrency();
    int helpers = total_bytes >= ((size_t)16 << 20) ? (hw >= 8 ? 4 : (hw >= 4 ? 2 : (hw >= 2 ? 1 : 0))) : 0;
    if (const char *e = getenv("AMWG_PREFAULT_THREADS")) helpers = atoi(e) < 0 ? 0 : (atoi(e) > 16 ? 16 : atoi(e));
    pf.start(helpers);
  }
  if (!marks) HIP_TRY(hipStreamSynchronize(s->stream));
  int64_t r0 = 0;
  for (size_t j = 0; j < n_chunks; ++j) {
    const int64_t r1 = marks ? s->chunk_rows[j] : s->last_rows;
    if (r1 > r0) {
      pf.wait_chunk(j);      // (while launch j still runs, usually: the helpers are ahead)
      if (marks) HIP_TRY(hipEventSynchronize(s->chunk_ev[j]));
      for (int k = 0; k < n_slices; ++k) {
        if (!len[k]) continue;
        const size_t width = (size_t)len[k] * C * 8, spitch = (size_t)PR * C * 8;
        const char *src = reinterpret_cast<const char *>(s->d_draws) + (size_t)r0 * spitch + (size_t)base[k] * C * 8;
        char *dst = reinterpret_cast<char *>(out[k]) + (size_t)r0 * width;
        if (len[k] == PR) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)(r1 - r0) * width, hipMemcpyDeviceToHost, s->copy_stream));
        else HIP_TRY(hipMemcpy2DAsync(dst, width, src, spitch, width, (size_t)(r1 - r0), hipMemcpyDeviceToHost, s->copy_stream));
      }
      HIP_TRY(hipStreamSynchronize(s->copy_stream));
    }
    r0 = r1;
  }
  return finish_timing(s);      // (kernel_ms / launch_info of the LATEST call on the stream, whichever path was taken)
}

int amwg_fetch_draws(amwg_sampler *s, double *out, size_t out_bytes) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_fetch_draws: null sampler");
  const int32_t base = 0, len = s->P + s->D;
  return amwg_fetch_draws_slices(s, 1, &base, &len, &out, &out_bytes);
}

int amwg_sample(amwg_sampler *s, int64_t n, int64_t thin, double *out, size_t out_bytes) {
  if (!s || n < 0 || thin < 1 || (!out && n > 0)) return amwg_fail(AMWG_EINVAL, "amwg_sample: bad argument");
  const int64_t rows = (n + thin - 1) / thin;
  const size_t need = (size_t)rows * (size_t)(s->P + s->D) * (size_t)s->C * 8;
  if (out_bytes < need) return amwg_fail(AMWG_ESIZE, "amwg_sample: output needs %zu bytes, got %zu", need, out_bytes);
  TRYB(amwg_sample_async(s, n, thin));
  return amwg_fetch_draws(s, out, out_bytes);
}

int amwg_sync(amwg_sampler *s) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_sync: null sampler");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return finish_timing(s);
}

int amwg_set_adapting(amwg_sampler *s, int32_t flag) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_set_adapting: null sampler");
  HIP_TRY(hipSetDevice(s->device));
  for (auto &b : s->h_adapt) b = flag ? 1 : 0;
  HIP_TRY(hipMemcpyAsync(s->d_adapt, s->h_adapt.data(), s->h_adapt.size(), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMWG_OK;
}

int amwg_get_state(amwg_sampler *s, double *out, size_t out_bytes) {
  if (!s || !out) return amwg_fail(AMWG_EINVAL, "amwg_get_state: null argument");
  const size_t need = (size_t)s->P * (size_t)s->C * 8;
  if (out_bytes < need) return amwg_fail(AMWG_ESIZE, "amwg_get_state: output needs %zu bytes, got %zu", need, out_bytes);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipMemcpyAsync(out, s->ch.state, need, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMWG_OK;
}

int amwg_set_state(amwg_sampler *s, const double *state, size_t state_bytes) {
  if (!s || !state) return amwg_fail(AMWG_EINVAL, "amwg_set_state: null argument");
  const size_t need = (size_t)s->P * (size_t)s->C * 8;
  if (state_bytes != need) return amwg_fail(AMWG_ESIZE, "amwg_set_state: expected %zu bytes, got %zu", need, state_bytes);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(s->ch.state, state, need, hipMemcpyHostToDevice));
  s->lp_ready = false;   // the next launch recomputes log_post(state) first
  return AMWG_OK;
}
#if defined(AMWG_AUDIT) || defined(AMWG_X_PHASES)
// include/amwg_selftest.h: what the audited launches of this sampler have recorded so far (and optionally a reset)
int amwg_audit_fetch(amwg_sampler *s, double *per_chain, uint64_t *hist, int32_t reset) {
  if (!s) return amwg_fail(AMWG_EINVAL, "amwg_audit_fetch: null sampler");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (per_chain) HIP_TRY(hipMemcpy(per_chain, s->ch.audit, (size_t)4 * s->C * 8, hipMemcpyDeviceToHost));
  if (hist) HIP_TRY(hipMemcpy(hist, s->ch.audit_hist, 128 * 8, hipMemcpyDeviceToHost));
  if (reset) { HIP_TRY(hipMemset(s->ch.audit, 0, (size_t)4 * s->C * 8)); HIP_TRY(hipMemset(s->ch.audit_hist, 0, 128 * 8)); }
  return AMWG_OK;
}
#endif

}  // extern "C"
