// amwg_fold.h -- summaries without stored draws (amwg_sample_summarize): the ONE Welford update every per-chain reduction of this library is made of, and
// what the host units share about folding a window of recorded rows into per-chain accumulators.  Not a source of the step kernels (tools/build_id.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct amwg_sampler;

namespace amwg {

// x is the k-th value (1-based) of its sequence; m its running mean, m2 the running sum of squares about the mean.  chain_halves_kernel (which amwg_group.hip
// launches too, through amwg_chain_halves) and fold_window_kernel (both amwg_diag.hip) step through this, in row order: with -ffp-contract=off every operation
// rounds once, so a sequence gives the same bits whichever kernel walks it and however it is cut into windows.  The division stays a division.
__device__ __forceinline__ void welford_add(double x, int64_t k, double &m, double &m2) {
  const double dlt = x - m;
  m += dlt / (double)k;
  m2 += dlt * (x - m);
}

// The sum of v over the workgroup (a power-of-two size), in every thread: a halving tree over red[blockDim.x] (LDS).  The per-dataset reductions of amwg_diag.hip
// and amwg_covariance.hip share it, so that a sum over a dataset's chains has one order wherever it is formed.
__device__ inline double block_sum(double v, double *red) {
  const int tid = threadIdx.x, nt = blockDim.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = nt / 2; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
  return red[0];
}

// The accumulators of a summarising call, device, [kFoldStats][PR][C]: (m, M2) of the first half of a chain's kept draws, of the second half, of the whole chain.
// half = rows / 2: rows [0, half) are the first half, [half, 2 half) the second; an odd last row enters the whole-chain pair only (chain_halves_kernel ignores it too).
constexpr int kFoldStats = 6;
// The default window (window_rows = 0): the rows that fit into 64 MiB.  A choice, not a measurement: large enough that a fold is a few launches' worth of rows at the
// flagship shapes (64 rows of 65 536 chains x 2 values), small enough to be no burden beside the chains' own state.
constexpr size_t kFoldWindowBytes = (size_t)64 << 20;

}  // namespace amwg

#pragma GCC visibility push(hidden)
// what a summarising call left behind (kept per sampler in amwg_run.hip: the handle's own layout, amwg_sampler.h, is a source of the step kernels and stays as it is)
struct FoldSummary {
  double *acc = nullptr;      // [kFoldStats][PR][C]; lives as long as the sampler (dev_allocs)
  size_t acc_bytes = 0;
  int64_t rows = 0, window_rows = 0, windows = 0;      // kept rows, rows of the window, folds of the last summarising call
  size_t window_bytes = 0;
};
// a window for launch_steps' loop: the recorded rows go to rows [0, window_rows) of the draw buffer, and each time they are full (and at the end) they are folded into acc
struct HistArm;      // (amwg_histogram.h)
struct CovArm;       // (amwg_covariance.h)
struct AutocovArm;   // (amwg_autocov.h)
struct FoldWindow {
  int64_t window_rows = 0, total_rows = 0;
  double *acc = nullptr;
  int64_t windows = 0;      // out: folds enqueued
  const HistArm *hist = nullptr;      // the histogram armed for the call (amwg_set_histogram): after each fold, the window's rows are counted into it too
  const CovArm *cov = nullptr;        // the covariance armed for the call (amwg_set_covariance): BEFORE each fold, the window's co-moments are added from the means it starts at
  const AutocovArm *acf = nullptr;    // the autocovariance armed for the call (amwg_set_autocovariance): after the fold and the histogram, the window's lag sums, then its carry
};
// true when the last sample call of `s` was a summarising one (its draws were folded, not kept): last_rows > 0 without last_draws
bool amwg_summarised(const amwg_sampler *s);
const FoldSummary *amwg_summary_of(const amwg_sampler *s);      // nullptr: none
void amwg_summary_forget(const amwg_sampler *s);                // (amwg_destroy)
// AMWG_EINVAL "<call>: ... amwg_sample_summarize ... the draws were not kept" when amwg_summarised(s), else AMWG_OK
int amwg_refuse_summarised(const amwg_sampler *s, const char *call);

// ---- amwg_diag.hip: the kernels, enqueued on `stream`
// rows [g0, g0 + nrows) of a chain's kept draws stand in window[0 .. nrows)[PR][C]: add them to acc
int amwg_fold_window(const double *window, int64_t g0, int64_t nrows, int64_t half, int PR, int64_t C, double *acc, hipStream_t stream);
// acc -> chain_halves_kernel's layout [4][PR][C]: the half means, and the half M2 as variances M2 / (half - 1) (0 when half <= 1)
int amwg_fold_halves(const double *acc, int64_t rows, int PR, int64_t C, double *halves, hipStream_t stream);
// acc -> mean, sd [D][PR] (device) over D datasets of C / D chains each, from the whole-chain pairs
int amwg_fold_moments(const double *acc, int64_t rows, int PR, int64_t C, int D, double *mean, double *sd, hipStream_t stream);
// chain_halves_kernel on a stored array draws [rows][PR][C] -> halves [4][PR][C] (the selftest entry compares the fold with it)
int amwg_chain_halves(const double *draws, int64_t rows, int PR, int64_t C, double *halves, hipStream_t stream);

// ---- amwg_diag.hip: the summaries of stored draws and of halves over a DEVICE array, D datasets of C / D chains each (D = 1: pooled over all chains).  The
// sampler's calls and the selftest entry (amwg_summaries_check) go through these; mean, sd, rhat, ess are HOST arrays, complete on return (`stream` has drained).
// What split-R-hat / ESS refuse, in one place: AMWG_EINVAL "<call>: needs a sample() of >= 4 kept draws on >= 2 chains[ per dataset]" unless there is a sample
// (`have`) of rows >= 4 on C / D >= 2 chains per dataset (D >= 1).  Host only: no device call.
int amwg_diagnostics_refusal(const char *call, bool have, int64_t rows, int64_t C, int D, bool per_dataset);
// dataset_moments_kernel on draws [rows][PR][C] -> mean, sd [D][PR]
int amwg_moments_launch(const double *draws, int64_t rows, int PR, int64_t C, int D, double *mean, double *sd, hipStream_t stream);
// dataset_diagnostics_kernel on halves [4][PR][C] (chain_halves_kernel's layout) of chains of `rows` kept draws -> rhat, ess [D][PR]
int amwg_dataset_diagnostics_launch(const double *halves, int64_t rows, int PR, int64_t C, int D, double *rhat, double *ess, hipStream_t stream);
// the pooled call's reduction: the halves come to the host and are summed there in long double over all C chains -> rhat, ess [PR]
int amwg_pooled_diagnostics(const double *halves, int64_t rows, int PR, int64_t C, double *rhat, double *ess, hipStream_t stream);
#pragma GCC visibility pop
