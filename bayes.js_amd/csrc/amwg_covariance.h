// amwg_covariance.h -- posterior covariance matrices over a subset of the recorded values (amwg_last_sample_dataset_covariance, amwg_set_covariance): what the host
// units share about the launchers of amwg_covariance.hip and about the covariance a sampler has armed for its summarising calls.  Internal to the shared objects; no
// device code here, and not a source of the step kernels (tools/build_id.py).
//
// THE ARITHMETIC (include/amwg.h states it in full).  Per chain, in row order, for the k-th kept draw: dx_i = x_i - m_i; m_i += dx_i / k (welford_add's mean line:
// m_i is, bit for bit, the whole-chain mean acc[4] of the fold); for every pair C_ij += dx_i * (x_j - m_j), m_j already advanced.  Of a pair, i is the value with
// the SMALLER index among the recorded values, wherever the two stand in the caller's list: a matrix does not depend on the order its values were asked for in.
// Per (dataset, pair): cov_ij = (sum_c C_ijc + rows sum_c (m_ic - gm_i)(m_jc - gm_j)) / (rows cpd - 1) in fold_moments_kernel's order; the diagonal is that
// kernel's own ss / (n - 1) from the whole-chain M2 (acc[5]).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

struct amwg_sampler;

#pragma GCC visibility push(hidden)
// AMWG_EINVAL "<call>: ..." unless values[0 .. n_values) are distinct indices in [0, PR), 1 <= n_values <= PR.  Host only: no device call.
int amwg_covariance_values_check(const char *call, const int32_t *values, int32_t n_values, int PR);
// AMWG_EINVAL "<call>: ..." unless the shape can be served: rows, PR, C, D >= 1, PR and D <= 65535, D dividing C, rows C / D >= 2, and no byte count (the array,
// the fold's accumulators, the co-moments, the matrices) beyond size_t.  Host only: no device call.
int amwg_covariance_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int32_t n_values);
// the co-moments of K values on C chains: K (K - 1) / 2 pairs x C doubles
size_t amwg_covariance_pairs(int32_t n_values);
// `sorted` = values in ascending order; where[k] = the place of values[k] in it (the device works on the ascending list, the host puts the matrix back)
void amwg_covariance_order(const int32_t *values, int32_t n_values, std::vector<int32_t> *sorted, std::vector<int32_t> *where);
// rows [g0, g0 + nrows) of a chain's kept draws stand in window[0 .. nrows)[PR][C]: add their co-moments to d_co [pairs][C] for the K ascending values d_values.
// Reads the running means at the start of the window from acc[4] (amwg_fold.h), so it is enqueued BEFORE amwg_fold_window of the same window, on the same stream.
int amwg_comoment_window(const double *window, int64_t g0, int64_t nrows, int PR, int64_t C, const int32_t *d_values, int32_t n_values, const double *acc, double *d_co,
                         hipStream_t stream);
// acc (the fold's accumulators after the last window) and d_co -> d_cov [D][K][K] (device), in the ascending order of d_values
int amwg_covariance_finish(const double *acc, const double *d_co, int64_t rows, int PR, int64_t C, int D, const int32_t *d_values, int32_t n_values, double *d_cov,
                           hipStream_t stream);
// The stored path: draws [rows][PR][C] on the current device, in windows of window_rows rows (0: the whole array as one window) through the co-moment kernel and the
// fold, from zeroed scratch -> cov [D][K][K] (HOST, in the order of `values`; complete on return).  Checks values and shape first.
int amwg_covariance_of_array(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const int32_t *values, int32_t n_values, int64_t window_rows,
                             double *cov, hipStream_t stream);

// ---- the covariance armed for a sampler's summarising calls (amwg_set_covariance), kept beside the handle as FoldSummary and HistArm are
struct CovArm {
  int32_t n_values = 0;              // 0: nothing armed
  std::vector<int32_t> values;       // as the caller listed them
  std::vector<int32_t> where;        // (amwg_covariance_order)
  int32_t *d_values = nullptr;       // ascending, [K]
  double *d_co = nullptr;            // [K (K - 1) / 2][C]
  size_t bytes = 0;                  // of the co-moments and the list on the device
  bool folded = false;               // the co-moments are those of the sampler's last summarising call
};
CovArm *amwg_covariance_armed(const amwg_sampler *s);      // nullptr: none armed
// amwg_sample_summarize_async, before its launches: zeroes the armed co-moments on the sampler's stream and marks them as this call's.  -> the arm, or nullptr
int amwg_covariance_begin(amwg_sampler *s, CovArm **arm);
void amwg_covariance_forget(const amwg_sampler *s);      // (amwg_destroy, after the device is set)
#pragma GCC visibility pop
