// amwg_autocov.h -- autocovariance along the chains at lags 0 .. L over a subset of the recorded values (amwg_last_sample_dataset_autocovariance,
// amwg_set_autocovariance): what the host units share about the launchers of amwg_autocov.hip and about the autocovariance a sampler has armed for its summarising
// calls.  Internal to the shared objects; no device code here, and not a source of the step kernels (tools/build_id.py).
//
// THE ARITHMETIC (include/amwg.h states it in full).  Per chain and value, x_0 .. x_(n-1) its kept draws in row order: the pilot a = x_0, y_t = x_t - a; in row
// order Y += y_t and, for every lag l = 0 .. min(t, L), S_l += y_t * y_(t-l).  At the end ybar = Y / n; H_(l+1) = H_l + y_l, T_(l+1) = T_l + y_(n-1-l) from 0;
// gamma_l = ((S_l - ybar * ((Y - H_l) + (Y - T_l))) + (double)(n - l) * (ybar * ybar)) / (double)n; m_c = a + ybar.  Per (dataset, value), in fold_moments_kernel's
// order: acov_l = sum_c gamma_lc / cpd, gm = sum_c m_c / cpd, between = sum_c (m_c - gm)^2 / (cpd - 1) (0.0 when cpd = 1).  Where acov_0 is not finite -- a NaN or
// an infinity among the draws, or sums that overflowed -- every acov_l is NaN by IEEE arithmetic, and mean and between are set to NaN.
//
// THE STATE, for K values, C chains, L = max_lag, one allocation of (3 L + 2) K C doubles:
//   S [L + 1][K][C]   the lagged sums                       Y [K][C]   the sum of the deviations
//   ring [L][K][C]    the raw x of the last L kept rows, row g at slot g mod L
//   head [L][K][C]    the raw x of rows 0 .. L - 1; head[0] is the pilot.  y is recomputed as x - a wherever it is needed: the same bits everywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

struct amwg_sampler;

constexpr int32_t kAutocovMaxLag = 1024;      // a chosen cap: the state grows with it, and amwg_autocovariance_info reports the bytes

#pragma GCC visibility push(hidden)
// AMWG_EINVAL "<call>: ..." unless 1 <= max_lag <= kAutocovMaxLag.  Host only.
int amwg_autocov_lag_check(const char *call, int32_t max_lag);
// AMWG_EINVAL "<call>: ..." unless the shape can be served: rows, PR, C, D >= 1, PR and D <= 65535, D dividing C, 1 <= n_values <= PR, max_lag in range and
// < rows, and no byte count (the array, the state, the per-chain autocovariances, the outputs) beyond size_t.  Host only: no device call.
int amwg_autocov_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int32_t n_values, int32_t max_lag);
// (3 L + 2) K C, the doubles of the state; false when the count (in bytes) does not fit size_t
bool amwg_autocov_state_elems(int32_t n_values, int64_t C, int32_t max_lag, size_t *elems);
// rows [g0, g0 + nrows) of a chain's kept draws stand in window[0 .. nrows)[PR][C]: the lag-sum kernel adds them to S and Y of `state` for the K ascending values
// d_values, then the carry kernel copies the window's last min(nrows, L) rows into the ring and its rows g < L into the head -- in that order, on `stream`.
int amwg_autocov_window(const double *window, int64_t g0, int64_t nrows, int PR, int64_t C, const int32_t *d_values, int32_t n_values, int32_t max_lag, double *state,
                        hipStream_t stream);
// the state after the last window of chains of `rows` kept draws -> acov [D][K][L + 1], mean, between [D][K] (HOST, in the caller's order: entry k of the output
// is entry where[k] of the ascending list; complete on return)
int amwg_autocov_collect(const double *state, int64_t rows, int64_t C, int D, int32_t n_values, int32_t max_lag, const std::vector<int32_t> &where, double *acov,
                         double *mean, double *between, hipStream_t stream);
// The stored path: draws [rows][PR][C] on the current device, in windows of window_rows rows (0: the whole array as one window) through the same kernels, from a
// zeroed state -> acov, mean, between (HOST, in the order of `values`; complete on return).  Checks values and shape first.
int amwg_autocov_of_array(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const int32_t *values, int32_t n_values, int32_t max_lag,
                          int64_t window_rows, double *acov, double *mean, double *between, hipStream_t stream);

// ---- the autocovariance armed for a sampler's summarising calls (amwg_set_autocovariance), kept beside the handle as FoldSummary, HistArm and CovArm are
struct AutocovArm {
  int32_t n_values = 0;              // 0: nothing armed
  int32_t max_lag = 0;
  std::vector<int32_t> values;       // as the caller listed them
  std::vector<int32_t> where;        // (amwg_covariance_order)
  int32_t *d_values = nullptr;       // ascending, [K]
  double *d_state = nullptr;         // (3 L + 2) K C doubles
  size_t state_bytes = 0, bytes = 0; // of the state; of the state and the list on the device
  bool folded = false;               // the state is that of the sampler's last summarising call
};
AutocovArm *amwg_autocov_armed(const amwg_sampler *s);      // nullptr: none armed
// amwg_sample_summarize_async, before its launches: refuses (AMWG_EINVAL "amwg_sample_summarize: ...") a call whose kept rows are <= the armed max_lag, else zeroes
// the armed state on the sampler's stream and marks it as this call's.  -> the arm, or nullptr
int amwg_autocov_begin(amwg_sampler *s, int64_t rows, AutocovArm **arm);
void amwg_autocov_forget(const amwg_sampler *s);      // (amwg_destroy, after the device is set)
#pragma GCC visibility pop
