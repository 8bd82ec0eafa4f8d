// amwg_dataset_quantiles.h -- the launcher behind amwg_last_sample_dataset_quantiles (amwg_summaries.hip), over a device pointer, so that the test library
// (amwg_selftest.hip: amwg_dataset_quantiles_check) drives the same kernel on arbitrary arrays.  Internal to the shared objects; no device code here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#pragma GCC visibility push(hidden)
// AMWG_EINVAL (message in amwg_last_error(), `call` named) unless the shape can be served: rows, PR, C, D, n_probs >= 1, D <= 65535 dividing C, and at most
// 2^31 - 1 values per dataset and component.  Host only: no device call.
int amwg_dataset_quantiles_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int n_probs);
// draws [rows][PR][C] on the current device, D datasets of C / D columns each; probs [n_probs] and out [D][PR][n_probs] on the host.  `call` names the caller in
// amwg_last_error().  Returns after `stream` has drained: out is complete.  Checks the shape first (amwg_dataset_quantiles_shape).
int amwg_dataset_quantiles_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const double *probs, int n_probs, double *out,
                                  hipStream_t stream);
#pragma GCC visibility pop
