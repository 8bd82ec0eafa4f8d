// amwg_hpd.h -- the launcher behind amwg_last_sample_dataset_hpd (amwg_hpd.hip), over a device pointer, so that the test library (amwg_selftest.hip:
// amwg_hpd_check) drives the same kernels on arbitrary arrays.  Internal to the shared objects; no device code here, and not a source of the step kernels
// (tools/build_id.py).  The rule is stated in include/amwg.h.
//
// THE ROUTE, per probability p (all (dataset, value) pairs share N, g and k = N - g, so one grid covers them):
//   1 thresholds   t_lo = x_(k-1), t_hi = x_(g): a radix select of two ranks per pair (the pieces of amwg_select.h), which also notices a non-finite draw
//   2 compaction   lo takes every key below key(t_lo), hi every key above key(t_hi), through a cursor per tail; the k - cursor entries left are copies of the
//                  threshold (ties at a threshold are the common case), and the pad up to the next power of two holds maximal keys
//   3 sort         both tails ascending, keys only: a bitonic network, in LDS by one workgroup where the padded tail fits, else LDS-sized chunks + global steps
//   4 argmin       w_i = value(hi[i]) - value(lo[i]), the smallest i of the smallest width, one workgroup per pair
// SCRATCH: 2 x pad(k) keys per pair, allocated per call and freed before it returns; the pairs go in batches under kHpdScratchBytes, and a pair whose two
// tails exceed the budget runs alone.  As p -> 0, k -> N: the tails approach the whole slice, twice.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

constexpr size_t kHpdScratchBytes = (size_t)256 << 20;      // the default scratch budget of a call: 256 MiB (the fold's window is 64 MiB)

#pragma GCC visibility push(hidden)
// AMWG_EINVAL "<call>: ..." unless the shape can be served: amwg_dataset_quantiles_shape's limits, and at least 2 values per dataset and value.  Host only.
int amwg_hpd_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int n_probs);
// draws [rows][PR][C] on the current device, D datasets of C / D columns each; probs [n_probs] and out [D][PR][n_probs][2] on the host.  `call` names the caller
// in amwg_last_error().  Returns after `stream` has drained: out is complete.  Checks the shape first (amwg_hpd_shape).
int amwg_hpd_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const double *probs, int n_probs, double *out, hipStream_t stream);
// the keys one workgroup sorts in LDS on the current device: the largest power of two that fits what the device reports per workgroup
int amwg_hpd_lds_keys(int64_t *keys);
// the scratch budget of later calls in bytes (0: kHpdScratchBytes); returns the budget in force before.  For the test library: the product never calls it.
size_t amwg_hpd_set_budget(size_t bytes);
#pragma GCC visibility pop
