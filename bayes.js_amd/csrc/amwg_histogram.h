// amwg_histogram.h -- posterior histograms over caller-given edges (amwg_last_sample_dataset_histogram, amwg_set_histogram): what the host units share about the
// launcher of amwg_histogram.hip and about the histogram a sampler has armed for its summarising calls.  Internal to the shared objects; no device code here, and
// not a source of the step kernels (tools/build_id.py).
//
// THE BIN RULE is comparisons with the edges and nothing else: of edges e[0] < ... < e[bins], a value x belongs to bin i iff e[i] <= x < e[i + 1]; x < e[0] is
// counted as UNDER, x >= e[bins] as OVER (so +inf is over and -inf under), a NaN as NAN; -0 compares equal to +0.  That is np.searchsorted(e, x, side="right") - 1.
// A cell of counts is [bins + 3]: the bins, then under, over, nan.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct amwg_sampler;

namespace amwg {
constexpr int kHistMaxBins = 4096;
}  // namespace amwg

#pragma GCC visibility push(hidden)
// AMWG_EINVAL "<call>: ..." unless 1 <= bins <= 4096 and edges [PR][bins + 1] are finite and strictly ascending per recorded value.  Host only: no device call.
int amwg_histogram_edges_check(const char *call, const double *edges, int PR, int bins);
// AMWG_EINVAL "<call>: ..." unless the shape can be served: rows, PR, C, D >= 1, D <= 65535 dividing C, and fewer than 2^32 values in the part of a cell that one
// workgroup counts (its counters in LDS are 32 bits wide).  Host only: no device call.
int amwg_histogram_shape(const char *call, int64_t rows, int PR, int64_t C, int D, int bins);
// draws [rows][PR][C] on the current device, D datasets of C / D columns each; d_edges [PR][bins + 1] and d_counts [D][PR][bins + 3] on the device.  The kernel
// ADDS to d_counts: the caller zeroes them, once for a stored array and once for all windows of a summarising call.  Enqueued on `stream`; no synchronisation.
// Checks the shape first (amwg_histogram_shape).
// `uniform`: amwg_histogram_uniform(edges) of the host copy -- the kernel then finds a bin by a corrected guess instead of a binary search; the counts are the same.
int amwg_histogram_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const double *d_edges, int bins, bool uniform,
                          uint64_t *d_counts, hipStream_t stream);
// true when, for every recorded value, floor((e[i] - e[0]) bins / (e[bins] - e[0])) is within one of i for every edge: a (nearly) uniform grid.  Host only.
bool amwg_histogram_uniform(const double *edges, int PR, int bins);
// the grid the launcher uses for a shape: PR x D x (row_slices * column_slices) workgroups, each over rows_per_slice rows of columns_per_slice columns of a cell
void amwg_histogram_grid(int64_t rows, int PR, int64_t C, int D, int *row_slices, int *column_slices, int64_t *rows_per_slice, int64_t *columns_per_slice);

// ---- the histogram armed for a sampler's summarising calls (amwg_set_histogram), kept beside the handle as FoldSummary is (amwg_fold.h)
struct HistArm {
  int bins = 0;                  // 0: nothing armed
  bool uniform = false;          // amwg_histogram_uniform of the armed edges
  double *d_edges = nullptr;     // [PR][bins + 1]
  uint64_t *d_counts = nullptr;  // [D][PR][bins + 3]
  size_t bytes = 0;              // of edges and counts on the device
  bool folded = false;           // the counts are those of the sampler's last summarising call
};
// the armed histogram of `s`, or nullptr (none armed)
HistArm *amwg_histogram_armed(const amwg_sampler *s);
// amwg_sample_summarize_async, before its launches: zeroes the armed counts on the sampler's stream and marks them as this call's.  -> the arm, or nullptr
int amwg_histogram_begin(amwg_sampler *s, HistArm **arm);
void amwg_histogram_forget(const amwg_sampler *s);      // (amwg_destroy, after the device is set: frees edges and counts)
#pragma GCC visibility pop
