// amwg_heldout.h -- the launcher behind amwg_last_sample_dataset_heldout (amwg_heldout.hip), over device draws and host descriptions of the held-out data, so that
// the test library (amwg_selftest.hip: amwg_heldout_check) drives the same kernels on arbitrary draws.  Internal to the shared objects, and not a source of the step
// kernels (tools/build_id.py).  The rule is stated in include/amwg.h.
//
// THE ROUTE.  S = rows * (C / D) draws per dataset in WAIC's order; m = the dataset's held-out observations: FEW OBSERVATIONS x MANY DRAWS, where WAIC's kernel -- a
// lane per observation -- would leave most of a wavefront idle.
//   1 partials     heldout_partial_kernel<Family>: a workgroup of 256 threads serves a tile of Mt <= 64 observations and one of the dataset's `splits` contiguous runs
//                  of draws.  Np = Mt rounded up to a power of two; an observation is owned by sub = 64 / Np lanes of every wavefront (slot = lane & (Np - 1)), and
//                  lane unit = wave * sub + lane / Np walks the staged draws unit, unit + 4 sub, ...: with one observation all 256 threads work on it.  The draws
//                  are staged as WAIC stages them (draw_at, stage_len); the observation stays in registers.  Only (m, sum exp(l - m)) is kept: a lane takes its
//                  draws in blocks of R = group_block<F>() terms, forms the block's maximum, rescales the running sum once and adds R independent exponentials.
//                  The sub lanes of an observation merge by an xor butterfly over the lane distances Np, 2 Np, ... 32 -- DPP moves up to 8, v_permlane16_swap and
//                  v_permlane32_swap beyond, no LDS; a step is max, two rescales, one add, symmetric, so every lane of the observation ends with the same bytes --
//                  and the four wavefronts through LDS in the order 0, 1, 2, 3, into scratch [split][observation].
//   2 finish       heldout_finish_kernel: a WAVEFRONT per observation -- lane k merges the splits k, k + 64, ... in ascending order, the 64 lanes merge by the same
//                  butterfly -- and writes lppd_j = m + log(sum) - log(S); a non-finite term anywhere gives NaN.  (A thread per observation walking all the
//                  splits took five times the partial kernel at m = 1.)
//   3 totals       on the host, in index order (amwg_heldout_totals).
// splits = heldout_splits(S, m), a function of those two alone: a dataset's bytes do not depend on its neighbours, on D, or on the scratch budget.
// SCRATCH: splits * m partials of 16 bytes per dataset; the datasets go in batches under the call's budget (kPointwiseScratchBytes by default).  The held-out
// arrays are packed as the sampler lays its own (so Family<MODEL>::load_obs and ::term read them: no second spelling of a term), uploaded per call and freed before
// it returns.  The Poisson family's positions ride in a fifth array, at WaicDataset::off_xb (which that family does not use).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "amwg_host.h"
#include "amwg_pointwise.h"
#include "amwg_waic.h"

// the number of contiguous runs a dataset's S draws are cut into, from S and its m held-out observations alone: WAIC's rule with m for n -- kTargetBlocks workgroups
// per dataset over the tiles of 64, a run at least one staged run long (amwg_pointwise.h)
__host__ __device__ inline int64_t heldout_splits(int64_t S, int64_t m) { return amwg::waic_splits(S, m); }

// held-out data on the device, packed as the sampler packs its own: what amwg_heldout_pack fills and a run reads (this call's kernels, and those of
// amwg_predictive.hip).  The host vectors back the asynchronous uploads; everything is freed with the struct.
struct HeldArrays {
  WaicModel M{};                       // base with x, y, lfact, xb, invalid pointing into the arrays below
  std::vector<WaicDataset> sets;       // [D], host: n_obs = m_d and the places of dataset d's arrays
  int64_t m_max = 0;
  const int32_t *index = nullptr;      // the Poisson family's positions on the device, at WaicDataset::off_xb; nullptr for the other families
  std::vector<double> hx, hy, hlf;
  std::vector<uint8_t> hxb, hbad;
  std::vector<int32_t> hidx;
  DevBuf dx, dy, dlf, dxb, dbad, didx;
};

#pragma GCC visibility push(hidden)
// held [D] and index (validated) into `h`, the uploads enqueued on `stream`; h must outlive the stream's drain
int amwg_heldout_pack(const WaicModel &base, int D, const amwg_model_desc *held, const int32_t *index, hipStream_t stream, HeldArrays &h);
// AMWG_EINVAL "<call>: ..." unless held[0 .. D) can be scored by a sampler of (model, G, K): the same model, K and G, n_obs >= 0, the arrays the family reads, labels
// in [0, G), the Poisson family's index >= 0 (the other families do not read it), the hierarchical family on one dataset.  Host only.
int amwg_heldout_validate(const char *call, int model, int G, int K, int D, const amwg_model_desc *held, const int32_t *index);
// The run.  draws [rows][PR][C] on the current device; base: model, G, exact_division and neg_half_log_2pi of the sampler (its arrays are not read); held [D] and index
// on the host, validated.  summary [D][2] = elpd_heldout, se; pointwise nullptr or [D][m_max].  Returns after `stream` has drained.
int amwg_heldout_launch(const char *call, const double *draws, int64_t rows, int PR, int64_t C, int D, const WaicModel &base, const amwg_model_desc *held, const int32_t *index,
                        double *summary, double *pointwise, size_t scratch_bytes, hipStream_t stream);
// the finish of include/amwg.h over one dataset's lppd_j [m]: summary[2]
void amwg_heldout_totals(const double *lppd, int64_t m, double *summary);
#pragma GCC visibility pop
