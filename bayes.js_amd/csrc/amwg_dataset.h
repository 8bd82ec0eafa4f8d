// amwg_dataset.h -- many datasets in one sampler (amwg_create_datasets): the kernels' second argument and the entry points that use it.
//
// Chains keep their one global numbering; dataset d owns the local chains [d * cpd, (d + 1) * cpd), cpd = chains / D.  A workgroup serves exactly ONE
// dataset -- the host only plans geometries whose chains per workgroup divide cpd (amwg_plan.hip) -- so everything that tells datasets apart is
// wave-uniform: d = blockIdx.x / blocks_per_dataset, the shifted data pointers and the data-dependent constants all sit in scalar registers, worked out
// once in the entry block.  The entry points below are twins of amwg_step_kernel / amwg_step_kernel_cert: they build the workgroup's DataRef and
// ModelConsts and hand them to the same step_body.  Nothing else changes: the per-chain arrays, the draws [row][P][C], the wavefront ids behind
// wave_scratch_of and the Philox key (seed, chain_offset + c) are those of an ordinary sampler, which is why dataset d's chains equal the chains of an
// ordinary sampler on dataset d with chain_offset = d * cpd, bit for bit (tests/test_gpu_datasets.py).
//
// The datasets need not have one size (amwg_create_datasets_ragged): n_obs is one more per-dataset constant.  The stepper state lies behind the data in
// LDS, so its offset then differs between workgroups, which is harmless; the launch's dynamic LDS covers the largest layout (amwg_plan.hip lds_of).
// tests/test_gpu_ragged_datasets.py holds the same parity statement for unequal sizes.
//
// StepArgs stays the kernels' FIRST parameter and keeps its size: cold_args() (amwg_kernel.h) reads it through the kernel-argument pointer, and what is
// read that way -- the per-chain arrays, the draws, the hyper-parameters of the Normal prior -- is the same for every dataset.
#pragma once
#include "amwg_kernel.h"

namespace amwg {

// what the host derives from ONE dataset's data or size (amwg_create.hip fills it, for an ordinary sampler too: its one dataset); the rest of ModelConsts
// follows from the hyper-parameters and the options, which all datasets share.
// Datasets may differ in SIZE (amwg_create_datasets_ragged): n_obs and what is formed from it -- the Poisson family's prior ld.unif(cp, 0, n - 1) -- are
// per-dataset constants like the others, and so is the place of the dataset's copy inside each of the six arrays.
struct DatasetConsts {
  int32_t data_mid_range, has_invalid, n_obs, reserved;
  double cp_upper, lunif_cp;
  double glm_xmax[7], glm_sum_y, glm_sum_lf;
  double suff_xbar_hi, suff_xbar_lo, suff_ss;
  // the datasets' copies lie back to back, one allocation per array, each copy starting on a 256-byte boundary: dataset d's begins at base + off_* (in ELEMENTS
  // of the array's type; 0 for an array the family does not have).  Offsets, not a stride: a dataset of 10^6 beside a thousand of 10^2 costs its own size once.
  int64_t off_x, off_y, off_lfact, off_xb, off_xw, off_arr0;      // (arr[0]: the beta-Bernoulli family's tables of two_valued_sum, 32-bit words)
};

struct DatasetArgs {
  int32_t blocks_per_dataset, n_datasets;
  const DatasetConsts *consts;                                                      // [n_datasets], device memory
};

// One dataset's constants where the kernels read them, ModelConsts.  THE list of the fields of DatasetConsts that are constants of the model -- the
// rest are the size and the offsets, which dataset_view below applies to DataRef.  Both sides go through it: the device per workgroup (dataset_view),
// the host once, for dataset 0, into the sampler's own ModelConsts (amwg_create.hip create_builtin: an ordinary sampler is dataset 0 of one).
__host__ __device__ __forceinline__ void dataset_constants(ModelConsts &mc, const DatasetConsts &k) {
  mc.data_mid_range = k.data_mid_range;
  mc.has_invalid = k.has_invalid;
  mc.cp_upper = k.cp_upper;
  mc.lunif_cp = k.lunif_cp;
#pragma unroll
  for (int j = 0; j < 7; ++j) mc.glm_xmax[j] = k.glm_xmax[j];
  mc.glm_sum_y = k.glm_sum_y;
  mc.glm_sum_lf = k.glm_sum_lf;
  mc.suff_xbar_hi = k.suff_xbar_hi;
  mc.suff_xbar_lo = k.suff_xbar_lo;
  mc.suff_ss = k.suff_ss;
}

// the argument block as the workgroup of dataset blockIdx.x / blocks_per_dataset sees it
__device__ __forceinline__ void dataset_view(StepArgs &v, const DatasetArgs &ds) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (made a scalar explicitly: the quotient of two scalars is formed with the vector unit's reciprocal)
  const int64_t d = (int64_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x / (uint32_t)ds.blocks_per_dataset));
#else
  const int64_t d = 0;
#endif
  const DatasetConsts &k = ds.consts[d];      // (a uniform address: scalar loads)
  v.d.n_obs = k.n_obs;                        // (wave-uniform, from a scalar load: log_post's fresh_uniform keeps it in a scalar register)
  v.d.x += k.off_x;
  v.d.y += k.off_y;
  v.d.lfact += k.off_lfact;
  v.d.xb += k.off_xb;
  v.d.xw += k.off_xw;
  v.d.arr[0] = static_cast<const uint32_t *>(v.d.arr[0]) + k.off_arr0;
  dataset_constants(v.mc, k);
}

template <class Model, int G, int BT>
__global__ void __launch_bounds__(BT, MinWavesOf<Model>::value) amwg_step_kernel_ds(const StepArgs a, const DatasetArgs ds) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  StepArgs v = a;
  dataset_view(v, ds);
  step_body<Model, G, BT>(v, smem);
}
template <class Model, int G, int BT>
__global__ void __launch_bounds__(BT, MinWavesOf<Model>::value) amwg_step_kernel_cert_ds(const StepArgs a, const DatasetArgs ds) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  StepArgs v = a;
  dataset_view(v, ds);
  step_body<Model, G, BT, false, false, true>(v, smem);
}

}  // namespace amwg
