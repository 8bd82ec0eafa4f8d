// amwg_user_dataset.h -- many datasets in one sampler for a TRANSLATED closure (amwg_create_user_datasets): the kernels' second argument and the entry points that use
// it.  The built-in families' counterpart is amwg_dataset.h, and everything said there holds here: chains keep their one global numbering, dataset d owns the local chains
// [d * cpd, (d + 1) * cpd), a workgroup serves exactly ONE dataset (amwg_plan.hip plans no other geometry), so d = blockIdx.x / blocks_per_dataset is wave-uniform.
//
// One generated source serves all datasets (translate.js translate_datasets: every dataset translates to the same text), and every data access of a closure goes
// through user_arr<J>(d) (amwg_user.h), i.e. through DataRef::arr and DataRef::arr_ext.  So a dataset is nothing but its row of a device table of pointers
// [n_datasets][row_stride]: the workgroup copies the row's first kInlineUserArrays entries into its DataRef and points arr_ext behind them.  The row's address is
// uniform -- scalar loads, the pointers live in scalar registers as the kernel arguments of an ordinary sampler do.  Nothing else changes: the per-chain arrays, the draws
// [row][P][C], the wavefront ids behind wave_scratch_of and the Philox key (seed, chain_offset + c) are those of an ordinary sampler, which is why dataset d's chains
// equal the chains of an amwg_create_user sampler on dataset d's arrays with chain_offset + d * cpd, bit for bit (tests/test_gpu_user_datasets.py).
//
// StepArgs stays the kernels' FIRST parameter and keeps its size: cold_args() (amwg_kernel.h) reads it through the kernel-argument pointer, and what is read that way --
// the per-chain arrays, the draws, thin -- is the same for every dataset.
//
// Compiled only for dataset samplers: amwg_user_kernels.h includes this header under AMWG_USER_DATASETS, which the host defines in the compile options (amwg_rtc.hip).
#pragma once
#include "amwg_kernel.h"

namespace amwg {

struct UserDatasetArgs {
  int32_t blocks_per_dataset, n_datasets;
  int32_t row_stride, n_arrays;             // entries per row: max(n_arrays, kInlineUserArrays), so that the copy below never reads past a row
  const void *const *table;                 // [n_datasets][row_stride], device memory: entry j of row d = array j of dataset d (nullptr past n_arrays)
};

// the argument block as the workgroup of dataset blockIdx.x / blocks_per_dataset sees it
__device__ __forceinline__ void user_dataset_view(StepArgs &v, const UserDatasetArgs &ds) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (made a scalar explicitly: the quotient of two scalars is formed with the vector unit's reciprocal)
  const int64_t d = (int64_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x / (uint32_t)ds.blocks_per_dataset));
#else
  const int64_t d = 0;
#endif
  const void *const *row = ds.table + d * (int64_t)ds.row_stride;      // (a uniform address: scalar loads)
#pragma unroll
  for (int j = 0; j < kInlineUserArrays; ++j) v.d.arr[j] = row[j];
  v.d.arr_ext = row + kInlineUserArrays;
}

}  // namespace amwg

// the dataset twins of amwg_user_step / amwg_user_step_cert (amwg_user_kernels.h): the same step_body on the workgroup's dataset.  (The host units include this
// header for UserDatasetArgs alone: no geometry, no kernels.)
// The certified twin instantiates the certified step_body for ANY CertifiedAt<UserModel, AMWG_USER_LANES> without rows: one lane per chain (the constant-mean normal
// tail) and 16 lanes per chain (the Poisson / logistic tails of a source marked kTailPerDataset: amwg_gtail.h).  At 16 lanes the four chains of a
// wavefront share every row of the data they read; a workgroup serves one dataset, so they share the constants of the bound too -- slots of that dataset's array
// `#tail:consts`, read through the same redirected user_arr<J>(d).
#if defined(AMWG_USER_LANES) && defined(AMWG_USER_BLOCK)
extern "C" __global__ void __launch_bounds__(AMWG_USER_BLOCK) amwg_user_step_ds(const amwg::StepArgs a, const amwg::UserDatasetArgs ds) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  amwg::StepArgs v = a;
  amwg::user_dataset_view(v, ds);
  amwg::step_body<amwg::UserModel, AMWG_USER_LANES>(v, smem);
}

extern "C" __global__ void __launch_bounds__(AMWG_USER_BLOCK) amwg_user_step_cert_ds(const amwg::StepArgs a, const amwg::UserDatasetArgs ds) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if constexpr (amwg::CertifiedAt<amwg::UserModel, AMWG_USER_LANES>::value && !amwg::CertNeedsRows<amwg::UserModel>::value) {
    amwg::StepArgs v = a;
    amwg::user_dataset_view(v, ds);
    amwg::step_body<amwg::UserModel, AMWG_USER_LANES, (AMWG_USER_BLOCK <= 256 ? 256 : 1024), false, false, true>(v, smem);
  } else amwg::device_error(a, amwg::kErrNoKernelBody);
}
#endif
