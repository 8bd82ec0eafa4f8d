// amwg_user_kernels.h -- the step kernels of a translated closure's code object.  amwg_core.hip (user_program) hands hiprtc the closure's text and then this
// header, for one geometry: AMWG_USER_LANES lanes per chain in workgroups of AMWG_USER_BLOCK threads.  The host launches the kernel of its launch plan
// (amwg_core.hip variant_for); a kernel the closure has no body for at this geometry reports kErrNoKernelBody instead of returning as if it had stepped.
#if !defined(AMWG_USER_LANES) || !defined(AMWG_USER_BLOCK)
#error "amwg_user_kernels.h: define AMWG_USER_LANES and AMWG_USER_BLOCK first"
#endif

// the step kernel for this geometry (amwg_step_kernel's twin)
extern "C" __global__ void __launch_bounds__(AMWG_USER_BLOCK) amwg_user_step(const amwg::StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  amwg::step_body<amwg::UserModel, AMWG_USER_LANES>(a, smem);
}

// a closure with a row plan (amwg_rows.h: UserModel::kLaneReuse) on a whole wavefront per chain: the same stepper with the sweep prefetch (amwg_sweep_kernel's twin)
extern "C" __global__ void __launch_bounds__(AMWG_USER_BLOCK) amwg_user_sweep(const amwg::StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if constexpr (amwg::LaneReuseOf<amwg::UserModel>::value && AMWG_USER_LANES == 64 && AMWG_USER_BLOCK <= 512) amwg::step_body<amwg::UserModel, 64, 512, false, true>(a, smem);
  else amwg::device_error(a, amwg::kErrNoKernelBody);
}

// a row plan the translator marked kRowCert (amwg_rows.h: certified values + the expression in the reference's order): amwg_sweep_kernel_cert's twin
extern "C" __global__ void __launch_bounds__(AMWG_USER_BLOCK) amwg_user_sweep_cert(const amwg::StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if constexpr (amwg::LaneReuseOf<amwg::UserModel>::value && amwg::CertifiedAt<amwg::UserModel, 64>::value && amwg::CertNeedsRows<amwg::UserModel>::value && AMWG_USER_LANES == 64 &&
                AMWG_USER_BLOCK <= 512)
    amwg::step_body<amwg::UserModel, 64, 512, false, true, true>(a, smem);
  else amwg::device_error(a, amwg::kErrNoKernelBody);
}

// a closure with a certified tail (amwg_user.h norm_tail_approx, amwg_gtail.h glm_tail_approx<PoisLink>: UserModel::kCertified) at the lane count it has one for: the stepper
// that decides accept tests from it (amwg_step_kernel_cert's twin; BT: the wavefront's pass needs the 512 registers of a workgroup of at most 256 threads)
extern "C" __global__ void __launch_bounds__(AMWG_USER_BLOCK) amwg_user_step_cert(const amwg::StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if constexpr (amwg::CertifiedAt<amwg::UserModel, AMWG_USER_LANES>::value && !amwg::CertNeedsRows<amwg::UserModel>::value)
    amwg::step_body<amwg::UserModel, AMWG_USER_LANES, (AMWG_USER_BLOCK <= 256 ? 256 : 1024), false, false, true>(a, smem);
  else amwg::device_error(a, amwg::kErrNoKernelBody);
}

// a dataset sampler (amwg_create_user_datasets) launches the twins of the two step kernels; the host defines the macro in the compile options of such a sampler
// only, so an ordinary closure's code object stays what it was
#if defined(AMWG_USER_DATASETS)
#include "amwg_user_dataset.h"
#endif
