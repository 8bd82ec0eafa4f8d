// amwg_kernels.hip -- the step-kernel instantiations of ONE built-in model family (compiled once per family, -DAMWG_FAMILY=0..3, so the
// four families build in parallel): amwg_step_kernel<Model, G, BT> for every lane count G and every workgroup size class BT, and beside each its
// dataset twin amwg_step_kernel_ds<Model, G, BT> (amwg_dataset.h) where the family has one.
//
// BT is the register budget the instantiation is compiled for (__launch_bounds__): workgroups of up to 256 threads may use 512
// VGPRs per lane, 512 threads 256, 1024 threads 128.  A chain on G > 64 lanes is exactly one workgroup of G threads, so those have
// one class each.  The host (amwg_plan.hip) reads the family's row of facts (amwg_host.h FamilyRow), exported at the end of this file: the two lookups
// of the kernel for (G, workgroup size) -- each answers with the ordinary kernel and its twin together (KernelPair) --, the LDS bytes of the family's
// data and its largest workgroup.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "amwg_dataset.h"
#include "amwg_host.h"
#include "amwg_kernel.h"
#include "amwg_models.h"
#include "amwg_normal1.h"

using namespace amwg;

#if AMWG_FAMILY == 0
using Family = NormalModel;
#elif AMWG_FAMILY == 1
using Family = BetaBernModel;
#elif AMWG_FAMILY == 2
using Family = HierNormalModel;
#elif AMWG_FAMILY == 3
using Family = PoisGlmModel;
#else
#error "AMWG_FAMILY must be 0..3"
#endif

namespace {

#if defined(AMWG_X_BT1024)       // development experiment: every instantiation with the 1024-thread register budget, as in round 2
constexpr int class_of(int) { return 1024; }
#else
constexpr int class_of(int block) { return block <= 256 ? 256 : (block <= 512 ? 512 : 1024); }
#endif

// Which families have dataset twins: every one but the hierarchical family, whose plan depends on properties of the labels.  The pair of one
// instantiation: the branch a family has no twin for is never instantiated, so its object holds no kernel it cannot launch.
constexpr bool kHasTwin = !std::is_same_v<Family, HierNormalModel>;
template <int G, int BT>
KernelPair step_pair() {
  if constexpr (kHasTwin) return {amwg_step_kernel<Family, G, BT>, amwg_step_kernel_ds<Family, G, BT>};
  else return {amwg_step_kernel<Family, G, BT>, nullptr};
}

template <int G>
KernelPair single_wave(int block) {      // G <= 64: any workgroup size up to the family's cap
  switch (class_of(block)) {
    case 256: return step_pair<G, 256>();
    case 512: if constexpr (Family::kMaxThreads >= 512) return step_pair<G, 512>(); else return {};
    default: if constexpr (Family::kMaxThreads >= 1024) return step_pair<G, 1024>(); else return {};
  }
}
template <int G>
KernelPair multi_wave(int block) {       // G > 64: one chain = one workgroup of G threads
  if (block != G) return {};
  if constexpr (G <= Family::kMaxThreads) return step_pair<G, class_of(G)>();
  else return {};
}

}  // namespace

#if AMWG_FAMILY == 2
// the group-local kernel of the hierarchical family (amwg_gl.h): a chain on one wavefront, any workgroup size class
step_kernel_t amwg_kernel_hier_gl(int block) {
  switch (class_of(block)) {
    case 256: return amwg_gl_kernel<HierGlModel, 256>;
    case 512: return amwg_gl_kernel<HierGlModel, 512>;
    default: return amwg_gl_kernel<HierGlModel, 1024>;
  }
}
#endif

#if AMWG_FAMILY == 2
// the sweep kernel of the hierarchical family (row layout, 64 lanes per chain: amwg_kernel.h kSweep)
step_kernel_t amwg_kernel_hier_sweep(int block) {
  switch (class_of(block)) {
    case 256: return amwg_sweep_kernel<HierNormalModel, 256>;
    case 512: return amwg_sweep_kernel<HierNormalModel, 512>;
    default: return amwg_sweep_kernel<HierNormalModel, 1024>;
  }
}
#endif

// the kernel that decides from certified values (amwg_kernel.h kCert; options.full_evaluation = 0), for the lane count the family has one at: the ordinary
// stepper (Normal: one lane per chain; Poisson: 16), or -- families whose certified value needs the row layout -- the sweep kernel (hierarchical: 64 lanes,
// workgroups of at most 512 threads), which has no twin.  {}: none.
namespace {
template <class Family, int BT>      // (templates: the branches a family has no kernel for must not be instantiated)
KernelPair cert_pair() {
  constexpr int GC = CertifiedOf<Family>::lanes;
  if constexpr (CertNeedsRows<Family>::value) return {amwg_sweep_kernel_cert<Family, BT>, nullptr};
  else if constexpr (kHasTwin) return {amwg_step_kernel_cert<Family, GC, BT>, amwg_step_kernel_cert_ds<Family, GC, BT>};
  else return {amwg_step_kernel_cert<Family, GC, BT>, nullptr};
}
template <class Family>
KernelPair certified_lookup(int lanes, int block) {
  if constexpr (CertifiedOf<Family>::value) {
    if (lanes != CertifiedOf<Family>::lanes) return {};
    constexpr int cap = CertNeedsRows<Family>::value ? 512 : Family::kMaxThreads;
    switch (class_of(block)) {
      case 256: return cert_pair<Family, 256>();
      case 512: if constexpr (cap >= 512) return cert_pair<Family, 512>(); else return {};
      default: if constexpr (cap >= 1024) return cert_pair<Family, 1024>(); else return {};
    }
  }
  (void)lanes; (void)block;
  return {};
}
KernelPair certified(int lanes, int block) { return certified_lookup<Family>(lanes, block); }

KernelPair lookup(int lanes, int block) {
  switch (lanes) {
    case 1: return single_wave<1>(block);
    case 2: return single_wave<2>(block);
    case 4: return single_wave<4>(block);
    case 8: return single_wave<8>(block);
    case 16: return single_wave<16>(block);
    case 32: return single_wave<32>(block);
    case 64: return single_wave<64>(block);
    case 128: return multi_wave<128>(block);
    case 256: return multi_wave<256>(block);
    case 512: return multi_wave<512>(block);
    case 1024: return multi_wave<1024>(block);
  }
  return {};
}
}  // namespace

template <> FamilyRow amwg_family_row<AMWG_FAMILY>() {
  return {lookup, certified, [](int n_obs, int groups, int lanes) -> size_t { return Family::lds_bytes(n_obs, groups, lanes); }, Family::kMaxThreads};
}
