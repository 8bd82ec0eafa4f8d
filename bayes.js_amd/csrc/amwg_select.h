// amwg_select.h -- the device pieces of a most-significant-digit-first radix select over the monotone u64 key of an fp64 pattern, shared by the per-dataset
// quantiles (dataset_select_kernel, amwg_summaries.hip) and the thresholds of the highest-density interval (hpd_threshold_kernel, amwg_hpd.hip).  Device code
// only; internal to those two translation units, and not a source of the step kernels (tools/build_id.py).
#pragma once
#if !defined(__HIPCC_RTC__)      // (hiprtc -- amwg_pointwise.h for a translated closure -- has the runtime's names built in)
#include <hip/hip_runtime.h>

#include <cstdint>
#endif

__device__ inline uint64_t select_key(double v) {      // order of the doubles = order of the keys (-0 before +0)
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}
__device__ inline double select_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
}

// hist[slot] += 1 for every lane with `active`.  The draws of one posterior agree in sign, exponent and leading mantissa bits, so in the early passes all 64
// lanes name the same bin: the first lane still waiting broadcasts its slot, the lanes that agree are counted by a ballot and ONE lane adds the count; repeat
// while lanes wait.  The loop's trip count is the number of distinct slots in the wavefront.
__device__ inline void wave_count(uint32_t *hist, bool active, uint32_t slot) {
  const int lane = threadIdx.x & 63;
  uint64_t todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t ls = (uint32_t)__builtin_amdgcn_readlane((int)slot, leader);
    const uint64_t same = __ballot(active && slot == ls);
    if (lane == leader) atomicAdd(&hist[ls], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

// exclusive scan of one group's 256 bins in place, by one wavefront: four bins per lane
__device__ inline void select_scan(uint32_t *bins, int lane) {
  uint32_t *hb = bins + lane * 4;
  const uint32_t c0 = hb[0], c1 = hb[1], c2 = hb[2], c3 = hb[3], s = c0 + c1 + c2 + c3;
  uint32_t incl = s;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  const uint32_t excl = incl - s;
  hb[0] = excl; hb[1] = excl + c0; hb[2] = excl + c0 + c1; hb[3] = excl + c0 + c1 + c2;
}
