// amwg_lanes.h -- a double from lane ^ OFF of the wavefront without LDS: DPP moves inside a row of 16 lanes, v_permlane16_swap / v_permlane32_swap beyond.  dpp_xor
// serves the cross-lane butterflies of amwg_heldout.hip and amwg_predictive.hip; lane_pair is the latter's (the held-out merge is symmetric and keeps its own swap).  Device code; not a source of the step kernels (tools/build_id.py).
#pragma once
#include <hip/hip_runtime.h>

#include "amwg_math.h"

namespace amwg {

// the value of lane ^ OFF, OFF = 1, 2, 4, 8, by DPP moves in the VALU: quad permutes; row_half_mirror then the quad reversed (xor 7, xor 3); row_mirror then
// row_half_mirror (xor 15, xor 7)
template <int OFF> __device__ __forceinline__ double dpp_xor(double v) {
  int lo = (int)(uint32_t)f64_bits(v), hi = (int)(uint32_t)(f64_bits(v) >> 32);
  if constexpr (OFF == 1) {
    lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
  } else if constexpr (OFF == 2) {
    lo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true);
  } else if constexpr (OFF == 4) {
    lo = __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, true);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x1B, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x1B, 0xF, 0xF, true);
  } else {
    static_assert(OFF == 8, "DPP moves stay inside a row of 16 lanes");
    lo = __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, true);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, true);
  }
  return bits_f64(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

// v of the pair (lane, lane ^ OFF) IN LANE ORDER, the same in both lanes: low = the value of the lane whose bit OFF is clear, high = its partner's.  OFF = 16, 32:
// one swap with both operands the same register leaves exactly that -- the first result holds the even rows' (the lower half's) values, the second the others'.
// An asymmetric merge applied to (low, high) therefore gives both lanes the same bytes.
template <int OFF> __device__ __forceinline__ void lane_pair(double v, int lane, double &low, double &high) {
  if constexpr (OFF < 16) {
    const double p = dpp_xor<OFF>(v);
    const bool upper = (lane & OFF) != 0;
    low = upper ? p : v;
    high = upper ? v : p;
  } else {
    const uint32_t w0 = (uint32_t)f64_bits(v), w1 = (uint32_t)(f64_bits(v) >> 32);
    uint32_t x0, x1, y0, y1;
    if constexpr (OFF == 32) {
      const auto r0 = __builtin_amdgcn_permlane32_swap(w0, w0, false, false), r1 = __builtin_amdgcn_permlane32_swap(w1, w1, false, false);
      x0 = r0[0]; y0 = r0[1]; x1 = r1[0]; y1 = r1[1];
    } else {
      static_assert(OFF == 16, "lane distances 1, 2, 4, 8, 16, 32");
      const auto r0 = __builtin_amdgcn_permlane16_swap(w0, w0, false, false), r1 = __builtin_amdgcn_permlane16_swap(w1, w1, false, false);
      x0 = r0[0]; y0 = r0[1]; x1 = r1[0]; y1 = r1[1];
    }
    low = bits_f64(((uint64_t)x1 << 32) | x0);
    high = bits_f64(((uint64_t)y1 << 32) | y0);
  }
}

}  // namespace amwg
