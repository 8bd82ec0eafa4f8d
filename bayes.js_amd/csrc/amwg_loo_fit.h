// amwg_loo_fit.h -- what a workgroup of PSIS-LOO's fit does to one observation's tail in LDS, shared by loo_fit_kernel (amwg_loo.hip) and loo_pred_fit_kernel
// (amwg_loo_predictive.hip) so that both form the same khat_i from the same bytes: the workgroup's sums, the bitonic network, the excesses and the generalised
// Pareto fit of include/amwg.h (amwg_last_sample_dataset_loo).  Every function is called by ALL threads of the workgroup (blockDim.x = 64 or kThreads) and holds
// barriers.  Device code; not a source of the step kernels (tools/build_id.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "amwg_pointwise.h"
#include "amwg_select.h"

namespace amwg {

constexpr int kMaxTheta = 128;                                    // 30 + floor(sqrt(M)) <= 120 for M < kLooTailCap
constexpr int kFitExtra = 2 * kMaxTheta + 16;                     // doubles of LDS of the fit beside the tail: L_j, w_j, the wavefronts' partial sums

// the sum of v over the workgroup's threads (one wavefront, or four), the same double in every thread: a butterfly over the lanes, then the wavefronts in the
// order 0, 1, 2, 3
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return blockDim.x == 64 ? red[0] : ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the bitonic network over keys[0 .. cap), cap a power of two, ascending; PAIRS: over (keys[t], ix[t]) in lexicographic order, so that equal keys end in the order
// of their draw indices whatever order the compaction placed them in.  The slots are loaded and a barrier passed before the call; ends behind a barrier
template <bool PAIRS>
__device__ __forceinline__ void loo_sort(uint64_t *keys, uint32_t *ix, uint32_t cap) {
  const uint32_t tid = threadIdx.x, T = blockDim.x;
  for (uint32_t kk = 2; kk <= cap; kk <<= 1) {
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (cap >> 1); t += T) {
        const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = a | j;
        const bool up = (a & kk) == 0;
        const uint64_t x = keys[a], y = keys[l];
        if constexpr (PAIRS) {
          const uint32_t p = ix[a], q = ix[l];
          if ((x > y || (x == y && p > q)) == up) { keys[a] = y; keys[l] = x; ix[a] = q; ix[l] = p; }
        } else {
          if ((x > y) == up) { keys[a] = y; keys[l] = x; }
        }
      }
      __syncthreads();
    }
  }
}

// THE EXCESSES AND THE FIT.  keys[0 .. M]: the sorted keys; a0, aM: the values of keys[0] and keys[M].  Unless M < 5 the excesses take the place of the keys (x_r at
// X[M - r], X = keys as doubles) and stay there.  raw: the raw route (M < 5, x* <= 0, x_M <= 0 or a khat that is not finite), khat = +inf
struct LooFit { bool raw; double khat, sigma, ec; };
__device__ __forceinline__ LooFit loo_gpd_fit(uint64_t *keys, double *Lj, double *Wj, double *red, uint32_t Mlen, int mm, double a0, double aM) {
  double *X = reinterpret_cast<double *>(keys);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t T = blockDim.x;
  const int waves = (int)(T >> 6);
  const double Md = (double)Mlen;
  LooFit f{Mlen < 5, kInf, 0.0, 0.0};
  if (f.raw) return f;
  const double ec = exp_v8(a0 - aM);
  f.ec = ec;
  __syncthreads();
  for (uint32_t t = tid; t < Mlen; t += T) X[t] = exp_v8(a0 - select_value(keys[t])) - ec;      // (slot t is read and written by the same thread)
  __syncthreads();
  const double xM = X[0], xs = X[Mlen - (Mlen + 2) / 4];      // x_M; x* = x_{floor(M / 4 + 0.5)}
  f.raw = !(xs > 0.0) || !(xM > 0.0);
  if (f.raw) return f;
  const double mmd = (double)mm;
  for (int j = wave + 1; j <= mm; j += waves) {
    const double theta = 1.0 / xM + (1.0 - ::sqrt(mmd / ((double)j - 0.5))) / (3.0 * xs);
    double s = 0.0;
    for (uint32_t t = lane; t < Mlen; t += 64) s += log1p_v8(-theta * X[t]);
    const double k = wave_sum(s) / Md;
    if (lane == 0) Lj[j - 1] = Md * (log_v8(-theta / k) - k - 1.0);
  }
  __syncthreads();
  if (tid < mm) {
    double z = 0.0;
    for (int q = 0; q < mm; ++q) z += exp_v8(Lj[q] - Lj[tid]);
    Wj[tid] = 1.0 / z;
  }
  __syncthreads();
  double th = 0.0;
  for (int j = 1; j <= mm; ++j) th += (1.0 / xM + (1.0 - ::sqrt(mmd / ((double)j - 0.5))) / (3.0 * xs)) * Wj[j - 1];
  double s = 0.0;
  for (uint32_t t = tid; t < Mlen; t += T) s += log1p_v8(-th * X[t]);
  const double kp = block_sum(s, red) / Md;
  f.sigma = -kp / th;
  const double khat = (Md * kp + 5.0) / (Md + 10.0);
  f.raw = !(__builtin_fabs(khat) < kInf);
  f.khat = f.raw ? kInf : khat;
  return f;
}

}  // namespace amwg
