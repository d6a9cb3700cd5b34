// nd_amd/csrc/lanes.hpp -- what a lane takes from the other lanes of its wave (64 lanes), written once.  Device only.
//
//   lane_from_prev / lane_from_next   the value of lane i - 1 / i + 1 by a DPP wave shift (wave_shr:1 / wave_shl:1,
//       bound_ctrl: lane 0 / lane 63, which has no such neighbour, receives 0).  No LDS; a double crosses as two
//       moves.  The register-window filters (correlate.hip) and the paired patch sums of non-local means (nlmeans.hip).
//   wave_sum   the sum over the wave in EVERY lane by the xor butterfly (32, 16, .., 1): one fixed tree, so a
//       floating-point sum repeats bit for bit (kmeans_fit.hip).  (classify.hip's __shfl_down reductions leave
//       the sum in lane 0 only: another operation.)
#pragma once

#include <hip/hip_runtime.h>

namespace nd_amd {

template <int CTRL>
__device__ __forceinline__ int lane_shift(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ float lane_shift(float x)
{
    return __builtin_bit_cast(float, lane_shift<CTRL>(__builtin_bit_cast(int, x)));
}
template <int CTRL>
__device__ __forceinline__ double lane_shift(double x)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)lane_shift<CTRL>((int)(unsigned)u);
    const unsigned hi = (unsigned)lane_shift<CTRL>((int)(unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

template <typename T>
__device__ __forceinline__ T lane_from_prev(T x) { return lane_shift<0x138>(x); }      // lane i <- lane i - 1 (lane 0 <- 0)
template <typename T>
__device__ __forceinline__ T lane_from_next(T x) { return lane_shift<0x130>(x); }      // lane i <- lane i + 1 (lane 63 <- 0)

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace nd_amd
