// wave_dev.h -- what a wavefront does with one value of each of its lanes: the barriers of a wavefront that owns its work (wave_sync, wave_global_sync:
// common.h), butterfly sums, maxima and minima, and the DPP minima of the searches.  Reductions over a view of a TU or over a team of a search round
// are other operations and stay with their kernels.
#pragma once
#include "common.h"

// Sum over an aligned group of G lanes (G = 16: four descriptors side by side in a wave; G = 64: the wave); every lane of the group ends with it.
// T: int, unsigned, long long, unsigned long long.
template <int G, class T>
__device__ __forceinline__ T group_sum(T v)
{
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <class T> __device__ __forceinline__ T wave_sum(T v) { return group_sum<64>(v); }
template <class T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

// minimum of a 32-bit value over the wavefront with DPP row operations (no LDS traffic, 6 VALU); the result is wave-uniform
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
#define WMIN_STEP(CTRL, ROWMASK) v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROWMASK, 0xF, false))
  WMIN_STEP(0xB1, 0xF);      // quad_perm [1,0,3,2]
  WMIN_STEP(0x4E, 0xF);      // quad_perm [2,3,0,1]
  WMIN_STEP(0x141, 0xF);     // row_half_mirror
  WMIN_STEP(0x140, 0xF);     // row_mirror: every lane of a 16-lane row holds the row's minimum
  WMIN_STEP(0x142, 0xA);     // row_bcast15 into rows 1 and 3
  WMIN_STEP(0x143, 0xC);     // row_bcast31 into rows 2 and 3: lane 63 holds the minimum of all four rows
#undef WMIN_STEP
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// 64-bit minimum as two 32-bit passes: the high words first, then the low words of the lanes that hold the minimal high word
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k)
{
  const unsigned hi = (unsigned)(k >> 32), lo = (unsigned)k;
  const unsigned hmin = wave_min_u32(hi);
  const unsigned lmin = wave_min_u32(hi == hmin ? lo : 0xFFFFFFFFu);
  return ((unsigned long long)hmin << 32) | lmin;
}
