// intrachoose_dev.h -- what the two kernels of intrachoose.hip share: the candidate codes and the wavefront's copies of
// the winner (a sample block, a level block, a context row).
#pragma once
#include "common.h"
#include "dist_dev.h"

namespace {

constexpr int IC_WAVES = 4, IC_THREADS = 64 * IC_WAVES;                   // a wavefront per PU
constexpr int IC_MAX_CAND = 16 * 5;                                       // n_modes x n_tr
constexpr unsigned IC_EMT_SIG_NUM_THR = 2;                                // g_EmtSigNumThr (Rom.cpp:504)
constexpr unsigned IC_VALID = 1, IC_CBF = 2, IC_TS = 4, IC_PASSED = 8;

__device__ __forceinline__ unsigned ic_align_of(const void* a, const void* b) { return (unsigned)((uintptr_t)a | (uintptr_t)b); }

// w x h samples, w and h powers of two from 2: chunks of 4 samples (2 when w is 2) over the lanes.  Where both blocks start on an 8-byte boundary and
// both strides keep the rows there, every chunk is one 8-byte word; else the chunk's own two addresses decide between 8-, 4- and 2-byte words
__device__ __forceinline__ void ic_copy_block(const Pel* __restrict__ src, int sstride, Pel* __restrict__ dst, int dstride, int w, int h, int lane)
{
  const int lu = w >= 4 ? 2 : 1, lcpr = ilog2(w >> lu), total = h << lcpr, cmask = (1 << lcpr) - 1;
  if (lu == 2 && !(ic_align_of(src, dst) & 7u) && !((sstride | dstride) & 3))
  {
    int i = lane;
    for (; i + 192 < total; i += 256)                                     // four words in flight per lane
    {
      uint2 v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) { const int c = i + 64 * k; v[k] = *reinterpret_cast<const uint2*>(src + (long long)(c >> lcpr) * sstride + ((c & cmask) << 2)); }
#pragma unroll
      for (int k = 0; k < 4; k++) { const int c = i + 64 * k; *reinterpret_cast<uint2*>(dst + (long long)(c >> lcpr) * dstride + ((c & cmask) << 2)) = v[k]; }
    }
    for (; i < total; i += 64)
      *reinterpret_cast<uint2*>(dst + (long long)(i >> lcpr) * dstride + ((i & cmask) << 2)) =
          *reinterpret_cast<const uint2*>(src + (long long)(i >> lcpr) * sstride + ((i & cmask) << 2));
    return;
  }
  for (int i = lane; i < total; i += 64)
  {
    const Pel* const s = src + (long long)(i >> lcpr) * sstride + ((i & cmask) << lu);
    Pel* const d = dst + (long long)(i >> lcpr) * dstride + ((i & cmask) << lu);
    const unsigned al = ic_align_of(s, d);
    if (lu == 2 && !(al & 7u)) *reinterpret_cast<uint2*>(d) = *reinterpret_cast<const uint2*>(s);
    else if (!(al & 3u))
    {
      reinterpret_cast<unsigned*>(d)[0] = reinterpret_cast<const unsigned*>(s)[0];
      if (lu == 2) reinterpret_cast<unsigned*>(d)[1] = reinterpret_cast<const unsigned*>(s)[1];
    }
    else
    {
      d[0] = s[0]; d[1] = s[1];
      if (lu == 2) { d[2] = s[2]; d[3] = s[3]; }
    }
  }
}

// count contiguous levels, count a multiple of 4: 16-byte words where both blocks allow them, else 8- or 4-byte ones
__device__ __forceinline__ void ic_copy_levels(const TCoeff* __restrict__ src, TCoeff* __restrict__ dst, int count, int lane)
{
  const unsigned al = ic_align_of(src, dst);
  if (!(al & 15u))
  {
    const int total = count >> 2;
    const uint4* const s = reinterpret_cast<const uint4*>(src);
    uint4* const d = reinterpret_cast<uint4*>(dst);
    int i = lane;
    for (; i + 192 < total; i += 256)
    {
      uint4 v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = s[i + 64 * k];
#pragma unroll
      for (int k = 0; k < 4; k++) d[i + 64 * k] = v[k];
    }
    for (; i < total; i += 64) d[i] = s[i];
  }
  else if (!(al & 7u))
  {
    const uint2* const s = reinterpret_cast<const uint2*>(src);
    uint2* const d = reinterpret_cast<uint2*>(dst);
    for (int i = lane; i < (count >> 1); i += 64) d[i] = s[i];
  }
  else
    for (int i = lane; i < count; i += 64) dst[i] = src[i];
}

// one context row (VVCGPU_RESI_RATE_CTX_BYTES = 3 x 64 bytes)
__device__ __forceinline__ void ic_copy_row(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int lane)
{
  static_assert(VVCGPU_RESI_RATE_CTX_BYTES == 192, "three bytes per lane");
  if (!(ic_align_of(src, dst) & 3u))
  {
    if (lane < 48) reinterpret_cast<unsigned*>(dst)[lane] = reinterpret_cast<const unsigned*>(src)[lane];
  }
  else
  {
    const unsigned char b0 = src[lane], b1 = src[64 + lane], b2 = src[128 + lane];
    dst[lane] = b0; dst[64 + lane] = b1; dst[128 + lane] = b2;
  }
}

}  // namespace
