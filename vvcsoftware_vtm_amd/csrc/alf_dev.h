// alf_dev.h -- what the ALF kernels of alf.hip (classifier, filter) and of alfstats.hip (covariances) share on the device: the clamped tile loads
// and the tap index of the diamonds.  The block classifier they share is text, alf_quad_sums.inc and alf_class_key.inc, included where it runs.
#pragma once
#include "common.h"

// ---- clamped tile loads: rows [y0, y0+rows) x cols [x0, x0+PITCH) of the plane as int16 in LDS, replicating the picture border
// (== extendBorderPel).  x0 is a multiple of 4 samples, PITCH a multiple of 4; item v of a tile is the 8-byte vector (v / VPR, 4 (v % VPR)).
__device__ __forceinline__ bool tile_vec_ok(const Pel* src, int stride) { return ((stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(src) & 7) == 0); }

template <int PITCH>
__device__ __forceinline__ void load_tile_clamped(short* __restrict__ lds, const Pel* __restrict__ src,
                                                  int stride, int w, int h, int x0, int y0, int rows,
                                                  int tid, int nthreads)
{
  constexpr int VPR = PITCH / 4;                      // 8-byte vectors per row
  const int nvec = rows * VPR;
  const bool vec_ok = tile_vec_ok(src, stride);
  for (int v = tid; v < nvec; v += nthreads)
  {
    const int r = v / VPR, c = (v - r * VPR) * 4;
    pel4 val;
#define PEL4_DST val
#include "alf_pel4_clamped.inc"
#undef PEL4_DST
    *reinterpret_cast<pel4*>(lds + r * PITCH + c) = val;
  }
}

// the same in two halves, NB vectors per thread: tile_fetch issues every load into registers, tile_store writes them to LDS -- the simple
// loop pays one trip to memory per iteration, and a caller can put other work between the halves
template <int PITCH, int NB>
__device__ __forceinline__ void tile_fetch(pel4 (&val)[NB], const Pel* __restrict__ src, int stride, int w, int h, int x0, int y0, int rows,
                                           int tid, int nthreads)
{
  constexpr int VPR = PITCH / 4;
  const int nvec = rows * VPR;
  const bool vec_ok = tile_vec_ok(src, stride);
#pragma unroll
  for (int u = 0; u < NB; u++)
  {
    const int v = tid + u * nthreads;
    val[u] = pel4{ 0, 0, 0, 0 };
    if (v >= nvec) continue;
    const int r = v / VPR, c = (v - r * VPR) * 4;
#define PEL4_DST val[u]
#include "alf_pel4_clamped.inc"
#undef PEL4_DST
  }
}
template <int PITCH, int NB>
__device__ __forceinline__ void tile_store(short* __restrict__ lds, const pel4 (&val)[NB], int rows, int tid, int nthreads)
{
  constexpr int VPR = PITCH / 4;
  const int nvec = rows * VPR;
#pragma unroll
  for (int u = 0; u < NB; u++)
  {
    const int v = tid + u * nthreads;
    if (v >= nvec) continue;
    const int r = v / VPR, c = (v - r * VPR) * 4;
    *reinterpret_cast<pel4*>(lds + r * PITCH + c) = val[u];
  }
}

// coefficient index K(dy,dx) of the point-symmetric diamonds (AdaptiveLoopFilter.cpp:600-636 == calcCovariance t=0: the canonical tap index)
template <bool IS7>
__device__ __forceinline__ constexpr int tapIndex(int dy, int dx)
{
  if (dy < 0 || (dy == 0 && dx < 0)) { dy = -dy; dx = -dx; }
  if (IS7)
  {
    if (dy == 3) return dx == 0 ? 0 : -1;
    if (dy == 2) return dx == 1 ? 1 : dx == 0 ? 2 : dx == -1 ? 3 : -1;
    if (dy == 1) return (dx >= -2 && dx <= 2) ? 6 - dx : -1;
    return dx <= 3 ? 12 - dx : -1;
  }
  else
  {
    if (dy == 2) return dx == 0 ? 0 : -1;
    if (dy == 1) return (dx >= -1 && dx <= 1) ? 2 - dx : -1;
    if (dy == 0) return dx <= 2 ? 6 - dx : -1;
    return -1;
  }
}
