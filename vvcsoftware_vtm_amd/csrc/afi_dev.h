// afi_dev.h -- device functions of the affine gradient search shared by the per-iteration entry (affine.hip) and the whole-PU search
// (affine_me.hip, afm_dev.h): the transposed wave reduction, the error / Sobel / normal-equation pass and the distortion over a prediction held in LDS.
// Reference behaviour: AffineGradientSearch.cpp:66-174, InterSearch.cpp:3446-3534 (see affine.hip).
#pragma once
#include "common.h"
#include "dist_dev.h"

constexpr int AFI_MAX = 128, AFI_WAVE_MAX = 1024;          // PUs of up to AFI_WAVE_MAX samples are served by one wavefront each, larger ones by a workgroup
typedef const __attribute__((address_space(3))) Pel* AfiLdsPel;

// NT = 64: the wavefront owns the PU; NT = 256: the four wavefronts of the workgroup share it and their sums meet in `red`
// this lane's share of the P x (P + 1) sums; OrgPtr: the original's pointer type (plain: global memory; AfiLdsPel: a block the caller keeps in LDS)
template <int P, int NT, class OrgPtr = const Pel*>
__device__ __forceinline__ void afi_accumulate(const vvcgpu_affine_iter& d, OrgPtr __restrict__ org, const Pel* predL, int w, int h,
                                               long long (&acc)[P][P + 1], int tid)
{
#pragma unroll
  for (int c = 0; c < P; c++)
#pragma unroll
    for (int r = 0; r <= P; r++) acc[c][r] = 0;
  for (int i = tid; i < w * h; i += NT)
  {
    const int j = i / w, k = i - j * w;
    const int yy = min(max(j, 1), h - 2), xx = min(max(k, 1), w - 2);
    const Pel* c = predL + yy * w + xx;
    const int x = c[1 - w] - c[-1 - w] + (c[1] << 1) - (c[-1] << 1) + c[1 + w] - c[-1 + w];
    const int y = c[w - 1] - c[-w - 1] + (c[w] << 1) - (c[-w] << 1) + c[w + 1] - c[-w + 1];
    int iC[P];
    if (P == 4) { iC[0] = x; iC[1] = k * x + j * y; iC[2] = y; iC[3] = j * x - k * y; }
    else        { iC[0] = x; iC[1] = k * x; iC[2] = y; iC[3] = k * y; iC[4] = j * x; iC[5] = j * y; }
    const long long r = (long long)(Pel)((int)org[(size_t)j * d.org_stride + k] - (int)predL[j * w + k]);      // the error block is a Pel block
#pragma unroll
    for (int col = 0; col < P; col++)
    {
#pragma unroll
      for (int row = 0; row < P; row++) acc[col][row] += (long long)iC[col] * iC[row];
      acc[col][P] += ((long long)iC[col] * r) << 3;
    }
  }
}

// total: lane L holds this wave's sum of value L = acc[L / (P + 1)][L % (P + 1)]; -> out[7][7] (the wave's, or the workgroup's through `red`)
template <int P, int NT>
__device__ __forceinline__ void afi_publish(long long total, long long* out, long long (*red)[64], int tid)
{
  const int lane = tid & 63, wave = tid >> 6;
  const int row7 = lane / 7, col7 = lane - row7 * 7;
  const bool used = row7 >= 1 && row7 <= P && col7 <= P;
  const int src = used ? (row7 - 1) * (P + 1) + col7 : 0;
  if (NT == 64)
  {
    const long long val = __shfl(total, src & 63);
    if (lane < 49) out[lane] = used ? val : 0;
  }
  else
  {
    red[wave][lane] = total;
    __syncthreads();
    if (tid < 49) out[tid] = used ? red[0][src] + red[1][src] + red[2][src] + red[3][src] : 0;
  }
}

// The transposed wave reduction: sums of per-lane values over the wavefront with a halving butterfly.  At every stage a lane keeps one half of its
// values and hands the other half to its partner, so LEN - 1 shuffles replace 6 per value.  One stage per instantiation: every index is a constant, so
// v stays in registers.  v[0] of lane L ends as the sum of value L % LEN over the LEN lanes that share L / LEN.
template <int LEN>
__device__ __forceinline__ void afi_fold(long long (&v)[LEN], int lane)
{
  if constexpr (LEN > 1)
  {
    constexpr int s = LEN / 2;
    const bool up = (lane & s) != 0;
    long long u[s];
#pragma unroll
    for (int i = 0; i < s; i++)
    {
      const long long keep = up ? v[i + s] : v[i], send = up ? v[i] : v[i + s];
      u[i] = keep + __shfl_xor(send, s);
    }
    afi_fold<s>(u, lane);
    v[0] = u[0];
  }
}

// accumulate(acc) fills acc[P][P + 1], this lane's share of the sums (a callable, so that acc lives here: handing the array in changes the instruction
// streams of the whole-PU searches); then over the wavefront and into out[7][7], 32 values at a time (at most 32 + 16 for the 42 sums of the
// 6-parameter model: 64 registers, 49 shuffles); integer sums, so the result is the same whatever the order
template <int P, int NT, class Accumulate>
__device__ __forceinline__ void afi_reduce_publish(Accumulate accumulate, long long* out, long long (*red)[64], int tid)
{
  const int lane = tid & 63;
  long long acc[P][P + 1];
  accumulate(acc);
  long long a[32];
#pragma unroll
  for (int i = 0; i < 32; i++) a[i] = i < P * (P + 1) ? acc[i / (P + 1)][i % (P + 1)] : 0;
  afi_fold<32>(a, lane);
  long long total = a[0] + __shfl_xor(a[0], 32);                // lane L: value L % 32
  if constexpr (P * (P + 1) > 32)
  {
    long long b[16];
#pragma unroll
    for (int i = 0; i < 16; i++) b[i] = 32 + i < P * (P + 1) ? acc[(32 + i) / (P + 1)][(32 + i) % (P + 1)] : 0;
    afi_fold<16>(b, lane);
    long long tb = b[0] + __shfl_xor(b[0], 16);
    tb += __shfl_xor(tb, 32);                                    // lane L: value 32 + L % 16
    if (lane >= 32) total = tb;                                  // lanes 32 .. 47: value L
  }
  afi_publish<P, NT>(total, out, red, tid);
}

// the normal equations of one iteration: the error / Sobel pass over the PU, then the sums into out[7][7]
template <int P, int NT, class OrgPtr = const Pel*>
__device__ __forceinline__ void afi_equations(const vvcgpu_affine_iter& d, OrgPtr __restrict__ org, const Pel* predL, int w, int h, long long* out,
                                              long long (*red)[64], int tid)
{
  afi_reduce_publish<P, NT>([&](long long (&acc)[P][P + 1]) { afi_accumulate<P, NT, OrgPtr>(d, org, predL, w, h, acc, tid); }, out, red, tid);
}

// distortion of rows [r0, r1) x 16 of the PU against the prediction in LDS, by one wavefront
template <class OrgPtr = const Pel*>
__device__ __forceinline__ unsigned long long afi_dist(const vvcgpu_affine_iter& d, OrgPtr __restrict__ org, const Pel* predL, int w, int h,
                                                       int distKind, int band0, int bandStep, int lane)
{
  // bands of sixteen rows: every Hadamard tile of an affine PU (both sides >= 16) is at most sixteen rows high, the tile shape is the whole PU's
  unsigned long long sum = 0;
  for (int b = band0; b * 16 < h; b += bandStep)
  {
    OrgPtr o = org + (size_t)b * 16 * d.org_stride;
    AfiLdsPel c = (AfiLdsPel)predL + b * 16 * w;
    if (distKind == 1) sum += satd_block<64, AfiLdsPel, OrgPtr>(o, d.org_stride, c, w, w, 16, lane, 0, h);
    else
    {
      unsigned s = 0;
      for (int i = lane; i < 16 * w; i += 64) { const int j = i / w, k = i - j * w; s += (unsigned)abs((int)o[(size_t)j * d.org_stride + k] - (int)c[j * w + k]); }
      sum += wave_sum((unsigned long long)s);
    }
  }
  return sum;
}
