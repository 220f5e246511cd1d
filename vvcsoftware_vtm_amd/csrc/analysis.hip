// analysis.hip -- encoder picture analysis for gfx950: the per-picture scalars the reference computes outside its CTU loop, from planes that are
// already resident in HBM.  Every device result is an integer, bit-exact with the reference; where the reference goes on in double the host
// helpers at the end of this file finish the integers in the reference's order (no floating-point sum is formed on the device).
//
// Reference behaviour reproduced:
//   filterAndCalculateAverageEnergies        EncoderLib/EncSlice.cpp:156-184      (saAct; per CTU :1405-1448, whole plane :208-247)
//   calcWeightedSquaredError                 EncoderLib/EncGOP.cpp:2661-2717      (ssErr, saAct per WPSNR block)
//   EncGOP::xFindDistortionPlane             EncoderLib/EncGOP.cpp:2720-2828      (plain SSE; the WPSNR sum is finished on the host)
//   xCalcHistogram                           EncoderLib/WeightPredAnalysis.cpp:79-99
//   WeightPredAnalysis::xCalcACDCParamSlice  EncoderLib/WeightPredAnalysis.cpp:245-301  (host, from the histogram)
//   xCalcSADvalueWP / ...OptionalClip        EncoderLib/WeightPredAnalysis.cpp:653-735
//   EncCu::updateCtuDataISlice / xCalcHADs8x8_ISlice   EncoderLib/EncCu.cpp:374-485, EncSlice::calCostSliceI EncSlice.cpp:1163-1204
//
// All kernels are single streaming reads.  A lane owns SPL neighbouring samples of a row (one 16- or 8-byte load where base and stride allow,
// sample-wise loads otherwise and for the chunk that crosses the plane's right edge) and walks down a band of rows; the 3 x 3 high-pass filter takes its
// rows from the registers of the walk and its left / right samples from the neighbouring lanes (the wave's two outer lanes load one sample more).
// Per-lane partials are 32 bit only over a band (<= 64 samples a lane, see the bounds at each kernel), 64 bit from the wave reduction on.
#include <math.h>
#include "common.h"
#include "wave_dev.h"

namespace {

typedef unsigned long long u64;

// SPL samples of a row from column x on: one vector load when the chunk lies inside the row and the plane is aligned for it, else sample by
// sample; columns from w on read as 0 (the callers mask them)
template <int SPL>
__device__ __forceinline__ void load_chunk(const Pel* __restrict__ row, int x, int w, bool vec, int (&v)[SPL])
{
  if (vec && x + SPL <= w)
  {
    if constexpr (SPL == 8)
    {
      const pel8 q = *reinterpret_cast<const pel8*>(row + x);
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = q[j];
    }
    else
    {
      const pel4 q = *reinterpret_cast<const pel4*>(row + x);
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = q[j];
    }
  }
  else
  {
#pragma unroll
    for (int j = 0; j < SPL; j++) v[j] = x + j < w ? (int)row[x + j] : 0;
  }
}

// the neighbour lanes' values: every lane takes part (DPP wave_shr:1 / wave_shl:1, as the SAO strip walk); lanes 0 / 63 get 0 and use what they loaded
__device__ __forceinline__ int from_left_lane(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, false); }
__device__ __forceinline__ int from_right_lane(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xF, 0xF, false); }

template <int SPL> struct VecOf;
template <> struct VecOf<8> { typedef pel8 type; };
template <> struct VecOf<4> { typedef pel4 type; };

// ---- tile statistics and plain SSE -------------------------------------------------------------------------------------------------------------------
// fast: plane(s) aligned for the lane's vector load and the width a multiple of SPL -- every load of the walk is one unconditional vector load
struct TsPlane { const Pel* org; const Pel* rec; u64* out; int ostride, rstride, w, h, tile, tilesX, lpt, unitsX, unitEnd, fast, vec; };   // vec: bit 0 org, bit 1 rec may take vector loads
struct Ts3 { TsPlane a[3]; int total; };

// The band of one lane: RB rows x SPL columns from (x, y0).  FAST: all rows of the band (and the row above and below it for the filter) are requested
// before the first is used -- the pass is bound by memory-level parallelism; lanes right of the plane load the plane's last chunk (masked).  Else row by
// row, sample-wise wherever a vector load is not possible.
// 32-bit partials of a lane over its RB * SPL <= 64 samples: |f| <= 12 * 1023 -> 7.9e5, sum <= 6.6e4, squared error <= 1023^2 * 64 = 6.7e7.
template <int SPL, int RB, bool FILT, bool FAST>
__device__ __forceinline__ void ts_band(const TsPlane& a, int lane, int x, int y0, unsigned& act, unsigned& sum, unsigned& sse)
{
  typedef typename VecOf<SPL>::type V;
  constexpr int NR = FILT ? RB + 2 : RB, R0 = FILT ? -1 : 0;                  // rows held, first row relative to the band
  const int w = a.w, h = a.h;
  const bool hasRec = a.rec != nullptr;
  const bool edgeL = lane == 0, edgeR = lane == 63;
  const int xc = FAST ? min(x, w - SPL) : min(x, w - 1);
  // the wave's outer lanes fetch the one sample their neighbour lane cannot give; the other lanes read a sample of their own chunk
  const int ex = edgeL ? min(max(x - 1, 0), w - 1) : edgeR ? min(x + SPL, w - 1) : xc;
  V vo[NR], vr[RB];
  int eo[NR];
  if constexpr (FAST)
  {
#pragma unroll
    for (int i = 0; i < NR; i++)
    {
      const Pel* row = a.org + (size_t)min(max(y0 + R0 + i, 0), h - 1) * a.ostride;
      vo[i] = *reinterpret_cast<const V*>(row + xc);
      if constexpr (FILT) eo[i] = row[ex];
    }
    if (hasRec)
    {
#pragma unroll
      for (int i = 0; i < RB; i++) vr[i] = *reinterpret_cast<const V*>(a.rec + (size_t)min(y0 + i, h - 1) * a.rstride + xc);
    }
  }
  auto row_of = [&](int i, int (&A)[SPL + 2])                                // held row i with its left and right neighbours
  {
    int e = 0;
    if constexpr (FAST)
    {
#pragma unroll
      for (int j = 0; j < SPL; j++) A[j + 1] = vo[i][j];
      if constexpr (FILT) e = eo[i];
    }
    else
    {
      const Pel* row = a.org + (size_t)min(max(y0 + R0 + i, 0), h - 1) * a.ostride;
      int v[SPL];
      load_chunk<SPL>(row, xc, w, (a.vec & 1) != 0, v);
#pragma unroll
      for (int j = 0; j < SPL; j++) A[j + 1] = v[j];
      if constexpr (FILT) e = row[ex];
    }
    if constexpr (FILT)
    {
      const int fromL = from_left_lane(A[SPL]), fromR = from_right_lane(A[1]);
      A[0] = edgeL ? e : fromL;
      A[SPL + 1] = edgeR ? e : fromR;
    }
  };
  int A0[SPL + 2], A1[SPL + 2], A2[SPL + 2];                                  // rows y - 1, y, y + 1
  if constexpr (FILT) { row_of(0, A1); row_of(1, A2); }
#pragma unroll
  for (int i = 0; i < RB; i++)
  {
    const int y = y0 + i;
    if constexpr (FILT)
    {
#pragma unroll
      for (int j = 0; j < SPL + 2; j++) { A0[j] = A1[j]; A1[j] = A2[j]; }
      row_of(i + 2, A2);
    }
    else row_of(i, A1);
    const bool rowIn = y < h && x < w;
    if constexpr (FILT)
    {
      // f = 12 c - 2 (l + r + u + d) - diagonals = 16 c - S[j-1] - 2 S[j] - S[j+1] with the column sums S = up + 2 mid + down
      int S[SPL + 2];
#pragma unroll
      for (int j = 0; j < SPL + 2; j++) S[j] = A0[j] + 2 * A1[j] + A2[j];
      const bool rowAct = rowIn && y >= 1 && y <= h - 2;
#pragma unroll
      for (int j = 0; j < SPL; j++)
      {
        const int f = 16 * A1[j + 1] - S[j] - 2 * S[j + 1] - S[j + 2];
        const int xx = x + j;
        if (rowAct && xx >= 1 && xx <= w - 2) act += (unsigned)abs(f);
        if (rowIn && xx < w) sum += (unsigned)A1[j + 1];
      }
    }
    if (hasRec)
    {
      int r[SPL];
      if constexpr (FAST)
      {
#pragma unroll
        for (int j = 0; j < SPL; j++) r[j] = vr[i][j];
      }
      else load_chunk<SPL>(a.rec + (size_t)min(y, h - 1) * a.rstride, xc, w, (a.vec & 2) != 0, r);
#pragma unroll
      for (int j = 0; j < SPL; j++)
      {
        const int d = A1[j + 1] - r[j];
        if (rowIn && x + j < w) sse += (unsigned)(d * d);
      }
    }
  }
}

// One wave = one unit: RB rows x 64 * SPL columns of one plane.  RB and SPL divide the tile size, so a lane's samples lie in ONE tile.
template <int SPL, int RB>
__global__ __launch_bounds__(256) void tile_stats_kernel(Ts3 p)
{
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= p.total) return;                                                   // wave-uniform
  const int c = u < p.a[0].unitEnd ? 0 : u < p.a[1].unitEnd ? 1 : 2;
  const TsPlane& a = c == 0 ? p.a[0] : c == 1 ? p.a[1] : p.a[2];
  const int ui = u - (c == 0 ? 0 : c == 1 ? p.a[0].unitEnd : p.a[1].unitEnd);
  const int uy = ui / a.unitsX, ux = ui - uy * a.unitsX;
  const int x = (ux * 64 + lane) * SPL, y0 = uy * RB;
  unsigned act = 0, sum = 0, sse = 0;
  if (a.fast) ts_band<SPL, RB, true, true>(a, lane, x, y0, act, sum, sse);
  else ts_band<SPL, RB, true, false>(a, lane, x, y0, act, sum, sse);
  // lanes of one tile are a run of lpt lanes; a power of two is aligned in the wave (64 * SPL columns a unit) and reduced by lane exchanges, one lane
  // of the run writes.  Any other run length: every lane adds its own partials.  Rows of a band lie in one tile row (RB divides the tile size).
  u64 s0 = act, s1 = sum, s2 = sse;
  const int lpt = a.lpt;
  const bool pow2 = (lpt & (lpt - 1)) == 0;
  if (pow2)
  {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
      if (m < lpt) { s0 += __shfl_xor(s0, m); s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); }
  }
  if (x < a.w && (!pow2 || (lane & (lpt - 1)) == 0))
  {
    u64* o = a.out + ((size_t)(y0 / a.tile) * a.tilesX + x / a.tile) * 3;
    if (s0) atomicAdd(o, s0);
    atomicAdd(o + 1, s1);
    if (s2) atomicAdd(o + 2, s2);
  }
}

// plain SSE: the waves of the grid stride over the units of the three planes, one add per plane and workgroup at the end
template <int SPL, int RB>
__global__ __launch_bounds__(256) void picture_sse_kernel(Ts3 p)
{
  __shared__ u64 part[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 s[3] = { 0, 0, 0 };
  for (int u = blockIdx.x * 4 + wave; u < p.total; u += gridDim.x * 4)         // wave-uniform
  {
    const int c = u < p.a[0].unitEnd ? 0 : u < p.a[1].unitEnd ? 1 : 2;
    const TsPlane& a = c == 0 ? p.a[0] : c == 1 ? p.a[1] : p.a[2];
    const int ui = u - (c == 0 ? 0 : c == 1 ? p.a[0].unitEnd : p.a[1].unitEnd);
    const int uy = ui / a.unitsX, ux = ui - uy * a.unitsX;
    unsigned act = 0, sum = 0, sse = 0;
    if (a.fast) ts_band<SPL, RB, false, true>(a, lane, (ux * 64 + lane) * SPL, uy * RB, act, sum, sse);
    else ts_band<SPL, RB, false, false>(a, lane, (ux * 64 + lane) * SPL, uy * RB, act, sum, sse);
    s[c] += sse;
  }
#pragma unroll
  for (int c = 0; c < 3; c++)
  {
    const u64 t = wave_sum(s[c]);
    if (lane == 0) part[wave][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < 3)
  {
    const u64 t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    u64* o = threadIdx.x == 0 ? p.a[0].out : threadIdx.x == 1 ? p.a[1].out : p.a[2].out;
    if (t) atomicAdd(o, t);
  }
}

__global__ __launch_bounds__(256) void zero3_kernel(u64* a, long long na, u64* b, long long nb, u64* c, long long nc)
{
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < na) a[i] = 0;
  else if (i < na + nb) b[i - na] = 0;
  else if (i < na + nb + nc) c[i - na - nb] = 0;
}

// ---- plane walks of the histogram and the weighted SADs --------------------------------------------------------------------------------------------------
// A workgroup's 256 threads are rpp rows of lpr (a power of two) chunk lanes: thread t owns chunk columns t % lpr, + lpr, .. of rows t / lpr, + rows a pass
struct Walk { int lprShift, chunksX; };
static Walk walk_of(int w)
{
  Walk k; k.chunksX = cdiv(w, 8); k.lprShift = 0;
  while ((1 << k.lprShift) < k.chunksX && k.lprShift < 8) k.lprShift++;
  return k;
}

// ---- histogram --------------------------------------------------------------------------------------------------------------------------------------------
struct HsPlane { const Pel* src; int stride, w, h, blockEnd, vec; Walk k; };
struct Hs3 { HsPlane a[3]; int maxPel; unsigned* hist; };

// per-workgroup bins in LDS, flushed once with global adds; a lane adds a run of equal samples of its chunk as one count (flat areas would otherwise
// send 8 adds of every lane to one bin)
__global__ __launch_bounds__(256) void histogram_kernel(Hs3 p)
{
  __shared__ unsigned bins[1024];
  const int b = blockIdx.x;
  const int c = b < p.a[0].blockEnd ? 0 : b < p.a[1].blockEnd ? 1 : 2;
  const HsPlane& a = c == 0 ? p.a[0] : c == 1 ? p.a[1] : p.a[2];
  const int b0 = c == 0 ? 0 : c == 1 ? p.a[0].blockEnd : p.a[1].blockEnd, nb = a.blockEnd - b0;
  for (int i = threadIdx.x; i < p.maxPel; i += 256) bins[i] = 0;
  __syncthreads();
  const int top = p.maxPel - 1;
  const int lpr = 1 << a.k.lprShift, rpp = 256 >> a.k.lprShift;
  for (int y = (b - b0) * rpp + ((int)threadIdx.x >> a.k.lprShift); y < a.h; y += nb * rpp)
  {
    const Pel* row = a.src + (size_t)y * a.stride;
    for (int cx = threadIdx.x & (lpr - 1); cx < a.k.chunksX; cx += lpr)
    {
      const int x = cx * 8;
      int v[8];
      load_chunk<8>(row, x, a.w, a.vec != 0, v);
      const int n = a.w - x;
      int cur = min(max(v[0], 0), top);
      unsigned cnt = 1;
#pragma unroll
      for (int j = 1; j < 8; j++)
      {
        if (j < n)
        {
          const int t = min(max(v[j], 0), top);
          if (t == cur) cnt++;
          else { atomicAdd(&bins[cur], cnt); cur = t; cnt = 1; }
        }
      }
      atomicAdd(&bins[cur], cnt);
    }
  }
  __syncthreads();
  unsigned* out = p.hist + (size_t)c * p.maxPel;
  for (int i = threadIdx.x; i < p.maxPel; i += 256)
    if (bins[i]) atomicAdd(out + i, bins[i]);
}

// ---- weighted SADs of candidate (weight, offset) pairs --------------------------------------------------------------------------------------------
// unclipped: |(org << ld) - (ref * w + off)| with off = offset << realLog2Denom, evaluated as |((org << ld) + WS_BIAS) - (ref * w + off + WS_BIAS)| on
// unsigned operands (offB = off + WS_BIAS); clipped: |org - clip(((ref * w + rnd) >> ld) + off)|
constexpr int WS_BIAS = 1 << 25;
__device__ __forceinline__ unsigned sad_u32(unsigned a, unsigned b, unsigned s) { unsigned r; asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(s)); return r; }   // |a - b| + s
struct WsCand { int w, off, offB, ld, rnd, clipped, pad[2]; };
struct WsArgs { WsCand c[16]; const Pel* org; const Pel* ref; int ostride, rstride, w, h, vec, maxVal; Walk k; long long* out; };

// every term fits 32 bits for the accepted candidates (host check): |org << 7| < 2^17, |ref * w| <= 1023 * 1024 < 2^20, |off| <= 2^15 << 9 = 2^24, so both
// biased operands lie in (0, 2^26), one sample's difference is below 2^25 and the 8 samples of a chunk sum below 2^28; the lane's accumulators are
// 64 bit from there on
template <int NC>
__global__ __launch_bounds__(256) void wp_sad_kernel(WsArgs p, int nReal)
{
  __shared__ u64 part[4][NC];
  u64 acc[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) acc[k] = 0;
  const int lpr = 1 << p.k.lprShift, rpp = 256 >> p.k.lprShift;
  for (int y = blockIdx.x * rpp + ((int)threadIdx.x >> p.k.lprShift); y < p.h; y += gridDim.x * rpp)
  {
    for (int cx = threadIdx.x & (lpr - 1); cx < p.k.chunksX; cx += lpr)
    {
      const int x = cx * 8;
      int o[8], r[8];
      load_chunk<8>(p.org + (size_t)y * p.ostride, x, p.w, (p.vec & 1) != 0, o);
      load_chunk<8>(p.ref + (size_t)y * p.rstride, x, p.w, (p.vec & 2) != 0, r);
      const int n = p.w - x;
#pragma unroll
      for (int k = 0; k < NC; k++)
      {
        const WsCand& cd = p.c[k];
        unsigned s = 0;
        if (cd.clipped)
        {
#pragma unroll
          for (int j = 0; j < 8; j++)
          {
            const int sv = min(max(((r[j] * cd.w + cd.rnd) >> cd.ld) + cd.off, 0), p.maxVal);
            if (j < n) s = sad_u32((unsigned)o[j], (unsigned)sv, s);
          }
        }
        else
        {
#pragma unroll
          for (int j = 0; j < 8; j++)
            if (j < n) s = sad_u32((unsigned)((o[j] << cd.ld) + WS_BIAS), (unsigned)(r[j] * cd.w + cd.offB), s);
        }
        acc[k] += s;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NC; k++)
  {
    const u64 t = wave_sum(acc[k]);
    if (lane == 0) part[wave][k] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < nReal)
  {
    const u64 t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (t) atomicAdd(reinterpret_cast<u64*>(p.out) + threadIdx.x, t);
  }
}

// ---- intra cost of the CTUs of a picture --------------------------------------------------------------------------------------------------------------
// 8 x 8 Hadamard of the original samples, sum of magnitudes without the DC term: the butterflies' order only permutes the coefficients and changes
// signs, neither of which the sum of magnitudes sees; the DC coefficient is the sum of the 64 samples
__device__ __forceinline__ void had8(int (&v)[8])
{
#pragma unroll
  for (int s = 1; s < 8; s <<= 1)
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (!(i & s)) { const int a = v[i], b = v[i | s]; v[i] = a + b; v[i | s] = a - b; }
}

__global__ void intra_cost_kernel(const Pel* __restrict__ org, int stride, int w, int h, int ctu, int wCtu, int shift, int vec, int* __restrict__ cost)
{
  __shared__ int part[4];
  const int cx = blockIdx.x % wCtu, cy = blockIdx.x / wCtu;
  const int x0 = cx * ctu, y0 = cy * ctu;
  const int bw = min(ctu, w - x0) >> 3, bh = min(ctu, h - y0) >> 3;           // whole 8 x 8 blocks inside the clipped CTU
  int sum = 0;
  for (int b = threadIdx.x; b < bw * bh; b += blockDim.x)
  {
    const int by = b / bw, bx = b - by * bw;
    const Pel* src = org + (size_t)(y0 + by * 8) * stride + x0 + bx * 8;
    int m[8][8];
#pragma unroll
    for (int i = 0; i < 8; i++) { load_chunk<8>(src + (size_t)i * stride, 0, 8, vec != 0, m[i]); had8(m[i]); }
    int s = 0;
#pragma unroll
    for (int j = 0; j < 8; j++)
    {
      int col[8];
#pragma unroll
      for (int i = 0; i < 8; i++) col[i] = m[i][j];
      had8(col);
#pragma unroll
      for (int i = 0; i < 8; i++) if (i | j) s += abs(col[i]);
    }
    sum += (s + 2) >> 2;
  }
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    int t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) t += part[i];
    cost[blockIdx.x] = (t + (shift > 0 ? 1 << (shift - 1) : 0)) >> shift;
  }
}

bool aligned_for(const void* p, int stride, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0 && (stride * 2) % bytes == 0; }

int check_planes(const char* fn, const vvcgpu_planes* a, int width, int height, int n_planes)
{
  for (int c = 0; c < n_planes; c++)
  {
    const int w = c ? width >> 1 : width;
    VVC_CHECK_ARG(a->p[c], "%s: null plane %d", fn, c);
    VVC_CHECK_ARG(a->stride[c] >= w, "%s: plane %d stride %d < width %d", fn, c, a->stride[c], w);
  }
  return VVCGPU_OK;
}

// the three planes of one tile-statistics / SSE launch; returns the number of units
template <int SPL, int RB>
int ts_fill(Ts3& q, const vvcgpu_planes* org, const vvcgpu_planes* rec, int width, int height, int tile, int n_planes, u64* const out[3])
{
  int end = 0;
  for (int c = 0; c < 3; c++)
  {
    TsPlane& a = q.a[c];
    memset(&a, 0, sizeof(a));
    a.unitEnd = end;
    a.out = out[c];
    if (c >= n_planes) continue;
    a.w = c ? width >> 1 : width; a.h = c ? height >> 1 : height;
    a.org = org->p[c]; a.ostride = org->stride[c];
    a.rec = rec ? rec->p[c] : nullptr; a.rstride = rec ? rec->stride[c] : 0;
    a.tile = tile ? (c ? tile >> 1 : tile) : 1 << 30;                          // tile 0: the plain SSE
    a.tilesX = tile ? cdiv(a.w, a.tile) : 1;
    a.lpt = tile ? a.tile / SPL : 64;
    a.vec = (aligned_for(a.org, a.ostride, SPL * 2) ? 1 : 0) | (rec && aligned_for(a.rec, a.rstride, SPL * 2) ? 2 : 0);
    a.fast = a.w % SPL == 0 && (a.vec & 1) && (!rec || (a.vec & 2));
    a.unitsX = cdiv(cdiv(a.w, SPL), 64);
    end += a.unitsX * cdiv(a.h, RB);
    a.unitEnd = end;
  }
  q.total = end;
  return end;
}

}  // namespace

extern "C" {

int vvcgpu_tile_stats_picture(const vvcgpu_planes* org, const vvcgpu_planes* rec_or_null, int width, int height, int tile, int n_planes,
                              vvcgpu_tile_stats* out_y, vvcgpu_tile_stats* out_cb, vvcgpu_tile_stats* out_cr, void* stream)
{
  VVC_CHECK_ARG(org && out_y, "tile_stats_picture: null pointer");
  VVC_CHECK_ARG(n_planes == 1 || n_planes == 3, "tile_stats_picture: n_planes %d (1 or 3)", n_planes);
  VVC_CHECK_ARG(n_planes == 1 || (out_cb && out_cr), "tile_stats_picture: null chroma output");
  VVC_CHECK_ARG(width > 0 && height > 0 && (n_planes == 1 || (width % 2 == 0 && height % 2 == 0)), "tile_stats_picture: picture %dx%d", width, height);
  const int unit = n_planes == 3 ? 8 : 4;
  VVC_CHECK_ARG(tile >= unit && tile <= 128 && tile % unit == 0, "tile_stats_picture: tile %d (a multiple of %d up to 128)", tile, unit);
  if (int rc = check_planes("tile_stats_picture", org, width, height, n_planes)) return rc;
  if (rec_or_null) if (int rc = check_planes("tile_stats_picture", rec_or_null, width, height, n_planes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  u64* const out[3] = { reinterpret_cast<u64*>(out_y), reinterpret_cast<u64*>(out_cb), reinterpret_cast<u64*>(out_cr) };
  long long n[3] = { 0, 0, 0 };
  for (int c = 0; c < n_planes; c++)
  {
    const int t = c ? tile >> 1 : tile;
    n[c] = 3ll * cdiv(c ? width >> 1 : width, t) * cdiv(c ? height >> 1 : height, t);
  }
  hipLaunchKernelGGL(zero3_kernel, dim3((unsigned)((n[0] + n[1] + n[2] + 255) / 256)), dim3(256), 0, st, out[0], n[0], out[1], n[1], out[2], n[2]);
  VVC_LAUNCH_CHECK();
  // every plane's tile size a multiple of 8: 16-byte loads, bands of 8 rows; else 8-byte loads and bands of 4 rows (any multiple of 4)
  const int smallest = n_planes == 3 ? tile >> 1 : tile;
  Ts3 q;
  if (smallest % 8 == 0)
  {
    const int units = ts_fill<8, 8>(q, org, rec_or_null, width, height, tile, n_planes, out);
    hipLaunchKernelGGL((tile_stats_kernel<8, 8>), dim3(cdiv(units, 4)), dim3(256), 0, st, q);
  }
  else
  {
    const int units = ts_fill<4, 4>(q, org, rec_or_null, width, height, tile, n_planes, out);
    hipLaunchKernelGGL((tile_stats_kernel<4, 4>), dim3(cdiv(units, 4)), dim3(256), 0, st, q);
  }
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int vvcgpu_picture_sse(const vvcgpu_planes* a, const vvcgpu_planes* b, int width, int height, int n_planes, uint64_t* out3, void* stream)
{
  VVC_CHECK_ARG(a && b && out3, "picture_sse: null pointer");
  VVC_CHECK_ARG(n_planes == 1 || n_planes == 3, "picture_sse: n_planes %d (1 or 3)", n_planes);
  VVC_CHECK_ARG(width > 0 && height > 0 && (n_planes == 1 || (width % 2 == 0 && height % 2 == 0)), "picture_sse: picture %dx%d", width, height);
  if (int rc = check_planes("picture_sse", a, width, height, n_planes)) return rc;
  if (int rc = check_planes("picture_sse", b, width, height, n_planes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  VVC_HIP(hipMemsetAsync(out3, 0, 3 * sizeof(uint64_t), st));
  u64* const out[3] = { reinterpret_cast<u64*>(out3), reinterpret_cast<u64*>(out3) + 1, reinterpret_cast<u64*>(out3) + 2 };
  Ts3 q;
  const int units = ts_fill<8, 8>(q, a, b, width, height, 0, n_planes, out);
  const int wgs = cdiv(units, 4);
  hipLaunchKernelGGL((picture_sse_kernel<8, 8>), dim3(wgs < 512 ? wgs : 512), dim3(256), 0, st, q);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int vvcgpu_picture_histogram(const vvcgpu_planes* pic, int width, int height, int n_planes, int bit_depth, uint32_t* hist, void* stream)
{
  VVC_CHECK_ARG(pic && hist, "picture_histogram: null pointer");
  VVC_CHECK_ARG(n_planes == 1 || n_planes == 3, "picture_histogram: n_planes %d (1 or 3)", n_planes);
  VVC_CHECK_ARG(width > 0 && height > 0 && (n_planes == 1 || (width % 2 == 0 && height % 2 == 0)), "picture_histogram: picture %dx%d", width, height);
  if (bit_depth < 8 || bit_depth > 10) { vvcgpu_set_error("picture_histogram: bit depth %d (8..10)", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  if (int rc = check_planes("picture_histogram", pic, width, height, n_planes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Hs3 q;
  memset(&q, 0, sizeof(q));
  q.maxPel = 1 << bit_depth; q.hist = hist;
  VVC_HIP(hipMemsetAsync(hist, 0, 3 * sizeof(uint32_t) * (size_t)q.maxPel, st));
  int end = 0;
  for (int c = 0; c < 3; c++)
  {
    HsPlane& a = q.a[c];
    a.blockEnd = end;
    if (c >= n_planes) continue;
    a.w = c ? width >> 1 : width; a.h = c ? height >> 1 : height;
    a.src = pic->p[c]; a.stride = pic->stride[c];
    a.vec = aligned_for(a.src, a.stride, 16) ? 1 : 0;
    a.k = walk_of(a.w);
    const long long want = ((long long)a.k.chunksX * a.h + 256 * 8 - 1) / (256 * 8);      // >= 8 chunks a thread before a workgroup pays for its flush
    end += (int)(want < 1 ? 1 : want > (c ? 128 : 512) ? (c ? 128 : 512) : want);
    a.blockEnd = end;
  }
  hipLaunchKernelGGL(histogram_kernel, dim3(end), dim3(256), 0, st, q);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int vvcgpu_wp_sad_batch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, int w, int h, int bit_depth,
                        const vvcgpu_wp_sad_cand* cands_host, int n_cand, int64_t* out, void* stream)
{
  VVC_CHECK_ARG(n_cand >= 0 && n_cand <= 16, "wp_sad_batch: n_cand %d (0..16)", n_cand);
  if (n_cand == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org && ref && cands_host && out, "wp_sad_batch: null pointer");
  VVC_CHECK_ARG(w > 0 && h > 0 && org_stride >= w && ref_stride >= w, "wp_sad_batch: %dx%d strides %d, %d", w, h, org_stride, ref_stride);
  if (bit_depth < 8 || bit_depth > 10) { vvcgpu_set_error("wp_sad_batch: bit depth %d (8..10)", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  WsArgs q;
  memset(&q, 0, sizeof(q));
  for (int k = 0; k < n_cand; k++)
  {
    const vvcgpu_wp_sad_cand& cd = cands_host[k];
    VVC_CHECK_ARG(cd.log2_denom >= 0 && cd.log2_denom <= 7 && cd.weight >= -1024 && cd.weight <= 1024 && cd.offset >= -32768 && cd.offset <= 32767 &&
                  (cd.flags & ~3) == 0, "wp_sad_batch: candidate %d {%d, %d, %d, %d} outside log2_denom 0..7, |weight| <= 1024, 16-bit offset, flags 0..3",
                  k, cd.log2_denom, cd.weight, cd.offset, cd.flags);
    const bool hp = cd.flags & 1, clipped = cd.flags & 2;
    WsCand& o = q.c[k];
    o.w = cd.weight; o.ld = cd.log2_denom; o.clipped = clipped;
    if (clipped) { o.off = cd.offset * (1 << (hp ? 0 : bit_depth - 8)); o.rnd = cd.log2_denom ? 1 << (cd.log2_denom - 1) : 0; }
    else o.off = cd.offset * (1 << (hp ? cd.log2_denom : cd.log2_denom + bit_depth - 8));
    o.offB = o.off + WS_BIAS;
  }
  q.org = org; q.ref = ref; q.ostride = org_stride; q.rstride = ref_stride; q.w = w; q.h = h;
  q.k = walk_of(w);
  q.vec = (aligned_for(org, org_stride, 16) ? 1 : 0) | (aligned_for(ref, ref_stride, 16) ? 2 : 0);
  q.maxVal = (1 << bit_depth) - 1;
  q.out = reinterpret_cast<long long*>(out);
  hipStream_t st = (hipStream_t)stream;
  VVC_HIP(hipMemsetAsync(out, 0, sizeof(int64_t) * n_cand, st));
  const long long want = ((long long)q.k.chunksX * h + 256 * 4 - 1) / (256 * 4);
  const int grid = (int)(want < 1 ? 1 : want > 512 ? 512 : want);
  if (n_cand == 1)      hipLaunchKernelGGL(wp_sad_kernel<1>, dim3(grid), dim3(256), 0, st, q, n_cand);
  else if (n_cand <= 4) hipLaunchKernelGGL(wp_sad_kernel<4>, dim3(grid), dim3(256), 0, st, q, n_cand);
  else if (n_cand <= 8) hipLaunchKernelGGL(wp_sad_kernel<8>, dim3(grid), dim3(256), 0, st, q, n_cand);
  else                  hipLaunchKernelGGL(wp_sad_kernel<16>, dim3(grid), dim3(256), 0, st, q, n_cand);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int vvcgpu_intra_cost_ctus(const vvc_pel* org_y, int stride, int width, int height, int ctu_size, int bit_depth, int32_t* cost, void* stream)
{
  VVC_CHECK_ARG(org_y && cost, "intra_cost_ctus: null pointer");
  VVC_CHECK_ARG(width > 0 && height > 0 && stride >= width, "intra_cost_ctus: %dx%d stride %d", width, height, stride);
  VVC_CHECK_ARG(ctu_size == 16 || ctu_size == 32 || ctu_size == 64 || ctu_size == 128, "intra_cost_ctus: ctu_size %d (16, 32, 64, 128)", ctu_size);
  if (bit_depth < 8 || bit_depth > 10) { vvcgpu_set_error("intra_cost_ctus: bit depth %d (8..10)", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  const int wCtu = cdiv(width, ctu_size), hCtu = cdiv(height, ctu_size);
  const int blocks = (ctu_size / 8) * (ctu_size / 8);
  hipLaunchKernelGGL(intra_cost_kernel, dim3(wCtu * hCtu), dim3(blocks >= 256 ? 256 : 64), 0, (hipStream_t)stream, org_y, stride, width, height, ctu_size, wCtu,
                     bit_depth - 8, aligned_for(org_y, stride, 16) ? 1 : 0, cost);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

// ---- host helpers: the reference's double arithmetic on the device's integers, same operations in the same order --------------------------------------
int vvcgpu_wpsnr_block_size_host(int plane_w, int plane_h, int chroma_shift, int* block_size)
{
  VVC_CHECK_ARG(block_size, "wpsnr_block_size_host: null pointer");
  VVC_CHECK_ARG(plane_w > 0 && plane_h > 0 && chroma_shift >= 0 && chroma_shift <= 1, "wpsnr_block_size_host: plane %dx%d chroma shift %d", plane_w, plane_h,
                chroma_shift);
  const uint32_t W = (uint32_t)plane_w, H = (uint32_t)plane_h;
  const double R = double(W * H) / (1920.0 * 1080.0);
  const uint32_t hi = 128u >> chroma_shift, v = 4 * uint32_t(16.0 * sqrt(R) + 0.5);
  const uint32_t B = v < hi ? v : hi;                                          // Clip3<uint32_t>(0, 128 >> chromaShift, v)
  *block_size = B < 4 ? 0 : (int)B;
  return VVCGPU_OK;
}

int vvcgpu_wpsnr_finish_host(const vvcgpu_tile_stats* tiles_host, int plane_w, int plane_h, int chroma_shift, int bit_depth, uint64_t* ssd)
{
  VVC_CHECK_ARG(tiles_host && ssd, "wpsnr_finish_host: null pointer");
  if (bit_depth < 8 || bit_depth > 10) { vvcgpu_set_error("wpsnr_finish_host: bit depth %d (8..10)", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  int Bi = 0;
  if (int rc = vvcgpu_wpsnr_block_size_host(plane_w, plane_h, chroma_shift, &Bi)) return rc;
  VVC_CHECK_ARG(Bi >= 4, "wpsnr_finish_host: a %dx%d plane has no WPSNR block (the reference takes the plain SSE: vvcgpu_picture_sse)", plane_w, plane_h);
  const uint32_t W = (uint32_t)plane_w, H = (uint32_t)plane_h, B = (uint32_t)Bi, BD = (uint32_t)bit_depth;
  double wmse = 0.0;
  const vvcgpu_tile_stats* t = tiles_host;
  for (uint32_t y = 0; y < H; y += B)
  {
    for (uint32_t x = 0; x < W; x += B, t++)
    {
      int blockWidth = (int)B, blockHeight = (int)B;
      const int yAct = y > 0 ? 0 : 1, xAct = x > 0 ? 0 : 1;
      if (y + (uint32_t)blockHeight > H) blockHeight = H - y;
      if (x + (uint32_t)blockWidth > W) blockWidth = W - x;
      const int hAct = y + (uint32_t)blockHeight < H ? blockHeight : blockHeight - 1;
      const int wAct = x + (uint32_t)blockWidth < W ? blockWidth : blockWidth - 1;
      if (wAct <= xAct || hAct <= yAct) { wmse += (double)t->ss_err; continue; }
      double msAct = (double)t->sa_act / (double(wAct - xAct) * double(hAct - yAct));
      if (msAct < double(1 << (BD - 4))) msAct = double(1 << (BD - 4));
      msAct *= msAct;
      wmse += (double)t->ss_err * pow(msAct, -1.0 * 0.5);
    }
  }
  double sumAct = 32.0 * double(1 << BD);
  if ((W << chroma_shift) > 2048 && (H << chroma_shift) > 1280) sumAct *= 0.5;
  else if ((W << chroma_shift) <= 1024 || (H << chroma_shift) <= 640) sumAct *= 2.0;
  *ssd = (wmse <= 0.0) ? 0 : uint64_t(wmse * pow(sumAct, 0.5) + 0.5);
  return VVCGPU_OK;
}

int vvcgpu_wp_acdc_host(const uint32_t* hist_host, int bit_depth, int n_samples, int fixed_shift, int64_t* dc, int64_t* ac)
{
  VVC_CHECK_ARG(hist_host && dc && ac, "wp_acdc_host: null pointer");
  VVC_CHECK_ARG(n_samples > 0 && fixed_shift >= 0 && fixed_shift <= 16, "wp_acdc_host: %d samples, shift %d", n_samples, fixed_shift);
  if (bit_depth < 8 || bit_depth > 10) { vvcgpu_set_error("wp_acdc_host: bit depth %d (8..10)", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  const int n = 1 << bit_depth, sample = n_samples;
  int64_t orgDC = 0, total = 0;
  for (int v = 0; v < n; v++) { orgDC += (int64_t)v * hist_host[v]; total += hist_host[v]; }
  VVC_CHECK_ARG(total == sample, "wp_acdc_host: the histogram holds %lld samples, not %d", (long long)total, sample);
  const int64_t orgNormDC = (orgDC + (sample >> 1)) / sample;
  int64_t orgAC = 0;
  for (int v = 0; v < n; v++) orgAC += (int64_t)hist_host[v] * llabs((long long)v - (long long)orgNormDC);
  *dc = ((orgDC << fixed_shift) + (sample >> 1)) / sample;
  *ac = orgAC;
  return VVCGPU_OK;
}

}  // extern "C"
