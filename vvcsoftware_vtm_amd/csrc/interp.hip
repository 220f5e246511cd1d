// interp.hip -- DCTIF interpolation (I1), motion compensation of prediction blocks (I3, incl. bi-pred average B1)
//               and the PelBuffer element-wise operations (B1-B4) for gfx950.
//
// Reference behaviour reproduced (bit-exact, bit depth <= 10):
//   InterpolationFilter::filter<N,isVertical,isFirst,isLast>   CommonLib/InterpolationFilter.cpp:290-379
//   InterpolationFilter::filterCopy<isFirst,isLast>            :205-264
//   InterPrediction::xPredInterBlk                             CommonLib/InterPrediction.cpp:480-547
//   AreaBuf<Pel>::addAvg / reconstruct / linearTransform       CommonLib/Buffer.cpp:114-151, 225-293 (+ cores :50-94)
//   AreaBuf::subtract / removeHighFreq / copyClip              CommonLib/Buffer.h:321-339, 389-416; Buffer.cpp:197-222
//   `Pel val = (sum + offset) >> shift` narrows to int16 BEFORE the clip (InterpolationFilter.cpp:368).
//
// Design: one 64-lane wave per descriptor.  MC works on 16x16 sub-tiles: the (16+7)^2 reference window is staged once
// in LDS, the horizontal pass writes the 14-bit intermediate to LDS (never to HBM -- the reference's m_filteredBlockTmp),
// the vertical pass and, for bi-prediction, the second list and the average stay in registers.
#include "common.h"
#include "dist_dev.h"
#include "mfma_tr.h"
#include "mc_dev.h"

// the generic MC scan loads bytes 32..47 of a descriptor as ONE uint4 (dst_stride | w, h | the four phases | is_luma, bi, reserved): the layout is part of
// the ABI, and the descriptor array must be 16-byte aligned (include/vvcgpu.h)
static_assert(offsetof(vvcgpu_mc_desc, dst_stride) == 32 && offsetof(vvcgpu_mc_desc, w) == 36 && offsetof(vvcgpu_mc_desc, frac_x0) == 40 &&
              offsetof(vvcgpu_mc_desc, is_luma) == 44 && sizeof(vvcgpu_mc_desc) == 48, "vvcgpu_mc_desc layout");

namespace {

// (the filter tables, rounding modes, weighted epilogue, the packed tile path and the generic body of a PU are in mc_dev.h)

// ------------------------------------------------------------------------------------------------ I1
// four samples of a row in ONE 8-byte access whatever the address (blocks start at any sample: 2-byte alignment).  gfx950 under HSA runs with
// unaligned global access enabled and the compiler knows it: a load / store through a 2-byte-aligned type is one global_load / store_dwordx2.  (Until
// round 4 the access branched three ways on the address -- 8-, 4-, 2-byte aligned -- and a wave whose lanes disagreed walked all three.)
struct __attribute__((packed, aligned(2))) PelQuad { short v[4]; };
__device__ __forceinline__ void if_load4(const Pel* p, int (&v)[4])
{
  const PelQuad q = *reinterpret_cast<const PelQuad*>(p);
  v[0] = q.v[0]; v[1] = q.v[1]; v[2] = q.v[2]; v[3] = q.v[3];
}

// one descriptor by a group of G lanes (lane = index inside the group)
// rows [y0, y1) only (default: all of them): dist-like band splitting of heavy calls
template <int G>
__device__ __forceinline__ void if_one(const vvcgpu_if_desc& d, const Pel* __restrict__ srcBase, Pel* __restrict__ dstBase, int lane, bool act, int bd,
                                       int cmin, int cmax, int y0 = 0, int y1 = 1 << 20)
{
  const int hh = min((int)d.h, y1) - y0;
  const Pel* src = srcBase + d.src_off + (ptrdiff_t)y0 * d.src_stride;
  Pel* dst = dstBase + d.dst_off + (ptrdiff_t)y0 * d.dst_stride;
  const int N = d.taps, w = d.w, count = act ? w * hh : 0;
  if (N == 0)
  {
    for (int i = lane; i < count; i += G)
    {
      const int y = i / w, x = i - y * w;
      dst[(size_t)y * d.dst_stride + x] = (short)if_copy(src[(size_t)y * d.src_stride + x], d.is_first, d.is_last, bd, cmin, cmax);
    }
    return;
  }
  const int cStride = d.is_vertical ? d.src_stride : 1;
  src -= (N / 2 - 1) * cStride;
  const IfMode m = if_mode(d.is_first, d.is_last, bd);
  int c[8];
#pragma unroll
  for (int k = 0; k < 8; k++) c[k] = k < N ? d.coeff[k] : 0;
  {
    // four consecutive outputs of a row per lane: N + 3 samples (horizontal) or N loads of four samples (vertical) instead of 4 N two-byte loads.
    // Widths that are not a multiple of four (the W + 1 wide planes of xExtDIFUpSamplingH / Q: 5, 9, 17, 33, 65, 129 -- 13 % of the samples of a real
    // call mix and, with a sample-by-sample partial unit per row that every wave walked beside its full units, half of if_batch's time on it): the
    // LAST unit of a row starts at w - 4 and overlaps its neighbour, so it is a full unit too -- the overlapped outputs are written twice with the
    // same values, and it reads exactly up to the last sample the reference reads (x + 3 + N - 1 = w + N - 2), nothing beyond the reference's window.
    // Only rows narrower than four samples keep a partial unit (nv < 4, sample-by-sample loads).
    const int upr = (w + 3) >> 2, units = act ? upr * hh : 0;
    for (int u = lane; u < units; u += G)
    {
      const int y = u / upr, xu = (u - y * upr) << 2, x = w >= 4 ? min(xu, w - 4) : xu, nv = min(4, w - x);
      const Pel* s = src + (size_t)y * d.src_stride + x;
      int sum[4] = { 0, 0, 0, 0 };
      if (d.is_vertical)
      {
#pragma unroll
        for (int k = 0; k < 8; k++)
          if (k < N)
          {
            int v[4];
            if (nv == 4) if_load4(s + (size_t)k * d.src_stride, v);
            else
            {
#pragma unroll
              for (int j = 0; j < 4; j++) v[j] = j < nv ? (int)s[(size_t)k * d.src_stride + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) sum[j] += v[j] * c[k];
          }
      }
      else
      {
        int v[12];                                        // exactly the N + 3 samples the four outputs read: nothing beyond the reference's window
        if (nv == 4)
        {
          int q[4];
          if_load4(s, q); v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
          if (N == 8) { if_load4(s + 4, q); v[4] = q[0]; v[5] = q[1]; v[6] = q[2]; v[7] = q[3]; v[8] = s[8]; v[9] = s[9]; v[10] = s[10]; }
          else if (N == 4) { v[4] = s[4]; v[5] = s[5]; v[6] = s[6]; }
          else v[4] = s[4];
        }
        else
        {
#pragma unroll
          for (int j = 0; j < 11; j++) v[j] = j < nv + N - 1 ? (int)s[j] : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
          for (int k = 0; k < 8; k++) if (k < N) sum[j] += v[j + k] * c[k];
      }
      pel4 o;
#pragma unroll
      for (int j = 0; j < 4; j++)
      {
        int val = (short)((sum[j] + m.offset) >> m.shift);
        if (d.is_last) val = clip3(cmin, cmax, val);
        o[j] = (short)val;
      }
      Pel* dp = dst + (size_t)y * d.dst_stride + x;
      if (nv == 4) { PelQuad q; q.v[0] = o[0]; q.v[1] = o[1]; q.v[2] = o[2]; q.v[3] = o[3]; *reinterpret_cast<PelQuad*>(dp) = q; }
      else
      {
#pragma unroll
        for (int j = 0; j < 4; j++) if (j < nv) dp[j] = o[j];
      }
    }
  }
}

// A workgroup takes 64 consecutive descriptors and BINS them first (one ballot of its first wave): calls of at most 256 samples -- the reference
// encoder's table-slot calls are mostly 4 wide: tests/golden/trace_*.npz -- run four side by side in a wave, 16 lanes each; larger ones take a whole
// wave each; HEAVY calls (more than 512 samples) are listed for if_heavy_kernel, which splits them into bands of rows over many waves: one wave needs
// ~70 us for 128 x 135 samples, and that was the run time of the whole launch on a real call mix.  (Until round 4 a wave took four CONSECUTIVE
// descriptors and ran them side by side only when all four were small: on the real call mix three of four waves lost that form to one larger
// neighbour -- the mixed batch took 2.5 x the time of its parts, profiles/r04_entry_shapes.txt.)
constexpr int IF_HEAVY = 2048, IF_HEAVY_FILTER = 512;   // the filter does 8 multiply-adds per sample: its heavy threshold is lower than the element-wise ops'
constexpr int IF_WG_DESCS = 64;
// a heavy call is cut into at most 16 bands of rows: band height = 512 samples' worth, more when that would give more than 16
__device__ __forceinline__ int if_filter_band_rows(int w, int h) { return max(max(2, IF_HEAVY_FILTER / w), (h + 15) >> 4); }
__device__ __forceinline__ int if_band_rows(int w, int h) { return max(max(4, IF_HEAVY / w), (h + 15) >> 4); }
__global__ __launch_bounds__(256) void if_batch_kernel(const Pel* __restrict__ srcBase, Pel* __restrict__ dstBase,
                                                       const vvcgpu_if_desc* __restrict__ descs, int n, int perWg, int localHeavy, int bd,
                                                       int cmin, int cmax, int* __restrict__ heavyCount, int* __restrict__ heavyList, int* __restrict__ nextCounters)
{
  if (blockIdx.x == 0 && threadIdx.x < VVC_CTR_INTS) nextCounters[threadIdx.x] = 0;       // the counter set of the next call on this stream (vvcgpu_counters)
  __shared__ unsigned char tList[IF_WG_DESCS], sList[IF_WG_DESCS], mList[IF_WG_DESCS], hList[IF_WG_DESCS];
  __shared__ int cntT, cntS, cntM, cntH;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int base = blockIdx.x * perWg;
  if (wave == 0)
  {
    const int di = base + lane;
    int w = 0, h = 0;
    if (lane < perWg && di < n) { w = descs[di].w; h = descs[di].h; }
    const int sz = w * h;
    // tiny: at most four 4-output units (4 x 4 and smaller: half of the trace's calls) -- four lanes each, sixteen calls side by side
    const bool tiny = sz > 0 && ((w + 3) >> 2) * h <= 4, small = sz > 0 && !tiny && sz <= 256, heavy = sz > IF_HEAVY_FILTER, med = sz > 0 && !tiny && !small && !heavy;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long mt = __builtin_amdgcn_ballot_w64(tiny), ms = __builtin_amdgcn_ballot_w64(small), mm = __builtin_amdgcn_ballot_w64(med),
                             mh = __builtin_amdgcn_ballot_w64(heavy);
    if (tiny) tList[__popcll(mt & below)] = (unsigned char)lane;
    if (small) sList[__popcll(ms & below)] = (unsigned char)lane;
    if (med) mList[__popcll(mm & below)] = (unsigned char)lane;
    if (lane == 0) { cntT = (int)__popcll(mt); cntS = (int)__popcll(ms); cntM = (int)__popcll(mm); cntH = localHeavy ? (int)__popcll(mh) : 0; }
    // localHeavy (long lists: thousands of workgroups): the workgroup serves its own heavy calls, bands of rows dealt to its four waves -- a second
    // launch for them costs its own ~12 us of latency behind this one, a third of the call's time on a real encoder's call mix at the bench's batch size
    if (heavy && localHeavy) hList[__popcll(mh & below)] = (unsigned char)lane;
    if (mh != 0ull && !localHeavy)                      // ONE atomic per workgroup (same-address atomics retire at ~12 ns each)
    {
      int b = 0;
      if (lane == 0) b = atomicAdd(heavyCount, (int)__popcll(mh));
      b = __builtin_amdgcn_readfirstlane(b);
      // the entry carries the number of bands the call really has, so that the band walk of if_heavy_kernel skips the others without touching the descriptor
      if (heavy) heavyList[b + (int)__popcll(mh & below)] = di | (((h + if_filter_band_rows(w, h) - 1) / if_filter_band_rows(w, h) - 1) << 27);
    }
  }
  __syncthreads();
  const int nT = cntT, nS = cntS, nM = cntM;
  for (int g0 = wave * 16; g0 < nT; g0 += 64)
  {
    const int k = g0 + (lane >> 2);
    const bool act = k < nT;
    const vvcgpu_if_desc mine = descs[base + tList[act ? k : g0]];
    if_one<4>(mine, srcBase, dstBase, lane & 3, act, bd, cmin, cmax);
  }
  for (int g0 = wave * 4; g0 < nS; g0 += 16)
  {
    const int k = g0 + (lane >> 4);
    const bool act = k < nS;
    const vvcgpu_if_desc mine = descs[base + sList[act ? k : g0]];
    if_one<16>(mine, srcBase, dstBase, lane & 15, act, bd, cmin, cmax);
  }
  for (int k = wave; k < nM; k += 4)
  {
    const vvcgpu_if_desc d = descs[base + __builtin_amdgcn_readfirstlane((int)mList[k])];
    if_one<64>(d, srcBase, dstBase, lane, true, bd, cmin, cmax);
  }
  const int nH = cntH;
  for (int k = 0; k < nH; k++)
  {
    const vvcgpu_if_desc d = descs[base + __builtin_amdgcn_readfirstlane((int)hList[k])];
    const int br = if_filter_band_rows(d.w, d.h);
    for (int r0 = ((wave + k) & 3) * br; r0 < d.h; r0 += 4 * br) if_one<64>(d, srcBase, dstBase, lane, true, bd, cmin, cmax, r0, r0 + br);
  }
}
// one wave per (heavy call, band of rows)
__global__ __launch_bounds__(256) void if_heavy_kernel(const Pel* __restrict__ srcBase, Pel* __restrict__ dstBase, const vvcgpu_if_desc* __restrict__ descs,
                                                       int bd, int cmin, int cmax, const int* __restrict__ heavyCount, const int* __restrict__ heavyList)
{
  const int lane = threadIdx.x & 63;
  const int cnt = heavyCount[0], waves = gridDim.x * 4;
  // pair p = (band p / cnt, item p % cnt): BAND-major, so that the waves of one step hold neighbouring calls of the same band -- item-major
  // (p >> 4, p & 15) with a wave stride that is a multiple of 16 gave every wave the same band for the whole launch, and a call of two bands
  // (32 x 32: 3 % of the trace's samples) kept one wave in eight busy (0.131 ms per 4 M samples against 0.024 for 32 x 16)
  for (int p = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); p < cnt * 16; p += waves)
  {
    const int band = p / cnt, e = __builtin_amdgcn_readfirstlane(heavyList[p - band * cnt]);
    if (band > (e >> 27)) continue;
    const vvcgpu_if_desc d = descs[e & ((1 << 27) - 1)];
    const int br = if_filter_band_rows(d.w, d.h), r0 = band * br;
    if (r0 < d.h) if_one<64>(d, srcBase, dstBase, lane, true, bd, cmin, cmax, r0, r0 + br);
  }
}

// ------------------------------------------------------------------------------------------------ I3
// (ST / WP / WR, mc_stage, mc_tile_dot2, MC_LDS_DW, mc_luma4x4_chunk, mc_generic_pu: mc_dev.h)

// ---------------------------------------------------------------------------------------------------
// The fast shapes ON THE MATRIX CORES (round 5): 16x16 luma and 8x8 chroma PUs, uni- and bi-predictive, quarter- (chroma: eighth-) sample phases.
// The packed vector-pipe form (mc_tile_dot2) spends ~570 vector instructions per PU wave around 78 v_dot2 with the matrix pipe idle; here both filter passes are exact
// f16 products (the machinery of frac16m_kernel, fracsearch.hip): ~120 vector instructions per luma PU, ~100 per PAIR of chroma PUs.
//   window   rows through lanes, eight columns per lane as one 16-byte load (any alignment), samples as f16 bit patterns 0x6400 | v (= 1024 + v)
//   pass 1   W (A operand) x Toeplitz matrix of the taps (table, B operand); the constant that the sum has to start from travels in the product's
//            spare columns (operand constants 1.0 and 1024.0); one v_add_f32 with 2^23 S leaves u = plane + 16384 in the low mantissa bits (floor by
//            round-to-nearest at a chosen exponent); limbs lo = u & 127, hi = u >> 7 as 0x6400 | limb
//   pass 2   plane^T (A operand: the pass-1 result registers as they are) x Toeplitz matrix per limb (c and 128 c): lane = output row, registers = four
//            neighbouring columns -> one 8-byte store per lane; rounding shifts as fma + floor on exact f32 integers, the last one and the clip in
//            packed f16 (v_cvt_pkrtz in [1024, 2048) IS the floor; 0x6400 | v back to v by a mask)
//   chroma   two 8x8 PUs per product: block-diagonal Toeplitz matrices (pass 1: columns of PU 0 | PU 1 along k; pass 2: the table row a lane reads
//            belongs to ITS PU's phase), so every product is shared and half of the result lanes are real
//   the one branch of the reference that is not two passes -- a rounded, horizontal-only filter (uni, frac_y == 0, frac_x != 0) -- gets the last-stage
//   rounding and the clip in pass 1 (own constants) and a copy in pass 2.
// PUs it cannot take (bi == 2, other phases, reference samples outside the bit depth) are flagged for the generic kernel behind it.
typedef _Float16 mm_h2 __attribute__((ext_vector_type(2)));
constexpr int MM_TAL = 0;                                    // [4 phases][23 columns x + shift][4 lane groups]  luma pass 1
constexpr int MM_TBL = MM_TAL + 4 * 23 * 4;                  // [4 phases][2 row chunks][64 lanes]          luma pass 2
constexpr int MM_TAC = MM_TBL + 4 * 2 * 64;                  // [2 variants][8 phases][8 x][2] + a zero row   chroma pass 1
constexpr int MM_TBC = MM_TAC + 2 * 8 * 16 + 1;              // [8 phases][8 y][4 lane groups]               chroma pass 2
constexpr int MM_ENTRIES = MM_TBC + 8 * 32;                  // 16-byte entries (eight f16 each)

__global__ void mm_build_tables_kernel(_Float16* __restrict__ tab, int bd)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= MM_ENTRIES * 8) return;
  const int ent = i >> 3, e = i & 7;
  const int hr = max(2, IF_INTERNAL_PREC - bd);
  const float S = (float)(1 << (IF_FILTER_PREC - hr));
  // start value of a pass-1 sum, as b0 * 1.0 + b1 * 1024.0.  variant 0: 8192 S - 65536 - (S - 1) / 2 (removes the sample bias 1024 x 64, adds 16384 S
  // and the first-stage offset -8192 S, centres the floor); variant 1 (rounded horizontal-only): 32 + 16384 x 64 - 65536 - 31.5
  const float b0[2] = { -0.5f * (S - 1.f), 0.5f }, b1[2] = { 8.f * S - 64.f, 960.f };
  float v = 0.f;
  if (ent < MM_TBL)
  {
    // luma pass 1 reads whole ALIGNED 16-byte words: k = 8 g + e is the column of the aligned row segment, the window starts `shift` (0..7) columns into
    // it, and output x takes its taps from columns x + shift .. + 7: the table row depends on x + shift only (the start value of the sum travels in the
    // accumulator)
    const int q = ent / 92, xs = (ent % 92) >> 2, g = ent & 3;
    const int t = 8 * g + e - xs;
    if (t >= 0 && t <= 7) v = (float)c_lumaFilter[4 * q][t];
  }
  else if (ent < MM_TAC)
  {
    const int r = ent - MM_TBL, q = r / 128, ch = (r / 64) & 1, lane = r & 63, y = lane & 15, g = lane >> 4;
    const int row = 16 * ch + 4 * g + (e & 3), t = row - y;
    if (t >= 0 && t <= 7 && row <= 22) v = (float)c_lumaFilter[4 * q][t] * (e >= 4 ? 128.f : 1.f);
    if (ch == 1 && g == 2 && e < 2) v = e == 0 ? 0.f : -9280.f;     // x 1024: -(64 x 1024 x 129 + 16384 x 64), the limb biases and the 16384 of u
  }
  else if (ent < MM_TBC)
  {
    const int r = ent - MM_TAC;
    if (r < 2 * 8 * 16)
    {
      const int var = r / 128, q = (r / 16) & 7, x = (r >> 1) & 7, gl = r & 1;
      if (gl == 1 && e < 2) v = e == 0 ? b0[var] : b1[var];
      else
      {
        // phases != 0: lane group pair loads columns 0..7 | 3..10, of which 3, 4 give way to the constants and 5, 6, 7 are there already: 8, 9, 10 count; phase 0: 1..8
        const int col = q == 0 ? (gl == 0 ? 1 + e : -100) : (gl == 0 ? e : (e >= 5 ? 3 + e : -100));
        const int t = col - x;
        if (t >= 0 && t <= 3) v = (float)c_chromaFilter[4 * q][t];
      }
    }
  }
  else
  {
    const int r = ent - MM_TBC, q = r / 32, y = (r >> 2) & 7, g = r & 3;
    const int row = 4 * g + (e & 3), t = row - y;
    if (t >= 0 && t <= 3 && row <= 10) v = (float)c_chromaFilter[4 * q][t] * (e >= 4 ? 128.f : 1.f);
    if (g == 3 && e < 2) v = e == 0 ? 0.f : -9280.f;
  }
  tab[i] = (_Float16)v;
}

// which of the kernel's shapes a descriptor is: 1 luma 16x16, 2 chroma 8x8 (phases on the quarter / eighth grid, bi 0 or 1), 0 other; -1: a fast SHAPE
// that is left to the generic kernel
__device__ __forceinline__ int mm_kind(const vvcgpu_mc_desc& d)
{
  if (!mc_is_fast(d.is_luma, d.w, d.h)) return 0;
  const int m = (d.frac_x0 | d.frac_y0 | (d.bi == 1 ? d.frac_x1 | d.frac_y1 : 0));
  if ((m & 3) || m < 0 || m >= (d.is_luma ? 16 : 32) || d.bi < 0 || d.bi > 1) return -1;
  return d.is_luma ? 1 : 2;
}

struct MmK                                                   // lane constants of mc_mfma_kernel
{
  const _Float16* tabS;
  int lane, c16, g, hr;
  unsigned m7[3], m8[3], orX[3], orR[3];                     // limb masks / exponent patterns of a pass-1 result by row-chunk kind (see the kernel)
  unsigned rangeMask, uLo, uHi;
  float magicN, magicH, scBi1, scUni1, ofUni1, scBi2, ofBi2, cinN, cinH;
  mm_h2 pmin, pmax, pmin0, pmaxF;                            // packed clip bounds (+ 1024): the caller's range; the bit depth's range (a uni-predictive full-sample copy is NOT clipped: filterCopy, isFirst == isLast)
  int perm;                                                  // ds_bpermute address: lane (row & 15) + 16 chunk <- lane 4 (row & 15) + chunk
  int* genCount;                                             // PUs left to the generic kernel behind this one (it leaves at once when there are none)
  int cmin, cmax;                                            // the caller's clip range (the weighted tail: mm_tail_wp)
};

// pass-1 result registers -> limb operand (kind: 0 every row real; 1 luma rows 16..31; 2 chroma rows 0..15); hclip (per lane): the rounded horizontal-only
// filter's clip of the last stage, on u = sample + 16384
template <bool ANYH>
__device__ __forceinline__ h8 mm_limbs(const MmK& K, const f4& acc, float magic, int kind, bool hclip)
{
  unsigned u[4];
#pragma unroll
  for (int j = 0; j < 4; j++) u[j] = __builtin_bit_cast(unsigned, acc[j] + magic);
  unsigned p01 = __builtin_amdgcn_perm(u[1], u[0], 0x05040100u), p23 = __builtin_amdgcn_perm(u[3], u[2], 0x05040100u);
  if (ANYH)
  {
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const unsigned lo = hclip ? K.uLo : 0u, hi = hclip ? K.uHi : 0xFFFFFFFFu;
    p01 = __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(us2, p01), __builtin_bit_cast(us2, lo)), __builtin_bit_cast(us2, hi)));
    p23 = __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(us2, p23), __builtin_bit_cast(us2, lo)), __builtin_bit_cast(us2, hi)));
  }
  uint4 o;
  o.x = (p01 & K.m7[kind]) | K.orX[kind];
  o.y = (p23 & K.m7[kind]) | K.orR[kind];
  o.z = ((p01 >> 7) & K.m8[kind]) | K.orR[kind];
  o.w = ((p23 >> 7) & K.m8[kind]) | K.orR[kind];
  return __builtin_bit_cast(h8, o);
}
// window registers as loaded -> A operand; cst: this lane's first two columns are the product's constants (chroma) / the whole lane is (luma)
__device__ __forceinline__ h8 mm_window(const MmK& K, uint4 u, bool cst, bool wholeLane, unsigned& bad)
{
  bad |= (u.x | u.y | u.z | u.w) & ~K.rangeMask;
  const unsigned andX = cst ? 0u : 0xFFFFFFFFu, orXw = cst ? 0x64003C00u : 0x64006400u;
  const unsigned andR = (cst && wholeLane) ? 0u : 0xFFFFFFFFu, orRw = (cst && wholeLane) ? 0u : 0x64006400u;
  u.x = (u.x & andX) | orXw; u.y = (u.y & andR) | orRw; u.z = (u.z & andR) | orRw; u.w = (u.w & andR) | orRw;
  return __builtin_bit_cast(h8, u);
}
// the tail of a PU: (f0 + f1 + offset) >> shiftNum for bi, f0 for uni (w1 = 0, sc2 = 1), + 1024 so that the truncating f16 conversion is the floor and the
// clip is packed; the four samples as two dwords.  copy: a uni-predictive full-sample PU -- InterpolationFilter::filterCopy with isFirst == isLast
// stores the sample as it is (HM_JEM_CLIP_PEL, InterpolationFilter.cpp:210-227); the samples are inside the bit depth here, so "no clip" = its range
__device__ __forceinline__ uint2 mm_tail(const MmK& K, const float (&f0)[4], const float (&f1)[4], float w1, float sc2, float of2, bool copy)
{
  float t[4];
#pragma unroll
  for (int j = 0; j < 4; j++) t[j] = __builtin_fmaf(__builtin_fmaf(f1[j], w1, f0[j]), sc2, of2);
  mm_h2 q0 = __builtin_bit_cast(mm_h2, __builtin_amdgcn_cvt_pkrtz(t[0], t[1])), q1 = __builtin_bit_cast(mm_h2, __builtin_amdgcn_cvt_pkrtz(t[2], t[3]));
  const mm_h2 lo = copy ? K.pmin0 : K.pmin, hi = copy ? K.pmaxF : K.pmax;
  q0 = __builtin_elementwise_min(__builtin_elementwise_max(q0, lo), hi);
  q1 = __builtin_elementwise_min(__builtin_elementwise_max(q1, lo), hi);
  uint2 o;
  o.x = __builtin_bit_cast(unsigned, q0) & 0x03FF03FFu;
  o.y = __builtin_bit_cast(unsigned, q1) & 0x03FF03FFu;
  return o;
}
// the weighted tail (vvcgpu_mc_wp_batch): f0 / f1 are the unrounded intermediates of the two lists (exact f32 integers, |P| < 2^15: the conversion is exact),
// wp_apply in integers -- the products w (P + 8192) of a bi sum may reach 2^24, beyond what an f32 sum keeps exact
__device__ __forceinline__ uint2 mm_tail_wp(const MmK& K, const float (&f0)[4], const float (&f1)[4], bool bi, const vvcgpu_wp_param& e)
{
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = wp_apply((int)f0[j], (int)f1[j], bi, e, K.hr, K.cmin, K.cmax);
  uint2 o;
  o.x = ((unsigned)v[0] & 0xFFFFu) | ((unsigned)v[1] << 16);
  o.y = ((unsigned)v[2] & 0xFFFFu) | ((unsigned)v[3] << 16);
  return o;
}
struct __attribute__((packed, aligned(2))) MmQuad { uint2 v; };
struct MmRaw { uint4 w[2][2]; unsigned dstLo, dstHi, ds, frac, flg; };    // samples as loaded [reference][row chunk] (+ chroma: the output PU's descriptor fields)
struct MmWin { h8 w[2][2]; unsigned bad, dstLo, dstHi, ds, frac, flg; };   // a step's window operands; the loaded registers are free again

// ---- luma PU: everything about the descriptor is wave-uniform (scalar registers)
// window origin of a luma PU in reference rf as (16-byte aligned pointer, shift): the window's column 0 is `shift` samples into the aligned row segment
__device__ __forceinline__ const Pel* mm_luma_origin(const vvcgpu_mc_desc& d, int rf, const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base, int& shift)
{
  const Pel* p0 = (rf ? ref1Base + d.ref1_off : ref0Base + d.ref0_off) - (ptrdiff_t)3 * (rf ? d.ref1_stride : d.ref0_stride) - 3;
  shift = (int)((reinterpret_cast<uintptr_t>(p0) >> 1) & 7);
  return p0 - shift;
}
// Loads in ROW-MAJOR lane order -- lane 4 r + c takes aligned word c of row r: the four lanes of a row are one 64-byte access of the vector cache, 16
// accesses per instruction instead of the 64+ that a lane per (row, eight unaligned columns) costs (measured: the cache's access rate, not bandwidth or
// latency, bound the kernel at 65 us).  Requires strides that are multiples of 8 samples (the caller of this function checks); words that hold no
// column the reference reads are not touched (the lane repeats a neighbour's word).
__device__ __forceinline__ void mm_fetch_luma(const MmK& K, const vvcgpu_mc_desc& d, const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base, MmRaw& r)
{
  const int nRef = d.bi == 1 ? 2 : 1;
#pragma unroll
  for (int rf = 0; rf < 2; rf++)
  {
    if (rf >= nRef) { r.w[1][0] = r.w[1][1] = make_uint4(0u, 0u, 0u, 0u); break; }     // (constants: a copy of list 0's registers would wait for its loads right here)
    int shift;
    const Pel* pA = mm_luma_origin(d, rf, ref0Base, ref1Base, shift);
    const int rs = rf ? d.ref1_stride : d.ref0_stride, fx = rf ? d.frac_x1 : d.frac_x0, fy = rf ? d.frac_y1 : d.frac_y0;
    const int cLo = fx ? 0 : (3 + shift) >> 3, cHi = fx ? (22 + shift) >> 3 : (18 + shift) >> 3;
    const int word = min(max(K.lane & 3, cLo), cHi);
#pragma unroll
    for (int ch = 0; ch < 2; ch++)
    {
      const int row = fy ? min(16 * ch + (K.lane >> 2), 22) : min(max(16 * ch + (K.lane >> 2), 3), 18);
      r.w[rf][ch] = *reinterpret_cast<const uint4*>(pA + (ptrdiff_t)row * rs + 8 * word);
    }
  }
}
__device__ __forceinline__ void mm_luma_win(const MmK& K, const MmRaw& raw, MmWin& W)
{
  W.bad = 0;
#pragma unroll
  for (int rf = 0; rf < 2; rf++)
#pragma unroll
    for (int ch = 0; ch < 2; ch++)
    {
      uint4 u = raw.w[rf][ch];
      W.bad |= (u.x | u.y | u.z | u.w) & ~K.rangeMask;       // (over the whole aligned words: a neighbour outside the bit depth costs the PU the fast path, no more)
      // operand layout: lane (row & 15) + 16 word; every sample masked to the bit depth first: 0x6400 | v must stay a finite f16 whatever the word held
      u.x = (unsigned)__builtin_amdgcn_ds_bpermute(K.perm, (int)((u.x & K.rangeMask) | 0x64006400u));
      u.y = (unsigned)__builtin_amdgcn_ds_bpermute(K.perm, (int)((u.y & K.rangeMask) | 0x64006400u));
      u.z = (unsigned)__builtin_amdgcn_ds_bpermute(K.perm, (int)((u.z & K.rangeMask) | 0x64006400u));
      u.w = (unsigned)__builtin_amdgcn_ds_bpermute(K.perm, (int)((u.w & K.rangeMask) | 0x64006400u));
      W.w[rf][ch] = __builtin_bit_cast(h8, u);
    }
}
// WPF: both lists unrounded (the bi form of the second stage), the weighted tail with entry e
template <bool WPF = false>
__device__ __forceinline__ void mm_luma(const MmK& K, const vvcgpu_mc_desc& d, const MmWin& W, const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base,
                                        Pel* __restrict__ dstBase, int* __restrict__ flags, int idx, const vvcgpu_wp_param* e = nullptr)
{
  const int nRef = d.bi == 1 ? 2 : 1;
  const bool hOnly = !WPF && d.bi == 0 && d.frac_y0 == 0 && d.frac_x0 != 0;
  float fr[2][4] = { { 0.f, 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f, 0.f } };
#pragma unroll
  for (int rf = 0; rf < 2; rf++)
  {
    if (rf >= nRef) break;
    const int fx = (rf ? d.frac_x1 : d.frac_x0) >> 2, fy = (rf ? d.frac_y1 : d.frac_y0) >> 2;
    const int shift = (int)(((reinterpret_cast<uintptr_t>(rf ? ref1Base + d.ref1_off : ref0Base + d.ref0_off) >> 1) - 3 - 3 * (rf ? d.ref1_stride : d.ref0_stride)) & 7);
    const h8 ta = *reinterpret_cast<const h8*>(K.tabS + ((MM_TAL + fx * 92 + (K.c16 + shift) * 4 + K.g) * 8));
    const float cin = hOnly ? K.cinH : K.cinN;
    const f4 cin4 = { cin, cin, cin, cin };
    const h8 tb0 = *reinterpret_cast<const h8*>(K.tabS + ((MM_TBL + fy * 128 + K.lane) * 8));
    const h8 tb1 = *reinterpret_cast<const h8*>(K.tabS + ((MM_TBL + fy * 128 + 64 + K.lane) * 8));
    const f4 a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(W.w[rf][0], ta, cin4, 0, 0, 0);
    const f4 a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(W.w[rf][1], ta, cin4, 0, 0, 0);
    h8 p0, p1;
    if (hOnly) { p0 = mm_limbs<true>(K, a0, K.magicH, 0, true); p1 = mm_limbs<true>(K, a1, K.magicH, 1, true); }
    else       { p0 = mm_limbs<false>(K, a0, K.magicN, 0, false); p1 = mm_limbs<false>(K, a1, K.magicN, 1, false); }
    f4 acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(p0, tb0, f4{ 0.f, 0.f, 0.f, 0.f }, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(p1, tb1, acc, 0, 0, 0);
    // second-stage rounding of this list: bi acc >> 6; uni (acc + offset) >> (6 + headroom); rounded horizontal-only: the pass-2 copy, acc / 64
    const float sc = (WPF || d.bi == 1 || hOnly) ? K.scBi1 : K.scUni1, of = (WPF || d.bi == 1 || hOnly) ? 0.f : K.ofUni1;
#pragma unroll
    for (int j = 0; j < 4; j++) fr[rf][j] = floorf(__builtin_fmaf(acc[j], sc, of));
  }
  const bool isBad = __ballot(W.bad != 0) != 0ull;           // a reference sample outside the bit depth: the generic kernel takes the PU
  if (K.lane == 0) { flags[idx] = isBad; if (isBad) atomicAdd(K.genCount, 1); }
  if (isBad) return;
  uint2 o;
  if constexpr (WPF) o = mm_tail_wp(K, fr[0], fr[1], d.bi == 1, *e);
  else o = mm_tail(K, fr[0], fr[1], d.bi == 1 ? 1.f : 0.f, d.bi == 1 ? K.scBi2 : 1.f, d.bi == 1 ? K.ofBi2 : 1024.f, d.bi == 0 && (d.frac_x0 | d.frac_y0) == 0);
  Pel* dp = dstBase + d.dst_off + (ptrdiff_t)K.c16 * d.dst_stride + 4 * K.g;                 // lane (c16, g): row c16, columns 4 g .. 4 g + 3
  reinterpret_cast<MmQuad*>(dp)->v = o;
}

// ---- chroma: PUs iA (columns 0..7 of the products) and iB (8..15; < 0: absent).  A lane reads the descriptor fields it needs from ITS PU as vector loads:
// lane groups 2, 3 LOAD the samples of PU B; lanes with c16 >= 8 hold PU B's table rows and output
struct MmCDesc { uint4 q0, q1; unsigned frac, flg, dstLo, dstHi, ds; };    // per lane: bytes 0..31 + phases / flags of the PU it LOADS, output fields of the PU it WRITES
__device__ __forceinline__ void mm_chroma_desc(const MmK& K, const vvcgpu_mc_desc* __restrict__ descs, int iA, int iB, MmCDesc& c)
{
  const int iF = (K.g >= 2 && iB >= 0) ? iB : iA, iO = (K.c16 >= 8 && iB >= 0) ? iB : iA;
  const uint4* pF = reinterpret_cast<const uint4*>(descs + iF);
  const uint4* pO = reinterpret_cast<const uint4*>(descs + iO);
  c.q0 = pF[0]; c.q1 = pF[1];
  const uint4 q2 = pF[2], q1O = pO[1], q2O = pO[2];
  c.frac = q2.z; c.flg = q2.w;
  c.dstLo = q1O.x; c.dstHi = q1O.y; c.ds = q2O.x;
  // (the output PU's phases / flags ride in the same registers as the loaded PU's when they are the same PU; otherwise in the high halves below)
  c.q1.x = q2O.z; c.q1.y = q2O.w;                            // q1.x / q1.y (dst_off of the loaded PU) are not needed: reused for the OUTPUT PU's phases / flags
}
__device__ __forceinline__ void mm_fetch_chroma(const MmK& K, const MmCDesc& c, const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base, MmRaw& r)
{
  r.dstLo = c.dstLo; r.dstHi = c.dstHi; r.ds = c.ds; r.frac = c.q1.x; r.flg = c.q1.y;
  const bool biF = (int)(signed char)((c.flg >> 8) & 0xFFu) == 1;
#pragma unroll
  for (int rf = 0; rf < 2; rf++)
  {
    const bool second = rf == 1 && biF;
    const long long off = second ? (long long)(((unsigned long long)c.q0.w << 32) | c.q0.z) : (long long)(((unsigned long long)c.q0.y << 32) | c.q0.x);
    const int rs = second ? (int)c.q1.w : (int)c.q1.z;
    const int fx = (int)(signed char)((c.frac >> (second ? 16 : 0)) & 0xFFu), fy = (int)(signed char)((c.frac >> (second ? 24 : 8)) & 0xFFu);
    const Pel* base = (second ? ref1Base : ref0Base) + off;
    const int col = fx ? ((K.g & 1) ? 3 : 0) : 1, row = fy ? min(K.c16, 10) : min(max(K.c16, 1), 8);
    const Pel* q = base + (ptrdiff_t)(row - 1) * rs + (col - 1);
    pel8 v;
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = q[e];
    r.w[rf][0] = __builtin_bit_cast(uint4, v);
  }
}
__device__ __forceinline__ void mm_chroma_win(const MmK& K, const MmRaw& raw, MmWin& W)
{
  W.bad = 0;
  W.w[0][0] = mm_window(K, raw.w[0][0], (K.g & 1) == 1, false, W.bad);
  W.w[1][0] = mm_window(K, raw.w[1][0], (K.g & 1) == 1, false, W.bad);
  W.dstLo = raw.dstLo; W.dstHi = raw.dstHi; W.ds = raw.ds; W.frac = raw.frac; W.flg = raw.flg;
}
// WPF: as mm_luma; a lane's table entry is its OUTPUT PU's (the index rides in the high half of raw.flg), both entries read as scalars
template <bool WPF = false>
__device__ __forceinline__ void mm_chroma(const MmK& K, const MmWin& raw, int iA, int iB, Pel* __restrict__ dstBase, int* __restrict__ flags,
                                          const vvcgpu_wp_param* __restrict__ wp = nullptr)
{
  const bool hasB = iB >= 0;
  // the lane's OUTPUT PU (by c16 >> 3)
  const int bi = (int)(signed char)((raw.flg >> 8) & 0xFFu);
  const int fx0 = (int)(signed char)(raw.frac & 0xFFu) >> 2, fy0 = (int)(signed char)((raw.frac >> 8) & 0xFFu) >> 2;
  const int fx1 = (int)(signed char)((raw.frac >> 16) & 0xFFu) >> 2, fy1 = (int)(signed char)((raw.frac >> 24) & 0xFFu) >> 2;
  const bool hOnly = !WPF && bi == 0 && fy0 == 0 && fx0 != 0;
  const bool anyH = __ballot(hOnly) != 0ull;
  const int nRef = __ballot(bi == 1) != 0ull ? 2 : 1;
  const bool mineCols = (K.g >> 1) == (K.c16 >> 3) && (K.c16 < 8 || hasB);      // pass 1: this lane's table row is non-zero only in the k range of ITS PU
  float fr[2][4] = { { 0.f, 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f, 0.f } };
#pragma unroll
  for (int rf = 0; rf < 2; rf++)
  {
    if (rf >= nRef) break;
    const int fx = rf ? fx1 : fx0, fy = rf ? fy1 : fy0;
    const bool hO = rf == 0 && hOnly;
    const h8 w0 = raw.w[rf][0];
    const int rowA = mineCols ? ((hO ? 128 : 0) + fx * 16 + (K.c16 & 7) * 2 + (K.g & 1)) : 2 * 8 * 16;
    const h8 ta = *reinterpret_cast<const h8*>(K.tabS + ((MM_TAC + rowA) * 8));
    const h8 tb = *reinterpret_cast<const h8*>(K.tabS + ((MM_TBC + fy * 32 + (K.c16 & 7) * 4 + K.g) * 8));
    const f4 a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, ta, f4{ 0.f, 0.f, 0.f, 0.f }, 0, 0, 0);
    const float magic = hO ? K.magicH : K.magicN;
    const h8 p0 = anyH ? mm_limbs<true>(K, a0, magic, 2, hO) : mm_limbs<false>(K, a0, magic, 2, false);
    const f4 acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(p0, tb, f4{ 0.f, 0.f, 0.f, 0.f }, 0, 0, 0);
    const float sc = (WPF || bi == 1 || hO) ? K.scBi1 : K.scUni1, of = (WPF || bi == 1 || hO) ? 0.f : K.ofUni1;
#pragma unroll
    for (int j = 0; j < 4; j++) fr[rf][j] = floorf(__builtin_fmaf(acc[j], sc, of));
  }
  const unsigned long long badLanes = __ballot(raw.bad != 0);
  // a sample outside the bit depth is no f16 integer pattern (0x6400 | v reaches the exponent): in a product it poisons every output of its ROW, also the
  // other PU's, whose table entries for it are zero (0 x NaN) -- both PUs of the pair go to the generic kernel
  const bool badA = badLanes != 0ull, badB = hasB && badLanes != 0ull;
  if (K.lane == 0) { flags[iA] = badA; if (hasB) flags[iB] = badB; if (badA) atomicAdd(K.genCount, 1 + (badB ? 1 : 0)); }
  uint2 o;
  if constexpr (WPF)
  {
    const int ix = (int)(short)(raw.flg >> 16);                 // lane 0 writes PU A, lane 8 PU B (A again when there is none)
    const vvcgpu_wp_param eA = wp_load(wp, __builtin_amdgcn_readlane(ix, 0)), eB = wp_load(wp, __builtin_amdgcn_readlane(ix, 8));
    o = mm_tail_wp(K, fr[0], fr[1], bi == 1, K.c16 >= 8 ? eB : eA);
  }
  else o = mm_tail(K, fr[0], fr[1], bi == 1 ? 1.f : 0.f, bi == 1 ? K.scBi2 : 1.f, bi == 1 ? K.ofBi2 : 1024.f, bi == 0 && (fx0 | fy0) == 0);
  // lane (c16, g): row c16 & 7 of PU c16 >> 3, columns 4 (g & 1) ..; real when g >> 1 == c16 >> 3
  const bool outB = K.c16 >= 8;
  if ((K.g >> 1) == (K.c16 >> 3) && (outB ? (hasB && !badB) : !badA))
  {
    const long long dstOff = (long long)(((unsigned long long)raw.dstHi << 32) | raw.dstLo);
    Pel* dp = dstBase + dstOff + (ptrdiff_t)(K.c16 & 7) * (int)raw.ds + 4 * (K.g & 1);
    reinterpret_cast<MmQuad*>(dp)->v = o;
  }
}

// KIND_T 1: the luma PUs of the list, 2: the chroma PUs (two launches: A/B switch), 0: ONE launch whose workgroups alternate between the two shapes -- each
// workgroup with the LDS tables and the loop of one shape.  Persistent waves; wave w of W owns the descriptors w, w + W, ... (chroma: the descriptor PAIRS,
// so that two chroma PUs share the products): neighbouring PUs at the same time in neighbouring waves, and whatever runs of shapes the list has are dealt
// round the waves.  What bound the earlier forms of this kernel, in the order found (profiles/r05_mc_forms.txt): chunks of 64 descriptors per workgroup
// (a picture's list is rows of luma, then rows of chroma PUs: a third of the waves had all the luma work); a shared claim counter (same-address atomics:
// ~30 ns each); the scalar unit (one per CU: a descriptor-by-descriptor walk cost 400 scalar instructions per PU -- now a gather load and a ballot
// classify 64 of the wave's descriptors at once); the vector cache's access rate (a lane per row and eight unaligned columns: 64+ accesses per load).
__device__ __forceinline__ int mm_kind_of(const uint4& q)   // bytes 32..47 of a descriptor: dst_stride | w, h | phases | is_luma, bi
{
  vvcgpu_mc_desc d;
  d.w = (short)(q.y & 0xFFFFu); d.h = (short)(q.y >> 16);
  d.frac_x0 = (signed char)(q.z & 0xFFu); d.frac_y0 = (signed char)((q.z >> 8) & 0xFFu); d.frac_x1 = (signed char)((q.z >> 16) & 0xFFu); d.frac_y1 = (signed char)(q.z >> 24);
  d.is_luma = (signed char)(q.w & 0xFFu); d.bi = (signed char)((q.w >> 8) & 0xFFu);
  return mm_kind(d);
}
// the generic body for the PUs this kernel cannot take, served by the wave that found them BEHIND its walk (round 6, vvcgpu_mc_picture_batch: the launch of
// mc_batch_kernel behind this kernel cost 4.9 us per 4K picture for an empty list).  The second pass is a REAL call that takes everything it needs from
// a record in LDS: values kept alive for it across the walks cost the walks' loops spilled registers (190 instead of 49 us).  Defined below mc_generic_pu.
struct MmServe { const Pel* ref0Base; const Pel* ref1Base; Pel* dstBase; const vvcgpu_mc_desc* descs; const int* flags; int n, bd, cmin, cmax, w0, W, luma; };
struct MmServeWp : MmServe { const vvcgpu_wp_param* wp; int nWp, allGen; };             // vvcgpu_mc_wp_batch: the weight table (mm_wp_kind)
template <bool WPF> __device__ __forceinline__ void mm_second_pass(const MmServe* sv, short* gen, unsigned* genT);
__device__ __noinline__ void mm_serve_one(const MmServe* sv, int li, short* gen, unsigned* genT);
__device__ __noinline__ void mm_serve_one_wp(const MmServeWp* sv, int li, short* gen, unsigned* genT);
// vvcgpu_mc_wp_batch: the kind of mm_kind_of / the stride check, MM_SKIP for a descriptor the call skips (wp_skip: neither a walk's shape, 1 / 2, nor the
// generic body's, <= 0); allGen (VVCGPU_NO_MFMA): every PU to the generic body
constexpr int MM_SKIP = 3;
__device__ __forceinline__ int mm_wp_kind(int k, const uint4& q2, const vvcgpu_wp_param* __restrict__ wp, int nWp, int bd, int allGen)
{
  if (wp_skip(q2, wp, nWp, bd)) return MM_SKIP;
  return allGen && k > 0 ? 0 : k;
}
constexpr int MM_GEN_SHORTS = 23 * 24 + 23 * 16;                               // WR x WP + WR x ST (declared below)

// The matrix-core kernels (their body: mc_mfma_body.inc).  WPF (mc_mfma_wp_kernel, vvcgpu_mc_wp_batch): the same walks and passes with the weighted
// epilogue; descriptors the call skips (mm_wp_kind MM_SKIP) are neither taken nor served.
template <int KIND_T>
__global__ __launch_bounds__(256, 4) void mc_mfma_kernel(const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base, Pel* __restrict__ dstBase,
                                                                         const vvcgpu_mc_desc* __restrict__ descs, int n, int bd, int cmin, int cmax,
                                                                         const _Float16* __restrict__ image, int* __restrict__ flags, unsigned long long* __restrict__ diag,
                                                                         int* __restrict__ genCount, int* __restrict__ nextCounters, int serve)
{
  constexpr bool WPF = false;
  const vvcgpu_wp_param* const wp = nullptr;
  const int nWp = 0, allGen = 0;
#include "mc_mfma_body.inc"
}
// vvcgpu_mc_wp_batch: ONE launch, the picture form (both shapes, the generic body served behind the walks) with the weighted epilogue
__global__ __launch_bounds__(256, 4) void mc_mfma_wp_kernel(const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base, Pel* __restrict__ dstBase,
                                                            const vvcgpu_mc_desc* __restrict__ descs, int n, int bd, int cmin, int cmax,
                                                            const _Float16* __restrict__ image, int* __restrict__ flags, int* __restrict__ nextCounters,
                                                            const vvcgpu_wp_param* __restrict__ wp, int nWp, int allGen)
{
  constexpr bool WPF = true;
  constexpr int KIND_T = 0, serve = 1;
  unsigned long long* const diag = nullptr;
  int* const genCount = nullptr;
#include "mc_mfma_body.inc"
}

// the table image of mc_mfma_kernel per device and bit depth
static int mm_build(void* dst, const void* bd)
{
  hipLaunchKernelGGL(mm_build_tables_kernel, dim3(cdiv(MM_ENTRIES * 8, 256)), dim3(256), 0, (hipStream_t)0, static_cast<_Float16*>(dst), *static_cast<const int*>(bd));
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
static const _Float16* mm_image(int bd)
{
  void* p = nullptr;
  return vvcgpu_device_image(VVC_IMAGE_MC + bd - 8, MM_ENTRIES * 16, mm_build, &bd, &p) == VVCGPU_OK ? static_cast<const _Float16*>(p) : nullptr;
}


// (a real call: it runs for the rare PU only.  The scan below is inline in the kernel -- as a call of its own it saved and restored ~90 callee-saved
// registers through scratch memory in EVERY wave: 190 MB of traffic, 30 us)
__device__ __noinline__ void mm_serve_one(const MmServe* sv, int li, short* gen, unsigned* genT)
{
  static_assert(MM_GEN_SHORTS == WR * WP + WR * ST, "LDS of the generic body inside mc_mfma_kernel");
  const MmServe S = *sv;
  const vvcgpu_mc_desc d = S.descs[li];
  mc_generic_pu<false, 1>(d, S.ref0Base, S.ref1Base, S.dstBase, S.bd, S.cmin, S.cmax, (int)threadIdx.x & 63, gen, gen + WR * WP, genT, nullptr);
}
__device__ __noinline__ void mm_serve_one_wp(const MmServeWp* sv, int li, short* gen, unsigned* genT)
{
  const MmServeWp S = *sv;
  const vvcgpu_mc_desc d = S.descs[li];
  const vvcgpu_wp_param e = wp_load(S.wp, d.reserved);
  mc_generic_pu<false, 2, true>(d, S.ref0Base, S.ref1Base, S.dstBase, S.bd, S.cmin, S.cmax, (int)threadIdx.x & 63, gen, gen + WR * WP, genT, nullptr,
                                &e);
}
template <bool WPF>
__device__ __forceinline__ void mm_second_pass(const MmServe* sv, short* gen, unsigned* genT)
{
  // flags[] was written by this wave in its walk: its stores are complete behind the wait (vector stores write through to the L2), and the loads below are
  // agent-scope atomic loads (served by the L2).  NOT __threadfence(): on this chip that is an L2 write-back + invalidate per wave -- 4096 of them took
  // the kernel from 49 to 245 us
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  const MmServe S = *sv;
  const int lane = (int)threadIdx.x & 63, w = S.w0 + ((int)threadIdx.x >> 6);
  const MmServeWp* svW = static_cast<const MmServeWp*>(sv);            // (WPF only)
  auto serve = [&](int li) { if constexpr (WPF) mm_serve_one_wp(svW, li, gen, genT); else mm_serve_one(sv, li, gen, genT); };
  if (S.luma)
  {
    // what this wave's descriptors leave to the generic body: every shape that is not a fast one (luma or chroma), the fast shapes the walk rejected
    // (phases, strides) and the luma PUs whose samples left the bit depth
    for (int j0 = 0; w + (long long)j0 * S.W < S.n; j0 += 64)
    {
      const long long iL = w + (long long)(j0 + lane) * S.W;
      bool gen1 = false;
      if (iL < S.n)
      {
        const uint4 q1 = reinterpret_cast<const uint4*>(S.descs + iL)[1], q2 = reinterpret_cast<const uint4*>(S.descs + iL)[2];
        int k = mm_kind_of(q2);
        const int bi = (int)(signed char)((q2.w >> 8) & 0xFFu);
        if (k == 1 && ((q1.z | (bi == 1 ? q1.w : 0u)) & 7u)) k = -1;
        if constexpr (WPF) k = mm_wp_kind(k, q2, svW->wp, svW->nWp, S.bd, svW->allGen);
        gen1 = k <= 0 || (k == 1 && __hip_atomic_load(S.flags + iL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
      }
      unsigned long long todo = __ballot(gen1);
      while (todo)
      {
        const int j = (int)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        serve(w + (j0 + j) * S.W);
      }
    }
  }
  else
  {
    // the chroma PUs of this wave's pairs whose samples left the bit depth
    const int units = (S.n + 1) >> 1;
    for (int j0 = 0; w + (long long)j0 * S.W < units; j0 += 64)
    {
      const long long uL = w + (long long)(j0 + lane) * S.W;
      int g0 = -1, g1 = -1;
      if (uL < units)
      {
        const uint4* q0 = reinterpret_cast<const uint4*>(S.descs + 2 * uL) + 2;
        const int k0 = WPF ? mm_wp_kind(mm_kind_of(*q0), *q0, svW->wp, svW->nWp, S.bd, svW->allGen) : mm_kind_of(reinterpret_cast<const uint4*>(S.descs + 2 * uL)[2]);
        const int k1 = 2 * uL + 1 < S.n ? (WPF ? mm_wp_kind(mm_kind_of(q0[3]), q0[3], svW->wp, svW->nWp, S.bd, svW->allGen)
                                                : mm_kind_of(reinterpret_cast<const uint4*>(S.descs + 2 * uL + 1)[2])) : 0;
        if (k0 == 2 && __hip_atomic_load(S.flags + 2 * uL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) g0 = (int)(2 * uL);
        if (k1 == 2 && __hip_atomic_load(S.flags + 2 * uL + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) g1 = (int)(2 * uL + 1);
      }
      unsigned long long todo = __ballot(g0 >= 0 || g1 >= 0);
      while (todo)
      {
        const int j = (int)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int a0 = __builtin_amdgcn_readlane(g0, j), a1 = __builtin_amdgcn_readlane(g1, j);
        if (a0 >= 0) serve(a0);
        if (a1 >= 0) serve(a1);
      }
    }
  }
}

// generic kernel: any size, one wave per PU, persistent over the list of PUs the fast kernel left.
// DIST (vvcgpu_mc_dist_batch): the prediction goes into an LDS tile instead of dst, and the wave returns its distortion against the original
// (descriptor field dst_off / dst_stride = the original block, reserved = row sub-sampling shift of the SAD); list == nullptr: every descriptor.
template <bool DIST, bool SUB44 = false>
__global__ __launch_bounds__(64) void mc_batch_kernel(const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base,
                                                      Pel* __restrict__ dstBase, const vvcgpu_mc_desc* __restrict__ descs,
                                                      int bd, int cmin, int cmax,
                                                      int nDirect, int distKind, const Pel* __restrict__ orgBase, unsigned long long* __restrict__ out, int chunk,
                                                      const int* __restrict__ flags, int takeFast, const int* __restrict__ genCount = nullptr)
{
  // behind the matrix-core kernel: nothing left for this one (a picture of conforming 16x16 / 8x8 PUs) -- every wave leaves at once
  if (!DIST && genCount && __builtin_amdgcn_readfirstlane(*genCount) == 0) return;
  __shared__ short win[WR * WP];
  __shared__ short tmp[WR * ST];
  __shared__ __align__(16) short predT[DIST ? 128 * 128 : 8];
  __shared__ __align__(16) unsigned tileL[DIST ? 4 : MC_LDS_DW];
  const int lane = threadIdx.x;
  // !DIST: a wave looks at `chunk` consecutive descriptors at a time, one per lane, and serves those the fast kernel leaves.  (A list of them filled
  // by the fast kernel cost one same-address atomic per PU: 6 of the 7 ms of an affine prediction of 518 k 4x4 sub-blocks.)  chunk (host): 64 for
  // long lists, down to 1 for short ones -- a wave serves its PUs one after the other, and a short list of large PUs needs every wave it can get
  // (1947 PUs of 64x64 in chunks of 64: 31 busy waves, 2.2 ms instead of 0.08).
  const int STEP = DIST ? 1 : chunk;
  for (int base0 = (int)blockIdx.x * STEP; base0 < nDirect; base0 += (int)gridDim.x * STEP)
  {
  unsigned long long todo = 1ull;
  if (!DIST)
  {
    bool mine = false, sub44 = false;
    if (lane < chunk && base0 + lane < nDirect)
    {
      const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(descs + base0 + lane) + 32);     // dst_stride | w, h | phases | is_luma, bi
      const int isLuma = (int)(signed char)(q.w & 0xFFu), qw = (int)(short)(q.y & 0xFFFFu), qh = (int)(short)(q.y >> 16);
      mine = takeFast || !mc_is_fast(isLuma, qw, qh) || (flags && flags[base0 + lane] != 0);       // (flags: the fast shapes the matrix-core kernel in front has left; takeFast: there is none)
      sub44 = SUB44 && isLuma && qw == 4 && qh == 4;
    }
    todo = __builtin_amdgcn_ballot_w64(mine);
    unsigned long long todo44 = __builtin_amdgcn_ballot_w64(sub44);        // 4x4 luma (affine sub-blocks): four at a time, see mc_luma4x4_quad
    todo &= ~todo44;
    if (SUB44 && todo44) todo |= mc_luma4x4_chunk(todo44, descs + base0, ref0Base, ref1Base, dstBase, bd, cmin, cmax, lane, tileL);
  }
  while (todo)
  {
  const int li = base0 + (DIST ? 0 : (int)__builtin_ctzll(todo));
  todo &= todo - 1ull;
  const vvcgpu_mc_desc d = descs[li];
  // descriptors live in device memory, the host cannot validate them: a shape outside the contract (the prediction tile of the fused form is
  // 128 x 128, bi is 0 or 1 there) is skipped with the sentinel ~0 as its distortion instead of overrunning LDS (wave-uniform)
  if (DIST && (d.w < 1 || d.h < 1 || d.w > 128 || d.h > 128 || d.bi < 0 || d.bi > 1))
  {
    if (lane == 0) out[li] = ~0ull;
    continue;
  }
  mc_generic_pu<DIST, 0>(d, ref0Base, ref1Base, dstBase, bd, cmin, cmax, lane, win, tmp, tileL, predT);
  if (DIST)
  {
    __syncthreads();                                   // the tile is complete
    const Pel* org = orgBase + d.dst_off;
    const int os = d.dst_stride, w = d.w, h = d.h;
    unsigned long long res;
    typedef const __attribute__((address_space(3))) short* LdsPel;
    if (distKind == 1) res = satd_block<64, LdsPel>(org, os, (LdsPel)predT, w, w, h, lane);
    else
    {
      const int ss = distKind == 0 ? d.reserved : 0, rows = h >> ss;
      unsigned long long acc = 0;
      for (int i = lane; i < rows * w; i += 64)
      {
        const int r = i / w, x = i - r * w;
        const int df = (int)org[(size_t)(r << ss) * os + x] - (int)predT[(r << ss) * w + x];
        acc += distKind == 2 ? (unsigned)(df * df) : (unsigned)abs(df);
      }
      res = wave_sum(acc) << ss;
    }
    if (lane == 0) out[li] = res;
    __syncthreads();                                   // before the next descriptor overwrites the tile
  }
  }
  }
}

// ------------------------------------------------------------------------------------------------ B1-B4
__device__ __forceinline__ int pelop_apply(int op, int a, int b, const vvcgpu_pelop_cfg& c)
{
  switch (op)
  {
  case 0: return clip3(c.clp_min, c.clp_max, (a + b + c.offset) >> c.shift);
  case 1: return clip3(c.clp_min, c.clp_max, a + b);
  case 2: { const int t = (c.shift >= 0 ? (c.scale * a) >> c.shift : (c.scale * a) << -c.shift) + c.offset;
            return c.clip ? clip3(c.clp_min, c.clp_max, t) : t; }
  case 3: return a - b;
  case 4: return c.clip ? clip3(c.clp_min, c.clp_max, 2 * a - b) : 2 * a - b;
  default: return clip3(c.clp_min, c.clp_max, a);
  }
}

// rows [y0, y1) of one descriptor by `nthr` threads (t = index among them); each lane moves 8 samples (16 bytes) per access when the three
// operands allow it
__device__ __forceinline__ void pelop_one(int op, const vvcgpu_pelop_desc& d, const Pel* __restrict__ s0Base, const Pel* __restrict__ s1Base, Pel* dstBase,
                                          const vvcgpu_pelop_cfg& c, int t, int nthr, int y0, int y1)
{
  const Pel* s0 = s0Base + d.src0_off;
  const Pel* s1 = s1Base ? s1Base + d.src1_off : nullptr;
  Pel* dst = dstBase + d.dst_off;
  const bool vec = ((d.w & 7) == 0) && ((d.src0_stride & 7) == 0) && ((d.dst_stride & 7) == 0) &&
                   ((reinterpret_cast<uintptr_t>(s0) & 15) == 0) && ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) &&
                   (!s1 || (((d.src1_stride & 7) == 0) && ((reinterpret_cast<uintptr_t>(s1) & 15) == 0)));
  if (vec)
  {
    const int wv = d.w >> 3;
    for (int i = t + y0 * wv; i < wv * y1; i += nthr)
    {
      const int y = i / wv, x = (i - y * wv) << 3;
      const pel8 a = *reinterpret_cast<const pel8*>(s0 + (size_t)y * d.src0_stride + x);
      pel8 b = { 0, 0, 0, 0, 0, 0, 0, 0 };
      if (s1) b = *reinterpret_cast<const pel8*>(s1 + (size_t)y * d.src1_stride + x);
      pel8 r;
#pragma unroll
      for (int k = 0; k < 8; k++) r[k] = (short)pelop_apply(op, a[k], b[k], c);
      *reinterpret_cast<pel8*>(dst + (size_t)y * d.dst_stride + x) = r;
    }
    return;
  }
  for (int i = t + y0 * d.w; i < d.w * y1; i += nthr)
  {
    const int y = i / d.w, x = i - y * d.w;
    const int a = s0[(size_t)y * d.src0_stride + x];
    const int b = s1 ? s1[(size_t)y * d.src1_stride + x] : 0;
    dst[(size_t)y * d.dst_stride + x] = (short)pelop_apply(op, a, b, c);
  }
}

// perWg == 1: one workgroup per descriptor (the reference calls these per CU: up to 128x128 samples; few descriptors = plane-sized bands: gridDim.y
// workgroups share a descriptor, each takes a contiguous share of the rows).  perWg > 1 (long lists: blocks): a workgroup takes perWg consecutive
// descriptors, one per wave at a time -- a workgroup per 8 x 4 block is bound by the dispatcher.
__global__ __launch_bounds__(256) void pelop_batch_kernel(int op, const Pel* __restrict__ s0Base, const Pel* __restrict__ s1Base,
                                                          Pel* dstBase, const vvcgpu_pelop_desc* __restrict__ descs, int n,
                                                          vvcgpu_pelop_cfg c, int perWg, int* __restrict__ heavyCount, int* __restrict__ heavyList,
                                                          int* __restrict__ nextCounters)
{
  const int tid = threadIdx.x;
  if (nextCounters && blockIdx.x == 0 && blockIdx.y == 0 && tid < VVC_CTR_INTS) nextCounters[tid] = 0;   // the counter set of the next call on this stream
  if (perWg > 1)                                          // the workgroup bins its perWg (<= 64) consecutive descriptors first, as if_batch_kernel does:
  {                                                       // at most 256 samples: four side by side in a wave; larger: a wave each; heavy: listed
    __shared__ unsigned char sList[64], mList[64];
    __shared__ int cntS, cntM;
    const int lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.x * perWg;
    if (wave == 0)
    {
      const int di = base + lane;
      int sz = 0;
      if (lane < perWg && di < n) sz = (int)descs[di].w * (int)descs[di].h;
      const bool small = sz > 0 && sz <= 256, heavy = sz > IF_HEAVY, med = sz > 0 && !small && !heavy;
      const unsigned long long below = (1ull << lane) - 1ull;
      const unsigned long long ms = __builtin_amdgcn_ballot_w64(small), mm = __builtin_amdgcn_ballot_w64(med), mh = __builtin_amdgcn_ballot_w64(heavy);
      if (small) sList[__popcll(ms & below)] = (unsigned char)lane;
      if (med) mList[__popcll(mm & below)] = (unsigned char)lane;
      if (lane == 0) { cntS = (int)__popcll(ms); cntM = (int)__popcll(mm); }
      if (mh != 0ull)                                     // bands over many waves (pelop_heavy_kernel): one wave per 128 x 128 block was the launch's run time
      {
        int b = 0;
        if (lane == 0) b = atomicAdd(heavyCount, (int)__popcll(mh));
        b = __builtin_amdgcn_readfirstlane(b);
        if (heavy) heavyList[b + (int)__popcll(mh & below)] = di;
      }
    }
    __syncthreads();
    const int nS = cntS, nM = cntM;
    for (int g0 = wave * 4; g0 < nS; g0 += 16)
    {
      const int k = g0 + (lane >> 4);
      if (k < nS) { const vvcgpu_pelop_desc mine = descs[base + sList[k]]; pelop_one(op, mine, s0Base, s1Base, dstBase, c, lane & 15, 16, 0, mine.h); }
    }
    for (int k = wave; k < nM; k += 4)
    {
      const vvcgpu_pelop_desc d = descs[base + mList[k]];
      pelop_one(op, d, s0Base, s1Base, dstBase, c, lane, 64, 0, d.h);
    }
    return;
  }
  const vvcgpu_pelop_desc d = descs[blockIdx.x];
  const int rows = (d.h + (int)gridDim.y - 1) / (int)gridDim.y, y0 = (int)blockIdx.y * rows, y1 = min(d.h, y0 + rows);
  if (y0 >= y1) return;
  pelop_one(op, d, s0Base, s1Base, dstBase, c, tid, 256, y0, y1);
}

// one wave per (heavy block, band of rows)
__global__ __launch_bounds__(256) void pelop_heavy_kernel(int op, const Pel* __restrict__ s0Base, const Pel* __restrict__ s1Base, Pel* dstBase,
                                                          const vvcgpu_pelop_desc* __restrict__ descs, vvcgpu_pelop_cfg c,
                                                          const int* __restrict__ heavyCount, const int* __restrict__ heavyList)
{
  const int lane = threadIdx.x & 63;
  const int cnt = heavyCount[0], waves = gridDim.x * 4;
  for (int p = blockIdx.x * 4 + (threadIdx.x >> 6); p < cnt * 16; p += waves)       // band-major pairs (see if_heavy_kernel)
  {
    const int band = p / cnt;
    const vvcgpu_pelop_desc d = descs[heavyList[p - band * cnt]];
    const int br = if_band_rows(d.w, d.h), r0 = band * br;
    if (r0 < d.h) pelop_one(op, d, s0Base, s1Base, dstBase, c, lane, 64, r0, min((int)d.h, r0 + br));
  }
}

}  // namespace

__attribute__((visibility("hidden"))) int vvcgpu_mc_image_build(int bit_depth) { return mm_image(bit_depth) ? VVCGPU_OK : VVCGPU_E_DEVICE; }

extern "C" {

int vvcgpu_if_batch(const vvc_pel* src_base, vvc_pel* dst_base, const vvcgpu_if_desc* descs, int n,
                    int bit_depth, int clp_min, int clp_max, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "if_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(src_base && dst_base && descs, "if_batch: null pointer");
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("if_batch: bit depth %d outside 8..10", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  VvcScratch sc(st);
  int* heavyList = sc.take<int>(n);
  if (!heavyList) return VVCGPU_E_DEVICE;
  int cur = 0;
  int* counters = vvcgpu_counters(st, &cur);
  if (!counters) return VVCGPU_E_DEVICE;
  VVC_CHECK_ARG(n < (1 << 27), "if_batch: n %d", n);
  int perWg = IF_WG_DESCS;                                // fewer descriptors per workgroup when 64 would leave compute units without one
  while (perWg > 16 && cdiv(n, perWg) < 4096) perWg >>= 1;
  // few calls: a heavy one may be most of the work of the whole launch -> bands over the machine; very many calls: the second launch is amortised and its
  // machine-wide bands beat a workgroup's four waves (real call mix: 0.042 -> 0.038 ms at 30 k calls, 0.093 -> 0.110 at 121 k)
  const int localHeavy = n >= 8192 && n < 65536;
  hipLaunchKernelGGL(if_batch_kernel, dim3(cdiv(n, perWg)), dim3(256), 0, st, src_base, dst_base, descs, n, perWg, localHeavy,
                     bit_depth, clp_min, clp_max, counters + VVC_CTR_INTS * cur, heavyList, counters + VVC_CTR_INTS * (cur ^ 1));
  if (!localHeavy)
    hipLaunchKernelGGL(if_heavy_kernel, dim3(1024), dim3(256), 0, st, src_base, dst_base, descs, bit_depth, clp_min, clp_max, counters + VVC_CTR_INTS * cur, heavyList);
  VVC_LAUNCH_CHECK_COUNTERS(st);
  return VVCGPU_OK;
}

int vvcgpu_mc_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base,
                    const vvcgpu_mc_desc* descs, int n, int bit_depth, int clp_min, int clp_max, void* stream)
{
  VvcScratch sc((hipStream_t)stream);
  return vvcgpu_mc_batch_impl(ref0_base, ref1_base, dst_base, descs, n, bit_depth, clp_min, clp_max, stream, sc, false, false);
}
// a picture's PU list as an encoder builds it for the common partition (16x16 luma / 8x8 chroma PUs): ONE launch -- what the matrix-core kernel cannot
// take (other shapes, phases, strides, samples outside the bit depth) is served by the wave that found it behind its walk, through the generic body
int vvcgpu_mc_picture_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base,
                            const vvcgpu_mc_desc* descs, int n, int bit_depth, int clp_min, int clp_max, void* stream)
{
  VvcScratch sc((hipStream_t)stream);
  return vvcgpu_mc_batch_impl(ref0_base, ref1_base, dst_base, descs, n, bit_depth, clp_min, clp_max, stream, sc, false, false, true);
}
// explicit weighted prediction: the launch of vvcgpu_mc_picture_batch with the weighted epilogue (mc_mfma_wp_kernel); reserved = index into wp
int vvcgpu_mc_wp_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base, const vvcgpu_mc_desc* descs, int n,
                       const vvcgpu_wp_param* wp, int n_wp, int bit_depth, int clp_min, int clp_max, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "mc_wp_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(ref0_base && dst_base && descs && wp, "mc_wp_batch: null pointer");
  VVC_CHECK_ARG(n_wp >= 1 && n_wp <= 32767, "mc_wp_batch: n_wp %d outside 1..32767", n_wp);
  VVC_CHECK_ARG(((uintptr_t)descs & 15) == 0, "mc_wp_batch: descriptor array must be 16-byte aligned");
  VVC_CHECK_ARG(((uintptr_t)wp & 15) == 0, "mc_wp_batch: weight table must be 16-byte aligned");
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("mc_wp_batch: bit depth %d outside 8..10", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  const _Float16* image = mm_image(bit_depth);
  if (!image) return VVCGPU_E_DEVICE;
  VvcScratch sc(st);
  int* fl = sc.take<int>(n);
  if (!fl) return VVCGPU_E_DEVICE;
  int cur = 0;
  int* counters = vvcgpu_counters(st, &cur);
  if (!counters) return VVCGPU_E_DEVICE;
  const int wgL = cdiv(n, 4) < 256 * 4 ? cdiv(n, 4) : 256 * 4;           // as vvcgpu_mc_batch_impl: persistent, four workgroups per CU, an even count
  hipLaunchKernelGGL(mc_mfma_wp_kernel, dim3(wgL < 2 ? 2 : (wgL & ~1)), dim3(256), 0, st, ref0_base, ref1_base ? ref1_base : ref0_base, dst_base, descs, n,
                     bit_depth, clp_min, clp_max, image, fl, counters + VVC_CTR_INTS * (cur ^ 1), wp, n_wp, vvcgpu_no_mfma());
  VVC_LAUNCH_CHECK_COUNTERS(st);
  return VVCGPU_OK;
}

}  // extern "C"

int vvcgpu_mc_batch_impl(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base, const vvcgpu_mc_desc* descs, int n, int bit_depth,
                         int clp_min, int clp_max, void* stream, VvcScratch& sc, bool skip_fast, bool sub44, bool serve_in_kernel)
{
  VVC_CHECK_ARG(n >= 0, "mc_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(ref0_base && dst_base && descs, "mc_batch: null pointer");
  VVC_CHECK_ARG(((uintptr_t)descs & 15) == 0, "mc_batch: descriptor array must be 16-byte aligned");
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("mc_batch: bit depth %d outside 8..10", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  const int mfmaOff = vvcgpu_no_mfma();                                   // VVCGPU_NO_MFMA (common.h): every PU through the generic kernel (its packed vector-pipe form takes the fast shapes)
  const int* flags = nullptr;
  int* genCount = nullptr;
  if (!skip_fast && !mfmaOff)
  {
    const _Float16* image = mm_image(bit_depth);
    if (!image) return VVCGPU_E_DEVICE;
    int* fl = sc.take<int>(n);
    if (!fl) return VVCGPU_E_DEVICE;
    const int wgL = cdiv(n, 4) < 256 * 4 ? cdiv(n, 4) : 256 * 4;   // persistent: four workgroups per CU
    unsigned long long* diag = nullptr;
    const bool wantDiag = getenv("VVCGPU_MC_DIAG") != nullptr;           // measurement aid: step stamps of one luma wave
    if (wantDiag) { VVC_HIP(hipMalloc(&diag, 64 * sizeof(unsigned long long))); VVC_HIP(hipMemsetAsync(diag, 0, 64 * sizeof(unsigned long long), st)); }
    int cur = 0;
    int* counters = vvcgpu_counters(st, &cur);
    if (!counters) return VVCGPU_E_DEVICE;
    genCount = counters + VVC_CTR_INTS * cur;
    hipLaunchKernelGGL(mc_mfma_kernel<0>, dim3(wgL < 2 ? 2 : (wgL & ~1)), dim3(256), 0, st, ref0_base, ref1_base ? ref1_base : ref0_base, dst_base, descs, n, bit_depth, clp_min, clp_max, image, fl, diag,
                       genCount, counters + VVC_CTR_INTS * (cur ^ 1), serve_in_kernel ? 1 : 0);
    if (wantDiag)
    {
      unsigned long long h[64];
      VVC_HIP(hipStreamSynchronize(st));
      VVC_HIP(hipMemcpy(h, diag, sizeof h, hipMemcpyDeviceToHost));
      (void)hipFree(diag);
      fprintf(stderr, "[vvcgpu mc diag] luma steps of one wave, cycles (wait + operands / request next / products + store | step):");
      for (int k = 0; k < 12; k++) if (h[4 * k + 3]) fprintf(stderr, " %llu/%llu/%llu|%llu", h[4 * k + 1] - h[4 * k], h[4 * k + 2] - h[4 * k + 1], h[4 * k + 3] - h[4 * k + 2], k ? h[4 * k] - h[4 * k - 4] : 0ull);
      fprintf(stderr, "\n");
    }
    flags = fl;
  }
  if (flags && serve_in_kernel)                                          // the matrix-core kernel has served what it could not take itself
  {
    VVC_LAUNCH_CHECK_COUNTERS(st);
    VVC_LAUNCH_CHECK();
    return VVCGPU_OK;
  }
  const int chunk = n >= 64 * 8192 ? 64 : (n + 8191) / 8192;            // ~8192 waves: 32 per CU
  // behind the matrix-core kernel the generic one usually finds nothing (or a few PUs) to do: a grid of 1024 waves that walk the list leaves sooner than 8192
  const int gridMax = flags ? 1024 : 8192;
  if (sub44)
    hipLaunchKernelGGL((mc_batch_kernel<false, true>), dim3(cdiv(n, chunk) < gridMax ? cdiv(n, chunk) : gridMax), dim3(64), 0, st, ref0_base,
                       ref1_base ? ref1_base : ref0_base, dst_base, descs, bit_depth, clp_min, clp_max, n, 0, nullptr, nullptr, chunk, flags, mfmaOff ? 1 : 0, genCount);
  else
    hipLaunchKernelGGL((mc_batch_kernel<false, false>), dim3(cdiv(n, chunk) < gridMax ? cdiv(n, chunk) : gridMax), dim3(64), 0, st, ref0_base,
                       ref1_base ? ref1_base : ref0_base, dst_base, descs, bit_depth, clp_min, clp_max, n, 0, nullptr, nullptr, chunk, flags, mfmaOff ? 1 : 0, genCount);
  if (genCount) VVC_LAUNCH_CHECK_COUNTERS(st);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

extern "C" {

int vvcgpu_mc_dist_batch(int kind, const vvc_pel* ref0_base, const vvc_pel* ref1_base, const vvc_pel* org_base, const vvcgpu_mc_desc* descs, int n,
                         int bit_depth, int clp_min, int clp_max, uint64_t* out, void* stream)
{
  VVC_CHECK_ARG(kind >= 0 && kind <= 2, "mc_dist_batch: kind %d (0 SAD, 1 Hadamard, 2 SSE)", kind);
  VVC_CHECK_ARG(n >= 0, "mc_dist_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(ref0_base && org_base && descs && out, "mc_dist_batch: null pointer");
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("mc_dist_batch: bit depth %d outside 8..10", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  hipLaunchKernelGGL((mc_batch_kernel<true, false>), dim3(n < 4096 ? n : 4096), dim3(64), 0, (hipStream_t)stream, ref0_base, ref1_base ? ref1_base : ref0_base,
                     nullptr, descs, bit_depth, clp_min, clp_max, n, kind, org_base, reinterpret_cast<unsigned long long*>(out), 1, nullptr, 0);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int vvcgpu_pelop_batch(int op, const vvc_pel* src0_base, const vvc_pel* src1_base, vvc_pel* dst_base,
                       const vvcgpu_pelop_desc* descs, int n, const vvcgpu_pelop_cfg* cfg_host, void* stream)
{
  VVC_CHECK_ARG(op >= 0 && op <= 5, "pelop_batch: op %d", op);
  VVC_CHECK_ARG(n >= 0, "pelop_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(src0_base && dst_base && descs && cfg_host, "pelop_batch: null pointer");
  VVC_CHECK_ARG(src1_base || op == 2 || op == 5, "pelop_batch: op %d needs src1", op);
  int perWg = n < 8192 ? 1 : 64;                          // long lists: up to 64 descriptors per workgroup, fewer when that would leave compute units without one
  while (perWg > 16 && cdiv(n, perWg) < 4096) perWg >>= 1;
  hipStream_t st = (hipStream_t)stream;
  VvcScratch sc(st);
  int* heavyList = nullptr; int* counters = nullptr; int cur = 0;
  if (perWg > 1)                                          // long lists: heavy blocks go to a list and a second launch
  {
    heavyList = sc.take<int>(n);
    if (!heavyList) return VVCGPU_E_DEVICE;
    counters = vvcgpu_counters(st, &cur);
    if (!counters) return VVCGPU_E_DEVICE;
  }
  hipLaunchKernelGGL(pelop_batch_kernel, dim3(cdiv(n, perWg), n < 2048 ? 8 : 1), dim3(256), 0, st, op, src0_base, src1_base,
                     dst_base, descs, n, *cfg_host, perWg, counters ? counters + VVC_CTR_INTS * cur : nullptr, heavyList, counters ? counters + VVC_CTR_INTS * (cur ^ 1) : nullptr);
  if (perWg > 1)
  {
    hipLaunchKernelGGL(pelop_heavy_kernel, dim3(1024), dim3(256), 0, st, op, src0_base, src1_base, dst_base, descs, *cfg_host, counters + VVC_CTR_INTS * cur, heavyList);
    VVC_LAUNCH_CHECK_COUNTERS(st);
    return VVCGPU_OK;
  }
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
