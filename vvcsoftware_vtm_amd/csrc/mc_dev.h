// mc_dev.h -- device bodies of the motion compensation of ONE prediction block, shared by interp.hip (vvcgpu_mc_batch and its relatives) and
// mergecand.hip (vvcgpu_merge_cand_batch): the DCTIF tables and rounding modes, the weighted epilogue, the packed 16x16 / 8x8 tile path (mc_stage,
// mc_tile_dot2), the four-at-a-time 4x4 luma path and the generic body of a PU by one wavefront (mc_generic_pu).  Reference behaviour: see interp.hip.
#pragma once
#include "common.h"

namespace {

__constant__ short c_lumaFilter[16][8] = {
  {  0, 0,   0, 64,  0,   0,  0,  0 }, {  0, 1,  -3, 63,  4,  -2,  1,  0 }, { -1, 2,  -5, 62,  8,  -3,  1,  0 },
  { -1, 3,  -8, 60, 13,  -4,  1,  0 }, { -1, 4, -10, 58, 17,  -5,  1,  0 }, { -1, 4, -11, 52, 26,  -8,  3, -1 },
  { -1, 3,  -9, 47, 31, -10,  4, -1 }, { -1, 4, -11, 45, 34, -10,  4, -1 }, { -1, 4, -11, 40, 40, -11,  4, -1 },
  { -1, 4, -10, 34, 45, -11,  4, -1 }, { -1, 4, -10, 31, 47,  -9,  3, -1 }, { -1, 3,  -8, 26, 52, -11,  4, -1 },
  {  0, 1,  -5, 17, 58, -10,  4, -1 }, {  0, 1,  -4, 13, 60,  -8,  3, -1 }, {  0, 1,  -3,  8, 62,  -5,  2, -1 },
  {  0, 1,  -2,  4, 63,  -3,  1,  0 } };
__constant__ short c_chromaFilter[32][4] = {
  {  0, 64,  0,  0 }, { -1, 63,  2,  0 }, { -2, 62,  4,  0 }, { -2, 60,  7, -1 }, { -2, 58, 10, -2 }, { -3, 57, 12, -2 },
  { -4, 56, 14, -2 }, { -4, 55, 15, -2 }, { -4, 54, 16, -2 }, { -5, 53, 18, -2 }, { -6, 52, 20, -2 }, { -6, 49, 24, -3 },
  { -6, 46, 28, -4 }, { -5, 44, 29, -4 }, { -4, 42, 30, -4 }, { -4, 39, 33, -4 }, { -4, 36, 36, -4 }, { -4, 33, 39, -4 },
  { -4, 30, 42, -4 }, { -4, 29, 44, -5 }, { -4, 28, 46, -6 }, { -3, 24, 49, -6 }, { -2, 20, 52, -6 }, { -2, 18, 53, -5 },
  { -2, 16, 54, -4 }, { -2, 15, 55, -4 }, { -2, 14, 56, -4 }, { -2, 12, 57, -3 }, { -2, 10, 58, -2 }, { -1,  7, 60, -2 },
  {  0,  4, 62, -2 }, {  0,  2, 63, -1 } };

constexpr int IF_INTERNAL_PREC = 14, IF_FILTER_PREC = 6, IF_INTERNAL_OFFS = 1 << 13;

struct IfMode { int shift, offset; };
__device__ __forceinline__ IfMode if_mode(bool isFirst, bool isLast, int bd)
{
  const int headRoom = max(2, IF_INTERNAL_PREC - bd);
  IfMode m;
  m.shift = IF_FILTER_PREC;
  if (isLast) { m.shift += isFirst ? 0 : headRoom; m.offset = (1 << (m.shift - 1)) + (isFirst ? 0 : IF_INTERNAL_OFFS << IF_FILTER_PREC); }
  else        { m.shift -= isFirst ? headRoom : 0; m.offset = isFirst ? -(IF_INTERNAL_OFFS << m.shift) : 0; }
  return m;
}
__device__ __forceinline__ int if_copy(int s, bool isFirst, bool isLast, int bd, int cmin, int cmax)
{
  const int shift = max(2, IF_INTERNAL_PREC - bd);
  if (isFirst == isLast) return s;
  if (isFirst) return (short)((short)(s << shift) - (short)IF_INTERNAL_OFFS);
  return clip3(cmin, cmax, (short)((s + IF_INTERNAL_OFFS + (1 << (shift - 1))) >> shift));
}

// explicit weighted prediction (vvcgpu_mc_wp_batch): the epilogue that replaces rndRes / addAvg, on P = the 14-bit intermediate of xPredInterBlk with
// rndRes = false (what bi = 2 stores).  WeightPrediction::addWeightBi / addWeightUni and their weightBidir / weightUnidir / noWeightUnidir cores
// (WeightPrediction.cpp:46-60, 157-300).  Integer arithmetic throughout: |P + 8192| < 2^16 (P is a Pel), |w| <= 255, |offset| <= 2^11 and shift <= 8
// keep every term and the bi sum below 2^31.  offset << (S - 1) of the reference is an arithmetic shift (gcc) also for a negative offset: a product here.
__device__ __forceinline__ int wp_apply(int p0, int p1, bool bi, const vvcgpu_wp_param& e, int shiftNum, int cmin, int cmax)
{
  const int S = e.shift + shiftNum;
  int v;
  if (bi) v = (e.w0 * (p0 + IF_INTERNAL_OFFS) + e.w1 * (p1 + IF_INTERNAL_OFFS) + (1 << (S - 1)) + e.offset * (1 << (S - 1))) >> S;
  else if (e.w0 != 1 << e.shift) v = ((e.w0 * (p0 + IF_INTERNAL_OFFS) + (1 << (S - 1))) >> S) + e.offset;
  else v = ((p0 + IF_INTERNAL_OFFS + (1 << (shiftNum - 1))) >> shiftNum) + e.offset;
  return clip3(cmin, cmax, v);
}
// the range a WPScalingParam can take after getWpScaling (log2WeightDenom <= 7, weights and offsets of the slice header scaled to the bit depth)
// -- outside it the descriptor is skipped
__device__ __forceinline__ bool wp_valid(const vvcgpu_wp_param& e, bool bi, int bd)
{
  return e.w0 >= -255 && e.w0 <= 255 && (!bi || (e.w1 >= -255 && e.w1 <= 255)) && e.shift >= 0 && e.shift <= 8 && e.offset >= -(2 << bd) && e.offset <= (2 << bd);
}
// a table entry as four scalars (the index is wave-uniform wherever this is called)
__device__ __forceinline__ vvcgpu_wp_param wp_load(const vvcgpu_wp_param* __restrict__ wp, int i)
{
  const int4 q = *reinterpret_cast<const int4*>(wp + i);
  vvcgpu_wp_param e;
  e.w0 = q.x; e.w1 = q.y; e.offset = q.z; e.shift = q.w;
  return e;
}
// a descriptor vvcgpu_mc_wp_batch skips, from bytes 32..47 (dst_stride | w, h | phases | is_luma, bi, reserved = table index): bi outside 0..1, index outside
// [0, nWp), w or h outside 1..128, a table entry outside wp_valid
__device__ __forceinline__ bool wp_skip(const uint4& q2, const vvcgpu_wp_param* __restrict__ wp, int nWp, int bd)
{
  const int w = (short)(q2.y & 0xFFFFu), h = (short)(q2.y >> 16), bi = (signed char)((q2.w >> 8) & 0xFFu), ix = (short)(q2.w >> 16);
  if (bi < 0 || bi > 1 || ix < 0 || ix >= nWp || w < 1 || w > 128 || h < 1 || h > 128) return true;
  return !wp_valid(wp_load(wp, ix), bi == 1, bd);
}

// ------------------------------------------------------------------------------------------------ I3
constexpr int ST = 16;                 // sub-tile
constexpr int WP = ST + 8;             // window pitch (samples)
constexpr int WR = ST + 7;             // window rows

__device__ __forceinline__ bool mc_is_fast(int is_luma, int w, int h) { return is_luma ? (w == 16 && h == 16) : (w == 8 && h == 8); }

typedef short mc_s2 __attribute__((ext_vector_type(2)));
// ---------------------------------------------------------------------------------------------------
// Fast path, packed form.  G lanes serve one PU (64: a 16x16 luma PU per wave; 32: two 8x8 chroma PUs per wave, one per half).
//   * window staging: a lane loads EIGHT bytes at the 4-byte-aligned address of its dword and shifts by the window's sub-dword phase
//     (`v_alignbit`), so LDS holds the window sample-aligned, 2 samples per dword, row pitch WD dwords -- 5 load instructions per reference
//     for the 23 x 23 luma window instead of 9 two-byte ones, both references requested before either is used.  Rows / columns that the
//     reference's branch does not read (fy == 0: rows outside the block, fx == 0: columns outside) are not loaded: their taps are 0.
//     A staged row may start and end up to two samples beyond the columns the reference touches (in the same row).
//   * both passes are the same code: a lane takes FOUR consecutive outputs along the filter direction from 11 (7) consecutive samples =
//     three (two) aligned ds_read_b64, pairs D_m = (s[2m], s[2m+1]) are the dwords themselves, the odd pairs E_m one `v_alignbit` each, and
//     every output is N/2 `v_dot2_i32_i16` -- the first pass writes the 14-bit intermediate TRANSPOSED (tmpT[x][row]) so that the second
//     pass reads its column as a row.  The unit filter (frac 0) through the same code equals the reference's copy / single-pass branches
//     bit for bit ((64 t) >> 6 == t, and (2^h S - 2^19) >> 6 == (S - 2^(19-h)) >> (6-h)) except ONE: a rounded (bi == 0) horizontal-only
//     filter, whose first pass therefore takes the last-stage rounding and whose second pass copies.
//   * the block leaves through LDS as rows: one 8-byte store per lane.
template <int N, int S, int G> struct McStaged
{
  static constexpr int NR = S + N - 1, WD = (NR + 2) / 2 + ((((NR + 2) / 2) & 1) ? 1 : 0), NL = (NR * WD + G - 1) / G;
  uint2 ld[2][NL];
  unsigned phase[2];                                                      // bit u: load u starts on an odd sample (odd strides: per row)
  unsigned bad;                                                           // non-zero: a loaded sample lies outside the bit depth (this lane's loads)
};

// requests both windows of a PU (see mc_tile_dot2)
template <int N, int S, int G>
__device__ __forceinline__ void mc_stage(const vvcgpu_mc_desc& d, bool active, const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base, int gl,
                                         McStaged<N, S, G>& st, int bd)
{
  constexpr int half = N / 2 - 1, NR = S + N - 1, WD = McStaged<N, S, G>::WD, LOADS = NR * WD;
  const int nRef = d.bi == 1 ? 2 : 1;
  auto& ld = st.ld;
  auto& phase = st.phase;
  phase[0] = phase[1] = 0u;
  // The two-pass form narrows its first pass to 16 bits sample by sample ((s << headroom) - 8192); the reference's one-dimensional branches
  // narrow only the filtered value.  The two agree for samples inside the bit depth; a window that holds anything else is reported here and the
  // PU takes the sample-wise body of the generic kernel (which follows the reference branch by branch).  Whole dwords are tested, so a sample
  // beside the window may report a PU that did not need it: speed only.
  const unsigned outside = ~(((1u << bd) - 1u) * 0x10001u);
  unsigned bad = 0u;
#pragma unroll
  for (int r = 0; r < 2; r++)
  {
    const int rs = r ? d.ref1_stride : d.ref0_stride;
    const Pel* ref = (r ? ref1Base + d.ref1_off : ref0Base + d.ref0_off) - (ptrdiff_t)half * rs - half;       // window origin
    const int fx = r ? d.frac_x1 : d.frac_x0, fy = r ? d.frac_y1 : d.frac_y0;
#pragma unroll
    for (int u = 0; u < (LOADS + G - 1) / G; u++)
    {
      const int i = gl + G * u, rr = i / WD, dw = i - rr * WD;
      ld[r][u] = make_uint2(0u, 0u);
      // samples 2 dw, 2 dw + 1 of the window row; needed when the row and one of the two columns are
      const bool rowOk = fy ? rr < NR : (rr >= half && rr < half + S);
      const bool colOk = fx ? 2 * dw < NR : (2 * dw + 1 >= half && 2 * dw < half + S);
      if (active && r < nRef && i < LOADS && rowOk && colOk)
      {
        const unsigned char* a = reinterpret_cast<const unsigned char*>(ref + (ptrdiff_t)rr * rs) + 4 * dw;
        const unsigned* a4 = reinterpret_cast<const unsigned*>(reinterpret_cast<uintptr_t>(a) & ~(uintptr_t)3);
        // On an odd phase sample 2 dw is the high half of a4[0] and sample 2 dw + 1 the low half of a4[1]: both dwords are read whole, so at
        // the two ends of a row up to TWO samples beyond the needed columns are touched (include/vvcgpu.h states this).  Reading only the needed
        // halves (predicated loads, or an address select that re-reads the other dword) was measured: 12 more spilled VGPRs at the kernel's
        // 80-register budget and 0.090 instead of 0.076 ms for the MC launches of a 4K picture.
        if (reinterpret_cast<uintptr_t>(a) & 2)
        {
          ld[r][u].x = a4[0];
          ld[r][u].y = a4[1];
          phase[r] |= 1u << u;
        }
        else ld[r][u].x = a4[0];
        bad |= (ld[r][u].x | ld[r][u].y) & outside;
      }
    }
  }
  st.bad = bad;
}

// WPF: the weighted epilogue (wp_apply) with entry e on the unrounded intermediates of both lists
template <int N, int S, int G, bool WPF = false>
__device__ __forceinline__ void mc_tile_dot2(const vvcgpu_mc_desc& d, bool active, const McStaged<N, S, G>& st, Pel* __restrict__ dstBase, int bd, int cmin, int cmax,
                                             int gl, unsigned* win, short* tmpT, short* outL, const vvcgpu_wp_param* e = nullptr)
{
  constexpr int half = N / 2 - 1, NR = S + N - 1, WD = McStaged<N, S, G>::WD;                              // dwords per window row (even: 8-byte reads)
  constexpr int TP = 2 * WD;                                             // tmpT pitch in samples
  constexpr int NG = S / 4, NP = N / 2, ND = NP + 2;                     // output groups per line, coefficient pairs, dwords read per lane
  constexpr int HITEMS = NR * NG, VITEMS = S * NG, LOADS = NR * WD;
  if (!active) return;                                                    // (the wave barriers below only order this wave's own LDS accesses)
  const int hr = max(2, IF_INTERNAL_PREC - bd);
  const bool rndRes = WPF ? false : d.bi == 0;
  const int nRef = d.bi == 1 ? 2 : 1;
  const auto& ld = st.ld;
  const auto& phase = st.phase;
  int pred[2][4] = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 } };
#pragma unroll
  for (int r = 0; r < 2; r++)
  {
    if (r >= nRef) break;                                                 // uniform per group; the other half of a chroma wave follows its own d
    const int fx = r ? d.frac_x1 : d.frac_x0, fy = r ? d.frac_y1 : d.frac_y0;
    const unsigned* cxp = reinterpret_cast<const unsigned*>(N == 8 ? c_lumaFilter[fx] : c_chromaFilter[fx]);
    const unsigned* cyp = reinterpret_cast<const unsigned*>(N == 8 ? c_lumaFilter[fy] : c_chromaFilter[fy]);
    unsigned cx[NP], cy[NP];
#pragma unroll
    for (int m = 0; m < NP; m++) { cx[m] = cxp[m]; cy[m] = cyp[m]; }
    const bool hOnly = rndRes && fy == 0 && fx != 0;                      // the one branch the two-pass form does not reproduce: see above
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < (LOADS + G - 1) / G; u++)
    {
      const int i = gl + G * u;
      if (i < LOADS) win[i] = (phase[r] >> u) & 1u ? __builtin_amdgcn_alignbit(ld[r][u].y, ld[r][u].x, 16) : ld[r][u].x;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    // four outputs from ND consecutive dwords
    auto four = [&](const unsigned (&D)[ND], const unsigned (&c)[NP], int (&o)[4])
    {
      unsigned E[ND - 1];
#pragma unroll
      for (int m = 0; m < ND - 1; m++) E[m] = __builtin_amdgcn_alignbit(D[m + 1], D[m], 16);
      o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
      for (int m = 0; m < NP; m++)
      {
        const mc_s2 cm = __builtin_bit_cast(mc_s2, c[m]);
        o[0] = __builtin_amdgcn_sdot2(__builtin_bit_cast(mc_s2, D[m]), cm, o[0], false);
        o[1] = __builtin_amdgcn_sdot2(__builtin_bit_cast(mc_s2, E[m]), cm, o[1], false);
        o[2] = __builtin_amdgcn_sdot2(__builtin_bit_cast(mc_s2, D[m + 1]), cm, o[2], false);
        o[3] = __builtin_amdgcn_sdot2(__builtin_bit_cast(mc_s2, E[m + 1]), cm, o[3], false);
      }
    };
    {
      const int shift1 = hOnly ? IF_FILTER_PREC : IF_FILTER_PREC - hr;
      const int off1 = hOnly ? (1 << (IF_FILTER_PREC - 1)) : -(IF_INTERNAL_OFFS << shift1);
#pragma unroll
      for (int u = 0; u < (HITEMS + G - 1) / G; u++)
      {
        const int it = gl + G * u, rr = it / NG, g = it - rr * NG;
        if (it < HITEMS)
        {
          unsigned D[ND];
          const uint2* wp = reinterpret_cast<const uint2*>(win + rr * WD + 2 * g);
#pragma unroll
          for (int m = 0; m < ND / 2; m++) { const uint2 q = wp[m]; D[2 * m] = q.x; D[2 * m + 1] = q.y; }
          int o[4];
          four(D, cx, o);
#pragma unroll
          for (int j = 0; j < 4; j++)
          {
            int t = (short)((o[j] + off1) >> shift1);
            if (hOnly) t = clip3(cmin, cmax, t);
            tmpT[(4 * g + j) * TP + rr] = (short)t;
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    if (gl < VITEMS)
    {
      const int x = gl % S, yg = gl / S;
      if (hOnly)
      {
#pragma unroll
        for (int j = 0; j < 4; j++) pred[r][j] = tmpT[x * TP + half + 4 * yg + j];
      }
      else
      {
        unsigned D[ND];
        const uint2* tp = reinterpret_cast<const uint2*>(tmpT + x * TP + 4 * yg);
#pragma unroll
        for (int m = 0; m < ND / 2; m++) { const uint2 q = tp[m]; D[2 * m] = q.x; D[2 * m + 1] = q.y; }
        int o[4];
        four(D, cy, o);
        const int shift2 = rndRes ? IF_FILTER_PREC + hr : IF_FILTER_PREC;
        const int off2 = rndRes ? (1 << (shift2 - 1)) + (IF_INTERNAL_OFFS << IF_FILTER_PREC) : 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
          int v = (short)((o[j] + off2) >> shift2);
          if (rndRes && (fx | fy) != 0) v = clip3(cmin, cmax, v);        // (a uni-predictive full-sample copy is not clipped: filterCopy with isFirst == isLast)
          pred[r][j] = v;
        }
      }
    }
  }
  // average, rows through LDS, 8-byte stores
  const int shiftNum = max(2, IF_INTERNAL_PREC - bd) + 1, offset = (1 << (shiftNum - 1)) + 2 * IF_INTERNAL_OFFS;
  if (gl < VITEMS)
  {
    const int x = gl % S, yg = gl / S;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
      int v = pred[0][j];
      if (WPF) v = wp_apply(pred[0][j], pred[1][j], d.bi == 1, *e, shiftNum - 1, cmin, cmax);
      else if (d.bi == 1) v = clip3(cmin, cmax, (pred[0][j] + pred[1][j] + offset) >> shiftNum);
      outL[(4 * yg + j) * S + x] = (short)v;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
  if (active && gl < VITEMS)
  {
    const int row = gl / NG, seg = gl - row * NG;
    Pel* o = dstBase + d.dst_off + (ptrdiff_t)row * d.dst_stride + 4 * seg;
    const uint2 v = *reinterpret_cast<const uint2*>(outL + row * S + 4 * seg);
    if ((reinterpret_cast<uintptr_t>(o) & 7) == 0) *reinterpret_cast<uint2*>(o) = v;
    else { o[0] = (short)(v.x & 0xFFFF); o[1] = (short)(v.x >> 16); o[2] = (short)(v.y & 0xFFFF); o[3] = (short)(v.y >> 16); }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
}

constexpr int MC_LDS_DW = 23 * 12 + 16 * 12 + 128;                       // per wave: window, transposed intermediate, output rows (luma sizes)

// four 4x4 luma PUs side by side, sixteen lanes each, through the packed code of the fast kernel (N = 8 taps, tile 4, 16 lanes: 11 window rows of
// 6 dwords, 11 first-pass items, 4 second-pass items per PU).  Affine prediction is made of these: a whole wave per sub-block through the
// sample-wise body was 0.6 ms for the 518 k sub-blocks of a 4K picture.  Only in the SUB44 variant of the generic kernel (the affine entry points
// launch it): with this path the kernel needs 214 VGPRs instead of 127 -- inline or as a real call -- which costs every other PU size a wave per SIMD.
constexpr int MC44_DW = 11 * 6 + 4 * 6 + 8;                               // per group: window, transposed intermediate (4 x 12 shorts), output (16 shorts)
// Returns the PUs (bits of todo44) whose windows hold a sample outside the bit depth: the packed two-pass form is not the reference's for those (mc_stage),
// the caller serves them with the sample-wise body.
__device__ __forceinline__ unsigned long long mc_luma4x4_chunk(unsigned long long todo44, const vvcgpu_mc_desc* __restrict__ descs, const Pel* __restrict__ ref0Base,
                                                 const Pel* __restrict__ ref1Base, Pel* __restrict__ dstBase, int bd, int cmin, int cmax, int lane, unsigned* tileL)
{
  unsigned* L = tileL + (lane >> 4) * MC44_DW;
  const int gl = lane & 15;
  // the next four PUs' descriptors and windows are requested before the current four are computed
  auto pick = [&](int& sel)
  {
    const int firstSel = (int)__builtin_ctzll(todo44);
    sel = -1;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (todo44) { const int b = (int)__builtin_ctzll(todo44); todo44 &= todo44 - 1ull; if (k == (lane >> 4)) sel = b; }
    return descs[sel >= 0 ? sel : firstSel];
  };
  int selC, selN = -1;
  vvcgpu_mc_desc dC = pick(selC), dN = dC;
  McStaged<8, 4, 16> sC, sN;
  mc_stage<8, 4, 16>(dC, selC >= 0, ref0Base, ref1Base, gl, sC, bd);
  unsigned redoLo = 0u, redoHi = 0u;
  for (;;)
  {
    const bool more = todo44 != 0ull;
    if (more) { dN = pick(selN); mc_stage<8, 4, 16>(dN, selN >= 0, ref0Base, ref1Base, gl, sN, bd); }
    const unsigned long long bm = __builtin_amdgcn_ballot_w64(selC >= 0 && sC.bad != 0u);
    const bool grpBad = ((bm >> (lane & 48)) & 0xFFFFull) != 0ull;           // this lane group's PU
    if (grpBad && selC >= 0) { if (selC < 32) redoLo |= 1u << selC; else redoHi |= 1u << (selC - 32); }
    mc_tile_dot2<8, 4, 16>(dC, selC >= 0 && !grpBad, sC, dstBase, bd, cmin, cmax, gl, L, reinterpret_cast<short*>(L + 11 * 6), reinterpret_cast<short*>(L + 11 * 6 + 4 * 6));
    if (!more) break;
    dC = dN; selC = selN; sC = sN;
  }
  unsigned lo = 0u, hi = 0u;
#pragma unroll
  for (int g4 = 0; g4 < 64; g4 += 16) { lo |= (unsigned)__builtin_amdgcn_readlane((int)redoLo, g4); hi |= (unsigned)__builtin_amdgcn_readlane((int)redoHi, g4); }
  return ((unsigned long long)hi << 32) | lo;
}

#define MC_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)
// The sample-wise body: one block by a group of G lanes (gl = lane index inside the group) in sub-tiles of T x T samples, following the reference branch by
// branch.  win / tmp: the group's LDS ((T + 7) x (T + 8) and (T + 7) x T shorts).  G = 64, T = 16: a wavefront per block (mc_generic_pu); G = 16, T = 4:
// four blocks of at most 4x4 samples side by side in a wavefront (the ATMVP sub-blocks of mergecand.hip) -- the groups may differ in every field, the
// synchronisation orders each group's own LDS accesses.  DIST: the prediction goes to predT (pitch d.w) instead of dst.
template <int G, int T, bool DIST, bool WPF>
__device__ __forceinline__ void mc_samplewise(const vvcgpu_mc_desc& d, const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base, Pel* __restrict__ dstBase,
                                              int bd, int cmin, int cmax, int gl, short* win, short* tmp, short* predT, const vvcgpu_wp_param* e)
{
  constexpr int WPT = T + 8, PER = T * T / G;
  const int N = d.is_luma ? 8 : 4, half = N / 2 - 1;
  const bool rndRes = WPF ? false : d.bi == 0;
  const int nRef = d.bi == 1 ? 2 : 1;

  for (int sy = 0; sy < d.h; sy += T)
    for (int sx = 0; sx < d.w; sx += T)
    {
      const int tw = min(T, d.w - sx), th = min(T, d.h - sy);
      const int npx = tw * th;
      int pred[2][PER];
      if (WPF) { for (int j = 0; j < PER; j++) pred[1][j] = 0; }      // (uni: the second list's operand of wp_apply is not read)
#pragma unroll
      for (int r = 0; r < 2; r++)
      {
        if (r >= nRef) break;
        const Pel* ref = (r ? ref1Base + d.ref1_off : ref0Base + d.ref0_off) + (size_t)sy * (r ? d.ref1_stride : d.ref0_stride) + sx;
        const int rs = r ? d.ref1_stride : d.ref0_stride;
        const int fx = r ? d.frac_x1 : d.frac_x0, fy = r ? d.frac_y1 : d.frac_y0;
        const short* cx = d.is_luma ? c_lumaFilter[fx] : c_chromaFilter[fx];
        const short* cy = d.is_luma ? c_lumaFilter[fy] : c_chromaFilter[fy];
        // stage only what the branch needs: rows [-half, th+N-1-half) when fy != 0, cols likewise when fx != 0
        const int r0 = fy ? -half : 0, nr = fy ? th + N - 1 : th;
        const int c0 = fx ? -half : 0, nc = fx ? tw + N - 1 : tw;
        MC_WAVE_SYNC();                               // previous users of win/tmp are done
        for (int i = gl; i < nr * nc; i += G)
        {
          const int rr = i / nc, cc = i - rr * nc;
          win[rr * WPT + cc] = ref[(ptrdiff_t)(r0 + rr) * rs + c0 + cc];
        }
        MC_WAVE_SYNC();
        if (fx && fy)
        {
          const IfMode mh = if_mode(true, false, bd);
          for (int i = gl; i < nr * tw; i += G)
          {
            const int rr = i / tw, x = i - rr * tw;
            int sum = 0;
            for (int k = 0; k < N; k++) sum += win[rr * WPT + x + k] * cx[k];
            tmp[rr * T + x] = (short)((sum + mh.offset) >> mh.shift);
          }
          MC_WAVE_SYNC();
          const IfMode mv = if_mode(false, rndRes, bd);
#pragma unroll
          for (int j = 0; j < PER; j++)
          {
            const int p = gl + G * j;
            if (p < npx)
            {
              const int y = p / tw, x = p - y * tw;
              int sum = 0;
              for (int k = 0; k < N; k++) sum += tmp[(y + k) * T + x] * cy[k];
              int v = (short)((sum + mv.offset) >> mv.shift);
              if (rndRes) v = clip3(cmin, cmax, v);
              pred[r][j] = v;
            }
          }
        }
        else
        {
          const IfMode m1 = if_mode(true, rndRes, bd);
#pragma unroll
          for (int j = 0; j < PER; j++)
          {
            const int p = gl + G * j;
            if (p < npx)
            {
              const int y = p / tw, x = p - y * tw;
              int v;
              if (!fx && !fy) v = if_copy(win[y * WPT + x], true, rndRes, bd, cmin, cmax);
              else
              {
                int sum = 0;
                if (fx) { for (int k = 0; k < N; k++) sum += win[y * WPT + x + k] * cx[k]; }
                else    { for (int k = 0; k < N; k++) sum += win[(y + k) * WPT + x] * cy[k]; }
                v = (short)((sum + m1.offset) >> m1.shift);
                if (rndRes) v = clip3(cmin, cmax, v);
              }
              pred[r][j] = v;
            }
          }
        }
      }
      Pel* dst = DIST ? predT + sy * d.w + sx : dstBase + d.dst_off + (size_t)sy * d.dst_stride + sx;
      const int dstStride = DIST ? (int)d.w : d.dst_stride;
      const int shiftNum = max(2, IF_INTERNAL_PREC - bd) + 1, offset = (1 << (shiftNum - 1)) + 2 * IF_INTERNAL_OFFS;
#pragma unroll
      for (int j = 0; j < PER; j++)
      {
        const int p = gl + G * j;
        if (p < npx)
        {
          const int y = p / tw, x = p - y * tw;
          int v = pred[0][j];
          if (WPF) v = wp_apply(pred[0][j], pred[1][j], d.bi == 1, *e, shiftNum - 1, cmin, cmax);
          else if (d.bi == 1) v = clip3(cmin, cmax, (pred[0][j] + pred[1][j] + offset) >> shiftNum);
          dst[(size_t)y * dstStride + x] = (short)v;
        }
      }
    }
}

// One PU through the generic body: tiles of the packed form where the PU is a grid of them, else (or when a sample leaves the bit depth) sample by sample.
// ONE wave; win / tmp / tileL: that wave's LDS (WR x WP, WR x ST shorts, MC_LDS_DW dwords); DIST: the prediction goes to predT (pitch d.w) instead of dst.
// TAG separates the copies by caller: a function that is not inlined takes the loosest register budget of the kernels that call it.  WPF: the weighted
// epilogue with entry e (vvcgpu_mc_wp_batch): both lists unrounded, then wp_apply.
template <bool DIST, int TAG, bool WPF = false>
__device__ __forceinline__ void mc_generic_pu(const vvcgpu_mc_desc& d, const Pel* __restrict__ ref0Base, const Pel* __restrict__ ref1Base, Pel* __restrict__ dstBase,
                                              int bd, int cmin, int cmax, int lane, short* win, short* tmp, unsigned* tileL, short* predT,
                                              const vvcgpu_wp_param* e = nullptr)
{
  // descriptors live in device memory, the host cannot validate them: a shape outside the contract (the prediction tile of the fused form is
  // 128 x 128, bi is 0 or 1 there) is skipped with the sentinel ~0 as its distortion instead of overrunning LDS (wave-uniform)
  // a PU whose sides are multiples of the packed path's tile (16 luma / 8 chroma samples) is a grid of tiles with the same fractional phase: the
  // wave walks them with the packed code of the fast kernel (here, not there: inlined into the fast kernel the loop cost it its 80-VGPR budget and
  // the MC stage of the canonical workload went from 0.075 to 0.18 ms)
  if (!DIST && (d.w % (d.is_luma ? 16 : 8)) == 0 && (d.h % (d.is_luma ? 16 : 8)) == 0)
  {
    const int T = d.is_luma ? 16 : 8, tx = d.w / T, nt = tx * (d.h / T);
    auto tile = [&](int t) { vvcgpu_mc_desc q = d; const int y = (t / tx) * T, x = (t - (t / tx) * tx) * T; q.w = q.h = (short)T;
                             q.ref0_off += (int64_t)y * d.ref0_stride + x; q.ref1_off += (int64_t)y * d.ref1_stride + x; q.dst_off += (int64_t)y * d.dst_stride + x; return q; };
    unsigned* L = tileL;
    bool outsideDepth = false;                               // a reference sample outside the bit depth (mc_stage): the whole PU again, sample-wise, below
    if (d.is_luma)
    {
      for (int t = 0; t < nt; t++)
      {
        const vvcgpu_mc_desc q = tile(t);
        McStaged<8, 16, 64> st;
        mc_stage<8, 16, 64>(q, true, ref0Base, ref1Base, lane, st, bd);
        if (__builtin_amdgcn_ballot_w64(st.bad != 0u) != 0ull) { outsideDepth = true; break; }
        mc_tile_dot2<8, 16, 64, WPF>(q, true, st, dstBase, bd, cmin, cmax, lane, L, reinterpret_cast<short*>(L + 23 * 12), reinterpret_cast<short*>(L + 23 * 12 + 16 * 12), e);
      }
    }
    else
    {
      const bool hi = lane >= 32;                            // two chroma tiles side by side in the wave's halves
      unsigned* Lh = L + (hi ? MC_LDS_DW / 2 : 0);
      for (int t = 0; t < nt; t += 2)
      {
        const bool on = t + (hi ? 1 : 0) < nt;
        const vvcgpu_mc_desc q = tile(on ? t + (hi ? 1 : 0) : t);
        McStaged<4, 8, 32> st;
        mc_stage<4, 8, 32>(q, on, ref0Base, ref1Base, lane & 31, st, bd);
        if (__builtin_amdgcn_ballot_w64(st.bad != 0u) != 0ull) { outsideDepth = true; break; }
        mc_tile_dot2<4, 8, 32, WPF>(q, on, st, dstBase, bd, cmin, cmax, lane & 31, Lh, reinterpret_cast<short*>(Lh + 11 * 6), reinterpret_cast<short*>(Lh + 11 * 6 + 8 * 6), e);
      }
    }
    if (!outsideDepth) return;
  }
  mc_samplewise<64, ST, DIST, WPF>(d, ref0Base, ref1Base, dstBase, bd, cmin, cmax, lane, win, tmp, predT, e);
}

}  // namespace
