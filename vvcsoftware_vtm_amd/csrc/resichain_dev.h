// resichain_dev.h -- device functions of the residual chain shared by resichain.hip and the fused entries (intratu.hip, intrachroma.hip,
// interresi.hip): the quantiser / de-quantiser of one TU with its sign bit hiding per coefficient group, the wave reductions, the single-wave
// matrix-core body of a TU with both sides in 16 / 32 / 64 (rc_tu_mfma), the integer wave-per-TU body for any shape (rc_tu_generic) and the lane-group
// bodies of 4x4 / 8x8 (rc_small_group) and 8x4 / 4x8 (rc_rect_group).  The arithmetic is stated here once; the kernels, their work lists and the
// co-operative and packed bodies are resichain.hip's.
// Reference behaviour: xTrMxN_EMT / xITrMxN_EMT (CommonLib/TrQuant.cpp:138-310), Quant::quant and xSignBitHidingHDQ (Quant.cpp:721-834, :142-273),
// Quant::dequant (Quant.cpp:277-428), the reconstruction clip (Buffer.cpp:66-79) -- see resichain.hip.
#pragma once
#include "common.h"
#include "wave_dev.h"
#include "mfma_tr.h"
#include "quant_dev.h"

namespace {

// Pointer arguments of functions that are NOT inlined arrive as generic pointers: every access through them is a FLAT instruction (both wait counters, no
// immediate offsets, LDS through the aperture).  This assumption lets the compiler infer the LDS address space again inside the callee (the pattern for global pointers,
// !is_shared & !is_private, does not survive the optimiser's De Morgan rewrite; global data through flat loads costs little).
#if defined(__HIP_DEVICE_COMPILE__)
#define RC_IS_LDS(p) __builtin_assume(__builtin_amdgcn_is_shared((const __attribute__((address_space(0))) void*)(p)))
#else
#define RC_IS_LDS(p) ((void)0)
#endif


typedef vvcgpu_resi_chain_desc RcDesc;

#define RC_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// ---------------------------------------------------------------------------------------------------
// Quantiser / de-quantiser of one TU (flat scaling lists), filled from quant_dev.h
struct RcQ
{
  unsigned mul;                       // quantiser scale * (181 for 2:1 shapes)
  int qBits, qBits8;
  long long add;
  VqInv dq;
  bool sbh;
};
__device__ __forceinline__ RcQ rc_qparams(int w, int h, int qp, int bd, int intraSlice, int signHiding)
{
  RcQ q;
  const int lw = ilog2(w), lh = ilog2(h), transformShift = vq_transform_shift(bd, lw, lh);
  const bool sqrt2 = vq_sqrt2(lw, lh);
  const VqFwd f = vq_fwd(qp, transformShift, sqrt2, vq_round9(intraSlice));
  q.mul = (unsigned)f.scale * (unsigned)f.whScale;
  q.qBits = f.qBits; q.qBits8 = f.qBits8; q.add = f.add;
  q.dq = vq_inv(qp, transformShift, sqrt2);
  q.sbh = signHiding && w >= 4 && h >= 4;
  return q;
}
// (64-bit arithmetic as the reference's: a 32-bit form of both -- 24-bit multiplies, a funnel shift for (tmp + add) >> qBits, exact for
// |c| < 2^24 and 16 <= qBits <= 31 -- was built and measured in round 6: 71.3 against 68.5 us for the 4K chain, the branch around the 64-bit
// form costs more than the quarter-rate multiplies it saves; docs/OPTIMISATION_LOG.md)
__device__ __forceinline__ int rc_quant_one(const RcQ& q, int c, int& deltaU, int& mag)
{
  const unsigned long long tmp = (unsigned long long)(unsigned)abs(c) * q.mul;
  mag = (int)((tmp + (unsigned long long)q.add) >> q.qBits);
  deltaU = (int)((long long)(tmp - ((unsigned long long)(unsigned)mag << q.qBits)) >> q.qBits8);
  return min(max(c < 0 ? -mag : mag, -32768), 32767);
}
__device__ __forceinline__ int rc_dequant_one(const RcQ& q, int lv) { return vq_dequant_one(q.dq, lv); }

__device__ __forceinline__ unsigned quad_or(unsigned v)
{
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);      // quad_perm [1,0,3,2]
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);      // quad_perm [2,3,0,1]
  return v;
}
__device__ __forceinline__ int quad_min(int v)
{
  v = min(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false));
  return v;
}
// scan position (diagonal 4x4 scan: 0 4 1 8 5 2 12 9 6 3 13 10 7 14 11 15 in raster terms) of (row r, column x) inside a coefficient group
__device__ __forceinline__ int rc_kpos(int r, int x)
{
  const unsigned tab = r == 0 ? 0x9520u : r == 1 ? 0xC841u : r == 2 ? 0xEB73u : 0xFDA6u;
  return (int)((tab >> (4 * x)) & 15u);
}

// any level of the quad's coefficient group non-zero?
__device__ __forceinline__ bool rc_cg_nonzero(const int (&lv)[4])
{
  return quad_or((unsigned)((lv[0] | lv[1] | lv[2] | lv[3]) != 0)) != 0u;
}

// Sign bit hiding of one coefficient group (xSignBitHidingHDQ, Quant.cpp:142-273; logic as quant_tu in quant.hip, which is pinned against
// the reference): the lane holds rows 0..3 of column x = lane & 3 of the group; cf = coefficients, du = the quantiser's deltaU.
__device__ __forceinline__ void rc_sbh_quad(int (&lv)[4], const int (&du)[4], const int (&cf)[4], bool isLast, int lane)
{
  const int x = lane & 3;
  unsigned mA = 0, mB = 0;                                    // mA: non-zero (low half) | odd (high half) per scan position; mB: negative
#pragma unroll
  for (int r = 0; r < 4; r++)
  {
    const int k = rc_kpos(r, x);
    if (lv[r] != 0) mA |= 1u << k;
    if (lv[r] & 1) mA |= 0x10000u << k;
    if (lv[r] < 0) mB |= 1u << k;
  }
  mA = quad_or(mA); mB = quad_or(mB);
  const unsigned nz = mA & 0xFFFFu;
  const int first = nz ? __ffs((int)nz) - 1 : 16, last = nz ? 31 - __clz((int)nz) : -1;
  const unsigned parity = (unsigned)__popc(mA >> 16) & 1u;
  const unsigned signbit = nz ? ((mB >> first) & 1u) : 1u;
  const bool fix = last - first >= 4 && signbit != parity;
  const int start = isLast ? last : 15;
  constexpr int BIG = 1 << 20;
  int bestKey = BIG * 32, bestChange = 0, bestR = 0;
#pragma unroll
  for (int r = 0; r < 4; r++)
  {
    const int k = rc_kpos(r, x);
    int cost = BIG, change = 0;
    if (k <= start)
    {
      if (lv[r] != 0)
      {
        if (du[r] > 0) { cost = -du[r]; change = 1; }
        else if (!(k == first && abs(lv[r]) == 1)) { cost = du[r]; change = -1; }
      }
      else if (k < first) { if ((cf[r] >= 0 ? 0u : 1u) == signbit) { cost = -du[r]; change = 1; } }
      else { cost = -du[r]; change = 1; }
    }
    const int key = cost * 32 + (15 - k);
    if (key < bestKey) { bestKey = key; bestChange = change; bestR = r; }
  }
  const int qmin = quad_min(bestKey);
  if (fix && bestKey == qmin)                                 // keys are distinct inside a group (the scan position is part of the key)
  {
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (r == bestR)
      {
        int change = bestChange;
        if (lv[r] == 32767 || lv[r] == -32768) change = -1;
        lv[r] += cf[r] >= 0 ? change : -change;
      }
  }
}

// ---------------------------------------------------------------------------------------------------
// One TU of W x H (W, H in {16, 32, 64}) on the matrix cores.  Returns false (nothing written) when a residual sample lies outside +-1023
// (precondition violated: the caller's generic path takes the TU).
// mode (workgroup-uniform; the plain transform entries run through the same bodies, vvcgpu_tr_chain_launch below): 0 = the chain; 1 = FORWARD
// transform only: the "original" plane holds the residual, no prediction is read, the coefficients (unquantised, int32) go where the chain writes
// levels, incl. the zero-out region; 2 = INVERSE transform only: the coefficients are read where the chain writes levels (16-bit values: a TU with
// a larger one returns false / goes to the fall-back list), the residual goes where the chain writes the reconstruction, no prediction, no pixel clip.
// 3 = the chain in the RESIDUAL domain (interresi.hip): the "original" plane holds org - pred as for 1, quantiser, levels and abs_sum as for 0, the
// de-quantised residual goes out unclipped as for 2; no prediction is read.  The wave-per-TU body also serves transform skip (tr_hor = 3) in this mode.
enum { RC_CHAIN = 0, RC_FWD = 1, RC_INV = 2, RC_RESI = 3 };
template <int W, int H, int MODE>
__device__ __forceinline__ bool rc_tu_mfma(const RcDesc& d, const Pel* __restrict__ orgBase, const Pel* __restrict__ predBase, Pel* __restrict__ recBase,
                                           TCoeff* __restrict__ levelBase, unsigned* __restrict__ absSumOut, int ti, int bd, int clpMin, int clpMax,
                                           const _Float16* tab, const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int lane)
{
  constexpr int mode = MODE;

  typedef MtShape<W, H> S;
  constexpr int LW = W == 16 ? 4 : W == 32 ? 5 : 6, LH = H == 16 ? 4 : H == 32 ? 5 : 6;
  const int c = lane & 15, g = lane >> 4;
  const Pel* org = orgBase + d.org_off;
  const Pel* pred = predBase + d.pred_off;
  const _Float16* Th = tab + rc_tab_off(d.tr_hor, W, 0);
  const _Float16* ThT = tab + rc_tab_off(d.tr_hor, W, 1);
  const _Float16* Tv = tab + rc_tab_off(d.tr_ver, H, 0);
  const _Float16* TvT = tab + rc_tab_off(d.tr_ver, H, 1);
  TCoeff* level = levelBase + d.level_off;
  const int4v z = { 0, 0, 0, 0 };
  int cq[S::JT][S::IT][4];                             // [column tile (i)][row tile (k)]: the inverse stages' input

  if (mode != RC_INV)
  {
    // ---- residual fragments of stage F1 (A = X from memory, natural k order)
    h8 x[S::RT][S::XS];
    bool inRange = true;
    if (W == 16)
    {
#pragma unroll
      for (int rt = 0; rt < S::RT; rt++)
      {
        const pel4 o = *reinterpret_cast<const pel4*>(org + (size_t)(16 * rt + c) * d.org_stride + 4 * g);
        pel4 p = { 0, 0, 0, 0 };
        if (mode == RC_CHAIN) p = *reinterpret_cast<const pel4*>(pred + (size_t)(16 * rt + c) * d.pred_stride + 4 * g);
        _Float16 a[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { const int v = (int)o[j] - (int)p[j]; inRange = inRange && v >= -1023 && v <= 1023; a[j] = (_Float16)(short)v; }
        x[rt][0] = h8{ a[0], a[1], a[2], a[3], a[0], a[1], a[2], a[3] };
      }
    }
    else
    {
      pel8 o[S::RT][S::XS], p[S::RT][S::XS];
#pragma unroll
      for (int rt = 0; rt < S::RT; rt++)
#pragma unroll
        for (int s = 0; s < S::XS; s++)
        {
          o[rt][s] = *reinterpret_cast<const pel8*>(org + (size_t)(16 * rt + c) * d.org_stride + 32 * s + 8 * g);
          p[rt][s] = pel8{ 0, 0, 0, 0, 0, 0, 0, 0 };
          if (mode == RC_CHAIN) p[rt][s] = *reinterpret_cast<const pel8*>(pred + (size_t)(16 * rt + c) * d.pred_stride + 32 * s + 8 * g);
        }
#pragma unroll
      for (int rt = 0; rt < S::RT; rt++)
#pragma unroll
        for (int s = 0; s < S::XS; s++)
#pragma unroll
          for (int j = 0; j < 8; j++)
          {
            const int v = (int)o[rt][s][j] - (int)p[rt][s][j];
            inRange = inRange && v >= -1023 && v <= 1023;
            x[rt][s][j] = (_Float16)(short)v;
          }
    }
    if (__builtin_amdgcn_ballot_w64(!inRange) != 0ull) return false;

    // rounding shifts of the forward stages (TrQuant.cpp:151-152, 214)
    const int s1 = LW + bd + 6 - 15 + 2, s2 = LH + 6 + 2;
    int t1[S::JT][S::RT][4];                             // [column tile][row tile]: the row tiles are the k dimension of the next product
    mt_fwd1<W, H>(t1, x, Th, s1, c, g);
    int cf[S::IT][S::JT][4];                             // [row tile of C (vertical frequency)][column tile (horizontal frequency)]
    mt_fwd2<W, H>(cf, t1, Tv, s2, c, g);

    // ---- quantiser: tile (it, jt) holds rows 16 it + 4 g + reg, column 16 jt + c; the quad c >> 2 of row group g is one coefficient group
    if (mode == RC_CHAIN || mode == RC_RESI)
    {
      const RcQ q = rc_qparams(W, H, d.qp, bd, d.intra_slice, d.sign_hiding);
      const unsigned short* inv = dqInv + scanOff[(LW - 1) * 6 + (LH - 1)];
      int lv[S::IT][S::JT][4], du[S::IT][S::JT][4];
      int sum = 0, lastCg = -1, cgIdx[S::IT][S::JT];
#pragma unroll
      for (int it = 0; it < S::IT; it++)
#pragma unroll
        for (int jt = 0; jt < S::JT; jt++)
        {
#pragma unroll
          for (int r = 0; r < 4; r++) { int mag; lv[it][jt][r] = rc_quant_one(q, cf[it][jt][r], du[it][jt][r], mag); sum += mag; }
          cgIdx[it][jt] = (int)inv[(16 * it + 4 * g) * W + 16 * jt + (c & ~3)] >> 4;
          if (rc_cg_nonzero(lv[it][jt])) lastCg = max(lastCg, cgIdx[it][jt]);
        }
      lastCg = wave_max(lastCg);
      sum = wave_sum(sum);
      if (lane == 0) absSumOut[ti] = (unsigned)sum;
#pragma unroll
      for (int it = 0; it < S::IT; it++)
#pragma unroll
        for (int jt = 0; jt < S::JT; jt++)
        {
          if (q.sbh) rc_sbh_quad(lv[it][jt], du[it][jt], cf[it][jt], cgIdx[it][jt] == lastCg, lane);
#pragma unroll
          for (int r = 0; r < 4; r++) { level[(16 * it + 4 * g + r) * W + 16 * jt + c] = lv[it][jt][r]; cq[jt][it][r] = rc_dequant_one(q, lv[it][jt][r]); }
        }
    }
    else
    {
#pragma unroll
      for (int it = 0; it < S::IT; it++)
#pragma unroll
        for (int jt = 0; jt < S::JT; jt++)
#pragma unroll
          for (int r = 0; r < 4; r++) level[(16 * it + 4 * g + r) * W + 16 * jt + c] = cf[it][jt][r];
    }
    // zero-out region of the level array: columns >= 32 of the kept rows, then the rows >= 32
    if (W == 64) for (int e = lane; e < S::HJ * 8; e += 64) *reinterpret_cast<int4v*>(level + (e >> 3) * 64 + 32 + 4 * (e & 7)) = z;
    if (H == 64) for (int e = lane; e < 32 * W / 4; e += 64) *reinterpret_cast<int4v*>(level + 32 * W + 4 * e) = z;
    if (mode == RC_FWD) return true;
  }
  else
  {
    bool fits = true;
#pragma unroll
    for (int it = 0; it < S::IT; it++)
#pragma unroll
      for (int jt = 0; jt < S::JT; jt++)
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
          const int v = level[(16 * it + 4 * g + r) * W + 16 * jt + c];
          fits = fits && v >= -32768 && v <= 32767;
          cq[jt][it][r] = v;
        }
    if (__builtin_amdgcn_ballot_w64(!fits) != 0ull) return false;
  }

  // ---- inverse stages, reconstruction
  int y1[S::RT][S::JT][4];                             // [row tile (r)][frequency tile (i)]: the frequency tiles are the k dimension of the last product
  mt_inv1<W, H>(y1, cq, TvT, c, g);
  const int s2i = (6 + 15 - 1) - bd + 2;
  Pel* rec = recBase + d.rec_off;
  mt_inv2<W, H>(y1, ThT, s2i, c, g, [&](int rt, int xt, const int (&resi)[4])
  {
    pel4 out;
    if (mode == RC_CHAIN)
    {
      const pel4 pv = *reinterpret_cast<const pel4*>(pred + (size_t)(16 * rt + c) * d.pred_stride + 16 * xt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; r++) out[r] = (short)clip3(clpMin, clpMax, (int)pv[r] + (int)(short)resi[r]);
    }
    else
    {
#pragma unroll
      for (int r = 0; r < 4; r++) out[r] = (short)resi[r];
    }
    *reinterpret_cast<pel4*>(rec + (size_t)(16 * rt + c) * d.rec_stride + 16 * xt + 4 * g) = out;
  });
  return true;
}

// the single-wave matrix-core bodies of the chain kernel's rarer classes (64x16 .. 16x32) as real calls: inline, the kernel's register need is the
// sum of what the compiler keeps live across its switch (docs/OPTIMISATION_LOG.md, round 6)
template <int W, int H, int MODE>
__device__ __noinline__ bool rc_tu_mfma_call(const RcDesc* __restrict__ descs, int ti, const Pel* __restrict__ orgBase, const Pel* __restrict__ predBase, Pel* __restrict__ recBase,
                                             TCoeff* __restrict__ levelBase, unsigned* __restrict__ absSumOut, int bd, int clpMin, int clpMax,
                                             const _Float16* tab, const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int lane)
{
  return rc_tu_mfma<W, H, MODE>(descs[ti], orgBase, predBase, recBase, levelBase, absSumOut, ti, bd, clpMin, clpMax, tab, dqInv, scanOff, lane);
}

// ---------------------------------------------------------------------------------------------------
// Generic path: one wave per TU, any W x H in 2..64; the residual / intermediates / coefficients live in two LDS buffers of the wave.
// Matrices come from global memory (int32 tables).  Exact 32-bit arithmetic as the reference's `int` loops.
__device__ __forceinline__ const int* rc_t32(const int* tr32, int type, int n) { return tr32 + type * 5460 + (n * n - 4) / 3; }
// LDS copy of the matrices the generic path reads (rc_generic_kernel<512, 4>): per type the sizes 2 .. 32 (1364 ints), then DCT-II 64
constexpr int RC_GT_TYPE = 1364, RC_GT_INTS = 3 * RC_GT_TYPE + 4096;
__device__ __forceinline__ const int* rc_t32_lds(const int* tabL, int type, int n) { return n == 64 ? tabL + 3 * RC_GT_TYPE : tabL + type * RC_GT_TYPE + (n * n - 4) / 3; }

template <int MODE = RC_CHAIN>
__device__ void rc_tu_generic(const RcDesc& d, const Pel* __restrict__ orgBase, const Pel* __restrict__ predBase, Pel* __restrict__ recBase,
                              TCoeff* __restrict__ levelBase, unsigned* __restrict__ absSumOut, int ti, int bd, int clpMin, int clpMax,
                              const int* __restrict__ tr32, const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff,
                              int* bufA, int* bufB, int lane, const int* tabL = nullptr)
{
  constexpr int mode = MODE;
  const int w = d.w, h = d.h, lw = ilog2(w), lh = ilog2(h);
  const int wj = w > 32 ? 32 : w, hj = h > 32 ? 32 : h;
  const Pel* org = orgBase + d.org_off;
  const Pel* pred = predBase + d.pred_off;
  const int* Th = tabL ? rc_t32_lds(tabL, d.tr_hor, w) : rc_t32(tr32, d.tr_hor, w);      // the matrix entries sit on the inner loops: LDS when the kernel has a copy
  const int* Tv = tabL ? rc_t32_lds(tabL, d.tr_ver, h) : rc_t32(tr32, d.tr_ver, h);
  TCoeff* level = levelBase + d.level_off;
  Pel* rec = recBase + d.rec_off;
  if ((mode == RC_FWD || mode == RC_INV) && d.tr_hor == 3)   // transform skip of the plain transform entries (TrQuant.cpp:795-847): element-wise
  {
    int shift = 15 - bd - ((lw + lh) >> 1), scale = 1;
    if ((lw + lh) & 1) { shift += mode == RC_FWD ? -8 : 7; scale = 181; }
    for (int e = lane; e < w * h; e += 64)
    {
      const int r = e >> lw, k = e & (w - 1);
      if (mode == RC_FWD)
      {
        const int v = (int)org[(size_t)r * d.org_stride + k] * scale;
        level[e] = shift >= 0 ? v << shift : (v + (1 << (-shift - 1))) >> -shift;
      }
      else
      {
        const int cc = level[e] * scale;
        rec[(size_t)r * d.rec_stride + k] = (short)(shift >= 0 ? (cc + (shift ? 1 << (shift - 1) : 0)) >> shift : cc << -shift);
      }
    }
    return;
  }
  const int s1 = lw + bd + 6 - 15 + 2, s2 = lh + 6 + 2;
  if (mode != RC_INV)
  {
  for (int e = lane; e < w * h; e += 64)
  {
    const int r = e >> lw, k = e & (w - 1);
    bufA[e] = (int)org[(size_t)r * d.org_stride + k] - (mode == RC_CHAIN ? (int)pred[(size_t)r * d.pred_stride + k] : 0);
    if (mode == RC_RESI && d.tr_hor == 3)                // xTransformSkip (TrQuant.cpp:1112-1163) in place of the two stages
    {
      const int sh = 15 - bd - ((lw + lh) >> 1) - (((lw + lh) & 1) ? 8 : 0), v = bufA[e] * (((lw + lh) & 1) ? 181 : 1);
      bufA[e] = sh >= 0 ? v << sh : (v + (1 << (-sh - 1))) >> -sh;
    }
  }
  RC_WAVE_SYNC();
  if (!(mode == RC_RESI && d.tr_hor == 3))
  {
  for (int e = lane; e < wj * h; e += 64)                // F1: bufB[j * h + r]
  {
    const int j = e >> lh, r = e & (h - 1);
    int sum = 0;
#pragma unroll 4
    for (int k = 0; k < w; k++) sum += bufA[r * w + k] * Th[j * w + k];
    bufB[e] = (sum + (1 << (s1 - 1))) >> s1;
  }
  RC_WAVE_SYNC();
  for (int e = lane; e < w * h; e += 64)                 // F2: coefficients, raster, zero outside the kept region
  {
    const int j2 = e >> lw, j1 = e & (w - 1);
    int v = 0;
    if (j2 < hj && j1 < wj)
    {
      int sum = 0;
#pragma unroll 4
      for (int r = 0; r < h; r++) sum += bufB[j1 * h + r] * Tv[j2 * h + r];
      v = (sum + (1 << (s2 - 1))) >> s2;
    }
    bufA[e] = v;
  }
  RC_WAVE_SYNC();
  }
  if (mode == RC_FWD)                                    // forward transform only: the coefficients (zero outside the kept region) are the result
  {
    for (int e = lane; e < w * h; e += 64) level[e] = bufA[e];
    RC_WAVE_SYNC();
    return;
  }
  // quantiser: lane = column (chunks of 64 columns never occur: w <= 64), four rows per pass
  const RcQ q = rc_qparams(w, h, d.qp, bd, d.intra_slice, d.sign_hiding);
  int sum = 0;
  if (!q.sbh)
  {
    for (int e = lane; e < w * h; e += 64)
    {
      int duu, mag;
      const int l = rc_quant_one(q, bufA[e], duu, mag);
      sum += mag;
      level[e] = l;
      bufA[e] = rc_dequant_one(q, l);
    }
  }
  else
  {
    const unsigned short* inv = dqInv + scanOff[(lw - 1) * 6 + (lh - 1)];
    const int col = lane & (w - 1), rowsPerPass = 4 * (64 >> lw);          // narrow TUs: several groups of 4 rows side by side in the wave
    const int rsub = (lane >> lw) * 4;
    int lastCg = -1;
    for (int r0 = 0; r0 < h; r0 += rowsPerPass)
    {
      const int row = r0 + rsub;
      int lv[4], duu[4];
      const bool on = row < h;
#pragma unroll
      for (int r = 0; r < 4; r++) { int mag; lv[r] = rc_quant_one(q, on ? bufA[(row + r) * w + col] : 0, duu[r], mag); sum += on ? mag : 0; }
      const bool nz = rc_cg_nonzero(lv);
      if (on && nz) lastCg = max(lastCg, (int)inv[row * w + (col & ~3)] >> 4);
    }
    lastCg = wave_max(lastCg);
    for (int r0 = 0; r0 < h; r0 += rowsPerPass)
    {
      const int row = r0 + rsub;
      const bool on = row < h;
      int lv[4], duu[4], cfv[4];
#pragma unroll
      for (int r = 0; r < 4; r++) { int mag; cfv[r] = on ? bufA[(row + r) * w + col] : 0; lv[r] = rc_quant_one(q, cfv[r], duu[r], mag); }
      const int cg = on ? (int)inv[row * w + (col & ~3)] >> 4 : -2;
      rc_sbh_quad(lv, duu, cfv, cg == lastCg, lane);
      if (on)
      {
#pragma unroll
        for (int r = 0; r < 4; r++) { level[(row + r) * w + col] = lv[r]; bufA[(row + r) * w + col] = rc_dequant_one(q, lv[r]); }
      }
    }
  }
  sum = wave_sum(sum);
  if (lane == 0) absSumOut[ti] = (unsigned)sum;
  }
  else
  {
    for (int e = lane; e < w * h; e += 64) bufA[e] = level[e];       // inverse transform only: the coefficients come from memory
  }
  RC_WAVE_SYNC();
  if (mode == RC_RESI && d.tr_hor == 3)                  // xITransformSkip (TrQuant.cpp:795-847)
  {
    const int sh = 15 - bd - ((lw + lh) >> 1) + (((lw + lh) & 1) ? 7 : 0), sc = ((lw + lh) & 1) ? 181 : 1;
    for (int e = lane; e < w * h; e += 64)
    {
      const int cc = bufA[e] * sc;
      rec[(size_t)(e >> lw) * d.rec_stride + (e & (w - 1))] = (short)(sh >= 0 ? (cc + (sh ? 1 << (sh - 1) : 0)) >> sh : cc << -sh);
    }
    RC_WAVE_SYNC();
    return;
  }
  for (int e = lane; e < wj * h; e += 64)                // I1 (vertical): bufB[i * h + r] = clip(sum_k Cq[k][i] Tv[k][r])
  {
    const int i = e >> lh, r = e & (h - 1);
    int acc = 0;
#pragma unroll 4
    for (int k = 0; k < hj; k++) acc += bufA[k * w + i] * Tv[k * h + r];
    bufB[e] = clip3(-(1 << 15), (1 << 15) - 1, (acc + 256) >> 9);
  }
  RC_WAVE_SYNC();
  const int s2i = (6 + 15 - 1) - bd + 2;
  for (int e = lane; e < w * h; e += 64)                 // I2 (horizontal) + reconstruction
  {
    const int r = e >> lw, x = e & (w - 1);
    int acc = 0;
#pragma unroll 4
    for (int i = 0; i < wj; i++) acc += bufB[i * h + r] * Th[i * w + x];
    const int resi = (short)clip3(-(1 << 15), (1 << 15) - 1, (acc + (1 << (s2i - 1))) >> s2i);
    rec[(size_t)r * d.rec_stride + x] = mode == RC_CHAIN ? (short)clip3(clpMin, clpMax, (int)pred[(size_t)r * d.pred_stride + x] + resi) : (short)resi;
  }
  RC_WAVE_SYNC();
}

// the 4- and 8-point matrices as int32 for the lane-group bodies, behind the f16 matrices in the table image (resichain.hip: rc_build_tables_kernel)
struct RcSmallTab { int t[3][16 + 64]; int tt[3][16 + 64]; };       // per type: size 4 at 0, size 8 at 16; tt = transposes
static_assert(sizeof(RcSmallTab) % 16 == 0, "copied with 16-byte loads");

// ---------------------------------------------------------------------------------------------------
// (multiplies: 24-bit, full rate -- operands are at most 18-bit intermediates and 8-bit matrix entries; the 32-bit v_mul_lo_u32 is a quarter-rate instruction)
// 4 x 4 and 8 x 8: lane groups of S lanes per TU, G = 64 / S TUs per wave.  Forward: lane = row (stage 1), transposed through LDS, lane = column
// (stage 2, quantiser, de-quantiser, vertical inverse stage), transposed back, lane = row (horizontal inverse stage + reconstruction: the
// prediction row is still in the lane's registers).
template <int S, int MODE>
__device__ __noinline__ void rc_small_group(const RcDesc* __restrict__ descs, const int* __restrict__ list, int cnt, int item,
                                               const Pel* __restrict__ orgBase, const Pel* __restrict__ predBase, Pel* __restrict__ recBase,
                                               TCoeff* __restrict__ levelBase, unsigned* __restrict__ absSumOut, int bd, int clpMin, int clpMax,
                                               const RcSmallTab& tabs, int* tmpL, int lane)
{
  constexpr int mode = MODE;
  RC_IS_LDS(tmpL);

  constexpr int G = 64 / S, LS = S == 4 ? 2 : 3, TO = S == 4 ? 0 : 16;
  typedef short pelS __attribute__((ext_vector_type(S)));
  const int tg = lane / S, li = lane % S;
  const int k = item * G + tg;
  const bool act = k < cnt;
  const int ti = list[act ? k : 0];
  const RcDesc d = descs[ti];
  int* tt = tmpL + tg * (S * (S + 1));
  const int* Th = tabs.t[d.tr_hor] + TO;
  const int* Tv = tabs.t[d.tr_ver] + TO;
  const int* ThT = tabs.tt[d.tr_hor] + TO;
  const int* TvT = tabs.tt[d.tr_ver] + TO;
  // stage F1: lane = row li
  pelS p;
#pragma unroll
  for (int jj = 0; jj < S; jj++) p[jj] = 0;
  const int s1 = LS + bd + 6 - 15 + 2, s2 = LS + 6 + 2;
  int cq[S];                                                              // the inverse stages' input: column li
  TCoeff* level = levelBase + d.level_off;
  if (mode != RC_INV)
  {
  const pelS o = *reinterpret_cast<const pelS*>(orgBase + d.org_off + (size_t)li * d.org_stride);
  if (mode == RC_CHAIN) p = *reinterpret_cast<const pelS*>(predBase + d.pred_off + (size_t)li * d.pred_stride);
  {
    int x[S];
#pragma unroll
    for (int j = 0; j < S; j++) x[j] = (int)o[j] - (int)p[j];
#pragma unroll
    for (int j = 0; j < S; j++)
    {
      int sum = 0;
#pragma unroll
      for (int kk = 0; kk < S; kk++) sum += __mul24(x[kk], Th[j * S + kk]);
      tt[j * (S + 1) + li] = (sum + (1 << (s1 - 1))) >> s1;
    }
  }
  RC_WAVE_SYNC();
  // stage F2: lane = column li (horizontal frequency), registers = rows
  int cf[S];
  {
    int t[S];
#pragma unroll
    for (int r = 0; r < S; r++) t[r] = tt[li * (S + 1) + r];
#pragma unroll
    for (int j = 0; j < S; j++)
    {
      int sum = 0;
#pragma unroll
      for (int r = 0; r < S; r++) sum += __mul24(t[r], Tv[j * S + r]);
      cf[j] = (sum + (1 << (s2 - 1))) >> s2;
    }
  }
  RC_WAVE_SYNC();
  if (mode == RC_FWD)                                                     // forward transform only: the coefficients are the result
  {
    if (act)
    {
#pragma unroll
      for (int j = 0; j < S; j++) level[j * S + li] = cf[j];
    }
    return;
  }
  // quantiser (coefficient groups: rows 4 R .. 4 R + 3 x the lane's aligned quad)
  const RcQ q = rc_qparams(S, S, d.qp, bd, d.intra_slice, d.sign_hiding);
  int lv[S], du[S], sum = 0;
#pragma unroll
  for (int j = 0; j < S; j++) { int mag; lv[j] = rc_quant_one(q, cf[j], du[j], mag); sum += mag; }
#pragma unroll
  for (int m = 1; m < S; m <<= 1) sum += __shfl_xor(sum, m);
  if (act && li == 0) absSumOut[ti] = (unsigned)sum;
  if (q.sbh)
  {
    // coefficient-group scan index inside the TU: 4x4: one group; 8x8: (cx, cy) -> 2 cx + cy (diagonal scan of the 2 x 2 group grid)
    int lastCg = -1;
#pragma unroll
    for (int R = 0; R < S / 4; R++)
    {
      int l4[4] = { lv[4 * R], lv[4 * R + 1], lv[4 * R + 2], lv[4 * R + 3] };
      if (rc_cg_nonzero(l4)) lastCg = max(lastCg, 2 * (li >> 2) + R);
    }
    if (S == 8) lastCg = max(lastCg, __shfl_xor(lastCg, 4));
#pragma unroll
    for (int R = 0; R < S / 4; R++)
    {
      int l4[4] = { lv[4 * R], lv[4 * R + 1], lv[4 * R + 2], lv[4 * R + 3] };
      const int d4[4] = { du[4 * R], du[4 * R + 1], du[4 * R + 2], du[4 * R + 3] };
      const int c4[4] = { cf[4 * R], cf[4 * R + 1], cf[4 * R + 2], cf[4 * R + 3] };
      rc_sbh_quad(l4, d4, c4, 2 * (li >> 2) + R == lastCg, lane);
#pragma unroll
      for (int r = 0; r < 4; r++) lv[4 * R + r] = l4[r];
    }
  }
  if (act)
  {
#pragma unroll
    for (int j = 0; j < S; j++) level[j * S + li] = lv[j];
  }
#pragma unroll
  for (int j = 0; j < S; j++) cq[j] = rc_dequant_one(q, lv[j]);
  }
  else
  {
#pragma unroll
    for (int j = 0; j < S; j++) cq[j] = act ? level[j * S + li] : 0;      // any 32-bit coefficient: exact 32-bit multiplies below
  }
  // stage I1 (vertical): y[r] = clip(sum_k Cq[k] Tv[k][r]); written transposed: tt[r][column li]
  {
    bool fits24 = true;                                                   // 24-bit multiplies when every coefficient of the wave allows it (always, for de-quantiser output)
    if (mode != RC_CHAIN)
    {
#pragma unroll
      for (int kk = 0; kk < S; kk++) fits24 = fits24 && cq[kk] >= -(1 << 23) && cq[kk] < (1 << 23);
    }
    const bool narrow = mode == RC_CHAIN || __builtin_amdgcn_ballot_w64(!fits24) == 0ull;
#pragma unroll
    for (int r = 0; r < S; r++)
    {
      int acc = 0;
      if (narrow)
      {
#pragma unroll
        for (int kk = 0; kk < S; kk++) acc += __mul24(cq[kk], TvT[r * S + kk]);
      }
      else
      {
#pragma unroll
        for (int kk = 0; kk < S; kk++) acc += cq[kk] * TvT[r * S + kk];
      }
      tt[r * (S + 1) + li] = clip3(-(1 << 15), (1 << 15) - 1, (acc + 256) >> 9);
    }
  }
  RC_WAVE_SYNC();
  // stage I2 (horizontal): lane = row li
  const int s2i = (6 + 15 - 1) - bd + 2;
  {
    int y[S];
#pragma unroll
    for (int i = 0; i < S; i++) y[i] = tt[li * (S + 1) + i];
    pelS out;
#pragma unroll
    for (int x = 0; x < S; x++)
    {
      int acc = 0;
#pragma unroll
      for (int i = 0; i < S; i++) acc += __mul24(y[i], ThT[x * S + i]);
      const int resi = (short)clip3(-(1 << 15), (1 << 15) - 1, (acc + (1 << (s2i - 1))) >> s2i);
      out[x] = mode == RC_CHAIN ? (short)clip3(clpMin, clpMax, (int)p[x] + resi) : (short)resi;
    }
    if (act) *reinterpret_cast<pelS*>(recBase + d.rec_off + (size_t)li * d.rec_stride) = out;
  }
  RC_WAVE_SYNC();
}

// 8 x 4 and 4 x 8 (the most frequent rectangles of a real encode: tests/golden/trace_*.npz): the same scheme with 8 lanes per TU -- lane = row
// in the horizontal stages (H rows), lane = column in the vertical stages and the quantiser (W columns; the other lanes of the group idle there).
// The TU has two coefficient groups side by side (8 x 4) or one above the other (4 x 8): the group's scan index is its position.
template <int W, int H, int MODE>
__device__ __noinline__ void rc_rect_group(const RcDesc* __restrict__ descs, const int* __restrict__ list, int cnt, int item,
                                              const Pel* __restrict__ orgBase, const Pel* __restrict__ predBase, Pel* __restrict__ recBase,
                                              TCoeff* __restrict__ levelBase, unsigned* __restrict__ absSumOut, int bd, int clpMin, int clpMax,
                                              const RcSmallTab& tabs, int* tmpL, int lane)
{
  constexpr int mode = MODE;

  constexpr int L = 8, G = 64 / L, LW = W == 4 ? 2 : 3, LH = H == 4 ? 2 : 3, TOW = W == 4 ? 0 : 16, TOH = H == 4 ? 0 : 16;
  typedef short pelW __attribute__((ext_vector_type(W)));
  const int tg = lane / L, li = lane % L;
  const int k = item * G + tg;
  const bool act = k < cnt;
  const int ti = list[act ? k : 0];
  const RcDesc d = descs[ti];
  int* tt = tmpL + tg * (L * (L + 1));
  const int* Th = tabs.t[d.tr_hor] + TOW;
  const int* Tv = tabs.t[d.tr_ver] + TOH;
  const int* ThT = tabs.tt[d.tr_hor] + TOW;
  const int* TvT = tabs.tt[d.tr_ver] + TOH;
  const bool isRow = li < H, isCol = li < W;
  const int rr = isRow ? li : 0;
  // stage F1: lane = row
  pelW p;
#pragma unroll
  for (int jj = 0; jj < W; jj++) p[jj] = 0;
  const int s1 = LW + bd + 6 - 15 + 2, s2 = LH + 6 + 2;
  int cq[H];                                                              // the inverse stages' input: column li
  TCoeff* level = levelBase + d.level_off;
  if (mode != RC_INV)
  {
  const pelW o = *reinterpret_cast<const pelW*>(orgBase + d.org_off + (size_t)rr * d.org_stride);
  if (mode == RC_CHAIN) p = *reinterpret_cast<const pelW*>(predBase + d.pred_off + (size_t)rr * d.pred_stride);
  if (isRow)
  {
    int x[W];
#pragma unroll
    for (int j = 0; j < W; j++) x[j] = (int)o[j] - (int)p[j];
#pragma unroll
    for (int j = 0; j < W; j++)
    {
      int sum = 0;
#pragma unroll
      for (int kk = 0; kk < W; kk++) sum += __mul24(x[kk], Th[j * W + kk]);
      tt[j * (L + 1) + li] = (sum + (1 << (s1 - 1))) >> s1;
    }
  }
  RC_WAVE_SYNC();
  // stage F2: lane = column (horizontal frequency), registers = rows
  int cf[H];
  {
    int t[H];
#pragma unroll
    for (int r = 0; r < H; r++) t[r] = isCol ? tt[li * (L + 1) + r] : 0;
#pragma unroll
    for (int j = 0; j < H; j++)
    {
      int sum = 0;
#pragma unroll
      for (int r = 0; r < H; r++) sum += __mul24(t[r], Tv[j * H + r]);
      cf[j] = (sum + (1 << (s2 - 1))) >> s2;
    }
  }
  RC_WAVE_SYNC();
  if (mode == RC_FWD)                                                     // forward transform only: the coefficients are the result
  {
    if (act && isCol)
    {
#pragma unroll
      for (int j = 0; j < H; j++) level[j * W + li] = cf[j];
    }
    return;
  }
  // quantiser (coefficient groups: rows 4 R .. 4 R + 3 x the lane's aligned quad); idle lanes carry zeros
  const RcQ q = rc_qparams(W, H, d.qp, bd, d.intra_slice, d.sign_hiding);
  int lv[H], du[H], sum = 0;
#pragma unroll
  for (int j = 0; j < H; j++) { int mag; lv[j] = rc_quant_one(q, cf[j], du[j], mag); sum += mag; }
#pragma unroll
  for (int m = 1; m < L; m <<= 1) sum += __shfl_xor(sum, m);
  if (act && li == 0) absSumOut[ti] = (unsigned)sum;
  if (q.sbh)
  {
    int lastCg = -1;
#pragma unroll
    for (int R = 0; R < H / 4; R++)
    {
      int l4[4] = { lv[4 * R], lv[4 * R + 1], lv[4 * R + 2], lv[4 * R + 3] };
      if (rc_cg_nonzero(l4)) lastCg = max(lastCg, (W == 8 ? (li >> 2) : 0) + R);
    }
    lastCg = max(lastCg, __shfl_xor(lastCg, 4));
#pragma unroll
    for (int R = 0; R < H / 4; R++)
    {
      int l4[4] = { lv[4 * R], lv[4 * R + 1], lv[4 * R + 2], lv[4 * R + 3] };
      const int d4[4] = { du[4 * R], du[4 * R + 1], du[4 * R + 2], du[4 * R + 3] };
      const int c4[4] = { cf[4 * R], cf[4 * R + 1], cf[4 * R + 2], cf[4 * R + 3] };
      rc_sbh_quad(l4, d4, c4, (W == 8 ? (li >> 2) : 0) + R == lastCg, lane);
#pragma unroll
      for (int r = 0; r < 4; r++) lv[4 * R + r] = l4[r];
    }
  }
  if (act && isCol)
  {
#pragma unroll
    for (int j = 0; j < H; j++) level[j * W + li] = lv[j];
  }
#pragma unroll
  for (int j = 0; j < H; j++) cq[j] = rc_dequant_one(q, lv[j]);
  }
  else
  {
#pragma unroll
    for (int j = 0; j < H; j++) cq[j] = (act && isCol) ? level[j * W + li] : 0;   // any 32-bit coefficient: exact 32-bit multiplies below
  }
  // stage I1 (vertical), written transposed: tt[r][column]
  bool fits24 = true;
  if (mode != RC_CHAIN)
  {
#pragma unroll
    for (int kk = 0; kk < H; kk++) fits24 = fits24 && cq[kk] >= -(1 << 23) && cq[kk] < (1 << 23);
  }
  const bool narrow = mode == RC_CHAIN || __builtin_amdgcn_ballot_w64(!fits24) == 0ull;
  if (isCol)
  {
#pragma unroll
    for (int r = 0; r < H; r++)
    {
      int acc = 0;
      if (narrow)
      {
#pragma unroll
        for (int kk = 0; kk < H; kk++) acc += __mul24(cq[kk], TvT[r * H + kk]);
      }
      else
      {
#pragma unroll
        for (int kk = 0; kk < H; kk++) acc += cq[kk] * TvT[r * H + kk];
      }
      tt[r * (L + 1) + li] = clip3(-(1 << 15), (1 << 15) - 1, (acc + 256) >> 9);
    }
  }
  RC_WAVE_SYNC();
  // stage I2 (horizontal): lane = row
  const int s2i = (6 + 15 - 1) - bd + 2;
  if (isRow)
  {
    int y[W];
#pragma unroll
    for (int i = 0; i < W; i++) y[i] = tt[li * (L + 1) + i];
    pelW out;
#pragma unroll
    for (int x = 0; x < W; x++)
    {
      int acc = 0;
#pragma unroll
      for (int i = 0; i < W; i++) acc += __mul24(y[i], ThT[x * W + i]);
      const int resi = (short)clip3(-(1 << 15), (1 << 15) - 1, (acc + (1 << (s2i - 1))) >> s2i);
      out[x] = mode == RC_CHAIN ? (short)clip3(clpMin, clpMax, (int)p[x] + resi) : (short)resi;
    }
    if (act) *reinterpret_cast<pelW*>(recBase + d.rec_off + (size_t)li * d.rec_stride) = out;
  }
  RC_WAVE_SYNC();
}

}  // namespace
