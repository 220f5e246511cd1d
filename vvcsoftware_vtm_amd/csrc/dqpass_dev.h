// dqpass_dev.h -- what the RD pass entries under DepQuant 1 share around the trellis of depquant_dev.h, stated once for interresidq.hip
// (vvcgpu_inter_resi_code_dq_batch) and intratudq.hip (vvcgpu_intra_tu_code_dq_batch): the transform bodies of resichain_dev.h as real calls on a
// wavefront's LDS tile (forward into the coefficient workspace, inverse out of it), the trellis over a work list, the dependent de-quantiser of one TU
// by one wavefront, and the workspace's slack.  A front kernel stages the residual in the tile and runs iq_transform<RC_FWD>, the trellis kernel is
// iq_trellis<true> behind its count, a back kernel runs iq_dequant and iq_transform<RC_INV>; the item walk around them is each file's own.
#pragma once
#include "common.h"
#include "depquant_dev.h"
#include "mfma_tr.h"
#include "quant_dev.h"
#include "resichain_dev.h"

namespace {

constexpr int IQ_TAB_BYTES = RC_TAB_HALVES * 2;                           // the f16 matrices of the matrix-core bodies
constexpr size_t IQ_WS_SLACK = 4096 * sizeof(TCoeff) + 256;               // a quad of the trellis that walks along with a larger TU of its wavefront reads up to 4095 coefficients past its own
inline size_t iq_extent16(size_t level_extent) { return (level_extent + 15) & ~(size_t)15; }

// the transform bodies as real calls (the descriptor and the tile are the wavefront's, in LDS)
template <int W, int H, int MODE>
__device__ __noinline__ bool iq_tu_mfma_call(const RcDesc* dS, const Pel* tile, Pel* __restrict__ outBase, TCoeff* __restrict__ coefBase, int bd, const _Float16* tab,
                                             const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int lane)
{
  RC_IS_LDS(dS); RC_IS_LDS(tile); RC_IS_LDS(tab);
  return rc_tu_mfma<W, H, MODE>(*dS, tile, tile, outBase, coefBase, nullptr, 0, bd, 0, 0, tab, dqInv, scanOff, lane);
}
template <int MODE>
__device__ __noinline__ void iq_tu_generic_call(const RcDesc* dS, const Pel* tile, Pel* __restrict__ outBase, TCoeff* __restrict__ coefBase, int bd,
                                                const int* __restrict__ tr32, const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff,
                                                int* bufA, int* bufB, int lane)
{
  rc_tu_generic<MODE>(*dS, tile, tile, outBase, coefBase, nullptr, 0, bd, 0, 0, tr32, dqInv, scanOff, bufA, bufB, lane, nullptr);
}
// one TU through the forward (MODE RC_FWD: tile -> coefficients) or the inverse transform (RC_INV: coefficients -> outBase + rec_off)
template <int MODE>
__device__ __forceinline__ void iq_transform(const RcDesc* dS, short* resiT, Pel* outBase, TCoeff* coefBase, int bd, const _Float16* tab, const VvcTrTables& tb,
                                             int* fbScr, int lane)
{
  const int w = dS->w, h = dS->h;
  if (w <= 8 || h <= 8)                                                   // at most 512 samples: the integer body, its two buffers behind them in the tile
  {
    iq_tu_generic_call<MODE>(dS, resiT, outBase, coefBase, bd, tb.tr32, tb.dqInv, tb.scanOff, reinterpret_cast<int*>(resiT + 1024), reinterpret_cast<int*>(resiT + 2048), lane);
    return;
  }
  bool done = true;
#define IQ_MF(W_, H_) case ((W_) << 8) | (H_): done = iq_tu_mfma_call<W_, H_, MODE>(dS, resiT, outBase, coefBase, bd, tab, tb.dqInv, tb.scanOff, lane); break;
  switch ((w << 8) | h)
  {
  IQ_MF(16, 16) IQ_MF(16, 32) IQ_MF(16, 64) IQ_MF(32, 16) IQ_MF(32, 32) IQ_MF(32, 64) IQ_MF(64, 16) IQ_MF(64, 32) IQ_MF(64, 64)
  default: break;
  }
#undef IQ_MF
  if (!done)                                                              // samples outside the bit depth (out of contract): exact all the same
    iq_tu_generic_call<MODE>(dS, resiT, outBase, coefBase, bd, tb.tr32, tb.dqInv, tb.scanOff, fbScr, fbScr + 4096, lane);
}

// the trellis over the work list: work item ti is descriptor list[ti].  (The body behind the kernel's early exit is a function of its own, and LISTED
// its template parameter, because the kernel's instruction stream is then what it was when the body was tq_trellis<true> of depquant_dev.h; included
// in the kernel itself it comes out five instructions shorter and unmeasured.)
template <bool LISTED>
__device__ __forceinline__ void iq_trellis(const TCoeff* __restrict__ coeffBase, TCoeff* __restrict__ levelBase,
                                           const vvcgpu_depquant_desc* __restrict__ descs, const int* __restrict__ list, int n,
                                           const vvcgpu_dq_rates* __restrict__ ratesBase, int bd, unsigned* __restrict__ absSumOut,
                                           unsigned* __restrict__ wsDec, unsigned char* __restrict__ wsCtx, VvcTrTables tb)
{
#include "depquant_body.inc"
}

// DQIntern::Quantizer::dequantBlock (DepQuant.cpp:708-785) of one TU by the wavefront: levels -> coefficients, both w x h with row pitch w.  The 4-state
// machine is linear over GF(2) (transform.hip, dq_group): with steps counted from the END of the scan, the state bit that enters the reconstruction of
// step t is the xor of the level parities of the earlier steps of the other step parity.  A lane takes a run of consecutive steps, folds its parities by
// step parity, a ballot gives the prefix over the lanes in front of it, a second pass reconstructs.
__device__ __forceinline__ void iq_dequant(const TCoeff* __restrict__ level, TCoeff* __restrict__ coef, int w, int h, int qp, int bd,
                                           const unsigned short* __restrict__ scan, int lane)
{
  const int lw = ilog2(w), lh = ilog2(h), cnt = w * h;
  const VqInv dep = vq_inv(qp + 1, vq_transform_shift(bd, lw, lh), vq_sqrt2(lw, lh));      // scale and shift of qp + 1 with one more bit (:758-759)
  int shift = dep.rightShift + 1;
  long long scale = dep.scale;
  if (shift < 0) { scale <<= -shift; shift = 0; }
  const long long add = (1ll << shift) >> 1;
  const int C = cnt >= 64 ? cnt >> 6 : 1, t0 = lane * C, t1 = min(t0 + C, cnt);
  int a0 = 0, a1 = 0;
  for (int t = t0; t < t1; t++)
  {
    const int lv = level[scan[cnt - 1 - t]];
    if (t & 1) a1 ^= lv; else a0 ^= lv;
  }
  const unsigned long long B0 = __builtin_amdgcn_ballot_w64((a0 & 1) != 0), B1 = __builtin_amdgcn_ballot_w64((a1 & 1) != 0);
  const unsigned long long below = (1ull << lane) - 1ull;
  int x0 = (int)__popcll(B0 & below) & 1, x1 = (int)__popcll(B1 & below) & 1;
  for (int t = t0; t < t1; t++)
  {
    const int pos = scan[cnt - 1 - t], lv = level[pos], hi = (t & 1) ? x0 : x1;
    int v = 0;
    if (lv != 0)
    {
      const int qIdx = 2 * lv + (lv > 0 ? -hi : hi);
      v = (int)min(max(((long long)qIdx * scale + add) >> shift, -(1ll << 15)), (1ll << 15) - 1);
    }
    coef[pos] = v;
    if (t & 1) x1 ^= lv & 1; else x0 ^= lv & 1;
  }
}

}  // namespace
