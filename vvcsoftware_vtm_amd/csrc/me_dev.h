// me_dev.h -- pieces of the translational inter search that the whole-PU entries share (bipredme.hip, unipredme.hip): the vector bits, the luma uni
// prediction of a PU handed to the caller sample by sample, and xCheckBestMVP.  The owner model (split, barrier, sum, reference-index bits, getCost)
// is owner_dev.h's; the owner's LDS header and work area are frac_dev.h's.
//
// Reference behaviour reproduced (bit-exact): motionCompensation -> xPredInterUni -> xPredInterBlk (CommonLib/InterPrediction.cpp:480-547) with
// InterpolationFilter::filter / filterCopy (InterpolationFilter.cpp:205-379), clipMv (Mv.cpp:64-80), RdCost::getBitsOfVectorWithPredictor / getCost
// (RdCost.h:172-199), InterSearch::xCheckBestMVP (EncoderLib/InterSearch.cpp:1537-1603).
#pragma once
#include "common.h"
#include "frac_dev.h"
#include "owner_dev.h"

namespace {

struct MePu
{
  const Pel* org; int os;
  int w, h, lgW, posX, posY, subShift;
  int horMin, horMax, verMin, verMax;          // clipMv, quarter units
};

__device__ __forceinline__ unsigned me_mvbits(int predH, int predV, int scale, int x, int y) { return eg_bits((x << scale) - predH) + eg_bits((y << scale) - predV); }

// motionCompensation (luma, uni, rounded and clipped) of the quarter-unit vector (mvX, mvY), clipMv applied, against `ref` (sample (0, 0) of the
// picture, pitch rs): emit(i, y, x, v) receives sample i = y * w + x of the prediction, each exactly once, from the lane that computed it.
// tmp: w x (h + 7) shorts of LDS.  Ends with the owner's barrier.
template <int NT, class Emit>
__device__ __forceinline__ void me_pred_uni(const MePu& u, const Pel* __restrict__ ref, int rs, int bitDepth, int clpMin, int clpMax, int mvX, int mvY, short* tmp,
                                            int tid, Emit emit)
{
  mvX = min(u.horMax, max(u.horMin, mvX));
  mvY = min(u.verMax, max(u.verMin, mvY));
  const int xFrac = (mvX & 3) << 2, yFrac = (mvY & 3) << 2, w = u.w, h = u.h;
  const Pel* blk = ref + (ptrdiff_t)(u.posY + (mvY >> 2)) * rs + u.posX + (mvX >> 2);
  const short* fx = c_lumaF[xFrac];
  const short* fy = c_lumaF[yFrac];
  const int headRoom = 14 - bitDepth;                                    // IF_INTERNAL_PREC - bit depth (8..10)
  const int sh1 = 6 - headRoom, off1 = -(OFFS << sh1);                   // first of two passes
  const int sh2 = 6 + headRoom, off2 = (1 << (sh2 - 1)) + (OFFS << 6);   // second of two passes
  const bool both = xFrac != 0 && yFrac != 0;
  if (both)
  {
    for (int i = tid; i < w * (h + 7); i += NT)
    {
      const int r = i >> u.lgW, x = i & (w - 1);
      const Pel* p = blk + (ptrdiff_t)(r - 3) * rs + x - 3;
      int sum = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) sum += (int)p[k] * fx[k];
      tmp[i] = (short)((sum + off1) >> sh1);
    }
  }
  owner_sync<NT>();
  for (int i = tid; i < w * h; i += NT)
  {
    const int y = i >> u.lgW, x = i & (w - 1);
    int v;
    if (both)
    {
      int sum = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) sum += (int)tmp[i + k * w] * fy[k];
      v = clip3(clpMin, clpMax, (int)(short)((sum + off2) >> sh2));
    }
    else if (yFrac != 0)
    {
      const Pel* p = blk + (ptrdiff_t)(y - 3) * rs + x;
      int sum = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) sum += (int)p[(ptrdiff_t)k * rs] * fy[k];
      v = clip3(clpMin, clpMax, (int)(short)((sum + 32) >> 6));
    }
    else if (xFrac != 0)
    {
      const Pel* p = blk + (ptrdiff_t)y * rs + x - 3;
      int sum = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) sum += (int)p[k] * fx[k];
      v = clip3(clpMin, clpMax, (int)(short)((sum + 32) >> 6));
    }
    else v = blk[(ptrdiff_t)y * rs + x];                                 // filterCopy, first and last: no clip
    emit(i, y, x, v);
  }
  owner_sync<NT>();
}

// xCheckBestMVP (:1537-1603) over the candidates cand[0 .. numCand); the reference's CHECK (cand[mvpIdx] == pred) is the caller's contract
__device__ __forceinline__ void me_check_best_mvp(const int32_t (*cand)[2], int numCand, const uint32_t* mvpIdxCost, double lambda, int mvX, int mvY, int& predX,
                                                  int& predY, int& mvpIdx, unsigned& bits, unsigned long long& cost)
{
  if (numCand < 2) return;
  const int orgBits = (int)(me_mvbits(predX, predY, 0, mvX, mvY) + mvpIdxCost[mvpIdx]);
  int bestBits = orgBits, bestIdx = mvpIdx;
  for (int i = 0; i < 2; i++)
  {
    if (i == mvpIdx) continue;
    const int b = (int)(me_mvbits(cand[i][0], cand[i][1], 0, mvX, mvY) + mvpIdxCost[i]);
    if (b < bestBits) { bestBits = b; bestIdx = i; }
  }
  if (bestIdx != mvpIdx)
  {
    predX = cand[bestIdx][0]; predY = cand[bestIdx][1];
    mvpIdx = bestIdx;
    const unsigned orgB = bits;
    bits = orgB - (unsigned)orgBits + (unsigned)bestBits;
    cost = (cost - pu_getcost(lambda, orgB)) + pu_getcost(lambda, bits);
  }
}

}  // namespace
