// me_dev.h -- pieces of the translational inter search that the whole-PU entries share (bipredme.hip, unipredme.hip): the vector bits, the luma uni
// prediction of a PU handed to the caller sample by sample, xCheckBestMVP, and the integer refinement of the AMVR passes (xPatternSearchIntRefine).
// The owner model (split, barrier, sum, reference-index bits, getCost) is owner_dev.h's; the owner's LDS header and work area are frac_dev.h's.
//
// Reference behaviour reproduced (bit-exact): motionCompensation -> xPredInterUni -> xPredInterBlk (CommonLib/InterPrediction.cpp:480-547) with
// InterpolationFilter::filter / filterCopy (InterpolationFilter.cpp:205-379), clipMv (Mv.cpp:64-80), RdCost::getBitsOfVectorWithPredictor / getCost
// (RdCost.h:172-199), InterSearch::xCheckBestMVP (EncoderLib/InterSearch.cpp:1537-1603), InterSearch::xPatternSearchIntRefine (:2408-2500) with
// roundMV (Mv.cpp:44-52) and xGetHADs / SAD (dist_dev.h).
#pragma once
#include "common.h"
#include "dist_dev.h"
#include "frac_dev.h"
#include "owner_dev.h"

namespace {

struct MePu
{
  const Pel* org; int os;
  int w, h, lgW, posX, posY, subShift;
  int horMin, horMax, verMin, verMax;          // clipMv, quarter units
};

__device__ __forceinline__ unsigned me_mvbits(int predH, int predV, int scale, int x, int y) { return expgolomb_bits((x << scale) - predH) + expgolomb_bits((y << scale) - predV); }
// getBitsOfVectorWithPredictor(x, y, imvShift) (RdCost.h:189)
__device__ __forceinline__ unsigned me_mvbits_imv(int predH, int predV, int scale, int sh, int x, int y)
{
  return expgolomb_bits(((x << scale) - predH) >> sh) + expgolomb_bits(((y << scale) - predV) >> sh);
}

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
    cost = (cost - rd_getcost(lambda, orgB)) + rd_getcost(lambda, bits);
  }
}

// xPatternSearchIntRefine (:2408-2500) of the AMVR passes (cu.imv != 0, sh = imvShift = imv << 1) by the owner's NT lanes, around the integer vector
// (ix, iy) of the search.  key: the w x h search key in the owner's LDS (the original, or 2 org - otherPred); ref: sample (0, 0) of the picture, pitch
// rs; weight: fWeight, 1.0 (uni) or 0.5 (bi).  The nine positions (the centre, then the order of :2432) x numCand candidates give up to 18 full-block
// distortions (SATD when useHad, else SAD; no row sub-sampling) of the block at clipMv(test) >> 2, an integer position read straight from global
// memory: the two candidates' position sets differ by up to 1 << sh quarter units and clipMv moves positions anywhere, so no window serves them.  The
// second candidate's set either equals the first's at every position or at none (the difference does not depend on the position): 9 or 18
// distortions, dealt to the owner's wavefronts, one whole block each, into dl (18 x 8 bytes of the work area); every lane then folds them in the
// reference's visiting order, strict '<'.  In: mvpIdx, (predX, predY) = cand[mvpIdx] (the reference's CHECK at :2411 is the caller's contract), bits
// with the predictor-index bits of mvpIdx in them.  Out: the refined vector, the predictor it is coded against, bits and cost as :2485-2497 leave them
// (the vector bits are in `bits` twice, as in the reference).  Candidate 1 is not read when numCand == 1.  Ends with the owner's barrier.
template <int NT>
__device__ __forceinline__ void me_imv_refine(const MePu& u, const short* key, const Pel* __restrict__ ref, int rs, int useHad, double weight, double lambda, int sh,
                                              const int32_t (*cand)[2], int numCand, const uint32_t* mvpIdxCost, unsigned long long* dl, int ix, int iy, int& mvX,
                                              int& mvY, int& predX, int& predY, int& mvpIdx, unsigned& bits, unsigned long long& cost, int tid)
{
  typedef const __attribute__((address_space(3))) short* LdsPel;
  constexpr int TEAM = NT >> 6;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), w = u.w, h = u.h;
  const int mvx = ix << 2, mvy = iy << 2, off = 1 << (sh - 1), step = 1 << sh;
  const int c0x = cand[0][0], c0y = cand[0][1], c1x = numCand > 1 ? cand[1][0] : c0x, c1y = numCand > 1 ? cand[1][1] : c0y;
  // cTestMv of the centre: roundMV(rcMv - mvCand[i], imvShift) + mvCand[i]
  const int b0x = ((((mvx - c0x) + off) >> sh) << sh) + c0x, b0y = ((((mvy - c0y) + off) >> sh) << sh) + c0y;
  const int b1x = ((((mvx - c1x) + off) >> sh) << sh) + c1x, b1y = ((((mvy - c1y) + off) >> sh) << sh) + c1y;
  const bool same = numCand < 2 || (b0x == b1x && b0y == b1y);
  const int nEval = same ? 9 : 18;
  for (int e = wave; e < nEval; e += TEAM)
  {
    const int pos = same ? e : e >> 1, i = same ? 0 : e & 1;
    const int q = pos == 0 ? 4 : (pos <= 4 ? pos - 1 : pos), dx = q / 3 - 1, dy = q % 3 - 1;      // testPos: the 3 x 3 grid, x-major, centre first
    const int tx = min(u.horMax, max(u.horMin, dx * step + (i ? b1x : b0x))), ty = min(u.verMax, max(u.verMin, dy * step + (i ? b1y : b0y)));
    const Pel* cur = ref + (ptrdiff_t)(u.posY + (ty >> 2)) * rs + u.posX + (tx >> 2);
    unsigned long long d;
    if (useHad) d = satd_block<64, const Pel*, LdsPel>((LdsPel)key, w, cur, rs, w, h, lane);
    else
    {
      unsigned acc = 0;
      for (int k = lane; k < w * h; k += 64) acc += (unsigned)abs((int)key[k] - (int)cur[(ptrdiff_t)(k >> u.lgW) * rs + (k & (w - 1))]);
      d = wave_sum(acc);
    }
    if (lane == 0) dl[e] = d;
  }
  owner_sync<NT>();
  unsigned long long bestDist = ~0ull;
  int bestX = mvx, bestY = mvy, bestIdx = mvpIdx, bestBits = 0;
  for (int pos = 0; pos < 9; pos++)
  {
    const int q = pos == 0 ? 4 : (pos <= 4 ? pos - 1 : pos), dx = q / 3 - 1, dy = q % 3 - 1;
    for (int i = 0; i < 2; i++)
    {
      if (i >= numCand) break;
      const int tx = dx * step + (i ? b1x : b0x), ty = dy * step + (i ? b1y : b0y);
      unsigned long long dist = (unsigned long long)((double)dl[same ? pos : 2 * pos + i] * weight);      // :2456; candidate 1 at candidate 0's position takes its distortion
      const unsigned vb = expgolomb_bits((tx - (i ? c1x : c0x)) >> sh) + expgolomb_bits((ty - (i ? c1y : c0y)) >> sh);
      dist += rd_getcost(lambda, vb);
      if (dist < bestDist) { bestDist = dist; bestX = tx; bestY = ty; bestIdx = i; bestBits = (int)(mvpIdxCost[i] + vb); }
    }
  }
  bits -= mvpIdxCost[mvpIdx];
  bits += (unsigned)bestBits;
  cost = bestDist - rd_getcost(lambda, (unsigned)bestBits) + rd_getcost(lambda, bits);
  mvX = bestX; mvY = bestY; mvpIdx = bestIdx; predX = bestIdx ? c1x : c0x; predY = bestIdx ? c1y : c0y;
  bits += expgolomb_bits((bestX - predX) >> sh) + expgolomb_bits((bestY - predY) >> sh);                                 // :2496: the vector bits a second time
  owner_sync<NT>();                                                                                          // dl lies in the work area, which is written again
}

}  // namespace
