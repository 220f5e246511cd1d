// afm_dev.h -- device functions of the whole affine gradient search shared by vvcgpu_affine_me_batch (affine_me.hip), the affine bi-predictive
// search (affine_bipredme.hip) and the affine uni-predictive stage (affine_unipredme.hip): the 4x4 sub-block prediction into an LDS tile, the
// vector bits, xCheckBestAffineMVP, the Hadamard distortion, the solve, the search body, and the dynamic-LDS layout of an owner (afm_lds).  The owner
// model (split, barrier, sum, reference-index bits, getCost) is owner_dev.h's.  Reference behaviour: see affine_me.hip.  The original of a search is
// read through OrgPtr: a plain pointer (global memory) or AfiLdsPel (the bi-predictive search key, which lives in LDS) -- a template parameter, so no
// sample pays a run-time choice.
#pragma once
#include "common.h"
#include "dist_dev.h"
#include "afi_dev.h"
#include "raster_dev.h"
#include "owner_dev.h"

namespace {

__constant__ short kAfmLuma[16][8] = {                        // m_lumaFilter, 1/16 sample phases
  {  0, 0,   0, 64,  0,   0,  0,  0 }, {  0, 1,  -3, 63,  4,  -2,  1,  0 }, { -1, 2,  -5, 62,  8,  -3,  1,  0 }, { -1, 3,  -8, 60, 13,  -4,  1,  0 },
  { -1, 4, -10, 58, 17,  -5,  1,  0 }, { -1, 4, -11, 52, 26,  -8,  3, -1 }, { -1, 3,  -9, 47, 31, -10,  4, -1 }, { -1, 4, -11, 45, 34, -10,  4, -1 },
  { -1, 4, -11, 40, 40, -11,  4, -1 }, { -1, 4, -10, 34, 45, -11,  4, -1 }, { -1, 4, -10, 31, 47,  -9,  3, -1 }, { -1, 3,  -8, 26, 52, -11,  4, -1 },
  {  0, 1,  -5, 17, 58, -10,  4, -1 }, {  0, 1,  -4, 13, 60,  -8,  3, -1 }, {  0, 1,  -3,  8, 62,  -5,  2, -1 }, {  0, 1,  -2,  4, 63,  -3,  1,  0 } };

constexpr int AFM_TMP = 11 * 4;            // first-pass rows of one 4x4 sub-block (8 taps: 11 rows) x 4 columns

// (int)double as x86 cvttsd2si gives it: truncation; the "integer indefinite" 0x80000000 for NaN and for values outside int (v_cvt_i32_f64 saturates)
__device__ __forceinline__ int afm_cvtt(double d) { return (d >= -2147483648.0 && d < 2147483648.0) ? (int)d : (int)0x80000000u; }
// (int)(d * 4 + SIGN(d) * 0.5) << 2  (:3627-3632); the shift wraps 0x80000000 to 0
__device__ __forceinline__ int afm_delta(double d) { return (int)((unsigned)afm_cvtt(d * 4 + (d >= 0 ? 1 : -1) * 0.5) << 2); }

// solveEqual (:3102-3179) on rows 1..P of the reference's matrix (m[r - 1] = dEqualCoeff[r]; its row 0 is only the scratch of the line swap)
template <int P>
__device__ __forceinline__ void afm_solve(double (&m)[P][P + 1], double (&para)[P])
{
#pragma unroll
  for (int k = 0; k < P; k++) para[k] = 0.;
#pragma unroll
  for (int i = 1; i < P; i++)
  {
    double temp = fabs(m[i - 1][i - 1]);
    int idx = i;
#pragma unroll
    for (int j = i + 1; j < P + 1; j++)
    {
      const double a = fabs(m[j - 1][i - 1]);
      if (a > temp) { temp = a; idx = j; }
    }
#pragma unroll
    for (int j = i + 1; j < P + 1; j++)
      if (idx == j)
      {
#pragma unroll
        for (int c = 0; c < P + 1; c++) { const double t = m[i - 1][c]; m[i - 1][c] = m[j - 1][c]; m[j - 1][c] = t; }
      }
    if (m[i - 1][i - 1] == 0.) return;
#pragma unroll
    for (int j = i + 1; j < P + 1; j++)
#pragma unroll
      for (int k = i; k < P + 1; k++) m[j - 1][k] = m[j - 1][k] - m[i - 1][k] * m[j - 1][i - 1] / m[i - 1][i - 1];
  }
  if (m[P - 1][P - 1] == 0.) return;
  para[P - 1] = m[P - 1][P] / m[P - 1][P - 1];
#pragma unroll
  for (int i = P - 2; i >= 0; i--)
  {
    if (m[i][i] == 0.)
    {
#pragma unroll
      for (int k = 0; k < P; k++) para[k] = 0.;
      return;
    }
    double temp = 0;
#pragma unroll
    for (int j = i + 1; j < P; j++) temp += m[i][j] * para[j];
    para[i] = (m[i][P] - temp) / m[i][i];
  }
}

// the sums (int64 in LDS, 7 x 7 as vvcgpu_affine_equal_coeff_batch) -> double, solve, dDeltaMv (:3612-3625), quantised vector deltas
template <int P>
__device__ __forceinline__ void afm_deltas(const long long* eq, int w, int h, int (&delta)[3][2])
{
  double m[P][P + 1], para[P];
#pragma unroll
  for (int r = 0; r < P; r++)
#pragma unroll
    for (int c = 0; c < P + 1; c++) m[r][c] = (double)eq[(r + 1) * 7 + c];
  afm_solve<P>(m, para);
  double d[6];
  d[0] = para[0];
  d[2] = para[2];
  if constexpr (P == 6)
  {
    d[1] = para[1] * w + para[0];
    d[3] = para[3] * w + para[2];
    d[4] = para[4] * h + para[0];
    d[5] = para[5] * h + para[2];
  }
  else
  {
    d[1] = para[1] * w + para[0];
    d[3] = -para[3] * w + para[2];
    d[4] = d[5] = 0.;
  }
  delta[0][0] = afm_delta(d[0]); delta[0][1] = afm_delta(d[2]);
  delta[1][0] = afm_delta(d[1]); delta[1][1] = afm_delta(d[3]);
  delta[2][0] = P == 6 ? afm_delta(d[4]) : 0; delta[2][1] = P == 6 ? afm_delta(d[5]) : 0;
}

struct AfmPu
{
  const Pel* ref;                        // reference sample (pos_x, pos_y) of the picture
  int os, rs, w, h, six, nmv;            // os: the row stride of the original (the PU's block in org_base, or the key in LDS)
  int posX, posY;
  int horMin, horMax, verMin, verMax;    // clipMv, 1/16 units
  int bitDepth, clpMin, clpMax;
};

// geometry and clipMv bounds (a high-precision vector: shift 2 + 2) of a PU at (posX, posY)
__device__ __forceinline__ void afm_set_pu(AfmPu& u, int posX, int posY, int w, int h, bool six, int picW, int picH, int maxCuW, int maxCuH, int bitDepth,
                                           int clpMin, int clpMax)
{
  u.w = w; u.h = h; u.six = six; u.nmv = six ? 3 : 2;
  u.posX = posX; u.posY = posY;
  u.horMax = (picW + 8 - posX - 1) << 4; u.horMin = (-maxCuW - 8 - posX + 1) << 4;
  u.verMax = (picH + 8 - posY - 1) << 4; u.verMin = (-maxCuH - 8 - posY + 1) << 4;
  u.bitDepth = bitDepth; u.clpMin = clpMin; u.clpMax = clpMax;
}

// xPredAffineBlk (luma, uni): sixteen lanes per 4x4 sub-block; tmpW = this wavefront's first-pass rows (4 x AFM_TMP)
template <int NT>
__device__ __forceinline__ void afm_predict(const AfmPu& u, const int (&mv)[3][2], Pel* predL, short* tmpW, int tid)
{
  const int lane = tid & 63, li = lane & 15, r = li >> 2, cc = li & 3;
  short* tmp = tmpW + (lane >> 4) * AFM_TMP;
  const int w = u.w, h = u.h, nbx = w >> 2, nsb = nbx * (h >> 2);
  const int iBit = 7, shift = iBit - 4 + 2 + 2;                          // MAX_CU_DEPTH; InterPrediction.cpp:658
  const int lgW = ilog2(w), lgH = ilog2(h);
  const int ltx = mv[0][0], lty = mv[0][1];
  const int dHorX = (mv[1][0] - ltx) << (iBit - lgW), dHorY = (mv[1][1] - lty) << (iBit - lgW);
  int dVerX, dVerY;
  if (u.six) { dVerX = (mv[2][0] - ltx) << (iBit - lgH); dVerY = (mv[2][1] - lty) << (iBit - lgH); }
  else { dVerX = -dHorY; dVerY = dHorX; }
  const int headRoom = 14 - u.bitDepth;                                  // IF_INTERNAL_PREC - bit depth (8..10)
  const int sh1 = 6 - headRoom, off1 = -(8192 << sh1);                   // first of two passes
  const int sh2 = 6 + headRoom, off2 = (1 << (sh2 - 1)) + (8192 << 6);   // second of two passes
  const int rs = u.rs;
  for (int sb0 = 0; sb0 < nsb; sb0 += NT / 16)                           // the same trip count in every lane
  {
    const int sb = sb0 + (tid >> 4);
    const bool act = sb < nsb;
    int xFrac = 0, yFrac = 0, wq = 0, hq = 0;
    const Pel* win = u.ref;
    if (act)
    {
      const int byI = sb / nbx, bxI = sb - byI * nbx;
      wq = bxI << 2; hq = byI << 2;
      int mh = (ltx << iBit) + dHorX * (2 + wq) + dVerX * (2 + hq);
      int mvv = (lty << iBit) + dHorY * (2 + wq) + dVerY * (2 + hq);
      const int off = 1 << (shift - 1);                                  // roundAffineMv
      mh = mh >= 0 ? (mh + off) >> shift : -((-mh + off) >> shift);
      mvv = mvv >= 0 ? (mvv + off) >> shift : -((-mvv + off) >> shift);
      mh = min(u.horMax, max(u.horMin, mh));                            // :650-676: the bounds of clipMv for a 1/16 vector
      mvv = min(u.verMax, max(u.verMin, mvv));
      xFrac = mh & 15; yFrac = mvv & 15;
      win += (ptrdiff_t)(hq + (mvv >> 4)) * rs + wq + (mh >> 4);          // sample (0, 0) of the sub-block's reference block
    }
    const short* fx = kAfmLuma[xFrac];
    const short* fy = kAfmLuma[yFrac];
    const bool both = act && xFrac != 0 && yFrac != 0;
    if (both)
    {
#pragma unroll
      for (int s = 0; s < 3; s++)
      {
        const int ri = r + 4 * s;                                        // first-pass row: reference row ri - 3
        if (ri < 11)
        {
          const Pel* p = win + (ptrdiff_t)(ri - 3) * rs + cc - 3;
          int sum = 0;
#pragma unroll
          for (int k = 0; k < 8; k++) sum += (int)p[k] * fx[k];
          tmp[ri * 4 + cc] = (short)((sum + off1) >> sh1);
        }
      }
    }
    owner_sync<64>();
    if (act)
    {
      int v;
      if (yFrac == 0)
      {
        if (xFrac == 0) v = win[(ptrdiff_t)r * rs + cc];                  // filterCopy, first and last: no clip
        else
        {
          const Pel* p = win + (ptrdiff_t)r * rs + cc - 3;
          int sum = 0;
#pragma unroll
          for (int k = 0; k < 8; k++) sum += (int)p[k] * fx[k];
          v = clip3(u.clpMin, u.clpMax, (int)(short)((sum + 32) >> 6));
        }
      }
      else if (xFrac == 0)
      {
        const Pel* p = win + (ptrdiff_t)(r - 3) * rs + cc;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += (int)p[(ptrdiff_t)k * rs] * fy[k];
        v = clip3(u.clpMin, u.clpMax, (int)(short)((sum + 32) >> 6));
      }
      else
      {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += (int)tmp[(r + k) * 4 + cc] * fy[k];
        v = clip3(u.clpMin, u.clpMax, (int)(short)((sum + off2) >> sh2));
      }
      predL[(hq + r) * w + wq + cc] = (Pel)v;
    }
    owner_sync<64>();                                                   // the next round overwrites tmp
  }
}

// ruiBits + the bits of the control-point vectors against their predictors (:3386-3410, cost scale 0, imv shift 0)
__device__ __forceinline__ unsigned afm_bits(unsigned bits, const int (&mvp)[3][2], int nmv, const int (&mv)[3][2])
{
#pragma unroll
  for (int i = 0; i < 3; i++)
  {
    if (i >= nmv) break;
    int px = mvp[i][0], py = mvp[i][1];
    if (i != 0) { px += mv[0][0] - mvp[0][0]; py += mv[0][1] - mvp[0][1]; }
    bits += expgolomb_bits((mv[i][0] >> 2) - (px >> 2)) + expgolomb_bits((mv[i][1] >> 2) - (py >> 2));
  }
  return bits;
}

// xCheckBestAffineMVP (:3181-3284) with the candidate set `cand` of `numCand` candidates: the vector bits (second-predictor rule for vectors 1 and 2)
// against the current predictors and against the other candidate; on a switch the predictors, the index, the bits (uint32) and the cost (wrapping
// uint64) follow
__device__ __forceinline__ void afm_check_best_mvp(const int32_t (&cand)[2][3][2], int numCand, const uint32_t (&mvpIdxCost)[3], double lambda, int nmv,
                                                   const int (&mv)[3][2], int (&pred)[3][2], int& mvpIdx, unsigned& bits, unsigned long long& cost)
{
  if (numCand < 2) return;
  const int orgBits = (int)(afm_bits(0u, pred, nmv, mv) + mvpIdxCost[mvpIdx]);
  int bestBits = orgBits, bestIdx = mvpIdx;
  for (int i = 0; i < 2; i++)
  {
    if (i == mvpIdx) continue;
    int cd[3][2];
#pragma unroll
    for (int k = 0; k < 3; k++) { cd[k][0] = cand[i][k][0]; cd[k][1] = cand[i][k][1]; }
    const int b = (int)(afm_bits(0u, cd, nmv, mv) + mvpIdxCost[i]);
    if (b < bestBits) { bestBits = b; bestIdx = i; }
  }
  if (bestIdx != mvpIdx)
  {
#pragma unroll
    for (int k = 0; k < 3; k++) { pred[k][0] = cand[bestIdx][k][0]; pred[k][1] = cand[bestIdx][k][1]; }
    mvpIdx = bestIdx;
    const unsigned orgB = bits;
    bits = orgB - (unsigned)orgBits + (unsigned)bestBits;
    cost = (cost - rd_getcost(lambda, orgB)) + rd_getcost(lambda, bits);
  }
}

struct AfmLds
{
  Pel* predL;                 // the owner's prediction tile
  short* tmpW;                // this wavefront's first-pass rows
  long long* eq;              // the owner's 49 sums
  long long (*red)[64];       // NT = 256: the wavefronts' partial sums
  unsigned long long* distW;  // NT = 256: the wavefronts' distortions
};

// The header in front of an owner's tiles in dynamic LDS: eq | EXTRA bytes of the entry's own state (at AFM_OFF_STATE) | tmp | red | dist.  A wavefront
// owner's header ends behind its one tmp block (WAVE bytes); the workgroup owner's holds four of them, red and dist (GROUP bytes).
constexpr int AFM_OFF_STATE = 400;                       // behind the 49 equation sums
constexpr int AFM_TMP_BYTES = 4 * AFM_TMP * 2;           // one wavefront's first-pass rows
template <int EXTRA> struct AfmHdr
{
  static constexpr int TMP = AFM_OFF_STATE + EXTRA;
  static constexpr int WAVE = (TMP + AFM_TMP_BYTES + 15) & ~15;
  static constexpr int RED = TMP + 4 * AFM_TMP_BYTES;
  static constexpr int DIST = RED + 4 * 64 * 8;
  static constexpr int GROUP = (DIST + 4 * 8 + 15) & ~15;
  static_assert(EXTRA % 8 == 0 && RED % 8 == 0 && DIST % 8 == 0, "alignment");
  static int bytes(int nt, int tileBytes) { return (nt == 64 ? WAVE : GROUP) + tileBytes; }      // host: an owner's LDS with its tiles
};

template <int NT, int EXTRA>
__device__ __forceinline__ AfmLds afm_lds(unsigned char* base, int wave)
{
  typedef AfmHdr<EXTRA> H;
  AfmLds L;
  L.eq = reinterpret_cast<long long*>(base);
  L.tmpW = reinterpret_cast<short*>(base + H::TMP) + (NT == 256 ? wave * 4 * AFM_TMP : 0);
  L.red = reinterpret_cast<long long (*)[64]>(base + H::RED);                 // NT = 256 only
  L.distW = reinterpret_cast<unsigned long long*>(base + H::DIST);            // NT = 256 only
  L.predL = reinterpret_cast<Pel*>(base + (NT == 256 ? H::GROUP : H::WAVE));
  return L;
}

template <int NT, class OrgPtr>
__device__ __forceinline__ unsigned long long afm_dist(const AfmPu& u, OrgPtr org, const AfmLds& L, int tid)
{
  const int lane = tid & 63, wave = tid >> 6;
  vvcgpu_affine_iter d;
  d.org_stride = u.os;
  unsigned long long sum;
  if ((u.h & 15) == 0) sum = afi_dist<OrgPtr>(d, org, L.predL, u.w, u.h, 1, NT == 256 ? wave : 0, NT == 256 ? 4 : 1, lane);
  else sum = (NT == 64 || wave == 0) ? satd_block<64, AfiLdsPel, OrgPtr>(org, u.os, (AfiLdsPel)L.predL, u.w, u.w, u.h, lane) : 0ull;   // no bands of sixteen rows
  return owner_sum_waves<NT>(sum, L.distW, tid);                         // afi_dist and satd_block return a wavefront's sum in each of its lanes
}

// xAffineMotionEstimation from the vectors `start` against the predictors `mvp` with ruiBits = bits0 on entry: the start vectors are clipped,
// predicted and costed as step 0, then the gradient iterations to the reference's termination rule.  -> best (acMv), bestBits (ruiBits), bestCost
// (ruiCost), steps (predictions evaluated).  trace (may be null): the vectors and the cost of every evaluated prediction.  Uniform per owner.
template <int NT, class OrgPtr>
__device__ __forceinline__ void afm_search_body(const AfmPu& u, OrgPtr org, double lambda, bool halfWeight, int affineType, unsigned bits0,
                                                const int (&mvp)[3][2], const int (&start)[3][2], const AfmLds& L, vvcgpu_affine_me_step* trace, int tid,
                                                int (&best)[3][2], unsigned& bestBits, unsigned long long& bestCost, unsigned& steps)
{
  const double weight = halfWeight ? 0.5 : 1.0;
  int iterTime = u.six ? (halfWeight ? 3 : 4) : (halfWeight ? 3 : 5);
  if (!affineType) iterTime = halfWeight ? 5 : 7;

  int cur[3][2];
#pragma unroll
  for (int i = 0; i < 3; i++) { cur[i][0] = start[i][0]; cur[i][1] = start[i][1]; }
#pragma unroll
  for (int i = 0; i < 3; i++)
    if (i < u.nmv) { cur[i][0] = min(u.horMax, max(u.horMin, cur[i][0])); cur[i][1] = min(u.verMax, max(u.verMin, cur[i][1])); }

  afm_predict<NT>(u, cur, L.predL, L.tmpW, tid);
  owner_sync<NT>();
  unsigned long long had = afm_dist<NT, OrgPtr>(u, org, L, tid);
  bestBits = afm_bits(bits0, mvp, u.nmv, cur);
  bestCost = (unsigned long long)(floor(weight * (double)had) + (double)(unsigned long long)(lambda * bestBits));
#pragma unroll
  for (int i = 0; i < 3; i++) { best[i][0] = cur[i][0]; best[i][1] = cur[i][1]; }
  steps = 1;
  if (trace && tid == 0)
  {
#pragma unroll
    for (int i = 0; i < 3; i++) { trace[0].mv[i][0] = cur[i][0]; trace[0].mv[i][1] = cur[i][1]; }
    trace[0].cost = bestCost;
  }

  vvcgpu_affine_iter d;
  d.org_stride = u.os;
  for (int iter = 0; iter < iterTime; iter++)
  {
    if (u.six) afi_equations<6, NT, OrgPtr>(d, org, L.predL, u.w, u.h, L.eq, L.red, tid);
    else       afi_equations<4, NT, OrgPtr>(d, org, L.predL, u.w, u.h, L.eq, L.red, tid);
    owner_sync<NT>();
    int delta[3][2];
    if (u.six) afm_deltas<6>(L.eq, u.w, u.h, delta);
    else       afm_deltas<4>(L.eq, u.w, u.h, delta);
    bool allZero = true;
#pragma unroll
    for (int i = 0; i < 3; i++)
      if (i < u.nmv && (delta[i][0] != 0 || delta[i][1] != 0)) allZero = false;
    if (allZero) break;
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
      if (i >= u.nmv) break;
#pragma unroll
      for (int k = 0; k < 2; k++)
      {
        int v = (int)((unsigned)cur[i][k] + (unsigned)delta[i][k]);
        v = clip3(-32768, 32767, v);
        v = (v >= 0 ? (v + 2) >> 2 : -((-v + 2) >> 2)) * 4;               // roundMV2SignalPrecision: to quarter sample and back
        cur[i][k] = k == 0 ? min(u.horMax, max(u.horMin, v)) : min(u.verMax, max(u.verMin, v));
      }
    }
    owner_sync<NT>();                                                    // every lane has read eq and the tile before they are overwritten
    afm_predict<NT>(u, cur, L.predL, L.tmpW, tid);
    owner_sync<NT>();
    had = afm_dist<NT, OrgPtr>(u, org, L, tid);
    const unsigned bits = afm_bits(bits0, mvp, u.nmv, cur);
    const unsigned long long cost = (unsigned long long)(floor(weight * (double)had) + (double)(unsigned long long)(lambda * bits));
    if (trace && tid == 0)
    {
#pragma unroll
      for (int i = 0; i < 3; i++) { trace[steps].mv[i][0] = cur[i][0]; trace[steps].mv[i][1] = cur[i][1]; }
      trace[steps].cost = cost;
    }
    steps++;
    if (cost < bestCost)
    {
      bestCost = cost; bestBits = bits;
#pragma unroll
      for (int i = 0; i < 3; i++) { best[i][0] = cur[i][0]; best[i][1] = cur[i][1]; }
    }
  }
}

}  // namespace
