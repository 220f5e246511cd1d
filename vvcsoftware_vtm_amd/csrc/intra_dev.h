// intra_dev.h -- device functions of the intra sample predictors shared by intra.hip, intracand.hip, intratu.hip and intrachroma.hip: the reference-length
// arithmetic, the luma filter rule, the staging of the packed reference samples, predIntraAng of one block by a group of lanes (sides 2..64: chroma's
// 2-sample sides run the same code), the reference sample gathering, and the cross-component linear model (luma down-sampling, parameters).
// Reference behaviour: IntraPrediction::predIntraAng CommonLib/IntraPrediction.cpp:251-347, setReferenceArrayLengths :233-249,
// xFilterReferenceSamples :1071-1104, xFillReferenceSamples :807-1004, xGetLumaRecPixels :1283-1581, xGetLMParameters :1597-1857 (see intra.hip).
#pragma once
#include "common.h"

namespace {

__constant__ short kAng[27]    = { 0, 1, 2, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 26, 29, 32, 35, 39, 45, 49, 54, 60, 68, 79, 93, 114 };
__constant__ short kInvAng[27] = { 0, 8192, 4096, 2731, 1638, 1170, 910, 745, 630, 546, 482, 431, 390, 356, 315, 282, 256, 234, 210, 182, 167, 152, 137, 120,
                                   104, 88, 72 };
enum { PLANAR = 0, DC = 1, HOR = 18, DIA = 34, VER = 50, VDIA = 66 };

constexpr int REF_MAX = 160;            // >= longest side reference + 2 (2 * 64 + 22 + 1)
constexpr int NEG_MAX = 64;             // projected samples left of the main reference

// m_topRefLength / m_leftRefLength of setReferenceArrayLengths :233-249
__device__ __forceinline__ void intra_ref_lengths(int w, int h, int& T, int& L)
{
  T = w << 1; L = h << 1;
  const int ratio = min(2, abs(ilog2(w) - ilog2(h)));
  if (w > h) L += (w >> ratio) - h + ((w + 31) >> 5);
  else if (h > w) T += (h >> ratio) - w + ((h + 31) >> 5);
}

// useFilteredIntraRefSamples(COMPONENT_Y, pu, modeSpecific = true, pu) :1107-1139 (HM_MDIS_AS_IN_JEM = 1, JVET_K0063_PDPC_SIMP, JVET_K0500_WAIP)
__device__ __forceinline__ bool intra_use_filtered(int w, int h, int mode, int noSmoothing)
{
  if (noSmoothing) return false;
  const int log2W = ilog2(w), log2H = ilog2(h);
  if (mode > DC)                                                          // a mode that getWideAngle moves leaves 2..66
  {
    const int modeShift = (min(2, abs(log2W - log2H)) << 2) + 2;
    if ((w > h && mode < 2 + modeShift) || (h > w && mode > VDIA - modeShift)) return true;
  }
  if (mode == DC) return false;
  if (mode == PLANAR) return w * h > 32;
  const int diff = min(abs(mode - HOR), abs(mode - VER));
  const int log2Size = (log2W + log2H) >> 1;                             // m_aucIntraFilter[CHANNEL_TYPE_LUMA]: 20, 14, 2, 0, 20 for 4, 8, 16, 32, 64
  const int thr = log2Size == 2 ? 20 : log2Size == 3 ? 14 : log2Size == 4 ? 2 : log2Size == 5 ? 0 : 20;
  return diff > thr;
}

// The packed references of a block (refs[0] = top-left, refs[1 .. T] above, refs[T + 1 .. T + L] left) into the wave's top / left arrays
// (top[0] = top-left, top[1 + x]; left[0] = top-left, left[1 + y]), through the regular reference sample filter if `filter`; tmpBuf: 2 REF_MAX shorts.
__device__ __forceinline__ void intra_stage_refs(const Pel* refs, bool filter, int T, int L, int lane, short* top, short* left, short* tmpBuf)
{
  if (!filter)
  {
    for (int i = lane; i <= T; i += 64) top[i] = refs[i];
    for (int i = lane; i <= L; i += 64) left[i] = i == 0 ? refs[0] : refs[T + i];
  }
  else
  {
    // regular reference sample filter along the chain  left[L] .. left[1], top-left, top[1] .. top[T]; the two ends stay
    short* c = tmpBuf;                                      // chain position L + i for top[i], L - i for left[i]
    for (int i = lane; i <= T + L; i += 64) c[i] = i <= L ? (i == L ? refs[0] : refs[T + (L - i)]) : refs[i - L];
    wave_sync();
    for (int i = lane; i <= T + L; i += 64)
    {
      const int v = (i == 0 || i == T + L) ? c[i] : (c[i - 1] + 2 * c[i] + c[i + 1] + 2) >> 2;
      if (i <= L) left[L - i] = (short)v;
      if (i >= L) top[i - L] = (short)v;
    }
  }
  wave_sync();
}

// predIntraAng of one w x h block from staged references by a group of G lanes (G = 64: the wave; G = 32, 16: two or four blocks of at most G samples
// side by side in a wave, each with its own mode, dst and mainX; the references may be shared) into `dst` (row pitch ds; global memory or LDS).
// lane: index inside the group.  mainX: room for the main reference with its projected extension, -H < index <= side + 1 (H, side: the block's sides
// across and along the main reference).  Rows [y0, y1) only (default: the whole block); dst addresses row y0.
template <int G>
__device__ __forceinline__ void intra_pred_samples(int w, int h, int mode, int T, int L, const short* top, const short* left, short* mainX, Pel* dst, int ds,
                                                   int clpMin, int clpMax, int lane, int y0 = 0, int y1 = 1 << 30)
{
  const int log2W = ilog2(w), log2H = ilog2(h);
  const int count = w * h;
  const int scale = (log2W - 2 + log2H - 2 + 2) >> 2;
  const int topLeft = top[0];

  if (mode == PLANAR || mode == DC)
  {
    int dc = 0;
    if (mode == DC)                                         // :173-211
    {
      int sum = 0;
      if (w >= h) for (int i = lane; i < w; i += G) sum += top[1 + i];
      if (w <= h) for (int i = lane; i < h; i += G) sum += left[1 + i];
#pragma unroll
      for (int m = 1; m < G; m <<= 1) sum += __shfl_xor(sum, m);
      const int denom = (w == h) ? (w << 1) : max(w, h);
      dc = (short)((sum + (denom >> 1)) >> ilog2(denom));
    }
    const int bottomLeft = left[h + 1], topRight = top[w + 1];
    for (int i = y0 * w + lane; i < min(y1, h) * w; i += G)
    {
      const int y = i >> log2W, x = i & (w - 1);
      const int l = left[y + 1], t = top[x + 1];
      const int wT = 32 >> min(31, (y << 1) >> scale), wL = 32 >> min(31, (x << 1) >> scale);
      int v;
      if (mode == PLANAR)                                   // :424-477 + PDPC :293-307
      {
        const int horPred = (l << log2W) + (x + 1) * (topRight - l), vertPred = (t << log2H) + (y + 1) * (bottomLeft - t);
        const int p = (short)(((horPred << log2H) + (vertPred << log2W) + count) >> (1 + log2W + log2H));
        v = (wL * l + wT * t + (64 - wL - wT) * p + 32) >> 6;
      }
      else                                                  // PDPC :308-323
      {
        const int wTL = (wL >> 4) + (wT >> 4);
        v = (wL * l + wT * t - wTL * topLeft + (64 - wL - wT + wTL) * dc + 32) >> 6;
      }
      dst[(ptrdiff_t)(y - y0) * ds + x] = (Pel)min(max(v, clpMin), clpMax);
    }
    return;
  }

  // angular :545-773
  int predMode = mode;                                      // getWideAngle :213-231
  {
    const int modeShift = (min(2, abs(log2W - log2H)) << 2) + 2;
    if (w > h && predMode < 2 + modeShift) predMode += VDIA - 1;
    else if (h > w && predMode > VDIA - modeShift) predMode -= VDIA - 1;
  }
  const bool isVer = predMode >= DIA;
  const int angMode = isVer ? predMode - VER : -(predMode - HOR);
  const int absAngMode = abs(angMode);
  const int invAngle = kInvAng[absAngMode], angle = (angMode < 0 ? -1 : 1) * (int)kAng[absAngMode];
  const short* mainR = isVer ? top : left;                  // index 0 = top-left
  const short* sideR = isVer ? left : top;
  const int H = isVer ? h : w, log2Wm = isVer ? log2W : log2H;   // block in the orientation of the main reference
  const int sideLen = isVer ? L : T;
  if (angle < 0)                                            // main reference with the projected extension to the left (:588-609)
  {
    const int mainLen = (isVer ? w : h) + 1;
    for (int i = lane; i <= mainLen; i += G) mainX[i] = mainR[i];
    const int lowest = (H * angle) >> 5;                    // k runs -1 ... > lowest
    for (int k = -1 - lane; k > lowest; k -= G) mainX[k] = sideR[(128 + (-k) * invAngle) >> 8];
    wave_sync();
    mainR = mainX;
  }
  const bool pdpcCorner = predMode == 2 || predMode == VDIA;
  const bool pdpcNear = !pdpcCorner && ((predMode >= VDIA - 8) || (predMode <= 2 + 8));
  const bool pdpcHV = angle == 0;                           // HOR / VER: PDPC of predIntraAng :324-346
  for (int i = y0 * w + lane; i < min(y1, h) * w; i += G)
  {
    const int dy = i >> log2W, dx = i & (w - 1);
    const int x = isVer ? dx : dy, y = isVer ? dy : dx;     // coordinates in the orientation of the main reference
    const int deltaPos = (y + 1) * angle, deltaInt = deltaPos >> 5, deltaFract = deltaPos & 31;
    int v;
    if (deltaFract) v = (short)(((32 - deltaFract) * mainR[x + deltaInt + 1] + deltaFract * mainR[x + deltaInt + 2] + 16) >> 5);
    else v = mainR[x + deltaInt + 1];
    if (pdpcHV)
    {
      // in destination coordinates: HOR uses the row above, VER the column to the left
      if (mode == HOR) { const int wT = 32 >> min(31, (dy << 1) >> scale); v = (wT * top[dx + 1] - wT * topLeft + 64 * v + 32) >> 6; }
      else             { const int wL = 32 >> min(31, (dx << 1) >> scale); v = (wL * left[dy + 1] - wL * topLeft + 64 * v + 32) >> 6; }
      v = min(max(v, clpMin), clpMax);
    }
    else if (pdpcCorner)                                    // :697-711
    {
      const int wT = 16 >> min(31, (y << 1) >> scale), wL = 16 >> min(31, (x << 1) >> scale);
      if (wT + wL != 0)
      {
        const int c = x + y + 1;
        const int l = wL != 0 ? sideR[c + 1] : 0, t = wT != 0 ? mainR[c + 1] : 0;
        v = min(max((wL * l + wT * t + (64 - wL - wT) * v + 32) >> 6, clpMin), clpMax);
      }
    }
    else if (pdpcNear)                                      // :717-743
    {
      const int deltaPos0 = (2 + (x + 1) * invAngle) >> 2, deltaFrac0 = deltaPos0 & 63, deltay = y + (deltaPos0 >> 6) + 1;
      const int wL = 32 >> min(31, (x << 1) >> scale);
      if (deltay <= sideLen - 1 && wL != 0)
      {
        const int l = (short)(((64 - deltaFrac0) * sideR[deltay] + deltaFrac0 * sideR[deltay + 1] + 32) >> 6);
        v = min(max((wL * l + (64 - wL) * v + 32) >> 6, clpMin), clpMax);
      }
    }
    (void)log2Wm;
    dst[(ptrdiff_t)(dy - y0) * ds + dx] = (Pel)v;
  }
}

// One prediction block by one wave: predIntraAng into `dst` (row pitch ds; global memory or the wave's LDS tile).  top / left / tmp / mainBuf:
// the wave's LDS work arrays (REF_MAX, REF_MAX, 2 REF_MAX, NEG_MAX + REF_MAX shorts).
// Rows [y0, y1) only (default: the whole block); dst addresses row y0.
__device__ __forceinline__ void intra_pred_block(const vvcgpu_intra_desc& d, const Pel* __restrict__ refsBase, Pel* dst, int ds, int clpMin, int clpMax, int lane,
                                                 short* top, short* left, short* tmpBuf, short* mainBuf, int y0 = 0, int y1 = 1 << 30)
{
  int T, L;
  intra_ref_lengths(d.w, d.h, T, L);
  intra_stage_refs(refsBase + d.ref_off, d.filter_refs != 0, T, L, lane, top, left, tmpBuf);
  intra_pred_samples<64>(d.w, d.h, d.mode, T, L, top, left, mainBuf + NEG_MAX, dst, ds, clpMin, clpMax, lane, y0, y1);
}

// xFillReferenceSamples :807-1004 of one block by one wave into refs[0 .. T + L] (global memory or LDS); su: 192 shorts of the wave's LDS, enough for
// the block's ceil(T / unit_w) + ceil(L / unit_h) + 1 units.
// The reference pads through a line buffer (an unavailable unit repeats the last sample of the unit before it, a leading unavailable run repeats the
// first sample of the first available unit); in closed form every sample of an unavailable unit is one fixed sample of the nearest available unit, so
// each lane resolves its output samples independently.
constexpr int FILL_UNITS_MAX = 192;
__device__ __forceinline__ void intra_fill_refs_block(const Pel* __restrict__ recBase, const unsigned char* __restrict__ flagsBase,
                                                      const vvcgpu_intra_fill_desc& d, int bitDepth, int lane, short* su, Pel* refs)
{
  const int w = d.w, h = d.h, uw = d.unit_w, uh = d.unit_h, rs = d.rec_stride;
  int T, L;
  intra_ref_lengths(w, h, T, L);
  const int aboveUnits = (T + uw - 1) / uw, leftUnits = (L + uh - 1) / uh, total = aboveUnits + leftUnits + 1;
  const unsigned char* flags = flagsBase + d.flags_off;
  int firstLocal = 0x7fff;
  for (int u = lane; u < total; u += 64)
  {
    int p = u;
    while (p >= 0 && !flags[p]) p--;
    su[u] = (short)p;                                     // nearest available unit at or before u, -1 if none
    if (flags[u]) firstLocal = min(firstLocal, u);
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) firstLocal = min(firstLocal, __shfl_xor(firstLocal, m));
  wave_sync();
  const int first = firstLocal;                           // 0x7fff: nothing available
  const Pel* rec = recBase + d.rec_off;
  const int dc = 1 << (bitDepth - 1);
  for (int i = lane; i <= T + L; i += 64)
  {
    int u, o;
    if (i <= T) { const int q = uw - 1 + i; u = leftUnits + q / uw; o = q % uw; }
    else { const int k = leftUnits * uh - (i - T); u = k / uh; o = k % uh; }
    int v = dc;
    if (first != 0x7fff)
    {
      int s = su[u];
      if (s != u) { if (s >= 0) o = (s < leftUnits ? uh : uw) - 1; else { s = first; o = 0; } }
      if (s < leftUnits) v = rec[(ptrdiff_t)((leftUnits - s) * uh - 1 - o) * rs - 1];
      else if (s == leftUnits) v = rec[-rs - 1];
      else v = rec[-rs + (s - leftUnits - 1) * uw + o];
    }
    refs[i] = (Pel)v;
  }
}

// ---- CCLM (JVET_K0190): xGetLumaRecPixels :1283-1581 + xGetLMParameters :1597-1857 -------------------------------------------------------------------
__device__ __forceinline__ int floor_log2(unsigned x) { return 31 - __clz((int)x); }     // x > 0

// one down-sampled luma sample at p (the co-located luma position of a chroma sample; rs: luma stride): [1 2 1; 1 2 1] / 8, or the two-sample form of
// the first column when the left neighbour is not available (:1381-1395, :1455-1469, :1505-1560)
__device__ __forceinline__ int cclm_down(const Pel* p, int rs, bool two)
{
  return two ? (p[0] + p[rs] + 1) >> 1 : (p[0] * 2 + p[-1] + p[1] + p[rs] * 2 + p[rs - 1] + p[rs + 1] + 4) >> 3;
}

// xGetLMParameters of one w x h chroma block by one wave: lumaAbove(idx) / lumaLeft(idx) return the down-sampled luma neighbour above column idx / left
// of row idx, nbAbove / nbLeft hold the reconstructed chroma neighbours of the component.  -> a, bb, shift of the model (a * s >> shift) + bb.
template <class LA, class LL>
__device__ __forceinline__ void cclm_params(int w, int h, bool aboveAvail, bool leftAvail, LA lumaAbove, LL lumaLeft, const Pel* nbAbove, const Pel* nbLeft,
                                            int bdLuma, int bdChroma, int lane, int& a, int& bb, int& shift)
{
  a = 0; bb = 1 << (bdChroma - 1); shift = 0;
  if (aboveAvail || leftAvail)
  {
    int x = 0, y = 0, xx = 0, xy = 0, countShift = 0;
    const int minDim = (leftAvail && aboveAvail) ? min(w, h) : (leftAvail ? h : w);
    const int lgMin = floor_log2((unsigned)minDim);
    if (aboveAvail)
    {
      for (int j = lane; j < minDim; j += 64)
      {
        const int idx = (j * w) >> lgMin;
        const int s = lumaAbove(idx), c = nbAbove[idx];
        x += s; y += c; xx += s * s; xy += s * c;
      }
      countShift = lgMin;
    }
    if (leftAvail)
    {
      for (int i = lane; i < minDim; i += 64)
      {
        const int idx = (i * h) >> lgMin;
        const int s = lumaLeft(idx), c = nbLeft[idx];
        x += s; y += c; xx += s * s; xy += s * c;
      }
      countShift += aboveAvail ? 1 : lgMin;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { x += __shfl_xor(x, m); y += __shfl_xor(y, m); xx += __shfl_xor(xx, m); xy += __shfl_xor(xy, m); }
    const int tempShift = bdChroma + countShift - 15;
    if (tempShift > 0)
    {
      const int r = 1 << (tempShift - 1);
      x = (x + r) >> tempShift; y = (y + r) >> tempShift; xx = (xx + r) >> tempShift; xy = (xy + r) >> tempShift;
      countShift -= tempShift;
    }
    const int avgX = x >> countShift, avgY = y >> countShift;
    const int rErrX = x & ((1 << countShift) - 1), rErrY = y & ((1 << countShift) - 1);
    const int iB = 7;
    shift = 13 - iB;
    if (countShift == 0) { a = 0; bb = 1 << (bdChroma - 1); shift = 0; }
    else
    {
      const int a1 = xy - ((avgX * avgY) << countShift) - avgX * rErrY - avgY * rErrX;
      const int a2 = xx - ((avgX * avgX) << countShift) - 2 * avgX * rErrX;
      int sA1 = a1 == 0 ? 0 : floor_log2((unsigned)abs(a1)) - (bdChroma - 2);
      int sA2 = a2 == 0 ? 0 : floor_log2((unsigned)abs(a2)) - 5;
      sA1 = max(sA1, 0); sA2 = max(sA2, 0);
      const int sA = sA2 + (bdChroma + 4) - shift - sA1;
      const int a2s = a2 >> sA2, a1s = a1 >> sA1;
      if (a2s >= 32) a = (int)((unsigned)a1s * (unsigned)(((1 << (bdLuma + 4)) + a2s / 2) / a2s));     // m_auShiftLM[a2s - 32]
      else a = 0;
      if (sA < 0) a = (int)((unsigned)a << -sA); else a = a >> sA;
      a = min(max(a, -(1 << (15 - iB))), (1 << (15 - iB)) - 1);
      a = a * (1 << iB);
      int nn = 0;
      if (a != 0) nn = (short)(floor_log2((unsigned)(abs(a) + ((a < 0 ? -1 : 1) - 1) / 2)) - 5);
      shift = (shift + iB) - nn;
      a = a >> nn;
      bb = avgY - ((a * avgX) >> shift);
    }
  }
}

}  // namespace
