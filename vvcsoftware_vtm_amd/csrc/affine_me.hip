// affine_me.hip -- the whole affine gradient search of a PU in one launch (vvcgpu_affine_me_batch) for gfx950.
//
// Reference behaviour reproduced (bit-exact, the double arithmetic included): InterSearch::xAffineMotionEstimation (EncoderLib/InterSearch.cpp:3286-3743)
// with solveEqual (:3102-3179), InterPrediction::xPredAffineBlk (CommonLib/InterPrediction.cpp:550-722; uni-prediction, rounded and clipped, with its
// yFrac == 0 / xFrac == 0 branches), InterpolationFilter::filter / filterCopy (InterpolationFilter.cpp:205-379, m_lumaFilter :59-77), clipMv
// (Mv.cpp:64-80), Mv::roundMV2SignalPrecision (Mv.h:242-257), RdCost::getBitsOfVectorWithPredictor / getCost (RdCost.h:172-199).
//
// Design: the owner of a PU -- one wavefront up to AFI_WAVE_MAX samples, the workgroup's four above -- carries it through the whole search.  The grid
// is cdiv(n, 4) workgroups of four wavefront owners followed by n workgroup owners; each item is served by exactly one of the two, by its size, which
// only the device knows (the other leaves at once): no work list, no atomics.  The prediction lives in LDS from the first step to the last: sixteen
// lanes interpolate one 4x4 sub-block (four per wavefront) from its 11x11 window of the reference plane straight into the tile; the error / Sobel /
// equation pass and the Hadamard distortion (afi_dev.h, shared with the per-iteration entry) read it there.  The equation sums meet in LDS; every
// lane of the owner then solves the system and updates the vectors with the same (uniform) values, so nothing is broadcast.
#include "common.h"
#include "dist_dev.h"
#include "afi_dev.h"
#include "raster_dev.h"

namespace {

__constant__ short kAfmLuma[16][8] = {                        // m_lumaFilter, 1/16 sample phases
  {  0, 0,   0, 64,  0,   0,  0,  0 }, {  0, 1,  -3, 63,  4,  -2,  1,  0 }, { -1, 2,  -5, 62,  8,  -3,  1,  0 }, { -1, 3,  -8, 60, 13,  -4,  1,  0 },
  { -1, 4, -10, 58, 17,  -5,  1,  0 }, { -1, 4, -11, 52, 26,  -8,  3, -1 }, { -1, 3,  -9, 47, 31, -10,  4, -1 }, { -1, 4, -11, 45, 34, -10,  4, -1 },
  { -1, 4, -11, 40, 40, -11,  4, -1 }, { -1, 4, -10, 34, 45, -11,  4, -1 }, { -1, 4, -10, 31, 47,  -9,  3, -1 }, { -1, 3,  -8, 26, 52, -11,  4, -1 },
  {  0, 1,  -5, 17, 58, -10,  4, -1 }, {  0, 1,  -4, 13, 60,  -8,  3, -1 }, {  0, 1,  -3,  8, 62,  -5,  2, -1 }, {  0, 1,  -2,  4, 63,  -3,  1,  0 } };

constexpr int AFM_TMP = 11 * 4;            // first-pass rows of one 4x4 sub-block (8 taps: 11 rows) x 4 columns

// NT = 64: the wavefront owns the PU; NT = 256: the workgroup does (every wavefront follows the same, uniform, control flow)
template <int NT> __device__ __forceinline__ void afm_sync()
{
  if (NT == 256) __syncthreads();
  else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
}

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
  const Pel* org; const Pel* ref;        // the PU's block in org_base; reference sample (pos_x, pos_y) of the picture
  int os, rs, w, h, six, nmv;
  int posX, posY;
  int horMin, horMax, verMin, verMax;    // clipMv, 1/16 units
};

// xPredAffineBlk (luma, uni): sixteen lanes per 4x4 sub-block; tmpW = this wavefront's first-pass rows (4 x AFM_TMP)
template <int NT>
__device__ __forceinline__ void afm_predict(const AfmPu& u, const vvcgpu_affine_me_cfg& c, const int (&mv)[3][2], Pel* predL, short* tmpW, int tid)
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
  const int headRoom = 14 - c.bit_depth;                                 // IF_INTERNAL_PREC - bit depth (8..10)
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
    afm_sync<64>();
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
          v = clip3(c.clp_min, c.clp_max, (int)(short)((sum + 32) >> 6));
        }
      }
      else if (xFrac == 0)
      {
        const Pel* p = win + (ptrdiff_t)(r - 3) * rs + cc;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += (int)p[(ptrdiff_t)k * rs] * fy[k];
        v = clip3(c.clp_min, c.clp_max, (int)(short)((sum + 32) >> 6));
      }
      else
      {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += (int)tmp[(r + k) * 4 + cc] * fy[k];
        v = clip3(c.clp_min, c.clp_max, (int)(short)((sum + off2) >> sh2));
      }
      predL[(hq + r) * w + wq + cc] = (Pel)v;
    }
    afm_sync<64>();                                                     // the next round overwrites tmp
  }
}

// ruiBits + the bits of the control-point vectors against their predictors (:3386-3410, cost scale 0, imv shift 0)
__device__ __forceinline__ unsigned afm_bits(const vvcgpu_affine_me_item& it, int nmv, const int (&mv)[3][2])
{
  unsigned bits = it.bits;
#pragma unroll
  for (int i = 0; i < 3; i++)
  {
    if (i >= nmv) break;
    int px = it.mvp[i][0], py = it.mvp[i][1];
    if (i != 0) { px += mv[0][0] - it.mvp[0][0]; py += mv[0][1] - it.mvp[0][1]; }
    bits += expgolomb_bits((mv[i][0] >> 2) - (px >> 2)) + expgolomb_bits((mv[i][1] >> 2) - (py >> 2));
  }
  return bits;
}

struct AfmLds
{
  Pel* predL;                 // the owner's prediction tile
  short* tmpW;                // this wavefront's first-pass rows
  long long* eq;              // the owner's 49 sums
  long long (*red)[64];       // NT = 256: the wavefronts' partial sums
  unsigned long long* distW;  // NT = 256: the wavefronts' distortions
};

template <int NT>
__device__ __forceinline__ unsigned long long afm_dist(const AfmPu& u, const AfmLds& L, int tid)
{
  const int lane = tid & 63, wave = tid >> 6;
  vvcgpu_affine_iter d;
  d.org_stride = u.os;
  unsigned long long sum;
  if ((u.h & 15) == 0) sum = afi_dist(d, u.org, L.predL, u.w, u.h, 1, NT == 256 ? wave : 0, NT == 256 ? 4 : 1, lane);
  else sum = (NT == 64 || wave == 0) ? satd_block<64, AfiLdsPel>(u.org, u.os, (AfiLdsPel)L.predL, u.w, u.w, u.h, lane) : 0ull;   // no bands of sixteen rows
  if (NT == 64) return sum;
  if (lane == 0) L.distW[wave] = sum;
  __syncthreads();
  sum = L.distW[0] + L.distW[1] + L.distW[2] + L.distW[3];
  __syncthreads();                                                       // distW is written again by the next step
  return sum;
}

template <int NT>
__device__ __forceinline__ void afm_search(const vvcgpu_affine_me_item& it, const vvcgpu_affine_me_cfg& c, const Pel* orgBase, const Pel* refBase,
                                           const AfmLds& L, vvcgpu_affine_me_result* res, vvcgpu_affine_me_step* trace, int tid)
{
  AfmPu u;
  u.w = it.pu.w; u.h = it.pu.h; u.six = it.pu.six_param != 0; u.nmv = u.six ? 3 : 2;
  u.posX = it.pu.pos_x; u.posY = it.pu.pos_y;
  u.os = it.org_stride; u.rs = c.ref_stride;
  u.org = orgBase + it.org_off;
  u.ref = refBase + (ptrdiff_t)(u.posY + c.ref_origin_y) * c.ref_stride + u.posX + c.ref_origin_x;
  u.horMax = (c.pic_w + 8 - u.posX - 1) << 4; u.horMin = (-c.max_cu_w - 8 - u.posX + 1) << 4;      // clipMv of a high-precision vector: shift 2 + 2
  u.verMax = (c.pic_h + 8 - u.posY - 1) << 4; u.verMin = (-c.max_cu_h - 8 - u.posY + 1) << 4;
  const double weight = it.half_weight ? 0.5 : 1.0;
  int iterTime = u.six ? (it.half_weight ? 3 : 4) : (it.half_weight ? 3 : 5);
  if (!c.affine_type) iterTime = it.half_weight ? 5 : 7;

  int cur[3][2], best[3][2];
#pragma unroll
  for (int i = 0; i < 3; i++) { cur[i][0] = it.pu.mv[0][i][0]; cur[i][1] = it.pu.mv[0][i][1]; }
#pragma unroll
  for (int i = 0; i < 3; i++)
    if (i < u.nmv) { cur[i][0] = min(u.horMax, max(u.horMin, cur[i][0])); cur[i][1] = min(u.verMax, max(u.verMin, cur[i][1])); }

  afm_predict<NT>(u, c, cur, L.predL, L.tmpW, tid);
  afm_sync<NT>();
  unsigned long long had = afm_dist<NT>(u, L, tid);
  unsigned bestBits = afm_bits(it, u.nmv, cur);
  unsigned long long bestCost = (unsigned long long)(floor(weight * (double)had) + (double)(unsigned long long)(c.lambda * bestBits));
#pragma unroll
  for (int i = 0; i < 3; i++) { best[i][0] = cur[i][0]; best[i][1] = cur[i][1]; }
  unsigned steps = 1;
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
    if (u.six) afi_equations_regs<6, NT>(d, u.org, L.predL, u.w, u.h, L.eq, L.red, tid);
    else       afi_equations_regs<4, NT>(d, u.org, L.predL, u.w, u.h, L.eq, L.red, tid);
    afm_sync<NT>();
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
    afm_sync<NT>();                                                      // every lane has read eq and the tile before they are overwritten
    afm_predict<NT>(u, c, cur, L.predL, L.tmpW, tid);
    afm_sync<NT>();
    had = afm_dist<NT>(u, L, tid);
    const unsigned bits = afm_bits(it, u.nmv, cur);
    const unsigned long long cost = (unsigned long long)(floor(weight * (double)had) + (double)(unsigned long long)(c.lambda * bits));
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
  if (tid == 0)
  {
#pragma unroll
    for (int i = 0; i < 3; i++) { res->mv[i][0] = best[i][0]; res->mv[i][1] = best[i][1]; }
    res->bits = bestBits; res->steps = steps; res->cost = bestCost;
    if (trace)
      for (unsigned s = steps; s < VVCGPU_AFFINE_ME_MAX_STEPS; s++)
      {
#pragma unroll
        for (int i = 0; i < 3; i++) { trace[s].mv[i][0] = 0; trace[s].mv[i][1] = 0; }
        trace[s].cost = 0;
      }
  }
}

__device__ __forceinline__ bool afm_item_ok(const vvcgpu_affine_me_item& it)
{
  const int w = it.pu.w, h = it.pu.h;
  return w >= 16 && h >= 16 && w <= AFI_MAX && h <= AFI_MAX && ((w | h) & 3) == 0 && it.pu.bi == 0 && it.org_stride > 0;
}

__global__ __launch_bounds__(256) void affine_me_kernel(const Pel* __restrict__ orgBase, const Pel* __restrict__ refBase,
                                                        const vvcgpu_affine_me_item* __restrict__ items, int n, const vvcgpu_affine_me_cfg c,
                                                        vvcgpu_affine_me_result* __restrict__ results, vvcgpu_affine_me_step* __restrict__ trace)
{
  __shared__ __align__(16) Pel predL[AFI_MAX * AFI_MAX];               // one workgroup owner's tile, or four wavefront owners' (AFI_WAVE_MAX each)
  __shared__ __align__(16) short tmpL[4][4 * AFM_TMP];
  __shared__ long long eqL[4][49];
  __shared__ long long red[4][64];
  __shared__ unsigned long long distW[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nWaveGroups = (n + 3) >> 2;
  AfmLds L;
  L.tmpW = tmpL[wave]; L.red = red; L.distW = distW;
  if ((int)blockIdx.x < nWaveGroups)
  {
    const int b = blockIdx.x * 4 + wave;                                 // wavefront owners
    if (b >= n) return;
    const vvcgpu_affine_me_item it = items[b];
    if (!afm_item_ok(it) || it.pu.w * it.pu.h > AFI_WAVE_MAX) return;    // the workgroup owner of this item answers
    L.predL = predL + wave * AFI_WAVE_MAX; L.eq = eqL[wave];
    afm_search<64>(it, c, orgBase, refBase, L, results + b, trace ? trace + (size_t)b * VVCGPU_AFFINE_ME_MAX_STEPS : nullptr, lane);
    return;
  }
  const int b = blockIdx.x - nWaveGroups;                                // workgroup owners
  if (b >= n) return;
  const vvcgpu_affine_me_item it = items[b];
  vvcgpu_affine_me_step* tr = trace ? trace + (size_t)b * VVCGPU_AFFINE_ME_MAX_STEPS : nullptr;
  if (!afm_item_ok(it))                                                  // outside the contract: the sentinel, nothing is read or predicted
  {
    if (tid == 0)
    {
      vvcgpu_affine_me_result r;
      memset(&r, 0, sizeof(r));
      r.cost = ~0ull;
      results[b] = r;
    }
    if (tr && tid < VVCGPU_AFFINE_ME_MAX_STEPS)
    {
      vvcgpu_affine_me_step s;
      memset(&s, 0, sizeof(s));
      tr[tid] = s;
    }
    return;
  }
  if (it.pu.w * it.pu.h <= AFI_WAVE_MAX) return;
  L.predL = predL; L.eq = eqL[0];
  afm_search<256>(it, c, orgBase, refBase, L, results + b, tr, tid);
}

}  // namespace

extern "C" int vvcgpu_affine_me_batch(const vvc_pel* org_base, const vvc_pel* ref_base, const vvcgpu_affine_me_item* items, int n,
                                      const vvcgpu_affine_me_cfg* cfg_host, vvcgpu_affine_me_result* results, vvcgpu_affine_me_step* trace, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "affine_me_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org_base && ref_base && items && cfg_host && results, "affine_me_batch: null pointer");
  const vvcgpu_affine_me_cfg c = *cfg_host;
  VVC_CHECK_ARG(c.pic_w > 0 && c.pic_h > 0 && c.max_cu_w > 0 && c.max_cu_h > 0 && c.ref_stride > 0, "affine_me_batch: geometry (picture %d x %d, CTU %d x %d, ref_stride %d)",
                c.pic_w, c.pic_h, c.max_cu_w, c.max_cu_h, c.ref_stride);
  VVC_CHECK_ARG(c.pic_w <= 65536 && c.pic_h <= 65536 && c.max_cu_w <= 256 && c.max_cu_h <= 256, "affine_me_batch: geometry (picture %d x %d, CTU %d x %d)", c.pic_w,
                c.pic_h, c.max_cu_w, c.max_cu_h);
  VVC_CHECK_ARG(c.clp_min <= c.clp_max, "affine_me_batch: clip range %d..%d", c.clp_min, c.clp_max);
  VVC_CHECK_ARG(c.lambda >= 0.0 && c.lambda < 1048576.0, "affine_me_batch: lambda out of range");
  if (c.bit_depth > 10 || c.bit_depth < 8) { vvcgpu_set_error("affine_me_batch: bit depth %d outside 8..10", c.bit_depth); return VVCGPU_E_UNSUPPORTED; }
  VVC_CHECK_ARG(n < (1 << 28), "affine_me_batch: n %d", n);
  hipLaunchKernelGGL(affine_me_kernel, dim3(cdiv(n, 4) + n), dim3(256), 0, (hipStream_t)stream, org_base, ref_base, items, n, c, results, trace);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
