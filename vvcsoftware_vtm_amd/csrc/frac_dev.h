// frac_dev.h -- the fractional-sample refinement of one PU whose original block and reference window are in LDS: the device body shared by
// vvcgpu_frac_refine's general kernel (fracsearch.hip) and the translational whole-PU entries (bipredme.hip, unipredme.hip), and the LDS carve of
// those entries' owners (frac_owner_lds).
//
// Reference behaviour reproduced (bit-exact): InterSearch::xPatternSearchFracDIF (EncoderLib/InterSearch.cpp:2503-2552): xExtDIFUpSamplingH
// (:3813-3869), xPatternRefinement (:634-689, candidate order s_acMvRefineH/Q :59-83, strict '<'), xExtDIFUpSamplingQ (:3882-4093); distortion =
// xGetHADs (CommonLib/RdCost.cpp:2855-2974) or SAD; MV cost RdCost.h:172-199 with cost scale 1 (half stage) / 0 (quarter stage).  The original may be
// any int16 block (a bi-predictive search key 2 org - otherPred): the Hadamards run in 32-bit registers.
#pragma once
#include "common.h"
#include "dist_dev.h"

namespace {

__constant__ short c_lumaF[16][8] = {
  {  0, 0,   0, 64,  0,   0,  0,  0 }, {  0, 1,  -3, 63,  4,  -2,  1,  0 }, { -1, 2,  -5, 62,  8,  -3,  1,  0 },
  { -1, 3,  -8, 60, 13,  -4,  1,  0 }, { -1, 4, -10, 58, 17,  -5,  1,  0 }, { -1, 4, -11, 52, 26,  -8,  3, -1 },
  { -1, 3,  -9, 47, 31, -10,  4, -1 }, { -1, 4, -11, 45, 34, -10,  4, -1 }, { -1, 4, -11, 40, 40, -11,  4, -1 },
  { -1, 4, -10, 34, 45, -11,  4, -1 }, { -1, 4, -10, 31, 47,  -9,  3, -1 }, { -1, 3,  -8, 26, 52, -11,  4, -1 },
  {  0, 1,  -5, 17, 58, -10,  4, -1 }, {  0, 1,  -4, 13, 60,  -8,  3, -1 }, {  0, 1,  -3,  8, 62,  -5,  2, -1 },
  {  0, 1,  -2,  4, 63,  -3,  1,  0 } };
__constant__ signed char c_refH[9][2] = { {0,0},{0,-1},{0,1},{-1,0},{1,0},{-1,-1},{1,-1},{-1,1},{1,1} };
__constant__ signed char c_refQ[9][2] = { {0,0},{0,-1},{0,1},{-1,-1},{1,-1},{-1,0},{1,0},{-1,1},{1,1} };

constexpr int OFFS = 1 << 13;

__device__ __forceinline__ unsigned long long mv_cost(double lambda, int predH, int predV, int scale, int x, int y)
{
  const unsigned bits = expgolomb_bits((x << scale) - predH) + expgolomb_bits((y << scale) - predV);
  return rd_getcost(lambda, bits);
}

// distortion of (org - pred), both in LDS with pitch w, spread over the lanes of `nw` waves; returns the partial sum of THIS wave in every lane
// (caller combines the waves)
__device__ __forceinline__ unsigned long long dist_lds(const short* org, const short* pred, int w, int h, int useHad, int lane, int wave, int nw)
{
  if (!useHad)
  {
    unsigned long long acc = 0;
    for (int i = wave * 64 + lane; i < w * h; i += nw * 64) acc += (unsigned)abs((int)org[i] - (int)pred[i]);
    return wave_sum(acc);
  }
  return satd_block<64>(org, w, pred, w, w, h, lane, 0, 0, wave, nw);
}

// one wave per PU needs no workgroup barrier: LDS operations of a wave execute in order; the fence keeps the compiler from
// moving LDS accesses across the point.  Four-wave groups (large PUs) use the real barrier.
#define GROUP_SYNC() do { if (nw == 1) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } else __syncthreads(); } while (0)

struct FracLds { short* org; short* win; short* hpl; short* pred; unsigned long long* cost; int* sel; };

// The LDS of an owner of a translational whole-PU entry: a header, the first FRAC_HDR bytes of which are laid out here (the entry's own fields follow
// up to its header size), then the w x h block F.org, then the work area: F.win | F.hpl | F.pred, or whatever else the entry keeps there in turn.
constexpr int FRAC_OFF_SEL = 512;          // F.cost: bytes 0..511
constexpr int FRAC_OFF_RES = 544;          // F.sel: bytes 512..543
constexpr int FRAC_HDR = 576;              // fres: bytes 544..575
static_assert(52 * 8 <= FRAC_OFF_SEL && FRAC_OFF_SEL + 2 * 4 <= FRAC_OFF_RES && FRAC_OFF_RES + sizeof(vvcgpu_frac_result) <= FRAC_HDR, "header fields overlap");

inline __host__ __device__ int frac_r8(int v) { return (v + 7) & ~7; }
// shorts of the fractional refinement's three buffers in the work area
inline __host__ __device__ int frac_work_shorts(int w, int h) { return frac_r8((w + 10) * (h + 9)) + frac_r8(w * (h + 8)) + frac_r8(w * h); }

struct FracOwnerLds
{
  FracLds F;
  vvcgpu_frac_result* fres;
  short* work;
};

// base: the owner's LDS; orgOff: the entry's header size (F.org starts there)
__device__ __forceinline__ void frac_owner_lds(FracOwnerLds& L, unsigned char* base, int orgOff, int w, int h)
{
  L.F.cost = reinterpret_cast<unsigned long long*>(base);
  L.F.sel = reinterpret_cast<int*>(base + FRAC_OFF_SEL);
  L.fres = reinterpret_cast<vvcgpu_frac_result*>(base + FRAC_OFF_RES);
  L.F.org = reinterpret_cast<short*>(base + orgOff);
  L.work = L.F.org + frac_r8(w * h);
  L.F.win = L.work;
  L.F.hpl = L.F.win + frac_r8((w + 10) * (h + 9));
  L.F.pred = L.F.hpl + frac_r8(w * (h + 8));
}

// One PU by `gsz` lanes (64: a wavefront, GROUP_SYNC is a wave barrier; 256: the workgroup, every wavefront of which makes the same calls).
// L.org = the w x h original (pitch w), L.win = reference rows -4 .. h+4, columns -4 .. w+4 around the integer position (pitch wp = w + 10); L.hpl
// (w x (h + 8)), L.pred (w x h), L.cost (8-byte units 0..51) and L.sel (2 ints) are work space.  (mvX, mvY) = the integer vector, for the vector cost.
// *res (global memory or LDS) is written by lane 0 of the group; the caller synchronises before reading it.
__device__ __forceinline__ void frac_refine_pu(const FracLds& L, int w, int h, int wp, int bd, int cmin, int cmax, int useHad, const vvcgpu_mvcost& mv,
                                               int mvX, int mvY, bool active, int tid, int gsz, vvcgpu_frac_result* res)
{
  const int lane = tid & 63, wave = tid >> 6, nw = gsz >> 6;
  const int headRoom = max(2, 14 - bd);
  int hx = 0, hy = 0;
  for (int stage = 0; stage < 2; stage++)
  {
    // candidate i of this stage sits at quarter offset (bx + dx_i * step, by + dy_i * step)
    const int step = stage == 0 ? 2 : 1;
    const int bx = stage == 0 ? 0 : 2 * hx, by = stage == 0 ? 0 : 2 * hy;
    for (int cxi = -1; cxi <= 1; cxi++)
    {
      const int qx = bx + cxi * step;
      const int ix = qx >> 2, fx = (qx & 3) << 2;
      GROUP_SYNC();                                           // window / previous users of hpl, pred done
      if (active)
      {
        // first-stage horizontal plane, rows -4 .. h+3 (h+8 rows), cols 0 .. w-1 at integer offset ix
        const short* cf = c_lumaF[fx];
        const int shift1 = 6 - headRoom, off1 = -(OFFS << shift1);
        for (int i = tid; i < w * (h + 8); i += gsz)
        {
          const int r = i / w, x = i - r * w;
          const short* s = L.win + r * wp + x + ix + 1;         // sample (x + ix - 3) of row r-4
          int v;
          if (fx == 0) v = (short)((short)(s[3] << headRoom) - (short)OFFS);
          else
          {
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) sum += s[k] * cf[k];
            v = (short)((sum + off1) >> shift1);
          }
          L.hpl[i] = (short)v;
        }
      }
      GROUP_SYNC();
      for (int cyi = -1; cyi <= 1; cyi++)
      {
        const int qy = by + cyi * step;
        const int iy = qy >> 2, fy = (qy & 3) << 2;
        if (active)
        {
          // last-stage vertical pass with a sliding 8-row window per column segment of 4 rows
          const short* cf = c_lumaF[fy];
          const int shift2 = 6 + headRoom, off2 = (1 << (shift2 - 1)) + (OFFS << 6);
          const int nseg = (h + 3) >> 2;
          for (int i = tid; i < w * nseg; i += gsz)
          {
            const int seg = i / w, x = i - seg * w;
            const int y0 = seg * 4;
            const short* hp = L.hpl + (y0 + iy + 1) * w + x;    // row (y0 + iy - 3) of the plane (plane row 0 = picture row -4)
            if (fy == 0)
            {
              for (int y = y0; y < min(y0 + 4, h); y++)
              {
                const int s = hp[(y - y0 + 3) * w];
                L.pred[y * w + x] = (short)clip3(cmin, cmax, (short)((s + OFFS + (1 << (headRoom - 1))) >> headRoom));
              }
            }
            else
            {
              int win8[8];
#pragma unroll
              for (int k = 0; k < 7; k++) win8[k + 1] = hp[k * w];
#pragma unroll
              for (int yy = 0; yy < 4; yy++)
              {
#pragma unroll
                for (int k = 0; k < 7; k++) win8[k] = win8[k + 1];
                if (y0 + yy < h)
                {
                  win8[7] = hp[(yy + 7) * w];
                  int sum = 0;
#pragma unroll
                  for (int k = 0; k < 8; k++) sum += win8[k] * cf[k];
                  L.pred[(y0 + yy) * w + x] = (short)clip3(cmin, cmax, (short)((sum + off2) >> shift2));
                }
              }
            }
          }
        }
        GROUP_SYNC();
        if (active)
        {
          const unsigned long long d = dist_lds(L.org, L.pred, w, h, useHad, lane, wave, nw);
          // which candidate index has offsets (cxi, cyi)?
          int ci = 0;
          for (int i = 0; i < 9; i++)
          {
            const int dx = stage == 0 ? c_refH[i][0] : c_refQ[i][0], dy = stage == 0 ? c_refH[i][1] : c_refQ[i][1];
            if (dx == cxi && dy == cyi) ci = i;
          }
          if (lane == 0) L.cost[16 + ci * 4 + wave] = d;              // per-wave partials, summed after the barrier
        }
        GROUP_SYNC();
        if (active && tid == 0)
        {
          int ci = 0;
          for (int i = 0; i < 9; i++)
          {
            const int dx = stage == 0 ? c_refH[i][0] : c_refQ[i][0], dy = stage == 0 ? c_refH[i][1] : c_refQ[i][1];
            if (dx == cxi && dy == cyi) ci = i;
          }
          unsigned long long s = 0;
          for (int k = 0; k < nw; k++) s += L.cost[16 + ci * 4 + k];
          L.cost[ci] = s;
        }
      }
    }
    GROUP_SYNC();
    if (active && tid == 0)
    {
      unsigned long long best = ~0ull;
      int bi = 0;
      for (int i = 0; i < 9; i++)
      {
        const int dx = stage == 0 ? c_refH[i][0] : c_refQ[i][0], dy = stage == 0 ? c_refH[i][1] : c_refQ[i][1];
        unsigned long long c;
        if (stage == 0) c = L.cost[i] + mv_cost(mv.lambda, mv.pred_hor, mv.pred_ver, 1, (mvX << 1) + dx, (mvY << 1) + dy);
        else c = L.cost[i] + mv_cost(mv.lambda, mv.pred_hor, mv.pred_ver, 0, (((mvX << 1) + hx) << 1) + dx, (((mvY << 1) + hy) << 1) + dy);
        if (c < best) { best = c; bi = i; }
      }
      const int dx = stage == 0 ? c_refH[bi][0] : c_refQ[bi][0], dy = stage == 0 ? c_refH[bi][1] : c_refQ[bi][1];
      L.sel[0] = dx; L.sel[1] = dy;
      if (stage == 0) { res->half_x = dx; res->half_y = dy; res->cost_half = best; }
      else { res->qter_x = dx; res->qter_y = dy; res->cost = best; }
    }
    GROUP_SYNC();
    if (stage == 0) { hx = L.sel[0]; hy = L.sel[1]; }
  }
}

}  // namespace
