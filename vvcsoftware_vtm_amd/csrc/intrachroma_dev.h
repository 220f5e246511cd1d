// intrachroma_dev.h -- what the two chroma mode passes share, stated once for intrachroma.hip (vvcgpu_intra_chroma_code_batch, the Quant::quant chain) and
// intrachromadq.hip (vvcgpu_intra_chroma_code_dq_batch, the DepQuant trellis): the PU list grouped by shape as a kernel argument, the contract of a PU,
// the markers of what is skipped, the staging of the down-sampled luma and of the references once per PU, and the prediction of one slot into the
// wavefront's tile.  What follows the prediction (the chain body, or the forward transform into the trellis workspace) is each file's own.
#pragma once
#include "common.h"
#include "intra_dev.h"

namespace {

typedef vvcgpu_intra_chroma_pu ChPu;
constexpr int CH_MAX_RUNS = 36, CH_LM = VVCGPU_INTRA_CHROMA_LM, CH_SLOTS = 6;

struct ChSeg { int first, count; short w, h; };                            // a run of the caller's list
struct ChArgs
{
  const Pel* rec; const unsigned char* flags; const vvcgpu_intra_fill_desc* fill; Pel* refs; const Pel* luma; const Pel* org; const ChPu* pus;
  Pel* pred; Pel* candRec; TCoeff* level; unsigned* absSum; unsigned long long* dist; int* fbScratch; const _Float16* image;
  int writePred, bd, cmin, cmax, nSeg, total;
  ChSeg seg[CH_MAX_RUNS];
};

// the PU behind work index q (wave-uniform, < a.total) of a launch and the shape of its run.  Unrolled, with constant indices: the runs stay kernel
// arguments read by scalar loads
__device__ __forceinline__ int ch_locate(const ChArgs& a, int q, int& rw, int& rh)
{
  int p = 0;
  bool found = false;
  rw = rh = 0;
#pragma unroll
  for (int s = 0; s < CH_MAX_RUNS; s++)
  {
    const ChSeg g = a.seg[s];
    if (!found && s < a.nSeg)
    {
      if (q < g.count) { p = g.first + q; rw = g.w; rh = g.h; found = true; }
      else q -= g.count;
    }
  }
  return p;
}

__device__ __forceinline__ bool ch_pu_ok(const ChArgs& a, const ChPu& u, int p, int rw, int rh, bool& anyLm)
{
  const int w = u.w, h = u.h;
  bool ok = side_ok(w, 2) && side_ok(h, 2) && w == rw && h == rh && (u.cand_off & 3) == 0 && (u.level_off & 3) == 0;
  anyLm = false;
#pragma unroll
  for (int k = 0; k < CH_SLOTS; k++) { const int m = u.mode[k]; ok = ok && m >= -1 && m <= CH_LM; anyLm = anyLm || m == CH_LM; }
  ok = ok && (!anyLm || a.luma != nullptr);
  if (ok && a.fill)
  {
    int T, L;
    intra_ref_lengths(w, h, T, L);
    for (int c = 0; c < 2; c++)
    {
      const vvcgpu_intra_fill_desc f = a.fill[2 * (size_t)p + c];
      ok = ok && f.w == w && f.h == h && f.ref_off == u.ref_off[c] && f.unit_w >= 1 && f.unit_h >= 1;
      ok = ok && (T + f.unit_w - 1) / f.unit_w + (L + f.unit_h - 1) / f.unit_h + 1 <= FILL_UNITS_MAX;
    }
  }
  return ok;
}

// fields of a PU by a run-time index without a private copy of the struct
__device__ __forceinline__ int ch_mode(const ChPu& u, int k)
{
  const unsigned lo = (unsigned)(unsigned char)u.mode[0] | (unsigned)(unsigned char)u.mode[1] << 8 | (unsigned)(unsigned char)u.mode[2] << 16 | (unsigned)(unsigned char)u.mode[3] << 24;
  const unsigned hi = (unsigned)(unsigned char)u.mode[4] | (unsigned)(unsigned char)u.mode[5] << 8;
  return (int)(signed char)((k < 4 ? lo >> (8 * k) : hi >> (8 * (k - 4))) & 0xFFu);
}
#define CH_SEL(field, c) ((c) ? u.field[1] : u.field[0])

// skipped: the markers of slots [k0, k1) of component c (c < 0: both), nothing else
__device__ __forceinline__ void ch_mark(const ChArgs& a, int p, int k0, int k1, int c, int lane)
{
  const int e = lane >> 1, cc = lane & 1;
  if (e >= k0 && e < k1 && (c < 0 || cc == c)) { a.absSum[12 * (size_t)p + 2 * e + cc] = 0xFFFFFFFFu; a.dist[12 * (size_t)p + 2 * e + cc] = ~0ull; }
}

// The down-sampled luma of a PU by its wavefront: the block into lumaS (row pitch w), the neighbour line into lumaTop (if above), the neighbour column
// into lumaLeft (if left) -- xGetLumaRecPixels, once per PU for both components
__device__ __forceinline__ void ch_stage_luma(const Pel* __restrict__ luma, int rs, int w, int h, bool aboveAvail, bool leftAvail, int lane, short* lumaS,
                                              short* lumaTop, short* lumaLeft)
{
  const int lw = ilog2(w), rs2 = 2 * rs;
  for (int e = lane; e < w * h; e += 64)
  {
    const int y = e >> lw, x = e & (w - 1);
    lumaS[e] = (short)cclm_down(luma + (ptrdiff_t)y * rs2 + 2 * x, rs, x == 0 && !leftAvail);
  }
  if (aboveAvail) for (int i = lane; i < w; i += 64) lumaTop[i] = (short)cclm_down(luma - rs2 + 2 * i, rs, i == 0 && !leftAvail);
  if (leftAvail) for (int j = lane; j < h; j += 64) lumaLeft[j] = (short)cclm_down(luma + (ptrdiff_t)j * rs2 - 2, rs, false);
}

// The references of component c of a PU into the wavefront's top / left arrays: gathered (packed: T + L + 1 shorts, su: FILL_UNITS_MAX shorts of the
// wavefront's LDS; also written to refs_base if there is one) or read from refs_base
__device__ __forceinline__ void ch_stage_refs(const ChArgs& a, const ChPu& u, int p, int c, int T, int L, int lane, short* packed, short* su, short* top, short* left)
{
  if (a.fill)
  {
    const vvcgpu_intra_fill_desc f = a.fill[2 * (size_t)p + c];
    intra_fill_refs_block(a.rec, a.flags, f, a.bd, lane, su, packed);
    wave_sync();
    if (a.refs) for (int i = lane; i <= T + L; i += 64) a.refs[CH_SEL(ref_off, c) + i] = packed[i];
    intra_stage_refs(packed, false, T, L, lane, top, left, nullptr);
  }
  else intra_stage_refs(a.refs + CH_SEL(ref_off, c), false, T, L, lane, top, left, nullptr);
}

// the prediction of one slot into the wavefront's tile (row pitch w): predIntraAng, or the linear model over the staged luma
__device__ __forceinline__ void ch_predict(int mode, int w, int h, int T, int L, const short* top, const short* left, short* mainX, const short* lumaS,
                                           int lmA, int lmB, int lmShift, int cmin, int cmax, int lane, short* tile)
{
  if (mode == CH_LM)
    for (int e = lane; e < w * h; e += 64) tile[e] = (short)min(max(((lmA * (int)lumaS[e]) >> lmShift) + lmB, cmin), cmax);
  else
    intra_pred_samples<64>(w, h, mode, T, L, top, left, mainX, tile, w, cmin, cmax, lane);
  wave_sync();
}

}  // namespace
