// intratu_dev.h -- the item contract of the intra RD loop's pixel passes, IntraSearch::xIntraCodingTUBlock (EncoderLib/IntraSearch.cpp:1147-1316), stated
// once for intratu.hip (vvcgpu_intra_tu_code_batch, the Quant::quant chain) and intratudq.hip (vvcgpu_intra_tu_code_dq_batch, the DepQuant trellis): a
// wavefront owns an item (the pair preds[i], tus[i]), decides whether it is served and with which mode, and forms the prediction in its LDS tile.  Here
// are the row layout of mode_list, the wavefront's part of the dynamic LDS, that decision, the prediction and the markers of a skipped item.  What
// follows the prediction (the chain body, or the forward transform into the trellis workspace) is each file's own.  The functions take the kernel's
// argument struct as a template parameter: the two structs (ItArgs, ItqArgs) name the fields they read alike.
#pragma once
#include "common.h"
#include "intra_dev.h"
#include "mfma_tr.h"
#include "resichain_dev.h"

namespace {

constexpr int IT_TILE = 64 * 64;                                          // samples of a wavefront's tile: the prediction (under DepQuant then the residual over it, in the back resi')
constexpr int IT_TAB_BYTES = RC_TAB_HALVES * 2;                           // the f16 matrices of the matrix-core bodies
constexpr int IT_WAVE_BYTES = (IT_TILE + 4 * REF_MAX + NEG_MAX + REF_MAX) * 2 + (int)sizeof(vvcgpu_resi_chain_desc);
static_assert(IT_TAB_BYTES % 16 == 0 && IT_WAVE_BYTES % 16 == 0, "LDS layout");
constexpr int IT_LIST_INTS = 16, IT_LIST_FIRST = 5, IT_LIST_MAX = 11;     // a row of list_out of vvcgpu_intra_mode_cand_batch: [0] size, [5 .. 15] uiRdModeList
constexpr int IT_FB_INTS = 2 * 4096;                                      // global scratch per wavefront: the integer body's two buffers for an item outside the matrix-core range

// the wavefront's part of the dynamic LDS: behind the f16 matrices, per wavefront the tile, the reference work arrays of intra_pred_block and the item's
// chain descriptor
struct ItLds { short* tile; short* topS; short* leftS; short* tmpS; short* mainS; RcDesc* dS; };
__device__ __forceinline__ ItLds it_lds(unsigned char* smem, int wave)
{
  unsigned char* const mine = smem + IT_TAB_BYTES + (size_t)wave * IT_WAVE_BYTES;
  ItLds l;
  l.tile = reinterpret_cast<short*>(mine);
  l.topS = l.tile + IT_TILE;                                              // top, left: REF_MAX each; tmp: 2 REF_MAX; main: NEG_MAX + REF_MAX
  l.leftS = l.topS + REF_MAX;
  l.tmpS = l.leftS + REF_MAX;
  l.mainS = l.tmpS + 2 * REF_MAX;
  l.dS = reinterpret_cast<RcDesc*>(mine + IT_WAVE_BYTES - sizeof(RcDesc));
  return l;
}

// Is the item served, and with which mode and filter decision?  also(): what the entry asks of the item beyond the shared rule, evaluated behind it (a
// callable and not a bool worked out in front: only so intra_tu_dq_front_kernel stays what it was, docs/MEASUREMENTS.md).  The row of mode_list is read
// only when everything else holds.
template <class Args, class Also>
__device__ __forceinline__ bool it_resolve(const Args& a, const vvcgpu_intra_desc& p, const RcDesc& t, Also also, int& mode, bool& filt)
{
  const int w = t.w, h = t.h;
  mode = p.mode;
  filt = p.filter_refs != 0;
  bool ok = side_ok(w, 4) && side_ok(h, 4) && p.w == w && p.h == h && mode >= VVCGPU_INTRA_TU_FROM_LIST && mode <= VDIA &&
            (mode != VVCGPU_INTRA_TU_PRED_GIVEN || a.pred != nullptr) &&
            t.tr_hor >= 0 && t.tr_hor <= 2 && t.tr_ver >= 0 && t.tr_ver <= 2 && (w <= 32 || t.tr_hor == 0) && (h <= 32 || t.tr_ver == 0) && also();
  if (ok && mode == VVCGPU_INTRA_TU_FROM_LIST)
  {
    const int row = t.reserved[0], slot = t.reserved[1];
    ok = a.modeList != nullptr && row >= 0 && slot >= 0 && slot < IT_LIST_MAX;
    if (ok) ok = slot < a.modeList[IT_LIST_INTS * (size_t)row];
    if (ok)
    {
      mode = a.modeList[IT_LIST_INTS * (size_t)row + IT_LIST_FIRST + slot];
      ok = mode >= PLANAR && mode <= VDIA;
      if (ok) filt = intra_use_filtered(w, h, mode, a.noSmoothing);
    }
  }
  return ok;
}
// skipped: the markers, nothing else
template <class Args>
__device__ __forceinline__ void it_mark(const Args& a, int item, int lane)
{
  if (lane == 0) { a.absSum[item] = 0xFFFFFFFFu; a.numSig[item] = 0xFFFFFFFFu; a.dist[item] = ~0ull; a.modeOut[item] = -1; }
}
// the prediction of a served item into the tile, rows w apart: read from pred_base, or predIntraAng
template <class Args>
__device__ __forceinline__ void it_predict(const Args& a, const vvcgpu_intra_desc& p, const RcDesc& t, int mode, bool filt, const ItLds& l, int lane)
{
  const int w = t.w, lw = ilog2(w), samples = w * t.h;
  if (mode == VVCGPU_INTRA_TU_PRED_GIVEN)
  {
    const Pel* src = a.pred + t.pred_off;
    for (int e = lane; e < samples; e += 64) l.tile[e] = src[(ptrdiff_t)(e >> lw) * t.pred_stride + (e & (w - 1))];
  }
  else
  {
    vvcgpu_intra_desc d = p;
    d.mode = (int8_t)mode; d.filter_refs = filt ? 1 : 0;
    intra_pred_block(d, a.refs, l.tile, w, a.cmin, a.cmax, lane, l.topS, l.leftS, l.tmpS, l.mainS);
  }
  wave_sync();
}

}  // namespace
