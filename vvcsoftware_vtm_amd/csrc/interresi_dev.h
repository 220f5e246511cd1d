// interresi_dev.h -- the item walk of the inter residual passes, InterSearch::encodeResAndCalcRdInterCU (EncoderLib/InterSearch.cpp:4752-4909), stated
// once for interresi.hip (vvcgpu_inter_resi_code_batch) and interresidq.hip (vvcgpu_inter_resi_code_dq_batch): a wavefront owns an item, stages
// orgResi = org - pred in its LDS tile, runs the item's slots through transform and quantiser -- that part is each file's own -- and closes every slot
// with both distortions, resi' and the reconstruction.  Here are the constants of that frame, the rd_list look-up, the staging
// loop, the tile layout, the closing loop and the host side the two entries share.  The closing loop takes the kernel's argument struct as a template
// parameter: the two structs (IrArgs, IqArgs) name the fields it reads alike.
#pragma once
#include "common.h"
#include "dist_dev.h"
#include "resichain_dev.h"

namespace {

typedef vvcgpu_inter_resi_item IrItem;
constexpr int IR_SLOTS = VVCGPU_INTER_RESI_SLOTS;
constexpr int IR_WAVES = 8, IR_THREADS = 64 * IR_WAVES;
constexpr int IR_TILE = 64 * 64;                                          // samples of a wavefront's tile: orgResi, the prediction, resi' (ir_tile)
constexpr int IR_LIST_INTS = 8, IR_LIST_MAX = 7;                          // a row of rd_list_out of vvcgpu_merge_cand_batch: [0] count, [1 .. 7] RdModeList
constexpr int IR_FB_INTS = 2 * 4096;                                      // global scratch per wavefront: the integer body's two buffers for an item outside the matrix-core range

// The rd_list look-up of an item that has passed the entry's own checks so far (ok): with list_row >= 0 it takes its prediction from the candidate
// that row list_row of rd_list names at list_slot, and predOff moves on by that candidate's pitch.  -> ok; false also: no list, or the slot or the
// candidate outside it
__device__ __forceinline__ bool ir_list_pred(bool ok, const int* rdList, const IrItem& t, long long& predOff)
{
  if (ok && t.list_row >= 0)
  {
    const int slot = t.list_slot;
    ok = rdList != nullptr && slot >= 0 && slot < IR_LIST_MAX;
    if (ok) ok = slot < rdList[IR_LIST_INTS * (size_t)t.list_row];
    if (ok)
    {
      const int c = rdList[IR_LIST_INTS * (size_t)t.list_row + 1 + slot];
      ok = c >= 0 && c < IR_LIST_MAX;
      predOff += (long long)c * t.pred_cand_pitch;
    }
  }
  return ok;
}

// The wavefront's tile: orgResi at 0; behind it the prediction (ir_tile_pred) and -- up to 1024 samples -- the place where the body leaves resi'
// (ir_tile_back), so that resi' returns through LDS instead of through a store, a fence and a load.  A shape with a side of at most 8 (narrow: w <= 8 ||
// h <= 8, at most 512 samples) also has the integer body's two buffers there, at 1024 and 2048.  64 x 64 fills the tile: its prediction is read again
// behind the body (null), and 2048 samples and more return resi' through the candidate buffer (null).  (Two functions of the caller's narrow and
// samples, not one of w and h that returns both: only so the kernels' instruction streams stay what they were, docs/MEASUREMENTS.md.)
__device__ __forceinline__ short* ir_tile_pred(short* resiT, bool narrow, int samples) { return samples > 2048 ? nullptr : resiT + (narrow ? 512 : samples <= 1024 ? 1024 : 2048); }
__device__ __forceinline__ short* ir_tile_back(short* resiT, bool narrow, int samples) { return narrow ? resiT + 3072 : samples <= 1024 ? resiT + 2048 : nullptr; }

// orgResi = org - pred into the tile (and the prediction into predT, if there is room for it) -> zero_dist: sum orgResi^2 over the wavefront
__device__ __forceinline__ unsigned long long ir_stage(const IrItem& t, const Pel* __restrict__ org, const Pel* __restrict__ predG, short* resiT, short* predT, int lane)
{
  const int w = t.w, samples = w * t.h, lw = ilog2(w);
  unsigned long long zd = 0ull;
  for (int e0 = lane; e0 < samples; e0 += 256)                             // four loads of each plane in flight: the item waits for one round trip per 256 samples
  {
    int ov[4], pv[4];
#pragma unroll
    for (int u = 0; u < 4; u++)
    {
      const int e = e0 + 64 * u, r = e >> lw, x = e & (w - 1);
      ov[u] = pv[u] = 0;
      if (e < samples) { pv[u] = predG[(ptrdiff_t)r * t.pred_stride + x]; ov[u] = org[(ptrdiff_t)r * t.org_stride + x]; }
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
    {
      const int e = e0 + 64 * u, df = ov[u] - pv[u];
      if (e < samples)
      {
        resiT[e] = (short)df;
        if (predT) predT[e] = (short)pv[u];
      }
      const unsigned ad = (unsigned)abs(df);
      zd += (unsigned long long)(ad * ad);
    }
  }
  return group_sum<64>(zd);
}

// The closing loop of slot k: xGetSSE(orgResi, resi') and xGetSSE(org, clip(pred + resi')) from resi' where the body left it -- backK in the tile, or the
// slot's candidate buffer (backK null); resi' (from backK) and the reconstruction go to the candidate buffers on the way.  The kernels call it through a
// lambda finish(k, backK) that binds the item's values: whether the loop is inlined at a call is then the compiler's choice, as it was for
// inter_resi_code_kernel's lambda before, and both kernels measured no slower that way (docs/MEASUREMENTS.md).
template <class Args>
__device__ __forceinline__ void ir_finish(const Args& a, const IrItem& t, int item, int k, const short* resiT, const short* predT, const Pel* predG,
                                          const short* backK, int lane)
{
  const int w = t.w, lw = ilog2(w), samples = w * t.h;
  const size_t out = IR_SLOTS * (size_t)item + k;
  const long long candOff = t.cand_off + (long long)k * samples;
  Pel* rs = a.resi + candOff;
  Pel* rec = a.writeRec ? a.rec + candOff : nullptr;
  unsigned long long dr = 0ull, dc = 0ull;                                // 64 x 64 x 1023^2 is beyond 2^31
  for (int e = lane; e < samples; e += 64)
  {
    int r2;
    if (backK) { r2 = backK[e]; rs[e] = (short)r2; }
    else r2 = rs[e];
    const int o = resiT[e], pv = predT ? (int)predT[e] : (int)predG[(ptrdiff_t)(e >> lw) * t.pred_stride + (e & (w - 1))];
    const int rc = clip3(a.cmin, a.cmax, pv + r2);
    const unsigned d1 = (unsigned)abs(o - r2), d2 = (unsigned)abs(o + pv - rc);
    dr += (unsigned long long)(d1 * d1);
    dc += (unsigned long long)(d2 * d2);
    if (rec) rec[e] = (short)rc;
  }
  dr = group_sum<64>(dr);
  dc = group_sum<64>(dc);
  if (lane == 0) { a.distResi[out] = dr; a.distRec[out] = dc; }
}

// ---- host side of the two entries.  `name` is the entry's name as the error text starts with it; a check returns VVCGPU_OK or the error code with the
// text set.  An entry calls ir_check_frame, returns for n == 0, makes its own checks, then ir_check_bit_depth: the order in which a call with several
// faults reports them.
// (known: the flag bits the entry knows -- VVCGPU_INTER_RESI_DQ_TS is the DepQuant entry's alone)
inline int ir_check_frame(const char* name, int n, bool pointers, int flags, const void* rec_base, int clp_min, int clp_max, int known = VVCGPU_INTER_RESI_WRITE_REC)
{
  VVC_CHECK_ARG(n >= 0, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;                                           // (nothing else is looked at)
  VVC_CHECK_ARG(pointers, "%s: null pointer", name);
  VVC_CHECK_ARG((flags & ~known) == 0, "%s: unknown flags 0x%x", name, flags);
  VVC_CHECK_ARG(rec_base || !(flags & VVCGPU_INTER_RESI_WRITE_REC), "%s: null pointer (rec_base with VVCGPU_INTER_RESI_WRITE_REC)", name);
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "%s: clip range %d..%d", name, clp_min, clp_max);
  return VVCGPU_OK;
}
inline int ir_check_bit_depth(const char* name, int bit_depth)
{
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("%s: bit depth %d outside 8..10", name, bit_depth); return VVCGPU_E_UNSUPPORTED; }
  return VVCGPU_OK;
}
// IR_FB_INTS of global scratch for each wavefront of the persistent workgroups
inline int* ir_fb_scratch(VvcScratch& sc, int wgs) { return sc.take<int>((size_t)wgs * IR_WAVES * IR_FB_INTS); }

}  // namespace
