// affine_me.hip -- the whole affine gradient search of a PU in one launch (vvcgpu_affine_me_batch) for gfx950.
//
// Reference behaviour reproduced (bit-exact, the double arithmetic included): InterSearch::xAffineMotionEstimation (EncoderLib/InterSearch.cpp:3286-3743)
// with solveEqual (:3102-3179), InterPrediction::xPredAffineBlk (CommonLib/InterPrediction.cpp:550-722; uni-prediction, rounded and clipped, with its
// yFrac == 0 / xFrac == 0 branches), InterpolationFilter::filter / filterCopy (InterpolationFilter.cpp:205-379, m_lumaFilter :59-77), clipMv
// (Mv.cpp:64-80), Mv::roundMV2SignalPrecision (Mv.h:242-257), RdCost::getBitsOfVectorWithPredictor / getCost (RdCost.h:172-199).
//
// Design: the owner of a PU -- one wavefront up to AFI_WAVE_MAX samples, the workgroup's four above -- carries it through the whole search (the owner
// model: owner_dev.h and docs/KERNELS.md, "Owners of the whole-PU entries").  The prediction lives in LDS from the first step to the last: sixteen
// lanes interpolate one 4x4 sub-block (four per wavefront) from its 11x11 window of the reference plane straight into the tile; the error / Sobel /
// equation pass and the Hadamard distortion (afi_dev.h, shared with the per-iteration entry) read it there; the search body itself is in afm_dev.h,
// shared with the affine bi-predictive and uni-predictive entries.  The equation sums meet in LDS; every lane of the owner then solves the system and
// updates the vectors with the same (uniform) values, so nothing is broadcast.  This kernel's LDS is static: the tiles of the largest PU.
#include "common.h"
#include "dist_dev.h"
#include "afi_dev.h"
#include "afm_dev.h"
#include "raster_dev.h"
#include "pu_entry_host.h"

namespace {

template <int NT>
__device__ __forceinline__ void afm_search(const vvcgpu_affine_me_item& it, const vvcgpu_affine_me_cfg& c, const Pel* orgBase, const Pel* refBase,
                                           const AfmLds& L, vvcgpu_affine_me_result* res, vvcgpu_affine_me_step* trace, int tid)
{
  AfmPu u;
  afm_set_pu(u, it.pu.pos_x, it.pu.pos_y, it.pu.w, it.pu.h, it.pu.six_param != 0, c.pic_w, c.pic_h, c.max_cu_w, c.max_cu_h, c.bit_depth, c.clp_min, c.clp_max);
  u.os = it.org_stride; u.rs = c.ref_stride;
  u.ref = refBase + (ptrdiff_t)(u.posY + c.ref_origin_y) * c.ref_stride + u.posX + c.ref_origin_x;
  int start[3][2], mvp[3][2], best[3][2];
#pragma unroll
  for (int i = 0; i < 3; i++) { start[i][0] = it.pu.mv[0][i][0]; start[i][1] = it.pu.mv[0][i][1]; mvp[i][0] = it.mvp[i][0]; mvp[i][1] = it.mvp[i][1]; }
  unsigned bestBits, steps;
  unsigned long long bestCost;
  afm_search_body<NT, const Pel*>(u, orgBase + it.org_off, c.lambda, it.half_weight != 0, c.affine_type, it.bits, mvp, start, L, trace, tid, best, bestBits,
                                  bestCost, steps);
  if (tid == 0)
  {
#pragma unroll
    for (int i = 0; i < 3; i++) { res->mv[i][0] = best[i][0]; res->mv[i][1] = best[i][1]; }
    res->bits = bestBits; res->steps = steps; res->cost = bestCost;
    if (trace)
      for (unsigned s = steps; s < VVCGPU_AFFINE_ME_MAX_STEPS; s++) zero_record(trace + s);
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
  const OwnerSlot o = owner_slot(n, wave);                               // wave is a per-lane value here, so each kind of owner keeps its own branch:
  if (o.leave) return;                                                   // the workgroup's unit stays in scalar registers, and the item with it
  AfmLds L;
  L.tmpW = tmpL[wave]; L.red = red; L.distW = distW;
  if (o.waveOwner)
  {
    const int b = o.unit;
    const vvcgpu_affine_me_item it = items[b];
    if (!afm_item_ok(it) || it.pu.w * it.pu.h > AFI_WAVE_MAX) return;    // the workgroup owner of this item answers
    L.predL = predL + wave * AFI_WAVE_MAX; L.eq = eqL[wave];
    afm_search<64>(it, c, orgBase, refBase, L, results + b, trace ? trace + (size_t)b * VVCGPU_AFFINE_ME_MAX_STEPS : nullptr, lane);
    return;
  }
  const int b = __builtin_amdgcn_readfirstlane(o.unit);                  // the workgroup's: uniform for the compiler too
  const vvcgpu_affine_me_item it = items[b];
  vvcgpu_affine_me_step* tr = trace ? trace + (size_t)b * VVCGPU_AFFINE_ME_MAX_STEPS : nullptr;
  if (!afm_item_ok(it))                                                  // outside the contract: nothing is read or predicted
  {
    owner_write_sentinel(results + b, tr, VVCGPU_AFFINE_ME_MAX_STEPS, tid);
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
  if (const int rc = pu_check_geometry("affine_me_batch", c)) return rc;
  VVC_CHECK_ARG(c.clp_min <= c.clp_max, "affine_me_batch: clip range %d..%d", c.clp_min, c.clp_max);
  VVC_CHECK_ARG(c.lambda >= 0.0 && c.lambda < 1048576.0, "affine_me_batch: lambda out of range");
  if (c.bit_depth > 10 || c.bit_depth < 8) { vvcgpu_set_error("affine_me_batch: bit depth %d outside 8..10", c.bit_depth); return VVCGPU_E_UNSUPPORTED; }
  VVC_CHECK_ARG(n < (1 << 28), "affine_me_batch: n %d", n);
  hipLaunchKernelGGL(affine_me_kernel, dim3(pu_owner_grid(n, true)), dim3(256), 0, (hipStream_t)stream, org_base, ref_base, items, n, c, results, trace);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
