// intratu.hip -- vvcgpu_intra_tu_code_batch: the pixel pass of the intra RD loop for a list of independent luma TUs, in one launch.
//
// Reference behaviour reproduced (bit-exact):
//   IntraSearch::xIntraCodingTUBlock                                                            EncoderLib/IntraSearch.cpp:1147-1316
//     predIntraAng (through intra_dev.h), org - pred, transformNxN, the numSig count :1257-1280, invTransformNxN, reconstruct (the residual chain of
//     resichain.hip, through resichain_dev.h), getDistPart(DF_SSE) = RdCost::xGetSSE
//   IntraPrediction::useFilteredIntraRefSamples(.., modeSpecific = true, ..) for a mode taken from a list (intra_dev.h)
//
// Design (docs/KERNELS.md, "The intra RD loop's pixel pass"): persistent workgroups of four wavefronts, each wavefront takes an item (the pair preds[i],
// tus[i]) and dispatches on its shape.  The prediction is formed in the wavefront's LDS tile (a given prediction is copied there) and is the `pred` operand
// of the chain body: it never goes through HBM, and reaches pred_base only under VVCGPU_INTRA_TU_WRITE_PRED.  Sides of 16 / 32 / 64 run the single-wave
// matrix-core body of the chain (rc_tu_mfma) as a real call per shape, so the kernel's register need is the largest body's; a shape with a side of 4 or 8
// runs the chain's integer body (rc_tu_generic) with its two buffers in the unused part of the tile.  Behind the chain body the wavefront reads back what
// it has just written -- the reconstruction against the original for the SSE, the kept region of the levels for num_sig -- while both are still in the
// caches; nothing is a separate launch.
#include "common.h"
#include "dist_dev.h"
#include "intra_dev.h"
#include "intratu_dev.h"
#include "mfma_tr.h"
#include "quant_dev.h"
#include "resichain_dev.h"

static_assert(sizeof(vvcgpu_intra_desc) == 32 && sizeof(vvcgpu_resi_chain_desc) == 64, "descriptor layouts");

namespace {

constexpr int IT_WGS_PER_CU = 2;
constexpr int IT_LDS_BYTES = IT_TAB_BYTES + 4 * IT_WAVE_BYTES;            // 79 296 bytes: two workgroups per compute unit
static_assert(IT_WGS_PER_CU * IT_LDS_BYTES <= 160 * 1024, "LDS budget");

struct ItArgs
{
  const Pel* refs; const vvcgpu_intra_desc* preds; const Pel* org; Pel* pred; Pel* rec; TCoeff* level; const RcDesc* tus; const int* modeList;
  unsigned* absSum; unsigned* numSig; unsigned long long* dist; int* modeOut; int* fbScratch; const _Float16* image;
  int n, writePred, noSmoothing, bd, cmin, cmax;
};

// the matrix-core body of one shape as a real call (the descriptor and the tile are the wavefront's, in LDS)
template <int W, int H>
__device__ __noinline__ bool it_tu_mfma_call(const RcDesc* dS, const Pel* __restrict__ orgBase, const Pel* tile, Pel* __restrict__ recBase, TCoeff* __restrict__ levelBase,
                                             unsigned* __restrict__ absSumItem, int bd, int clpMin, int clpMax, const _Float16* tab,
                                             const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int lane)
{
  RC_IS_LDS(dS); RC_IS_LDS(tile); RC_IS_LDS(tab);
  return rc_tu_mfma<W, H, RC_CHAIN>(*dS, orgBase, tile, recBase, levelBase, absSumItem, 0, bd, clpMin, clpMax, tab, dqInv, scanOff, lane);
}
// the integer body: a shape with a side of 4 or 8 (buffers of 512 ints in the tile), or an item whose residual leaves +-1023 (buffers of 4096 ints in global scratch)
__device__ __noinline__ void it_tu_generic_call(const RcDesc* dS, const Pel* __restrict__ orgBase, const Pel* tile, Pel* __restrict__ recBase, TCoeff* __restrict__ levelBase,
                                                unsigned* __restrict__ absSumItem, int bd, int clpMin, int clpMax, const int* __restrict__ tr32,
                                                const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int* bufA, int* bufB, int lane)
{
  rc_tu_generic<RC_CHAIN>(*dS, orgBase, tile, recBase, levelBase, absSumItem, 0, bd, clpMin, clpMax, tr32, dqInv, scanOff, bufA, bufB, lane, nullptr);
}

__global__ __launch_bounds__(256, IT_WGS_PER_CU) void intra_tu_code_kernel(const ItArgs a, const VvcTrTables tb)
{
  // dynamic LDS (IT_LDS_BYTES): the f16 matrices, then per wavefront the tile, the reference work arrays of intra_pred_block and the item's chain descriptor
  extern __shared__ __align__(16) unsigned char smem[];
  _Float16* const tab = reinterpret_cast<_Float16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    // (rc_load_image in words: as a call of it the kernel's first instructions come out in another order, docs/MEASUREMENTS.md)
    constexpr int NW4 = RC_TAB_HALVES / 8;
    const uint4* src = reinterpret_cast<const uint4*>(a.image);
    for (int i = tid; i < NW4; i += 256) reinterpret_cast<uint4*>(tab)[i] = src[i];
  }
  __syncthreads();                                                        // the only workgroup barrier: below every wavefront walks its own items
  const ItLds l = it_lds(smem, wave);
  short* const tile = l.tile;
  RcDesc* const dS = l.dS;
  int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * 4 + wave) * IT_FB_INTS;

  for (int item = (int)blockIdx.x * 4 + wave; item < a.n; item += (int)gridDim.x * 4)
  {
    const vvcgpu_intra_desc p = a.preds[item];
    const RcDesc t = a.tus[item];
    int mode; bool filt;
    if (!it_resolve(a, p, t, [] { return true; }, mode, filt)) { it_mark(a, item, lane); continue; }
    const int w = t.w, h = t.h, lw = ilog2(w), samples = w * h;
    it_predict(a, p, t, mode, filt, l, lane);
    if (a.writePred && mode >= 0)
    {
      Pel* dst = a.pred + t.pred_off;
      for (int e = lane; e < samples; e += 64) dst[(ptrdiff_t)(e >> lw) * t.pred_stride + (e & (w - 1))] = tile[e];
    }
    if (lane == 0)
    {
      RcDesc u = t;
      u.pred_off = 0; u.pred_stride = w;                                  // the chain's `pred` operand is the tile
      *dS = u;
      a.modeOut[item] = mode < 0 ? -1 : mode;
    }
    wave_sync();

    // ---- the residual chain
    bool done = true;
#define IT_MF(W_, H_) case ((W_) << 8) | (H_): \
      done = it_tu_mfma_call<W_, H_>(dS, a.org, tile, a.rec, a.level, a.absSum + item, a.bd, a.cmin, a.cmax, tab, tb.dqInv, tb.scanOff, lane); break;
    if (w <= 8 || h <= 8)                                                 // a side of 4 or 8: at most 512 samples, the buffers lie behind them in the tile
      it_tu_generic_call(dS, a.org, tile, a.rec, a.level, a.absSum + item, a.bd, a.cmin, a.cmax, tb.tr32, tb.dqInv, tb.scanOff,
                         reinterpret_cast<int*>(tile + 1024), reinterpret_cast<int*>(tile + 2048), lane);
    else switch ((w << 8) | h)
    {
    IT_MF(16, 16) IT_MF(16, 32) IT_MF(16, 64) IT_MF(32, 16) IT_MF(32, 32) IT_MF(32, 64) IT_MF(64, 16) IT_MF(64, 32) IT_MF(64, 64)
    default: break;
    }
#undef IT_MF
    if (!done)                                                            // samples outside the bit depth (out of contract): exact all the same
      it_tu_generic_call(dS, a.org, tile, a.rec, a.level, a.absSum + item, a.bd, a.cmin, a.cmax, tb.tr32, tb.dqInv, tb.scanOff, fbScr, fbScr + 4096, lane);

    // ---- what the wavefront has just written, read back: xGetSSE(org, rec) and the non-zero levels of the kept region
    wave_global_sync();
    {
      const Pel* org = a.org + t.org_off;
      const Pel* rec = a.rec + t.rec_off;
      unsigned long long sse = 0ull;                                      // 64 x 64 x 1023^2 is beyond 2^31
      for (int e = lane; e < samples; e += 64)
      {
        const int r = e >> lw, x = e & (w - 1);
        const int df = (int)org[(ptrdiff_t)r * t.org_stride + x] - (int)rec[(ptrdiff_t)r * t.rec_stride + x];
        sse += (unsigned long long)(unsigned)(df * df);
      }
      const TCoeff* level = a.level + t.level_off;
      const int wj = min(w, 32), hj = min(h, 32), lwj = ilog2(wj);
      int nz = 0;
      for (int e = lane; e < wj * hj; e += 64) nz += level[(e >> lwj) * w + (e & (wj - 1))] != 0;
      sse = group_sum<64>(sse);
      nz = wave_sum(nz);
      if (lane == 0) { a.dist[item] = sse; a.numSig[item] = (unsigned)nz; }
    }
    wave_sync();                                                          // the tile and the descriptor are free again
  }
}

}  // namespace

extern "C" int vvcgpu_intra_tu_code_batch(const vvc_pel* refs_base, const vvcgpu_intra_desc* preds, const vvc_pel* org_base, vvc_pel* pred_base, vvc_pel* rec_base,
                                          vvc_coef* level_base, const vvcgpu_resi_chain_desc* tus, int n, const int32_t* mode_list, int flags, int bit_depth,
                                          int clp_min, int clp_max, uint32_t* abs_sum, uint32_t* num_sig, uint64_t* dist, int32_t* mode_out, void* stream)
{
  const char* name = "intra_tu_code_batch";
  VVC_CHECK_ARG(n >= 0, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(refs_base && preds && org_base && rec_base && level_base && tus && abs_sum && num_sig && dist && mode_out, "%s: null pointer", name);
  VVC_CHECK_ARG((flags & ~(VVCGPU_INTRA_TU_WRITE_PRED | VVCGPU_INTRA_TU_NO_SMOOTHING)) == 0, "%s: unknown flags 0x%x", name, flags);
  VVC_CHECK_ARG(pred_base || !(flags & VVCGPU_INTRA_TU_WRITE_PRED), "%s: null pointer (pred_base with VVCGPU_INTRA_TU_WRITE_PRED)", name);
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "%s: clip range %d..%d", name, clp_min, clp_max);
  VVC_CHECK_ARG(((uintptr_t)preds & 15) == 0 && ((uintptr_t)tus & 15) == 0, "%s: descriptor array must be 16-byte aligned", name);
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("%s: bit depth %d outside 8..10", name, bit_depth); return VVCGPU_E_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  VvcTrTables tb; const _Float16* image = nullptr;
  const int rt = vvcgpu_tr_images(&tb, &image);
  if (rt) return rt;
  const int wgs = vvc_grid_cap(n, 4, IT_WGS_PER_CU);
  VvcScratch sc(st);
  int* fbScratch = sc.take<int>((size_t)wgs * 4 * IT_FB_INTS);            // touched only for an item outside the matrix-core range
  if (!fbScratch) return VVCGPU_E_DEVICE;
  ItArgs a;
  a.refs = refs_base; a.preds = preds; a.org = org_base; a.pred = pred_base; a.rec = rec_base; a.level = level_base; a.tus = tus; a.modeList = mode_list;
  a.absSum = abs_sum; a.numSig = num_sig; a.dist = reinterpret_cast<unsigned long long*>(dist); a.modeOut = mode_out; a.fbScratch = fbScratch; a.image = image;
  a.n = n; a.writePred = (flags & VVCGPU_INTRA_TU_WRITE_PRED) ? 1 : 0; a.noSmoothing = (flags & VVCGPU_INTRA_TU_NO_SMOOTHING) ? 1 : 0;
  a.bd = bit_depth; a.cmin = clp_min; a.cmax = clp_max;
  VVC_HIP(vvc_allow_lds(intra_tu_code_kernel, IT_LDS_BYTES));
  hipLaunchKernelGGL(intra_tu_code_kernel, dim3(wgs), dim3(256), IT_LDS_BYTES, st, a, tb);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
