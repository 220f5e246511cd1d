// intrachroma.hip -- vvcgpu_intra_chroma_code_batch: the pixel work of the intra chroma mode loop for a list of independent chroma PUs grouped by shape.
//
// Reference behaviour reproduced (bit-exact):
//   IntraSearch::estIntraPredChromaQT, the mode loop                                             EncoderLib/IntraSearch.cpp:704-852
//     xRecurIntraChromaCodingQT :1657-1843 = xIntraCodingTUBlock :1147-1316 for Cb and for Cr: initIntraPatternChType (xFillReferenceSamples,
//     CommonLib/IntraPrediction.cpp:807-1004), predIntraAng :251-354 from unfiltered references (useFilteredIntraRefSamples :1114), or xGetLumaRecPixels
//     :1283-1581 + xGetLMParameters :1597-1857 + predIntraChromaLM :390-403 (all through intra_dev.h), then org - pred, transformNxN, invTransformNxN,
//     reconstruct (the residual chain, through resichain_dev.h) and getDistPart(DF_SSE) = RdCost::xGetSSE
//
// Design (docs/KERNELS.md, "The intra chroma mode pass"): a wavefront owns a PU.  It stages the down-sampled luma block with its neighbour line and
// column once per PU, and once per component the references (gathered or given) and the original block; then it walks the six slots from LDS: the
// prediction is formed in the wavefront's tile and is the `pred` operand of the chain body, it reaches pred_base only under WRITE_PRED.  The shape runs
// let the host pick the kernel: chroma_small_kernel (both sides <= 16, nearly all of chroma) carries only the integer chain body, its two buffers, its
// reconstruction and the DCT-II matrices up to 16 points in LDS -- the SSE comes from LDS, nothing is read back; chroma_large_kernel (a side of 32 or
// 64) is persistent, carries the f16 matrices and runs the single-wave matrix-core bodies as real calls, as intra_tu_code_kernel does.
#include "common.h"
#include "dist_dev.h"
#include "intra_dev.h"
#include "intrachroma_dev.h"
#include "mfma_tr.h"
#include "quant_dev.h"
#include "resichain_dev.h"

static_assert(sizeof(vvcgpu_intra_chroma_pu) == 96 && sizeof(vvcgpu_intra_fill_desc) == 40, "descriptor layouts");

namespace {

__device__ __forceinline__ RcDesc ch_chain_desc(const ChPu& u, int c, int w, int h, int64_t recOff, int64_t levelOff)
{
  RcDesc d;
  d.org_off = 0; d.pred_off = 0; d.rec_off = recOff; d.level_off = levelOff;                // the original and the prediction are the wavefront's LDS blocks
  d.org_stride = w; d.pred_stride = w; d.rec_stride = w; d.w = (int16_t)w; d.h = (int16_t)h;
  d.tr_hor = 0; d.tr_ver = 0; d.intra_slice = u.intra_slice; d.sign_hiding = u.sign_hiding; d.qp = CH_SEL(qp, c);
  d.reserved[0] = 0; d.reserved[1] = 0;
  return d;
}

// ---------------------------------------------------------------------------------------------------
// both sides <= 16: at most 256 samples, an 8 x 8 block is one sample per lane
constexpr int CS_SIDE = 16, CS_TILE = CS_SIDE * CS_SIDE, CS_REF = 40, CS_NEG = 16;            // T, L <= 32 (16 x 16, 16 x 2); a side reference of at most 2 * 16 + 1
constexpr int CS_TAB_INTS = 340;                                                            // DCT-II 2, 4, 8, 16: the head of tr32's first type
struct CsWave
{
  int bufA[CS_TILE], bufB[CS_TILE];                                                           // the chain body's two buffers; bufA also holds the unit table of the gathering
  short lumaS[CS_TILE], orgS[CS_TILE], tile[CS_TILE], recS[CS_TILE];
  short top[CS_REF], left[CS_REF], packed[2 * CS_REF], mainX[CS_NEG + CS_REF], lumaTop[CS_SIDE], lumaLeft[CS_SIDE];
  RcDesc d;                                                                                   // the item's chain descriptor
};
static_assert(sizeof(CsWave) % 16 == 0 && CS_TILE * 4 >= FILL_UNITS_MAX * 2, "LDS layout");

// the integer chain body as a real call: the kernel's register need is this body's, not the sum of what is live across it
__device__ __noinline__ void cs_tu_call(const RcDesc* dS, const Pel* orgS, const Pel* tile, Pel* recS, TCoeff* __restrict__ levelBase, unsigned* __restrict__ absSumItem,
                                        int bd, int clpMin, int clpMax, const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int* bufA, int* bufB,
                                        int lane, const int* tabL)
{
  RC_IS_LDS(dS); RC_IS_LDS(orgS); RC_IS_LDS(tile); RC_IS_LDS(recS); RC_IS_LDS(bufA); RC_IS_LDS(bufB); RC_IS_LDS(tabL);
  rc_tu_generic<RC_CHAIN>(*dS, orgS, tile, recS, levelBase, absSumItem, 0, bd, clpMin, clpMax, nullptr, dqInv, scanOff, bufA, bufB, lane, tabL);
}

__global__ __launch_bounds__(256) void chroma_small_kernel(const ChArgs a, const VvcTrTables tb)
{
  __shared__ __align__(16) int tabL[CS_TAB_INTS];
  __shared__ __align__(16) CsWave waves[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < CS_TAB_INTS; i += 256) tabL[i] = tb.tr32[i];
  __syncthreads();                                                        // the only workgroup barrier
  const int q = (int)blockIdx.x * 4 + wave;                                 // wave-uniform, as `wave` is
  if (q >= a.total) return;
  CsWave& S = waves[wave];
  int rw, rh;
  const int p = ch_locate(a, q, rw, rh);
  const ChPu u = a.pus[p];
  bool anyLm;
  if (!ch_pu_ok(a, u, p, rw, rh, anyLm) || rw > CS_SIDE || rh > CS_SIDE) { ch_mark(a, p, 0, CH_SLOTS, -1, lane); return; }
  const int w = u.w, h = u.h, samples = w * h, lw = ilog2(w);
  const bool aboveAvail = u.above_avail != 0, leftAvail = u.left_avail != 0;
  int T, L;
  intra_ref_lengths(w, h, T, L);
  if (anyLm) ch_stage_luma(a.luma + u.luma_off, u.luma_stride, w, h, aboveAvail, leftAvail, lane, S.lumaS, S.lumaTop, S.lumaLeft);

#pragma nounroll
  for (int c = 0; c < 2; c++)
  {
    ch_stage_refs(a, u, p, c, T, L, lane, S.packed, reinterpret_cast<short*>(S.bufA), S.top, S.left);
    {
      const Pel* org = a.org + CH_SEL(org_off, c);
      for (int e = lane; e < samples; e += 64) S.orgS[e] = org[(ptrdiff_t)(e >> lw) * u.org_stride + (e & (w - 1))];
    }
    wave_sync();
    int lmA = 0, lmB = 0, lmShift = 0;
    if (anyLm)
      cclm_params(w, h, aboveAvail, leftAvail, [&](int i) { return (int)S.lumaTop[i]; }, [&](int i) { return (int)S.lumaLeft[i]; }, S.top + 1, S.left + 1,
                  a.bd, a.bd, lane, lmA, lmB, lmShift);
#pragma nounroll
    for (int k = 0; k < CH_SLOTS; k++)
    {
      const int mode = ch_mode(u, k);
      if (mode < 0) { ch_mark(a, p, k, k + 1, c, lane); continue; }
      const size_t item = 12 * (size_t)p + 2 * k + c;
      const int64_t off = (int64_t)(2 * k + c) * samples;
      ch_predict(mode, w, h, T, L, S.top, S.left, S.mainX + CS_NEG, S.lumaS, lmA, lmB, lmShift, a.cmin, a.cmax, lane, S.tile);
      if (a.writePred) { Pel* dst = a.pred + u.cand_off + off; for (int e = lane; e < samples; e += 64) dst[e] = S.tile[e]; }
      if (lane == 0) S.d = ch_chain_desc(u, c, w, h, 0, u.level_off + off);                 // the reconstruction stays in LDS
      wave_sync();
      cs_tu_call(&S.d, S.orgS, S.tile, S.recS, a.level, a.absSum + item, a.bd, a.cmin, a.cmax, tb.dqInv, tb.scanOff, S.bufA, S.bufB, lane, tabL);
      Pel* rec = a.candRec + u.cand_off + off;
      unsigned sse = 0u;                                                  // 256 x 1023^2 < 2^32
      for (int e = lane; e < samples; e += 64)
      {
        const int r = S.recS[e], df = (int)S.orgS[e] - r;
        rec[e] = (Pel)r;
        sse += (unsigned)(df * df);
      }
      const unsigned long long total = group_sum<64>((unsigned long long)sse);
      if (lane == 0) a.dist[item] = total;
      wave_sync();                                                        // the tile, the buffers and the reconstruction are free again
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// a side of 32 or 64: persistent workgroups of four wavefronts, the single-wave matrix-core bodies as real calls (as intra_tu_code_kernel)
constexpr int CL_TILE = 64 * 64;
constexpr int CL_TAB_BYTES = RC_TAB_HALVES * 2;
constexpr int CL_WAVE_BYTES = (3 * CL_TILE + 2 * REF_MAX + NEG_MAX + REF_MAX + 2 * 64) * 2 + (int)sizeof(RcDesc);
constexpr int CL_LDS_BYTES = CL_TAB_BYTES + 4 * CL_WAVE_BYTES;                                // one workgroup per compute unit
static_assert(CL_TAB_BYTES % 16 == 0 && CL_WAVE_BYTES % 16 == 0 && CL_LDS_BYTES <= 160 * 1024 && (NEG_MAX + REF_MAX) >= FILL_UNITS_MAX, "LDS budget");

template <int W, int H>
__device__ __noinline__ bool ch_tu_mfma_call(const RcDesc* dS, const Pel* orgS, const Pel* tile, Pel* __restrict__ recBase, TCoeff* __restrict__ levelBase,
                                             unsigned* __restrict__ absSumItem, int bd, int clpMin, int clpMax, const _Float16* tab,
                                             const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int lane)
{
  RC_IS_LDS(dS); RC_IS_LDS(orgS); RC_IS_LDS(tile); RC_IS_LDS(tab);
  return rc_tu_mfma<W, H, RC_CHAIN>(*dS, orgS, tile, recBase, levelBase, absSumItem, 0, bd, clpMin, clpMax, tab, dqInv, scanOff, lane);
}
// the integer body: a short side of 2, 4 or 8 (buffers of 512 ints in the tile), or an item whose residual leaves +-1023 (buffers of 4096 ints in global scratch)
__device__ __noinline__ void ch_tu_generic_call(const RcDesc* dS, const Pel* orgS, const Pel* tile, Pel* __restrict__ recBase, TCoeff* __restrict__ levelBase,
                                                unsigned* __restrict__ absSumItem, int bd, int clpMin, int clpMax, const int* __restrict__ tr32,
                                                const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int* bufA, int* bufB, int lane)
{
  RC_IS_LDS(dS); RC_IS_LDS(orgS); RC_IS_LDS(tile);
  rc_tu_generic<RC_CHAIN>(*dS, orgS, tile, recBase, levelBase, absSumItem, 0, bd, clpMin, clpMax, tr32, dqInv, scanOff, bufA, bufB, lane, nullptr);
}

__global__ __launch_bounds__(256, 1) void chroma_large_kernel(const ChArgs a, const VvcTrTables tb)
{
  // dynamic LDS (CL_LDS_BYTES): the f16 matrices, then per wavefront the tile, the luma block, the original block, top / left, the main reference buffer
  // (also the unit table of the gathering), the luma neighbours and the item's chain descriptor; the packed references of the gathering lie in the tile
  extern __shared__ __align__(16) unsigned char smem[];
  _Float16* const tab = reinterpret_cast<_Float16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    // (rc_load_image in words: as a call of it the kernel's first instructions come out in another order, docs/MEASUREMENTS.md)
    constexpr int NW4 = RC_TAB_HALVES / 8;
    const uint4* src = reinterpret_cast<const uint4*>(a.image);
    for (int i = tid; i < NW4; i += 256) reinterpret_cast<uint4*>(tab)[i] = src[i];
  }
  __syncthreads();                                                        // the only workgroup barrier: below every wavefront walks its own PUs
  unsigned char* const mine = smem + CL_TAB_BYTES + (size_t)wave * CL_WAVE_BYTES;
  short* const tile = reinterpret_cast<short*>(mine);
  short* const lumaS = tile + CL_TILE;
  short* const orgS = lumaS + CL_TILE;
  short* const topS = orgS + CL_TILE;
  short* const leftS = topS + REF_MAX;
  short* const mainS = leftS + REF_MAX;
  short* const lumaTop = mainS + NEG_MAX + REF_MAX;
  short* const lumaLeft = lumaTop + 64;
  RcDesc* const dS = reinterpret_cast<RcDesc*>(mine + CL_WAVE_BYTES - sizeof(RcDesc));
  int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * 4 + wave) * 8192;

  for (int q = (int)blockIdx.x * 4 + wave; q < a.total; q += (int)gridDim.x * 4)
  {
    int rw, rh;
    const int p = ch_locate(a, q, rw, rh);
    const ChPu u = a.pus[p];
    bool anyLm;
    if (!ch_pu_ok(a, u, p, rw, rh, anyLm)) { ch_mark(a, p, 0, CH_SLOTS, -1, lane); continue; }
    const int w = u.w, h = u.h, samples = w * h, lw = ilog2(w);
    const bool aboveAvail = u.above_avail != 0, leftAvail = u.left_avail != 0;
    int T, L;
    intra_ref_lengths(w, h, T, L);
    if (anyLm) ch_stage_luma(a.luma + u.luma_off, u.luma_stride, w, h, aboveAvail, leftAvail, lane, lumaS, lumaTop, lumaLeft);

#pragma nounroll
    for (int c = 0; c < 2; c++)
    {
      ch_stage_refs(a, u, p, c, T, L, lane, tile, mainS, topS, leftS);
      {
        const Pel* org = a.org + CH_SEL(org_off, c);
        for (int e = lane; e < samples; e += 64) orgS[e] = org[(ptrdiff_t)(e >> lw) * u.org_stride + (e & (w - 1))];
      }
      wave_sync();
      int lmA = 0, lmB = 0, lmShift = 0;
      if (anyLm)
        cclm_params(w, h, aboveAvail, leftAvail, [&](int i) { return (int)lumaTop[i]; }, [&](int i) { return (int)lumaLeft[i]; }, topS + 1, leftS + 1,
                    a.bd, a.bd, lane, lmA, lmB, lmShift);
#pragma nounroll
      for (int k = 0; k < CH_SLOTS; k++)
      {
        const int mode = ch_mode(u, k);
        if (mode < 0) { ch_mark(a, p, k, k + 1, c, lane); continue; }
        const size_t item = 12 * (size_t)p + 2 * k + c;
        const int64_t off = (int64_t)(2 * k + c) * samples;
        ch_predict(mode, w, h, T, L, topS, leftS, mainS + NEG_MAX, lumaS, lmA, lmB, lmShift, a.cmin, a.cmax, lane, tile);
        if (a.writePred) { Pel* dst = a.pred + u.cand_off + off; for (int e = lane; e < samples; e += 64) dst[e] = tile[e]; }
        if (lane == 0) *dS = ch_chain_desc(u, c, w, h, u.cand_off + off, u.level_off + off);
        wave_sync();

        bool done = true;
#define CH_MF(W_, H_) case ((W_) << 8) | (H_): \
        done = ch_tu_mfma_call<W_, H_>(dS, orgS, tile, a.candRec, a.level, a.absSum + item, a.bd, a.cmin, a.cmax, tab, tb.dqInv, tb.scanOff, lane); break;
        if (w <= 8 || h <= 8)                                             // at most 512 samples: the buffers lie behind them in the tile
          ch_tu_generic_call(dS, orgS, tile, a.candRec, a.level, a.absSum + item, a.bd, a.cmin, a.cmax, tb.tr32, tb.dqInv, tb.scanOff,
                             reinterpret_cast<int*>(tile + 1024), reinterpret_cast<int*>(tile + 2048), lane);
        else switch ((w << 8) | h)
        {
        CH_MF(16, 32) CH_MF(16, 64) CH_MF(32, 16) CH_MF(32, 32) CH_MF(32, 64) CH_MF(64, 16) CH_MF(64, 32) CH_MF(64, 64)
        default: break;
        }
#undef CH_MF
        if (!done)                                                        // samples outside the bit depth (out of contract): exact all the same
          ch_tu_generic_call(dS, orgS, tile, a.candRec, a.level, a.absSum + item, a.bd, a.cmin, a.cmax, tb.tr32, tb.dqInv, tb.scanOff, fbScr, fbScr + 4096, lane);

        // ---- the reconstruction the wavefront has just written, read back against the staged original: xGetSSE(org, rec)
        wave_global_sync();
        {
          const Pel* rec = a.candRec + u.cand_off + off;
          unsigned long long sse = 0ull;                                  // 64 x 64 x 1023^2 is beyond 2^31
          for (int e = lane; e < samples; e += 64) { const int df = (int)orgS[e] - (int)rec[e]; sse += (unsigned long long)(unsigned)(df * df); }
          sse = group_sum<64>(sse);
          if (lane == 0) a.dist[item] = sse;
        }
        wave_sync();                                                      // the tile and the descriptor are free again
      }
    }
  }
}

}  // namespace

extern "C" int vvcgpu_intra_chroma_code_batch(const vvc_pel* rec_base, const uint8_t* flags_base, const vvcgpu_intra_fill_desc* fill, vvc_pel* refs_base,
                                              const vvc_pel* luma_base, const vvc_pel* org_base, const vvcgpu_intra_chroma_pu* pus, int n,
                                              const int32_t* runs_host, int n_runs, vvc_pel* pred_base, vvc_pel* cand_rec_base, vvc_coef* level_base,
                                              int flags, int bit_depth, int clp_min, int clp_max, uint32_t* abs_sum, uint64_t* dist, void* stream)
{
  const char* name = "intra_chroma_code_batch";
  VVC_CHECK_ARG(n >= 0, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org_base && pus && runs_host && cand_rec_base && level_base && abs_sum && dist, "%s: null pointer", name);
  VVC_CHECK_ARG((fill != nullptr) == (rec_base != nullptr) && (fill != nullptr) == (flags_base != nullptr), "%s: fill, rec_base and flags_base go together", name);
  VVC_CHECK_ARG(fill || refs_base, "%s: neither fill nor refs_base", name);
  VVC_CHECK_ARG((flags & ~VVCGPU_INTRA_CHROMA_WRITE_PRED) == 0, "%s: unknown flags 0x%x", name, flags);
  VVC_CHECK_ARG(pred_base || !(flags & VVCGPU_INTRA_CHROMA_WRITE_PRED), "%s: null pointer (pred_base with VVCGPU_INTRA_CHROMA_WRITE_PRED)", name);
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "%s: clip range %d..%d", name, clp_min, clp_max);
  VVC_CHECK_ARG(((uintptr_t)pus & 15) == 0 && ((uintptr_t)fill & 15) == 0, "%s: descriptor array must be 16-byte aligned", name);
  VVC_CHECK_ARG(n_runs >= 1, "%s: n_runs %d", name, n_runs);
  // the runs by shape class: both sides <= 16, a side of 32 or 64
  ChArgs cls[2];
  cls[0].nSeg = cls[1].nSeg = 0; cls[0].total = cls[1].total = 0;
  long long sum = 0;
  unsigned long long seenShapes = 0ull;
  for (int r = 0; r < n_runs; r++)
  {
    const int w = runs_host[3 * r], h = runs_host[3 * r + 1], count = runs_host[3 * r + 2];
    VVC_CHECK_ARG(count >= 0 && side_ok(w, 2) && side_ok(h, 2), "%s: run %d (%d x %d, %d PUs)", name, r, w, h, count);
    VVC_CHECK_ARG(sum + count <= n, "%s: the runs hold more than n = %d PUs", name, n);
    if (count == 0) continue;
    int lw = 0, lh = 0; while ((1 << lw) < w) lw++; while ((1 << lh) < h) lh++;
    const unsigned long long bit = 1ull << (8 * lw + lh);
    VVC_CHECK_ARG(!(seenShapes & bit), "%s: shape %d x %d appears in two runs", name, w, h);
    seenShapes |= bit;
    ChArgs& k = cls[(w > 16 || h > 16) ? 1 : 0];
    ChSeg& s = k.seg[k.nSeg++];
    s.first = (int)sum; s.count = count; s.w = (short)w; s.h = (short)h;
    k.total += count;
    sum += count;
  }
  VVC_CHECK_ARG(sum == n, "%s: the run counts sum to %lld, n is %d", name, sum, n);
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("%s: bit depth %d outside 8..10", name, bit_depth); return VVCGPU_E_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  VvcTrTables tb; const _Float16* image = nullptr;
  const int rt = vvcgpu_tr_images(&tb, &image);
  if (rt) return rt;
  const int wgsL = vvc_grid_cap(cls[1].total, 4, 1);
  VvcScratch sc(st);
  int* fbScratch = nullptr;
  if (wgsL)
  {
    fbScratch = sc.take<int>((size_t)wgsL * 4 * 8192);                    // per wavefront two 4096-int buffers, touched only for an item outside the matrix-core range
    if (!fbScratch) return VVCGPU_E_DEVICE;
  }
  for (int k = 0; k < 2; k++)
  {
    ChArgs& a = cls[k];
    a.rec = rec_base; a.flags = flags_base; a.fill = fill; a.refs = refs_base; a.luma = luma_base; a.org = org_base; a.pus = pus; a.pred = pred_base;
    a.candRec = cand_rec_base; a.level = level_base; a.absSum = abs_sum; a.dist = reinterpret_cast<unsigned long long*>(dist); a.fbScratch = fbScratch;
    a.image = image; a.writePred = (flags & VVCGPU_INTRA_CHROMA_WRITE_PRED) ? 1 : 0; a.bd = bit_depth; a.cmin = clp_min; a.cmax = clp_max;
  }
  if (cls[0].total)
  {
    hipLaunchKernelGGL(chroma_small_kernel, dim3(cdiv(cls[0].total, 4)), dim3(256), 0, st, cls[0], tb);
    VVC_LAUNCH_CHECK();
  }
  if (cls[1].total)
  {
    VVC_HIP(vvc_allow_lds(chroma_large_kernel, CL_LDS_BYTES));
    hipLaunchKernelGGL(chroma_large_kernel, dim3(wgsL), dim3(256), CL_LDS_BYTES, st, cls[1], tb);
    VVC_LAUNCH_CHECK();
  }
  return VVCGPU_OK;
}
