// interresi.hip -- vvcgpu_inter_resi_code_batch: the pixel pass of the inter residual RD loop for a list of independent transform blocks, in one launch.
//
// Reference behaviour reproduced (bit-exact):
//   InterSearch::encodeResAndCalcRdInterCU                                                       EncoderLib/InterSearch.cpp:4752-4909
//     orgResi = org - pred :4816-4822, the skip leg / zeroDistortion, finalDistortion = xGetSSE(org, clip(pred + resi')) :4880-4900
//   InterSearch::xEstimateInterResidualQT, "check full"                                          :4254-4634
//     transformNxN :4409, invTransformNxN :4497, currCompDist = xGetSSE(orgResi, resi') :4504, nonCoeffDist = xGetSSE(0, orgResi) :4424
//   (the residual chain of resichain.hip in its residual-domain mode RC_RESI, through resichain_dev.h)
//
// Design (docs/KERNELS.md, "The inter residual pixel pass"): persistent workgroups of eight wavefronts, each wavefront takes an item.  It stages
// orgResi = org - pred and the prediction once in its LDS tile (the only reads of the two planes for all slots; a 64 x 64 item, which fills the tile
// with orgResi, reads its prediction a second time) and sums zero_dist on the way.  orgResi is the "original" operand of the chain bodies in mode
// RC_RESI, which quantise as the chain does and leave the de-quantised residual unclipped.  4x4, 8x8, 8x4 and 4x8 run ALL transform slots of the item
// side by side in the chain's lane-group bodies (rc_small_group / rc_rect_group: one call per item); sides of 16 / 32 / 64 run the single-wave
// matrix-core body (rc_tu_mfma) as a real call per shape and slot; every other shape with a side of 2, 4 or 8, and transform skip, runs the integer
// body (rc_tu_generic) with its two buffers in the tile.  Up to 1024 samples the body leaves resi' in the tile, and the wavefront forms both
// distortions from it while it copies it (and the reconstruction, under VVCGPU_INTER_RESI_WRITE_REC) to the candidate buffers; larger blocks
// read resi' back from the candidate buffer while it is in the caches.
#include "common.h"
#include "interresi_dev.h"
#include "mfma_tr.h"
#include "quant_dev.h"

static_assert(sizeof(vvcgpu_inter_resi_item) == 80 && sizeof(vvcgpu_resi_chain_desc) == 64, "descriptor layouts");

namespace {

constexpr int IR_TAB_BYTES = RC_TAB_HALVES * 2 + (int)sizeof(RcSmallTab); // the f16 matrices, then the 4- and 8-point matrices of the lane-group bodies
constexpr int IR_WAVE_BYTES = IR_TILE * 2 + IR_SLOTS * (int)sizeof(vvcgpu_resi_chain_desc) + 32;   // the tile, a chain descriptor per slot, the slot list
constexpr int IR_LDS_BYTES = IR_TAB_BYTES + IR_WAVES * IR_WAVE_BYTES;     // 110 144 bytes: one workgroup of eight wavefronts per compute unit
static_assert(IR_TAB_BYTES % 16 == 0 && IR_WAVE_BYTES % 16 == 0 && IR_LDS_BYTES <= 160 * 1024, "LDS budget");

struct IrArgs
{
  const Pel* org; const Pel* pred; const IrItem* items; const int* rdList; Pel* resi; Pel* rec; TCoeff* level;
  unsigned* absSum; unsigned long long* distResi; unsigned long long* distRec; unsigned long long* zeroDist; int* fbScratch; const _Float16* image;
  int n, writeRec, bd, cmin, cmax;
};

// the matrix-core body of one shape as a real call (the descriptor and the residual tile are the wavefront's, in LDS)
template <int W, int H>
__device__ __noinline__ bool ir_tu_mfma_call(const RcDesc* dS, const Pel* tile, Pel* __restrict__ resiBase, TCoeff* __restrict__ levelBase,
                                             unsigned* __restrict__ absSumSlot, int bd, const _Float16* tab,
                                             const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int lane)
{
  RC_IS_LDS(dS); RC_IS_LDS(tile); RC_IS_LDS(tab);
  return rc_tu_mfma<W, H, RC_RESI>(*dS, tile, tile, resiBase, levelBase, absSumSlot, 0, bd, 0, 0, tab, dqInv, scanOff, lane);
}
// the integer body: a shape with a side of 2, 4 or 8 (buffers of 512 ints in the tile), transform skip, or an item whose residual leaves +-1023
// (buffers of 4096 ints in global scratch)
__device__ __noinline__ void ir_tu_generic_call(const RcDesc* dS, const Pel* tile, Pel* __restrict__ resiBase, TCoeff* __restrict__ levelBase,
                                                unsigned* __restrict__ absSumSlot, int bd, const int* __restrict__ tr32,
                                                const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int* bufA, int* bufB, int lane)
{
  rc_tu_generic<RC_RESI>(*dS, tile, tile, resiBase, levelBase, absSumSlot, 0, bd, 0, 0, tr32, dqInv, scanOff, bufA, bufB, lane, nullptr);
}

__global__ __launch_bounds__(IR_THREADS, 1) void inter_resi_code_kernel(const IrArgs a, const VvcTrTables tb)
{
  // dynamic LDS (IR_LDS_BYTES): the matrices, then per wavefront the tile, the slots' chain descriptors and the slot list
  extern __shared__ __align__(16) unsigned char smem[];
  _Float16* const tab = reinterpret_cast<_Float16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    // (rc_load_image in words: as a call of it the kernel's first instructions come out in another order, docs/MEASUREMENTS.md)
    constexpr int NW4 = IR_TAB_BYTES / 16;                                // (the image holds both table sets back to back)
    const uint4* src = reinterpret_cast<const uint4*>(a.image);
    for (int i = tid; i < NW4; i += IR_THREADS) reinterpret_cast<uint4*>(tab)[i] = src[i];
  }
  __syncthreads();                                                        // the only workgroup barrier: below every wavefront walks its own items
  unsigned char* const mine = smem + IR_TAB_BYTES + (size_t)wave * IR_WAVE_BYTES;
  short* const resiT = reinterpret_cast<short*>(mine);
  RcDesc* const dS = reinterpret_cast<RcDesc*>(resiT + IR_TILE);          // dS[k]: slot k
  int* const lst = reinterpret_cast<int*>(dS + IR_SLOTS);                 // the slots that run in lane groups
  const RcSmallTab* const tabs = reinterpret_cast<const RcSmallTab*>(smem + RC_TAB_HALVES * 2);
  int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * IR_WAVES + wave) * IR_FB_INTS;

  const int first = (int)blockIdx.x * IR_WAVES + wave, step = (int)gridDim.x * IR_WAVES;
  IrItem tNext = a.items[first < a.n ? first : 0];
  for (int item = first; item < a.n; item += step)
  {
    const IrItem t = tNext;
    if (item + step < a.n) tNext = a.items[item + step];                  // the next record is on its way while this item runs
    const int w = t.w, h = t.h;
    long long predOff = t.pred_off;
    bool ok = side_ok(w, 2) && side_ok(h, 2) && (t.cand_off & 3) == 0 && (t.level_off & 3) == 0;
    // (the guard is ir_list_pred's own, repeated: without it the kernel compiles to other code, 520 instructions less -- docs/MEASUREMENTS.md)
    if (ok && t.list_row >= 0) ok = ir_list_pred(ok, a.rdList, t, predOff);
    if (!ok)                                                              // skipped: the markers, nothing else
    {
      if (lane < IR_SLOTS) { a.absSum[IR_SLOTS * (size_t)item + lane] = 0xFFFFFFFFu; a.distResi[IR_SLOTS * (size_t)item + lane] = ~0ull; a.distRec[IR_SLOTS * (size_t)item + lane] = ~0ull; }
      if (lane == 0) a.zeroDist[item] = ~0ull;
      continue;
    }
    const int samples = w * h;
    const bool narrow = w <= 8 || h <= 8;
    short* const predT = ir_tile_pred(resiT, narrow, samples);
    short* const backT = ir_tile_back(resiT, narrow, samples);
    const Pel* const predG = a.pred + predOff;

    // ---- orgResi and the prediction into the tile, zero_dist
    {
      const unsigned long long zd = ir_stage(t, a.org + t.org_off, predG, resiT, predT, lane);
      if (lane == 0) a.zeroDist[item] = zd;
    }

    // ---- the slots: which are served, which run side by side in lane groups (4x4, 8x8, 8x4, 4x8: every transform slot of the item in ONE call)
    const bool grouped = (w == 4 || w == 8) && (h == 4 || h == 8);
    unsigned long long trBits;
    __builtin_memcpy(&trBits, t.tr, 8);                                   // (tr[6] and reserved1[2]: the codes by shifts, not by a dynamic index)
    unsigned servedMask = 0u, groupMask = 0u;
#pragma unroll
    for (int k = 0; k < IR_SLOTS; k++)
    {
      const int code = (int)(signed char)(trBits >> (8 * k));
      const bool ts = code == VVCGPU_INTER_RESI_TS;
      const int th = ts ? 3 : code % 3, tv = ts ? 0 : code / 3;
      const bool served = ts ? (w <= 4 && h <= 4)
                             : (code >= 0 && code < 9 && (th == 0 || (w > 2 && w <= 32)) && (tv == 0 || (h > 2 && h <= 32)));
      const size_t out = IR_SLOTS * (size_t)item + k;
      if (!served)
      {
        if (lane == 0) { a.absSum[out] = 0xFFFFFFFFu; a.distResi[out] = ~0ull; a.distRec[out] = ~0ull; }
        continue;
      }
      const bool inGroup = grouped && !ts;
      if (lane == 0)
      {
        RcDesc u;
        // resi' goes to `back` (a lane-group slot: its own w h samples there) or to the slot's candidate buffer
        u.org_off = 0; u.pred_off = 0; u.rec_off = backT ? (inGroup ? k * samples : 0) : t.cand_off + (long long)k * samples;
        u.level_off = t.level_off + (long long)k * samples;
        u.org_stride = w; u.pred_stride = w; u.rec_stride = w; u.w = (int16_t)w; u.h = (int16_t)h;
        u.tr_hor = (int8_t)th; u.tr_ver = (int8_t)tv; u.intra_slice = t.intra_slice; u.sign_hiding = t.sign_hiding; u.qp = t.qp;
        u.reserved[0] = 0; u.reserved[1] = 0;
        dS[k] = u;
        if (inGroup) lst[__popc(groupMask)] = k;
      }
      servedMask |= 1u << k;
      if (inGroup) groupMask |= 1u << k;
    }
    wave_sync();

    // the closing loop of slot k of this item, resi' in backK (null: in the slot's candidate buffer)
    auto finish = [&](int k, const short* backK) { ir_finish(a, t, item, k, resiT, predT, predG, backK, lane); };

    // ---- the residual chain, in the residual domain
    unsigned* const absSumItem = a.absSum + IR_SLOTS * (size_t)item;
    Pel* const outBase = backT ? backT : a.resi;                          // what the bodies take as their `rec` plane
    if (groupMask)                                                        // abs_sum[list entry] = abs_sum of that slot: the list holds the slot numbers
    {
      const int cnt = __popc(groupMask);
      int* const tmpL = reinterpret_cast<int*>(resiT + 1024);
      if (w == 8 && h == 8)      rc_small_group<8, RC_RESI>(dS, lst, cnt, 0, resiT, resiT, outBase, a.level, absSumItem, a.bd, 0, 0, *tabs, tmpL, lane);
      else if (w == 4 && h == 4) rc_small_group<4, RC_RESI>(dS, lst, cnt, 0, resiT, resiT, outBase, a.level, absSumItem, a.bd, 0, 0, *tabs, tmpL, lane);
      else if (w == 8)           rc_rect_group<8, 4, RC_RESI>(dS, lst, cnt, 0, resiT, resiT, outBase, a.level, absSumItem, a.bd, 0, 0, *tabs, tmpL, lane);
      else                       rc_rect_group<4, 8, RC_RESI>(dS, lst, cnt, 0, resiT, resiT, outBase, a.level, absSumItem, a.bd, 0, 0, *tabs, tmpL, lane);
      wave_sync();
      for (int k = 0; k < IR_SLOTS; k++)
        if ((groupMask >> k) & 1u) finish(k, backT + k * samples);
    }
    for (int k = 0; k < IR_SLOTS; k++)
    {
      if (!(((servedMask & ~groupMask) >> k) & 1u)) continue;
      bool done = true;
#define IR_MF(W_, H_) case ((W_) << 8) | (H_): \
        done = ir_tu_mfma_call<W_, H_>(dS + k, resiT, outBase, a.level, absSumItem + k, a.bd, tab, tb.dqInv, tb.scanOff, lane); break;
      if (narrow)                                                         // at most 512 samples: the buffers lie behind them in the tile
        ir_tu_generic_call(dS + k, resiT, outBase, a.level, absSumItem + k, a.bd, tb.tr32, tb.dqInv, tb.scanOff,
                           reinterpret_cast<int*>(resiT + 1024), reinterpret_cast<int*>(resiT + 2048), lane);
      else switch ((w << 8) | h)
      {
      IR_MF(16, 16) IR_MF(16, 32) IR_MF(16, 64) IR_MF(32, 16) IR_MF(32, 32) IR_MF(32, 64) IR_MF(64, 16) IR_MF(64, 32) IR_MF(64, 64)
      default: break;
      }
#undef IR_MF
      if (!done)                                                          // samples outside the bit depth (out of contract): exact all the same
        ir_tu_generic_call(dS + k, resiT, outBase, a.level, absSumItem + k, a.bd, tb.tr32, tb.dqInv, tb.scanOff, fbScr, fbScr + 4096, lane);
      if (backT) wave_sync(); else wave_global_sync();
      finish(k, backT);
      wave_sync();                                                     // `back` is free again
    }
    wave_sync();                                                       // the tile and the descriptors are free again
  }
}

}  // namespace

extern "C" int vvcgpu_inter_resi_code_batch(const vvc_pel* org_base, const vvc_pel* pred_base, const vvcgpu_inter_resi_item* items, int n,
                                            const int32_t* rd_list, vvc_pel* resi_base, vvc_pel* rec_base, vvc_coef* level_base,
                                            int flags, int bit_depth, int clp_min, int clp_max,
                                            uint32_t* abs_sum, uint64_t* dist_resi, uint64_t* dist_rec, uint64_t* zero_dist, void* stream)
{
  const char* name = "inter_resi_code_batch";
  const bool pointers = org_base && pred_base && items && resi_base && level_base && abs_sum && dist_resi && dist_rec && zero_dist;
  if (const int rc = ir_check_frame(name, n, pointers, flags, rec_base, clp_min, clp_max)) return rc;
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(((uintptr_t)items & 15) == 0, "%s: item array must be 16-byte aligned", name);
  if (const int rc = ir_check_bit_depth(name, bit_depth)) return rc;
  hipStream_t st = (hipStream_t)stream;
  VvcTrTables tb; const _Float16* image = nullptr;
  const int rt = vvcgpu_tr_images(&tb, &image);
  if (rt) return rt;
  const int wgs = vvc_grid_cap(n, IR_WAVES, 1);
  VvcScratch sc(st);
  int* fbScratch = ir_fb_scratch(sc, wgs);
  if (!fbScratch) return VVCGPU_E_DEVICE;
  IrArgs a;
  a.org = org_base; a.pred = pred_base; a.items = items; a.rdList = rd_list; a.resi = resi_base; a.rec = rec_base; a.level = level_base;
  a.absSum = abs_sum; a.distResi = reinterpret_cast<unsigned long long*>(dist_resi); a.distRec = reinterpret_cast<unsigned long long*>(dist_rec);
  a.zeroDist = reinterpret_cast<unsigned long long*>(zero_dist); a.fbScratch = fbScratch; a.image = image;
  a.n = n; a.writeRec = (flags & VVCGPU_INTER_RESI_WRITE_REC) ? 1 : 0; a.bd = bit_depth; a.cmin = clp_min; a.cmax = clp_max;
  VVC_HIP(vvc_allow_lds(inter_resi_code_kernel, IR_LDS_BYTES));
  hipLaunchKernelGGL(inter_resi_code_kernel, dim3(wgs), dim3(IR_THREADS), IR_LDS_BYTES, st, a, tb);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
