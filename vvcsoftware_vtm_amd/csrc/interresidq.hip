// interresidq.hip -- vvcgpu_inter_resi_code_dq_batch: the pixel pass of the inter residual RD loop (interresi.hip) with the quantiser of the shipped
// configurations, the dependent-quantisation trellis, in three launches on the caller's stream.
//
// Reference behaviour reproduced (bit-exact):
//   InterSearch::encodeResAndCalcRdInterCU / xEstimateInterResidualQT "check full"                EncoderLib/InterSearch.cpp:4752-4909, :4254-4634 (see interresi.hip)
//   transformNxN :4409 under slice->getDepQuantEnabledFlag(): xT (TrQuant.cpp:694-739), DQIntern::DepQuant::quant   CommonLib/DepQuant.cpp:1323-1387
//   invTransformNxN :4497: DQIntern::Quantizer::dequantBlock :708-785, xIT (TrQuant.cpp:743-791)
//
// Design (docs/KERNELS.md, "The inter residual pass with DepQuant"):
//   front    persistent workgroups of eight wavefronts, a wavefront per item: validity and the rd_list look-up, orgResi = org - pred staged once in the
//            wavefront's LDS tile, zero_dist, per served slot the forward transform (the RC_FWD bodies of resichain_dev.h) into the coefficient workspace
//            -- the zeroed region of a 64-point side written as zeros: the trellis reads all w h coefficients -- and the slot's trellis record, whose
//            index 6 i + k it appends to the work list (one atomic add per wavefront on a counter of vvcgpu_counters).  A skipped item or slot gets its
//            markers here and no list entry.
//   trellis  the trellis of depquant_dev.h (vvcgpu_depquant_listed_launch of depquant.hip: depquant_kernel's body with the work list in front of the
//            descriptors) over the listed records: four lanes per TU, sixteen TUs per wavefront; levels and abs_sum of the served slots.  The grid is sized for 6 n records; workgroups behind the list's end leave at once.
//   back     the same wavefront-per-item walk: orgResi and the prediction re-formed in the tile; per served slot the dependent de-quantiser (the
//            GF(2)-linear state replay, as dq_group of transform.hip) into the coefficient workspace, the inverse transform (RC_INV bodies), resi'
//            unclipped to the candidate buffer, both distortions and the reconstruction as interresi.hip's.  A slot with abs_sum == 0 stores zeros.
//   VVCGPU_INTER_RESI_DQ_TS  the transform-skip slot of a 4x4 item (InterSearch.cpp:4340-4386) in the same two walks: xTransformSkip (TrQuant.cpp:1140-1148)
//            in place of the forward transform, xITransformSkip (:823-833) in place of the inverse one, sixteen lanes each (dqpass_dev.h); record, list
//            entry, trellis and de-quantiser as for every slot.  The flag selects the kernels, IqPass<true>'s.
#include "common.h"
#include "dqpass_dev.h"
#include "interresi_dev.h"

static_assert(sizeof(vvcgpu_inter_resi_item) == 80 && sizeof(vvcgpu_inter_resi_dq) == 16 && sizeof(vvcgpu_depquant_desc) == 40, "descriptor layouts");

namespace {

constexpr int IQ_WAVE_BYTES = IR_TILE * 2 + IR_SLOTS * (int)sizeof(vvcgpu_resi_chain_desc);      // the tile, a chain descriptor per slot
constexpr int IQ_LDS_BYTES = IQ_TAB_BYTES + IR_WAVES * IQ_WAVE_BYTES;
static_assert(IQ_TAB_BYTES % 16 == 0 && IQ_WAVE_BYTES % 16 == 0 && IQ_LDS_BYTES <= 160 * 1024 && IR_FB_INTS == IQ_FB_INTS, "LDS budget");

struct IqArgs
{
  const Pel* org; const Pel* pred; const IrItem* items; const IqDq* dq; const int* rdList; Pel* resi; Pel* rec; TCoeff* level;
  unsigned* absSum; unsigned long long* distResi; unsigned long long* distRec; unsigned long long* zeroDist; int* fbScratch; const _Float16* image;
  TCoeff* coef; vvcgpu_depquant_desc* recs; int* list; int* count; int* nextCounters; long long levelExtent;
  int n, nRates, writeRec, bd, cmin, cmax;
};

// is the item served, and where is its prediction?  (the rules of interresi.hip; here also: no side of 2, level_off a multiple of 16 -- the trellis
// workspace is indexed by it --, a rate table inside the array, a lambda above zero)
__device__ __forceinline__ bool iq_item_ok(const IqArgs& a, const IrItem& t, const IqDq& q, long long& predOff)
{
  predOff = t.pred_off;
  bool ok = side_ok(t.w, 4) && side_ok(t.h, 4) && (t.cand_off & 3) == 0 && (t.level_off & 15) == 0 && t.level_off >= 0
            && q.rates_idx >= 0 && q.rates_idx < a.nRates && q.lambda > 0.0;
  return ir_list_pred(ok, a.rdList, t, predOff);
}
// the served slots of a served item: DCT-II and the DCT-VIII / DST-VII pairs on sides up to 32 and -- TS: the call carries VVCGPU_INTER_RESI_DQ_TS --
// the transform-skip slot of a 4x4 block; the slot's levels inside level_extent
template <bool TS>
__device__ __forceinline__ unsigned iq_served_mask(const IqArgs& a, const IrItem& t)
{
  const int w = t.w, h = t.h, samples = w * h;
  unsigned long long trBits;
  __builtin_memcpy(&trBits, t.tr, 8);
  unsigned mask = 0u;
#pragma unroll
  for (int k = 0; k < IR_SLOTS; k++)
  {
    const int code = (int)(signed char)(trBits >> (8 * k));
    const int th = code % 3, tv = code / 3;
    bool served = code >= 0 && code < 9 && (th == 0 || w <= 32) && (tv == 0 || h <= 32);
    if constexpr (TS) served = served || (code == VVCGPU_INTER_RESI_TS && w == 4 && h == 4);
    if (served && t.level_off + (long long)(k + 1) * samples <= a.levelExtent) mask |= 1u << k;
  }
  return mask;
}
__device__ __forceinline__ int iq_code(const IrItem& t, int k)
{
  unsigned long long trBits;
  __builtin_memcpy(&trBits, t.tr, 8);
  return (int)(signed char)(trBits >> (8 * k));
}

// the chain descriptor of slot k for the transform bodies: the residual in the tile, the coefficients at the slot's place in the workspace
__device__ __forceinline__ RcDesc iq_desc(const IrItem& t, int k, long long recOff)
{
  const int code = iq_code(t, k), samples = t.w * t.h;
  RcDesc u;
  u.org_off = 0; u.pred_off = 0; u.rec_off = recOff; u.level_off = t.level_off + (long long)k * samples;
  u.org_stride = t.w; u.pred_stride = t.w; u.rec_stride = t.w; u.w = t.w; u.h = t.h;
  u.tr_hor = (int8_t)(code % 3); u.tr_ver = (int8_t)(code / 3); u.intra_slice = 0; u.sign_hiding = 0; u.qp = t.qp;
  u.reserved[0] = 0; u.reserved[1] = 0;
  return u;
}

// ---------------------------------------------------------------------------------------------------
// The two kernels are static members of a class template over TS (the call carries VVCGPU_INTER_RESI_DQ_TS), not function templates: the compiler
// numbers the kernels of a code object by their symbol names for the look-up of the dynamic LDS in the bodies they call, and only with the template
// argument in front of "front" / "back" do IqPass<false>'s keep the numbers, and with them every instruction, of the kernels before the flag existed
// (inter_resi_dq_front_kernel, inter_resi_dq_back_kernel; tools/kernel_streams.py, docs/MEASUREMENTS.md).
template <bool TS>
struct IqPass
{
  static __global__ __launch_bounds__(IR_THREADS, 1) void front(const IqArgs a, const VvcTrTables tb)
  {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const _Float16* const tab = rc_load_image<IR_THREADS>(smem, a.image, tid);   // below every wavefront walks its own items
    unsigned char* const mine = smem + IQ_TAB_BYTES + (size_t)wave * IQ_WAVE_BYTES;
    short* const resiT = reinterpret_cast<short*>(mine);
    RcDesc* const dS = reinterpret_cast<RcDesc*>(resiT + IR_TILE);
    int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * IR_WAVES + wave) * IR_FB_INTS;
    if (blockIdx.x == 0 && tid < VVC_CTR_INTS) a.nextCounters[tid] = 0;    // the counter set of the NEXT call on this stream (vvcgpu_counters)

    // the wavefront's run in the trellis' work list: its served slots are counted first, a lane per item
    const int first = (int)blockIdx.x * IR_WAVES + wave, step = (int)gridDim.x * IR_WAVES;
    int cnt = 0;
    for (int item = first + lane * step; item < a.n; item += 64 * step)
    {
      const IrItem t = a.items[item];
      long long predOff;
      if (iq_item_ok(a, t, a.dq[item], predOff)) cnt += __popc(iq_served_mask<TS>(a, t));
    }
    int listAt = iq_reserve(a.count, cnt, lane);

    for (int item = first; item < a.n; item += step)
    {
      const IrItem t = a.items[item];
      const IqDq q = a.dq[item];
      long long predOff;
      const bool ok = iq_item_ok(a, t, q, predOff);
      const unsigned servedMask = ok ? iq_served_mask<TS>(a, t) : 0u;
      if (lane < IR_SLOTS)                                                  // the slot's trellis record and list entry; the markers of a skipped slot
      {
        const size_t out = IR_SLOTS * (size_t)item + lane;
        if ((servedMask >> lane) & 1u)
        {
          a.recs[out] = iq_record(t.level_off + (long long)lane * t.w * t.h, t.qp, t.w, t.h, q, q.luma);
          a.list[listAt + __popc(servedMask & ((1u << lane) - 1u))] = (int)out;
        }
        else { a.absSum[out] = 0xFFFFFFFFu; a.distResi[out] = ~0ull; a.distRec[out] = ~0ull; }
      }
      listAt += __popc(servedMask);
      if (!ok)
      {
        if (lane == 0) a.zeroDist[item] = ~0ull;
        continue;
      }
      const unsigned long long zd = ir_stage(t, a.org + t.org_off, a.pred + predOff, resiT, nullptr, lane);
      if (lane == 0) a.zeroDist[item] = zd;
      if (lane < IR_SLOTS && ((servedMask >> lane) & 1u)) dS[lane] = iq_desc(t, lane, 0);
      wave_sync();
      for (int k = 0; k < IR_SLOTS; k++)
      {
        if (!((servedMask >> k) & 1u)) continue;
        if (TS && iq_code(t, k) == VVCGPU_INTER_RESI_TS)                     // (a 4x4 block: iq_served_mask) the scaled residual is the coefficient block
        {
          iq_ts_forward(resiT, a.coef + t.level_off + (long long)k * t.w * t.h, a.bd, lane);
          continue;
        }
        iq_transform<RC_FWD>(dS + k, resiT, nullptr, a.coef, a.bd, tab, tb, fbScr, lane);
        wave_sync();
      }
      wave_sync();                                                       // the tile and the descriptors are free again
    }
  }

  static __global__ __launch_bounds__(IR_THREADS, 1) void back(const IqArgs a, const VvcTrTables tb)
  {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const _Float16* const tab = rc_load_image<IR_THREADS>(smem, a.image, tid);   // below every wavefront walks its own items
    unsigned char* const mine = smem + IQ_TAB_BYTES + (size_t)wave * IQ_WAVE_BYTES;
    short* const resiT = reinterpret_cast<short*>(mine);
    RcDesc* const dS = reinterpret_cast<RcDesc*>(resiT + IR_TILE);
    int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * IR_WAVES + wave) * IR_FB_INTS;

    for (int item = (int)blockIdx.x * IR_WAVES + wave; item < a.n; item += (int)gridDim.x * IR_WAVES)
    {
      const IrItem t = a.items[item];
      const IqDq q = a.dq[item];
      long long predOff;
      if (!iq_item_ok(a, t, q, predOff)) continue;                          // (the front wrote the markers)
      const unsigned servedMask = iq_served_mask<TS>(a, t);
      if (!servedMask) continue;
      const int w = t.w, h = t.h, lw = ilog2(w), samples = w * h;
      const bool narrow = w <= 8 || h <= 8;
      short* const predT = ir_tile_pred(resiT, narrow, samples);
      short* const backT = ir_tile_back(resiT, narrow, samples);
      const Pel* const predG = a.pred + predOff;
      ir_stage(t, a.org + t.org_off, predG, resiT, predT, lane);
      if (lane < IR_SLOTS && ((servedMask >> lane) & 1u)) dS[lane] = iq_desc(t, lane, backT ? 0 : t.cand_off + (long long)lane * samples);
      wave_sync();

      const unsigned short* const scan = tb.scan + tb.scanOff[(lw - 1) * 6 + (ilog2(h) - 1)];
      Pel* const outBase = backT ? backT : a.resi;
      // the closing loop of slot k of this item, as in inter_resi_code_kernel
      auto finish = [&](int k, const short* backK) { ir_finish(a, t, item, k, resiT, predT, predG, backK, lane); };
      for (int k = 0; k < IR_SLOTS; k++)
      {
        if (!((servedMask >> k) & 1u)) continue;
        const size_t out = IR_SLOTS * (size_t)item + k;
        const long long candOff = t.cand_off + (long long)k * samples, levelOff = t.level_off + (long long)k * samples;
        Pel* const rs = a.resi + candOff;
        if (a.absSum[out] == 0u)                                            // all levels zero: resi' is stored as zeros
        {
          for (int e = lane; e < samples; e += 64) { if (backT) backT[e] = 0; else rs[e] = 0; }
        }
        else
        {
          iq_dequant(a.level + levelOff, a.coef + levelOff, w, h, t.qp, a.bd, scan, lane);
          wave_global_sync();
          if (TS && iq_code(t, k) == VVCGPU_INTER_RESI_TS) iq_ts_inverse(a.coef + levelOff, backT, a.bd, lane);     // (a 4x4 block: resi' returns through the tile)
          else iq_transform<RC_INV>(dS + k, resiT, outBase, a.coef, a.bd, tab, tb, fbScr, lane);
        }
        if (backT) wave_sync(); else wave_global_sync();
        finish(k, backT);
        wave_sync();                                                     // `back` and the integer body's buffers are free again
      }
      wave_sync();                                                       // the tile and the descriptors are free again
    }
  }
};

}  // namespace

extern "C" {

size_t vvcgpu_inter_resi_code_dq_workspace_bytes(size_t level_extent, int n)
{
  return iq_layout(level_extent, n, IR_SLOTS, false).bytes;               // nothing parked; per slot a trellis record and a list entry
}

int vvcgpu_inter_resi_code_dq_batch(const vvc_pel* org_base, const vvc_pel* pred_base, const vvcgpu_inter_resi_item* items, const vvcgpu_inter_resi_dq* dq,
                                    int n, const int32_t* rd_list, const vvcgpu_dq_rates* rates, int n_rates, int quantiser,
                                    vvc_pel* resi_base, vvc_pel* rec_base, vvc_coef* level_base, size_t level_extent,
                                    int flags, int bit_depth, int clp_min, int clp_max,
                                    uint32_t* abs_sum, uint64_t* dist_resi, uint64_t* dist_rec, uint64_t* zero_dist, void* ws, size_t ws_bytes, void* stream)
{
  const char* name = "inter_resi_code_dq_batch";
  const bool pointers = org_base && pred_base && items && dq && rates && resi_base && level_base && abs_sum && dist_resi && dist_rec && zero_dist && ws;
  if (const int rc = ir_check_frame(name, n, pointers, flags, rec_base, clp_min, clp_max, VVCGPU_INTER_RESI_WRITE_REC | VVCGPU_INTER_RESI_DQ_TS)) return rc;
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(((uintptr_t)items & 15) == 0 && ((uintptr_t)dq & 7) == 0, "%s: item array must be 16-byte, dq array 8-byte aligned", name);
  const IqLayout lay = iq_layout(level_extent, n, IR_SLOTS, false);
  if (const int rc = iq_check_frame(name, n, "items", n_rates, level_extent, ws, ws_bytes, lay.bytes, quantiser, quantiser == VVCGPU_INTER_RESI_Q_DEPQUANT, bit_depth))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int wgs = vvc_grid_cap(n, IR_WAVES, 1);
  // the flag selects the kernels: without it the front and the back are the ones that know no transform-skip slot
  const bool ts = (flags & VVCGPU_INTER_RESI_DQ_TS) != 0;
  const auto front = ts ? IqPass<true>::front : IqPass<false>::front;
  const auto back = ts ? IqPass<true>::back : IqPass<false>::back;
  VVC_HIP(vvc_allow_lds(front, IQ_LDS_BYTES));
  VVC_HIP(vvc_allow_lds(back, IQ_LDS_BYTES));
  VvcScratch sc(st);
  IqSetup s;
  if (const int rc = iq_setup(st, sc, (size_t)wgs * IR_WAVES, s)) return rc;
  IqArgs a;
  a.org = org_base; a.pred = pred_base; a.items = items; a.dq = dq; a.rdList = rd_list; a.resi = resi_base; a.rec = rec_base; a.level = level_base;
  a.absSum = abs_sum; a.distResi = reinterpret_cast<unsigned long long*>(dist_resi); a.distRec = reinterpret_cast<unsigned long long*>(dist_rec);
  a.zeroDist = reinterpret_cast<unsigned long long*>(zero_dist); a.fbScratch = s.fbScratch; a.image = s.image;
  a.coef = iq_at<TCoeff>(ws, 0); a.recs = iq_at<vvcgpu_depquant_desc>(ws, lay.recs); a.list = iq_at<int>(ws, lay.list);
  a.count = s.count; a.nextCounters = s.nextCounters; a.levelExtent = (long long)level_extent;
  a.n = n; a.nRates = n_rates; a.writeRec = (flags & VVCGPU_INTER_RESI_WRITE_REC) ? 1 : 0; a.bd = bit_depth; a.cmin = clp_min; a.cmax = clp_max;
  hipLaunchKernelGGL(front, dim3(wgs), dim3(IR_THREADS), IQ_LDS_BYTES, st, a, s.tb);
  VVC_LAUNCH_CHECK_COUNTERS(st);
  if (const int rc = vvcgpu_depquant_listed_launch(a.coef, level_base, a.recs, a.list, a.count, n * IR_SLOTS, rates, bit_depth, abs_sum,
                                                   iq_at<unsigned>(ws, lay.dec), iq_at<unsigned char>(ws, lay.ctx), s.tb, st)) return rc;
  hipLaunchKernelGGL(back, dim3(wgs), dim3(IR_THREADS), IQ_LDS_BYTES, st, a, s.tb);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
