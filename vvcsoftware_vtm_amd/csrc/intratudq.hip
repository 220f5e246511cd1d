// intratudq.hip -- vvcgpu_intra_tu_code_dq_batch: the pixel pass of the intra RD loop (intratu.hip) with the quantiser of the shipped configurations,
// the dependent-quantisation trellis, in three launches on the caller's stream.
//
// Reference behaviour reproduced (bit-exact):
//   IntraSearch::xIntraCodingTUBlock                                                            EncoderLib/IntraSearch.cpp:1147-1316 (see intratu.hip)
//   transformNxN :1253 under slice->getDepQuantEnabledFlag(): xT (TrQuant.cpp:694-739), DQIntern::DepQuant::quant   CommonLib/DepQuant.cpp:1323-1387
//   invTransformNxN :1289: DQIntern::Quantizer::dequantBlock :708-785, xIT (TrQuant.cpp:743-791); piResi.fill(0) :1293 when nothing was coded
//
// Design (docs/KERNELS.md, "The intra RD loop's pixel pass with DepQuant"):
//   front    persistent workgroups of twelve wavefronts, one per compute unit, a wavefront per item (the pair preds[i], tus[i], with dq[i]): validity and
//            the mode_list look-up, the prediction into the wavefront's LDS tile (stored under WRITE_PRED, and parked in the workspace for the back:
//            forming it a second time there measured slower, docs/OPTIMISATION_LOG.md), org - pred over it in place, the forward
//            transform (the RC_FWD bodies of resichain_dev.h through dqpass_dev.h) into the coefficient workspace -- the zeroed region of a 64-point
//            side written as zeros: the trellis reads all w h coefficients -- and the item's trellis record, whose index it appends to the work list
//            (one atomic add per wavefront on a counter of vvcgpu_counters).  A skipped item gets its markers here and no list entry.
//   trellis  the trellis of depquant_dev.h (vvcgpu_depquant_listed_launch of depquant.hip) over the listed records: levels and abs_sum of the served items.
//            The grid is sized for n records; workgroups behind the list's end leave at once.
//   back     the same wavefront-per-item walk: the dependent de-quantiser into the coefficient workspace, the inverse transform (RC_INV bodies) with
//            resi' left in the tile, then clip(pred + resi') with the parked prediction to rec_base, xGetSSE(org, rec) and the count of the non-zero
//            levels.  An item with abs_sum == 0 has resi' = 0.
//   VVCGPU_INTRA_TU_DQ_TS  a 4x4 item with tr_hor == 3, the checkTransformSkip candidate of xRecurIntraCodingLumaQT (IntraSearch.cpp:1347-1412), in the
//            same two walks: the scaling of dqpass_dev.h in place of the two transforms, everything else every item's.  The flag selects the kernels,
//            ItqPass<true>'s.
#include "common.h"
#include "dist_dev.h"
#include "dqpass_dev.h"
#include "intra_dev.h"
#include "intratu_dev.h"

static_assert(sizeof(vvcgpu_intra_desc) == 32 && sizeof(vvcgpu_resi_chain_desc) == 64 && sizeof(vvcgpu_inter_resi_dq) == 16 && sizeof(vvcgpu_depquant_desc) == 40,
              "descriptor layouts");

namespace {

constexpr int ITQ_WAVES = 12, ITQ_THREADS = 64 * ITQ_WAVES;               // one workgroup per compute unit, as many wavefronts as its LDS holds: neither parent's budget (eight
                                                                          // per compute unit in both) -- twelve measured 12 % faster on the 4K list (docs/OPTIMISATION_LOG.md)
constexpr int ITQ_LDS_BYTES = IT_TAB_BYTES + ITQ_WAVES * IT_WAVE_BYTES;   // 159 168 bytes
static_assert(IT_TAB_BYTES == IQ_TAB_BYTES && IT_FB_INTS == IQ_FB_INTS && ITQ_LDS_BYTES <= 160 * 1024, "LDS budget");

struct ItqArgs
{
  const Pel* refs; const vvcgpu_intra_desc* preds; const Pel* org; Pel* pred; Pel* rec; TCoeff* level; const RcDesc* tus; const IqDq* dq; const int* modeList;
  unsigned* absSum; unsigned* numSig; unsigned long long* dist; int* modeOut; int* fbScratch; const _Float16* image;
  TCoeff* coef; Pel* park; vvcgpu_depquant_desc* recs; int* list; int* count; int* nextCounters; long long levelExtent;
  int n, nRates, writePred, noSmoothing, bd, cmin, cmax;
};

// is the item served, and with which mode and filter decision?  The rule of intratu_dev.h; here also: level_off a multiple of 16 and not negative -- the
// trellis workspace is indexed by it --, the levels inside level_extent, a rate table inside the array, a lambda above zero.  TS (the call carries
// VVCGPU_INTRA_TU_DQ_TS): tr_hor == 3 on a 4x4 block is the checkTransformSkip candidate (itq_is_ts), tr_ver ignored; every other rule holds for it
template <bool TS>
__device__ __forceinline__ bool itq_is_ts(const RcDesc& t) { return TS && t.tr_hor == 3 && t.w == 4 && t.h == 4; }
template <bool TS>
__device__ __forceinline__ bool itq_resolve(const ItqArgs& a, const vvcgpu_intra_desc& p, const RcDesc& t, const IqDq& q, int& mode, bool& filt)
{
  auto also = [&] { return t.level_off >= 0 && (t.level_off & 15) == 0 && t.level_off <= a.levelExtent - (long long)t.w * t.h &&
                           q.rates_idx >= 0 && q.rates_idx < a.nRates && q.lambda > 0.0; };
  if constexpr (TS)
  {
    // (the shared rule knows the transform types alone: DCT-II in its eyes.  A copy of the descriptor, not another argument of it_resolve: with one,
    // intra_tu_code_kernel and the kernels of a call without the flag compile to other code, docs/MEASUREMENTS.md)
    RcDesc u = t;
    if (itq_is_ts<TS>(t)) { u.tr_hor = 0; u.tr_ver = 0; }
    return it_resolve(a, p, u, also, mode, filt);
  }
  return it_resolve(a, p, t, also, mode, filt);
}
// the chain descriptor of the item for the transform bodies: the residual (forward) or resi' (inverse) contiguous in the tile; the coefficients at the
// item's place in the workspace
__device__ __forceinline__ RcDesc itq_desc(const RcDesc& t)
{
  RcDesc u = t;
  u.org_off = 0; u.pred_off = 0; u.rec_off = 0; u.org_stride = t.w; u.pred_stride = t.w; u.rec_stride = t.w;
  u.intra_slice = 0; u.sign_hiding = 0; u.reserved[0] = 0; u.reserved[1] = 0;
  return u;
}

// ---------------------------------------------------------------------------------------------------
// The two kernels are static members of a class template over TS (the call carries VVCGPU_INTRA_TU_DQ_TS), not function templates, for the reason
// given at IqPass in interresidq.hip: ItqPass<false>'s are, to the instruction, intra_tu_dq_front_kernel and intra_tu_dq_back_kernel of before the flag.
template <bool TS>
struct ItqPass
{
  static __global__ __launch_bounds__(ITQ_THREADS, 1) void front(const ItqArgs a, const VvcTrTables tb)
  {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const _Float16* const tab = rc_load_image<ITQ_THREADS>(smem, a.image, tid);   // below every wavefront walks its own items
    const ItLds l = it_lds(smem, wave);
    int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * ITQ_WAVES + wave) * IQ_FB_INTS;
    if (blockIdx.x == 0 && tid < VVC_CTR_INTS) a.nextCounters[tid] = 0;    // the counter set of the NEXT call on this stream (vvcgpu_counters)

    // the wavefront's run in the trellis' work list: its served items are counted first, a lane per item
    const int first = (int)blockIdx.x + (int)gridDim.x * wave, step = (int)gridDim.x * ITQ_WAVES;
    int cnt = 0;
    for (int item = first + lane * step; item < a.n; item += 64 * step)
    {
      int mode; bool filt;
      cnt += itq_resolve<TS>(a, a.preds[item], a.tus[item], a.dq[item], mode, filt) ? 1 : 0;
    }
    int listAt = iq_reserve(a.count, cnt, lane);

    for (int item = first; item < a.n; item += step)
    {
      const vvcgpu_intra_desc p = a.preds[item];
      const RcDesc t = a.tus[item];
      const IqDq q = a.dq[item];
      int mode; bool filt;
      if (!itq_resolve<TS>(a, p, t, q, mode, filt)) { it_mark(a, item, lane); continue; }
      const int w = t.w, h = t.h, lw = ilog2(w), samples = w * h;
      it_predict(a, p, t, mode, filt, l, lane);
      if (a.writePred && mode >= 0)
      {
        Pel* dst = a.pred + t.pred_off;
        for (int e = lane; e < samples; e += 64) dst[(ptrdiff_t)(e >> lw) * t.pred_stride + (e & (w - 1))] = l.tile[e];
      }
      for (int e = lane; e < samples; e += 64) a.park[t.level_off + e] = l.tile[e];      // for the back (re-forming it there measured slower)
      if (lane == 0)                                                        // the chain descriptor, the trellis record and its list entry
      {
        *l.dS = itq_desc(t);
        a.modeOut[item] = mode < 0 ? -1 : mode;
        a.recs[item] = iq_record(t.level_off, t.qp, w, h, q, q.luma);
        a.list[listAt] = item;
      }
      listAt++;
      // org - pred over the prediction (four loads in flight: the item waits for one round trip per 256 samples)
      const Pel* org = a.org + t.org_off;
      for (int e0 = lane; e0 < samples; e0 += 256)
      {
        int ov[4];
  #pragma unroll
        for (int u = 0; u < 4; u++)
        {
          const int e = e0 + 64 * u;
          ov[u] = e < samples ? (int)org[(ptrdiff_t)(e >> lw) * t.org_stride + (e & (w - 1))] : 0;
        }
  #pragma unroll
        for (int u = 0; u < 4; u++)
        {
          const int e = e0 + 64 * u;
          if (e < samples) l.tile[e] = (short)(ov[u] - (int)l.tile[e]);
        }
      }
      wave_sync();
      if (itq_is_ts<TS>(t)) iq_ts_forward(l.tile, a.coef + t.level_off, a.bd, lane);      // the scaled residual is the coefficient block
      else iq_transform<RC_FWD>(l.dS, l.tile, nullptr, a.coef, a.bd, tab, tb, fbScr, lane);
      wave_sync();                                                          // the tile and the descriptor are free again
    }
  }

  static __global__ __launch_bounds__(ITQ_THREADS, 1) void back(const ItqArgs a, const VvcTrTables tb)
  {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const _Float16* const tab = rc_load_image<ITQ_THREADS>(smem, a.image, tid);   // below every wavefront walks its own items
    const ItLds l = it_lds(smem, wave);
    int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * ITQ_WAVES + wave) * IQ_FB_INTS;

    for (int item = (int)blockIdx.x + (int)gridDim.x * wave; item < a.n; item += (int)gridDim.x * ITQ_WAVES)
    {
      const vvcgpu_intra_desc p = a.preds[item];
      const RcDesc t = a.tus[item];
      int mode; bool filt;
      if (!itq_resolve<TS>(a, p, t, a.dq[item], mode, filt)) continue;          // (the front wrote the markers)
      short* const backT = iq_back_tile(l.tile, t.w, t.h);
      const bool coded = a.absSum[item] != 0u;                              // all levels zero: resi' is zero (piResi.fill(0), :1293)
      if (coded) iq_decode(itq_desc(t), l.dS, l.tile, backT, a.level, a.coef, a.bd, tab, tb, fbScr, lane, itq_is_ts<TS>(t));
      // clip(pred + resi') with the prediction as the front formed it to rec_base, xGetSSE(org, rec), the non-zero levels
      int nz = 0;
      const unsigned long long sse = iq_close(a.org + t.org_off, t.org_stride, a.park + t.level_off, backT, coded, a.rec + t.rec_off, t.rec_stride,
                                              a.level + t.level_off, t.w, t.w * t.h, a.cmin, a.cmax, lane, &nz);
      if (lane == 0) { a.dist[item] = sse; a.numSig[item] = (unsigned)nz; }
      wave_sync();                                                          // the tile and the descriptor are free again
    }
  }
};

}  // namespace

extern "C" {

size_t vvcgpu_intra_tu_code_dq_workspace_bytes(size_t level_extent, int n)
{
  return iq_layout(level_extent, n, 1, true).bytes;                       // parked predictions; per item a trellis record and a list entry
}

int vvcgpu_intra_tu_code_dq_batch(const vvc_pel* refs_base, const vvcgpu_intra_desc* preds, const vvc_pel* org_base, vvc_pel* pred_base, vvc_pel* rec_base,
                                  vvc_coef* level_base, size_t level_extent, const vvcgpu_resi_chain_desc* tus, const vvcgpu_inter_resi_dq* dq, int n,
                                  const int32_t* mode_list, const vvcgpu_dq_rates* rates, int n_rates, int quantiser, int flags, int bit_depth,
                                  int clp_min, int clp_max, uint32_t* abs_sum, uint32_t* num_sig, uint64_t* dist, int32_t* mode_out,
                                  void* ws, size_t ws_bytes, void* stream)
{
  const char* name = "intra_tu_code_dq_batch";
  VVC_CHECK_ARG(n >= 0, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(refs_base && preds && org_base && rec_base && level_base && tus && dq && rates && abs_sum && num_sig && dist && mode_out && ws, "%s: null pointer", name);
  VVC_CHECK_ARG((flags & ~(VVCGPU_INTRA_TU_WRITE_PRED | VVCGPU_INTRA_TU_NO_SMOOTHING | VVCGPU_INTRA_TU_DQ_TS)) == 0, "%s: unknown flags 0x%x", name, flags);
  VVC_CHECK_ARG(pred_base || !(flags & VVCGPU_INTRA_TU_WRITE_PRED), "%s: null pointer (pred_base with VVCGPU_INTRA_TU_WRITE_PRED)", name);
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "%s: clip range %d..%d", name, clp_min, clp_max);
  VVC_CHECK_ARG(((uintptr_t)preds & 15) == 0 && ((uintptr_t)tus & 15) == 0 && ((uintptr_t)dq & 7) == 0,
                "%s: descriptor arrays must be 16-byte, dq array 8-byte aligned", name);
  const IqLayout lay = iq_layout(level_extent, n, 1, true);
  if (const int rc = iq_check_frame(name, n, "items", n_rates, level_extent, ws, ws_bytes, lay.bytes, quantiser, quantiser == VVCGPU_INTRA_TU_Q_DEPQUANT, bit_depth))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int wgs = vvc_grid_cap(n, 1, 1);                                  // (the items are dealt to the workgroups first, then to their wavefronts: a short list spreads over the compute units)
  // the flag selects the kernels: without it the front and the back are the ones that know no transform-skip item
  const bool ts = (flags & VVCGPU_INTRA_TU_DQ_TS) != 0;
  const auto front = ts ? ItqPass<true>::front : ItqPass<false>::front;
  const auto back = ts ? ItqPass<true>::back : ItqPass<false>::back;
  VVC_HIP(vvc_allow_lds(front, ITQ_LDS_BYTES));
  VVC_HIP(vvc_allow_lds(back, ITQ_LDS_BYTES));
  VvcScratch sc(st);
  IqSetup s;
  if (const int rc = iq_setup(st, sc, (size_t)wgs * ITQ_WAVES, s)) return rc;
  ItqArgs a;
  a.refs = refs_base; a.preds = preds; a.org = org_base; a.pred = pred_base; a.rec = rec_base; a.level = level_base; a.tus = tus; a.dq = dq; a.modeList = mode_list;
  a.absSum = abs_sum; a.numSig = num_sig; a.dist = reinterpret_cast<unsigned long long*>(dist); a.modeOut = mode_out; a.fbScratch = s.fbScratch; a.image = s.image;
  a.coef = iq_at<TCoeff>(ws, 0); a.park = iq_at<Pel>(ws, lay.park); a.recs = iq_at<vvcgpu_depquant_desc>(ws, lay.recs); a.list = iq_at<int>(ws, lay.list);
  a.count = s.count; a.nextCounters = s.nextCounters; a.levelExtent = (long long)level_extent;
  a.n = n; a.nRates = n_rates; a.writePred = (flags & VVCGPU_INTRA_TU_WRITE_PRED) ? 1 : 0; a.noSmoothing = (flags & VVCGPU_INTRA_TU_NO_SMOOTHING) ? 1 : 0;
  a.bd = bit_depth; a.cmin = clp_min; a.cmax = clp_max;
  hipLaunchKernelGGL(front, dim3(wgs), dim3(ITQ_THREADS), ITQ_LDS_BYTES, st, a, s.tb);
  VVC_LAUNCH_CHECK_COUNTERS(st);
  if (const int rc = vvcgpu_depquant_listed_launch(a.coef, level_base, a.recs, a.list, a.count, n, rates, bit_depth, abs_sum, iq_at<unsigned>(ws, lay.dec),
                                                   iq_at<unsigned char>(ws, lay.ctx), s.tb, st)) return rc;
  hipLaunchKernelGGL(back, dim3(wgs), dim3(ITQ_THREADS), ITQ_LDS_BYTES, st, a, s.tb);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
