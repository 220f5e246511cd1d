// intrachromadq.hip -- vvcgpu_intra_chroma_code_dq_batch: the pixel work of the intra chroma mode loop (intrachroma.hip) with the quantiser of the shipped
// configurations, the dependent-quantisation trellis, in five launches on the caller's stream.
//
// Reference behaviour reproduced (bit-exact):
//   IntraSearch::estIntraPredChromaQT / xRecurIntraChromaCodingQT / xIntraCodingTUBlock                     (see intrachroma.hip)
//   transformNxN under slice->getDepQuantEnabledFlag(): xT (TrQuant.cpp:694-739), DQIntern::DepQuant::quant   CommonLib/DepQuant.cpp:1323-1387
//   invTransformNxN: DQIntern::Quantizer::dequantBlock :708-785, xIT (TrQuant.cpp:743-791); piResi.fill(0) when nothing was coded
//   the Cr rate table follows Cb's cbf: RateEstimator::xSetLastCoeffOffset (DepQuant.cpp:379-396) takes Ctx::QtCbf[Cr](CtxQtCbf(Cr, depth, tu.cbf[Cb])),
//   DeriveCtx::CtxQtCbf (ContextModelling.cpp:519-549) returns prevCbCbf for Cr, xRecurIntraChromaCodingQT (IntraSearch.cpp:1722-1843) codes Cb first
//
// Design (docs/KERNELS.md, "The intra chroma mode pass with DepQuant"):
//   front      persistent workgroups of six wavefronts, one per compute unit, a wavefront per PU: the contract, the staging of intrachroma_dev.h once per
//              PU, then per component and slot the prediction into the wavefront's LDS tile (stored under WRITE_PRED, parked in the workspace at the
//              item's level offset), org - pred over it in place, the forward transform (dqpass_dev.h) into the coefficient workspace, the item's
//              trellis record and its entry in the Cb or the Cr work list.  The two lists have one length: one atomic add per wavefront on one counter.
//   trellis Cb vvcgpu_depquant_listed_launch (depquant.hip) over the Cb list.
//   select     per entry of the Cr list: rates_idx and lambda of the record from dq[3 p + 1] or dq[3 p + 2] by abs_sum of the slot's Cb item.  A launch
//              of its own: the trellis reads its records through const __restrict__ pointers, and another compute unit's abs_sum is only guaranteed
//              visible across a kernel boundary.
//   trellis Cr the same launch over the Cr list.
//   back       persistent workgroups of twelve wavefronts, a wavefront per item (PU, slot, component): the dependent de-quantiser and the inverse
//              transform when abs_sum != 0, clip(parked pred + resi') to cand_rec_base, xGetSSE(org, rec).
#include "common.h"
#include "dist_dev.h"
#include "dqpass_dev.h"
#include "intra_dev.h"
#include "intrachroma_dev.h"

static_assert(sizeof(vvcgpu_intra_chroma_pu) == 96 && sizeof(vvcgpu_intra_fill_desc) == 40 && sizeof(vvcgpu_inter_resi_dq) == 16 && sizeof(vvcgpu_depquant_desc) == 40,
              "descriptor layouts");

namespace {

constexpr int CQ_TILE = 64 * 64;
// front: per wavefront the tile (also the packed references of the gathering), the luma block, top / left, the main reference buffer (also the unit
// table of the gathering), the luma neighbours and the item's chain descriptor
constexpr int CQF_WAVES = 6, CQF_THREADS = 64 * CQF_WAVES;
constexpr int CQF_WAVE_BYTES = (2 * CQ_TILE + 2 * REF_MAX + NEG_MAX + REF_MAX + 2 * 64) * 2 + (int)sizeof(RcDesc);
constexpr int CQF_LDS_BYTES = IQ_TAB_BYTES + CQF_WAVES * CQF_WAVE_BYTES;
// back: per wavefront the tile and the item's chain descriptor
constexpr int CQB_WAVES = 12, CQB_THREADS = 64 * CQB_WAVES;
constexpr int CQB_WAVE_BYTES = CQ_TILE * 2 + (int)sizeof(RcDesc);
constexpr int CQB_LDS_BYTES = IQ_TAB_BYTES + CQB_WAVES * CQB_WAVE_BYTES;
static_assert(IQ_TAB_BYTES % 16 == 0 && CQF_WAVE_BYTES % 16 == 0 && CQB_WAVE_BYTES % 16 == 0 && CQF_LDS_BYTES <= 160 * 1024 && CQB_LDS_BYTES <= 160 * 1024 &&
              (NEG_MAX + REF_MAX) >= FILL_UNITS_MAX, "LDS budget");

struct ChqArgs
{
  ChArgs ch;                                                              // one class: every run of the list, so work index q is PU q
  const IqDq* dq; TCoeff* coef; Pel* park; vvcgpu_depquant_desc* recs; int* listCb; int* listCr; int* count; int* nextCounters;
  long long levelExtent; int nRates;
};

// is the PU served?  The rules of the sibling (ch_pu_ok); here also: sides from 4, level_off a multiple of 16 and not negative -- the trellis workspace
// is indexed by it --, the twelve blocks inside level_extent, the three records with a rate table inside the array, a lambda above zero and luma 0
__device__ __forceinline__ bool chq_pu_ok(const ChqArgs& a, const ChPu& u, int p, int rw, int rh, bool& anyLm)
{
  bool ok = ch_pu_ok(a.ch, u, p, rw, rh, anyLm) && u.w >= 4 && u.h >= 4 && u.level_off >= 0 && (u.level_off & 15) == 0 &&
            u.level_off <= a.levelExtent - 2ll * CH_SLOTS * (int)u.w * (int)u.h;
#pragma unroll
  for (int j = 0; j < 3; j++)
  {
    const IqDq q = a.dq[3 * (size_t)p + j];
    ok = ok && q.rates_idx >= 0 && q.rates_idx < a.nRates && q.lambda > 0.0 && q.luma == 0;
  }
  return ok;
}
__device__ __forceinline__ int chq_slots(const ChPu& u)
{
  int s = 0;
#pragma unroll
  for (int k = 0; k < CH_SLOTS; k++) s += u.mode[k] >= 0 ? 1 : 0;
  return s;
}
// the chain descriptor of an item for the transform bodies: the residual (forward) or resi' (inverse) contiguous in the tile; the coefficients at the
// item's place in the workspace
__device__ __forceinline__ RcDesc chq_desc(int w, int h, int qp, int64_t levelOff)
{
  RcDesc d;
  d.org_off = 0; d.pred_off = 0; d.rec_off = 0; d.level_off = levelOff;
  d.org_stride = w; d.pred_stride = w; d.rec_stride = w; d.w = (int16_t)w; d.h = (int16_t)h;
  d.tr_hor = 0; d.tr_ver = 0; d.intra_slice = 0; d.sign_hiding = 0; d.qp = qp;
  d.reserved[0] = 0; d.reserved[1] = 0;
  return d;
}

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CQF_THREADS, 1) void chroma_dq_front_kernel(const ChqArgs a, const VvcTrTables tb)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const _Float16* const tab = rc_load_image<CQF_THREADS>(smem, a.ch.image, tid);   // below every wavefront walks its own work
  unsigned char* const mine = smem + IQ_TAB_BYTES + (size_t)wave * CQF_WAVE_BYTES;
  short* const tile = reinterpret_cast<short*>(mine);
  short* const lumaS = tile + CQ_TILE;
  short* const topS = lumaS + CQ_TILE;
  short* const leftS = topS + REF_MAX;
  short* const mainS = leftS + REF_MAX;
  short* const lumaTop = mainS + NEG_MAX + REF_MAX;
  short* const lumaLeft = lumaTop + 64;
  RcDesc* const dS = reinterpret_cast<RcDesc*>(mine + CQF_WAVE_BYTES - sizeof(RcDesc));
  int* const fbScr = a.ch.fbScratch + ((size_t)blockIdx.x * CQF_WAVES + wave) * IQ_FB_INTS;
  if (blockIdx.x == 0 && tid < VVC_CTR_INTS) a.nextCounters[tid] = 0;    // the counter set of the NEXT call on this stream (vvcgpu_counters)

  // the wavefront's run in the two work lists (they have one length: a served slot is one Cb and one Cr item): its served slots are counted first
  const int first = (int)blockIdx.x + (int)gridDim.x * wave, step = (int)gridDim.x * CQF_WAVES;
  // a lane per PU.  Its run is found by a ROLLED walk over the runs, not by ch_locate: ch_locate is unrolled over its 36 runs for a wave-uniform index,
  // and inside a loop as small as this one the compiler's loop unswitching takes up its 36 loop-invariant conditions (s < nSeg) one after the other
  // -- hipcc -O3 did not finish this file in 40 minutes with ch_locate here, and finishes it in 4 s with this walk.  Do not "restore" ch_locate.
  int cnt = 0;
  for (long long q = first + (long long)lane * step; q < a.ch.total; q += 64ll * step)
  {
    const int p = (int)q;                                                 // one class: work index q is PU q
    int rw = 0, rh = 0;
#pragma nounroll
    for (int s = 0; s < a.ch.nSeg; s++)
    {
      const ChSeg g = a.ch.seg[s];
      if (p >= g.first && p - g.first < g.count) { rw = g.w; rh = g.h; }
    }
    const ChPu u = a.ch.pus[p];
    bool anyLm;
    if (chq_pu_ok(a, u, p, rw, rh, anyLm)) cnt += chq_slots(u);
  }
  int listAt = iq_reserve(a.count, cnt, lane);

  for (int q = first; q < a.ch.total; q += step)
  {
    int rw, rh;
    const int p = ch_locate(a.ch, q, rw, rh);
    const ChPu u = a.ch.pus[p];
    bool anyLm;
    if (!chq_pu_ok(a, u, p, rw, rh, anyLm)) { ch_mark(a.ch, p, 0, CH_SLOTS, -1, lane); continue; }
    const int w = u.w, h = u.h, samples = w * h, lw = ilog2(w);
    const bool aboveAvail = u.above_avail != 0, leftAvail = u.left_avail != 0;
    int T, L;
    intra_ref_lengths(w, h, T, L);
    if (anyLm) ch_stage_luma(a.ch.luma + u.luma_off, u.luma_stride, w, h, aboveAvail, leftAvail, lane, lumaS, lumaTop, lumaLeft);

#pragma nounroll
    for (int c = 0; c < 2; c++)
    {
      ch_stage_refs(a.ch, u, p, c, T, L, lane, tile, mainS, topS, leftS);
      wave_sync();
      int lmA = 0, lmB = 0, lmShift = 0;
      if (anyLm)
        cclm_params(w, h, aboveAvail, leftAvail, [&](int i) { return (int)lumaTop[i]; }, [&](int i) { return (int)lumaLeft[i]; }, topS + 1, leftS + 1,
                    a.ch.bd, a.ch.bd, lane, lmA, lmB, lmShift);
      const Pel* org = a.ch.org + CH_SEL(org_off, c);
      const IqDq dq = a.dq[3 * (size_t)p + c];                           // Cr: the record of a Cb block without a level, until the select step has looked
      int* const list = c ? a.listCr : a.listCb;
      int at = listAt;
#pragma nounroll
      for (int k = 0; k < CH_SLOTS; k++)
      {
        const int mode = ch_mode(u, k);
        if (mode < 0) { ch_mark(a.ch, p, k, k + 1, c, lane); continue; }
        const int item = 12 * p + 2 * k + c;
        const int64_t off = (int64_t)(2 * k + c) * samples;
        ch_predict(mode, w, h, T, L, topS, leftS, mainS + NEG_MAX, lumaS, lmA, lmB, lmShift, a.ch.cmin, a.ch.cmax, lane, tile);
        if (a.ch.writePred) { Pel* dst = a.ch.pred + u.cand_off + off; for (int e = lane; e < samples; e += 64) dst[e] = tile[e]; }
        {
          Pel* park = a.park + u.level_off + off;                         // for the back
          for (int e = lane; e < samples; e += 64) park[e] = tile[e];
        }
        if (lane == 0)                                                    // the chain descriptor, the trellis record and its list entry
        {
          *dS = chq_desc(w, h, CH_SEL(qp, c), u.level_off + off);
          a.recs[item] = iq_record(u.level_off + off, CH_SEL(qp, c), w, h, dq, 0);
          list[at] = item;
        }
        at++;
        for (int e = lane; e < samples; e += 64) tile[e] = (short)((int)org[(ptrdiff_t)(e >> lw) * u.org_stride + (e & (w - 1))] - (int)tile[e]);
        wave_sync();
        iq_transform<RC_FWD>(dS, tile, nullptr, a.coef, a.ch.bd, tab, tb, fbScr, lane);
        wave_sync();                                                      // the tile and the descriptor are free again
      }
      if (c) listAt = at;
    }
  }
}

// the Cr records take the table and the lambda that Cb's result of the same slot asks for
__global__ __launch_bounds__(256) void chroma_dq_select_kernel(vvcgpu_depquant_desc* __restrict__ recs, const int* __restrict__ listCr, const int* __restrict__ count,
                                                               const unsigned* __restrict__ absSum, const IqDq* __restrict__ dq)
{
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= *count) return;
  const int item = listCr[t], p = item / 12;
  const IqDq q = dq[3 * (size_t)p + (absSum[item - 1] != 0u ? 2 : 1)];
  recs[item].lambda = q.lambda;
  recs[item].rates_idx = q.rates_idx;
}

__global__ __launch_bounds__(CQB_THREADS, 1) void chroma_dq_back_kernel(const ChqArgs a, const VvcTrTables tb)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const _Float16* const tab = rc_load_image<CQB_THREADS>(smem, a.ch.image, tid);   // below every wavefront walks its own work
  unsigned char* const mine = smem + IQ_TAB_BYTES + (size_t)wave * CQB_WAVE_BYTES;
  short* const tile = reinterpret_cast<short*>(mine);
  RcDesc* const dS = reinterpret_cast<RcDesc*>(mine + CQB_WAVE_BYTES - sizeof(RcDesc));
  int* const fbScr = a.ch.fbScratch + ((size_t)blockIdx.x * CQB_WAVES + wave) * IQ_FB_INTS;

  const long long items = 12ll * a.ch.total;
  for (long long item = (long long)blockIdx.x + (long long)gridDim.x * wave; item < items; item += (long long)gridDim.x * CQB_WAVES)
  {
    const int q = (int)(item / 12), s = (int)(item - 12ll * q), k = s >> 1, c = s & 1;
    int rw, rh;
    const int p = ch_locate(a.ch, q, rw, rh);
    const ChPu u = a.ch.pus[p];
    bool anyLm;
    if (!chq_pu_ok(a, u, p, rw, rh, anyLm) || ch_mode(u, k) < 0) continue;   // (the front wrote the markers)
    const int w = u.w, h = u.h, samples = w * h;
    const int64_t off = (int64_t)s * samples;
    short* const backT = iq_back_tile(tile, w, h);
    const bool coded = a.ch.absSum[item] != 0u;                           // all levels zero: resi' is zero (piResi.fill(0))
    if (coded) iq_decode(chq_desc(w, h, CH_SEL(qp, c), u.level_off + off), dS, tile, backT, a.ch.level, a.coef, a.ch.bd, tab, tb, fbScr, lane);
    // clip(pred + resi') with the prediction as the front formed it to cand_rec_base (rows w apart), xGetSSE(org, rec)
    const unsigned long long sse = iq_close(a.ch.org + CH_SEL(org_off, c), u.org_stride, a.park + u.level_off + off, backT, coded,
                                            a.ch.candRec + u.cand_off + off, w, nullptr, w, samples, a.ch.cmin, a.ch.cmax, lane, nullptr);
    if (lane == 0) a.ch.dist[item] = sse;
    wave_sync();                                                          // the tile and the descriptor are free again
  }
}

}  // namespace

extern "C" {

size_t vvcgpu_intra_chroma_code_dq_workspace_bytes(size_t level_extent, int n)
{
  // parked predictions; per item (twelve per PU) a trellis record and an entry of the Cb or the Cr work list
  return iq_layout(level_extent, n, 2 * CH_SLOTS, true).bytes;
}

int vvcgpu_intra_chroma_code_dq_batch(const vvc_pel* rec_base, const uint8_t* flags_base, const vvcgpu_intra_fill_desc* fill, vvc_pel* refs_base,
                                      const vvc_pel* luma_base, const vvc_pel* org_base, const vvcgpu_intra_chroma_pu* pus, const vvcgpu_inter_resi_dq* dq, int n,
                                      const int32_t* runs_host, int n_runs, const vvcgpu_dq_rates* rates, int n_rates, int quantiser,
                                      vvc_pel* pred_base, vvc_pel* cand_rec_base, vvc_coef* level_base, size_t level_extent,
                                      int flags, int bit_depth, int clp_min, int clp_max, uint32_t* abs_sum, uint64_t* dist,
                                      void* ws, size_t ws_bytes, void* stream)
{
  const char* name = "intra_chroma_code_dq_batch";
  VVC_CHECK_ARG(n >= 0, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(n <= 0x7FFFFFFF / 12, "%s: n %d", name, n);               // item indices are ints
  VVC_CHECK_ARG(org_base && pus && runs_host && cand_rec_base && level_base && abs_sum && dist && dq && rates && ws, "%s: null pointer", name);
  VVC_CHECK_ARG((fill != nullptr) == (rec_base != nullptr) && (fill != nullptr) == (flags_base != nullptr), "%s: fill, rec_base and flags_base go together", name);
  VVC_CHECK_ARG(fill || refs_base, "%s: neither fill nor refs_base", name);
  VVC_CHECK_ARG((flags & ~VVCGPU_INTRA_CHROMA_WRITE_PRED) == 0, "%s: unknown flags 0x%x", name, flags);
  VVC_CHECK_ARG(pred_base || !(flags & VVCGPU_INTRA_CHROMA_WRITE_PRED), "%s: null pointer (pred_base with VVCGPU_INTRA_CHROMA_WRITE_PRED)", name);
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "%s: clip range %d..%d", name, clp_min, clp_max);
  VVC_CHECK_ARG(((uintptr_t)pus & 15) == 0 && ((uintptr_t)fill & 15) == 0 && ((uintptr_t)dq & 7) == 0,
                "%s: descriptor arrays must be 16-byte, dq array 8-byte aligned", name);
  VVC_CHECK_ARG(n_runs >= 1, "%s: n_runs %d", name, n_runs);
  ChqArgs a;
  a.ch.nSeg = 0; a.ch.total = 0;
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
    ChSeg& s = a.ch.seg[a.ch.nSeg++];                                     // (a run with a 2-sample side too: its PUs get the markers on the device)
    s.first = (int)sum; s.count = count; s.w = (short)w; s.h = (short)h;
    a.ch.total += count;
    sum += count;
  }
  VVC_CHECK_ARG(sum == n, "%s: the run counts sum to %lld, n is %d", name, sum, n);
  const IqLayout lay = iq_layout(level_extent, n, 2 * CH_SLOTS, true);
  if (const int rc = iq_check_frame(name, n, "PUs", n_rates, level_extent, ws, ws_bytes, lay.bytes, quantiser, quantiser == VVCGPU_INTRA_CHROMA_Q_DEPQUANT, bit_depth))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int wgsF = vvc_grid_cap(n, 1, 1), wgsB = vvc_grid_cap(12ll * n, 1, 1);
  VVC_HIP(vvc_allow_lds(chroma_dq_front_kernel, CQF_LDS_BYTES));
  VVC_HIP(vvc_allow_lds(chroma_dq_back_kernel, CQB_LDS_BYTES));
  VvcScratch sc(st);
  IqSetup s;
  const size_t fbWaves = (size_t)wgsF * CQF_WAVES > (size_t)wgsB * CQB_WAVES ? (size_t)wgsF * CQF_WAVES : (size_t)wgsB * CQB_WAVES;
  if (const int rc = iq_setup(st, sc, fbWaves, s)) return rc;
  a.ch.rec = rec_base; a.ch.flags = flags_base; a.ch.fill = fill; a.ch.refs = refs_base; a.ch.luma = luma_base; a.ch.org = org_base; a.ch.pus = pus;
  a.ch.pred = pred_base; a.ch.candRec = cand_rec_base; a.ch.level = level_base; a.ch.absSum = abs_sum; a.ch.dist = reinterpret_cast<unsigned long long*>(dist);
  a.ch.fbScratch = s.fbScratch; a.ch.image = s.image; a.ch.writePred = (flags & VVCGPU_INTRA_CHROMA_WRITE_PRED) ? 1 : 0;
  a.ch.bd = bit_depth; a.ch.cmin = clp_min; a.ch.cmax = clp_max;
  const int slots = n * CH_SLOTS;                                         // the longest a list can be: the Cb list, and behind it the Cr list
  a.dq = dq; a.coef = iq_at<TCoeff>(ws, 0); a.park = iq_at<Pel>(ws, lay.park); a.recs = iq_at<vvcgpu_depquant_desc>(ws, lay.recs);
  a.listCb = iq_at<int>(ws, lay.list); a.listCr = a.listCb + slots;
  a.count = s.count; a.nextCounters = s.nextCounters; a.levelExtent = (long long)level_extent; a.nRates = n_rates;
  unsigned* const dec = iq_at<unsigned>(ws, lay.dec);
  unsigned char* const ctx = iq_at<unsigned char>(ws, lay.ctx);
  hipLaunchKernelGGL(chroma_dq_front_kernel, dim3(wgsF), dim3(CQF_THREADS), CQF_LDS_BYTES, st, a, s.tb);
  VVC_LAUNCH_CHECK_COUNTERS(st);
  if (const int rc = vvcgpu_depquant_listed_launch(a.coef, level_base, a.recs, a.listCb, a.count, slots, rates, bit_depth, abs_sum, dec, ctx, s.tb, st)) return rc;
  hipLaunchKernelGGL(chroma_dq_select_kernel, dim3(cdiv(slots, 256)), dim3(256), 0, st, a.recs, a.listCr, a.count, abs_sum, dq);
  VVC_LAUNCH_CHECK_COUNTERS(st);
  if (const int rc = vvcgpu_depquant_listed_launch(a.coef, level_base, a.recs, a.listCr, a.count, slots, rates, bit_depth, abs_sum, dec, ctx, s.tb, st)) return rc;
  hipLaunchKernelGGL(chroma_dq_back_kernel, dim3(wgsB), dim3(CQB_THREADS), CQB_LDS_BYTES, st, a, s.tb);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
