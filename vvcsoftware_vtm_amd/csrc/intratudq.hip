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
//   trellis  the trellis of depquant_dev.h (depquant_body.inc through dqpass_dev.h) over the listed records: levels and abs_sum of the served items.
//            The grid is sized for n records; workgroups behind the list's end leave at once.
//   back     the same wavefront-per-item walk: the dependent de-quantiser into the coefficient workspace, the inverse transform (RC_INV bodies) with
//            resi' left in the tile, then clip(pred + resi') with the parked prediction to rec_base, xGetSSE(org, rec) and the count of the non-zero
//            levels.  An item with abs_sum == 0 has resi' = 0.
#include "common.h"
#include "dist_dev.h"
#include "dqpass_dev.h"
#include "intra_dev.h"

static_assert(sizeof(vvcgpu_intra_desc) == 32 && sizeof(vvcgpu_resi_chain_desc) == 64 && sizeof(vvcgpu_inter_resi_dq) == 16 && sizeof(vvcgpu_depquant_desc) == 40,
              "descriptor layouts");

namespace {

typedef vvcgpu_inter_resi_dq ItqDq;
constexpr int ITQ_TILE = 64 * 64;                                         // samples of a wavefront's tile: the prediction, then the residual over it; in the back resi'
constexpr int ITQ_WAVES = 12, ITQ_THREADS = 64 * ITQ_WAVES;               // one workgroup per compute unit, as many wavefronts as its LDS holds: neither parent's budget (eight
                                                                          // per compute unit in both) -- twelve measured 12 % faster on the 4K list (docs/OPTIMISATION_LOG.md)
constexpr int ITQ_WAVE_BYTES = (ITQ_TILE + 4 * REF_MAX + NEG_MAX + REF_MAX) * 2 + (int)sizeof(vvcgpu_resi_chain_desc);
constexpr int ITQ_LDS_BYTES = IQ_TAB_BYTES + ITQ_WAVES * ITQ_WAVE_BYTES;  // 159 168 bytes
static_assert(IQ_TAB_BYTES % 16 == 0 && ITQ_WAVE_BYTES % 16 == 0 && ITQ_LDS_BYTES <= 160 * 1024, "LDS budget");
constexpr int ITQ_LIST_INTS = 16, ITQ_LIST_FIRST = 5, ITQ_LIST_MAX = 11;  // a row of list_out of vvcgpu_intra_mode_cand_batch: [0] size, [5 .. 15] uiRdModeList
constexpr int ITQ_FB_INTS = 2 * 4096;                                     // global scratch per wavefront: the integer body's two buffers for an item outside the matrix-core range

struct ItqArgs
{
  const Pel* refs; const vvcgpu_intra_desc* preds; const Pel* org; Pel* pred; Pel* rec; TCoeff* level; const RcDesc* tus; const ItqDq* dq; const int* modeList;
  unsigned* absSum; unsigned* numSig; unsigned long long* dist; int* modeOut; int* fbScratch; const _Float16* image;
  TCoeff* coef; Pel* park; vvcgpu_depquant_desc* recs; int* list; int* count; int* nextCounters; long long levelExtent;
  int n, nRates, writePred, noSmoothing, bd, cmin, cmax;
};

inline __host__ __device__ bool itq_side_ok(int v) { return v >= 4 && v <= 64 && (v & (v - 1)) == 0; }
__device__ __forceinline__ void itq_global_sync()                         // stores of the wavefront to global memory, read back by other lanes of it
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// is the item served, and with which mode and filter decision?  The rules of intratu.hip; here also: level_off a multiple of 16 and not negative -- the
// trellis workspace is indexed by it --, the levels inside level_extent, a rate table inside the array, a lambda above zero
__device__ __forceinline__ bool itq_resolve(const ItqArgs& a, const vvcgpu_intra_desc& p, const RcDesc& t, const ItqDq& q, int& mode, bool& filt)
{
  const int w = t.w, h = t.h;
  mode = p.mode;
  filt = p.filter_refs != 0;
  bool ok = itq_side_ok(w) && itq_side_ok(h) && p.w == w && p.h == h && mode >= VVCGPU_INTRA_TU_FROM_LIST && mode <= VDIA &&
            (mode != VVCGPU_INTRA_TU_PRED_GIVEN || a.pred != nullptr) &&
            t.tr_hor >= 0 && t.tr_hor <= 2 && t.tr_ver >= 0 && t.tr_ver <= 2 && (w <= 32 || t.tr_hor == 0) && (h <= 32 || t.tr_ver == 0) &&
            t.level_off >= 0 && (t.level_off & 15) == 0 && t.level_off <= a.levelExtent - (long long)w * h &&
            q.rates_idx >= 0 && q.rates_idx < a.nRates && q.lambda > 0.0;
  if (ok && mode == VVCGPU_INTRA_TU_FROM_LIST)
  {
    const int row = t.reserved[0], slot = t.reserved[1];
    ok = a.modeList != nullptr && row >= 0 && slot >= 0 && slot < ITQ_LIST_MAX;
    if (ok) ok = slot < a.modeList[ITQ_LIST_INTS * (size_t)row];
    if (ok)
    {
      mode = a.modeList[ITQ_LIST_INTS * (size_t)row + ITQ_LIST_FIRST + slot];
      ok = mode >= PLANAR && mode <= VDIA;
      if (ok) filt = intra_use_filtered(w, h, mode, a.noSmoothing);
    }
  }
  return ok;
}

// the wavefront's part of the dynamic LDS (ITQ_LDS_BYTES): behind the f16 matrices, per wavefront the tile, the reference work arrays of
// intra_pred_block and the item's chain descriptor
struct ItqLds { short* tile; short* topS; short* leftS; short* tmpS; short* mainS; RcDesc* dS; };
__device__ __forceinline__ ItqLds itq_lds(unsigned char* smem, int wave)
{
  unsigned char* const mine = smem + IQ_TAB_BYTES + (size_t)wave * ITQ_WAVE_BYTES;
  ItqLds l;
  l.tile = reinterpret_cast<short*>(mine);
  l.topS = l.tile + ITQ_TILE;                                             // top, left: REF_MAX each; tmp: 2 REF_MAX; main: NEG_MAX + REF_MAX
  l.leftS = l.topS + REF_MAX;
  l.tmpS = l.leftS + REF_MAX;
  l.mainS = l.tmpS + 2 * REF_MAX;
  l.dS = reinterpret_cast<RcDesc*>(mine + ITQ_WAVE_BYTES - sizeof(RcDesc));
  return l;
}
__device__ __forceinline__ _Float16* itq_load_tables(unsigned char* smem, const _Float16* image, int tid)
{
  _Float16* const tab = reinterpret_cast<_Float16*>(smem);
  const uint4* src = reinterpret_cast<const uint4*>(image);
  for (int i = tid; i < IQ_TAB_BYTES / 16; i += ITQ_THREADS) reinterpret_cast<uint4*>(tab)[i] = src[i];
  __syncthreads();                                                        // the only workgroup barrier: below every wavefront walks its own items
  return tab;
}
// the prediction of a served item into the tile, rows w apart: read from pred_base, or predIntraAng
__device__ __forceinline__ void itq_predict(const ItqArgs& a, const vvcgpu_intra_desc& p, const RcDesc& t, int mode, bool filt, const ItqLds& l, int lane)
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
__global__ __launch_bounds__(ITQ_THREADS, 1) void intra_tu_dq_front_kernel(const ItqArgs a, const VvcTrTables tb)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const _Float16* const tab = itq_load_tables(smem, a.image, tid);
  const ItqLds l = itq_lds(smem, wave);
  int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * ITQ_WAVES + wave) * ITQ_FB_INTS;
  if (blockIdx.x == 0 && tid < VVC_CTR_INTS) a.nextCounters[tid] = 0;    // the counter set of the NEXT call on this stream (vvcgpu_counters)

  // the wavefront's run in the trellis' work list: its served items are counted first, a lane per item, so that the counter sees one atomic add per
  // wavefront (docs/KERNELS.md: one per item was 0.9 ms for the inter pass on the 4K list)
  const int first = (int)blockIdx.x + (int)gridDim.x * wave, step = (int)gridDim.x * ITQ_WAVES;
  int listAt = 0;
  {
    int cnt = 0;
    for (int item = first + lane * step; item < a.n; item += 64 * step)
    {
      int mode; bool filt;
      cnt += itq_resolve(a, a.preds[item], a.tus[item], a.dq[item], mode, filt) ? 1 : 0;
    }
    cnt = wave_sum_i32(cnt);
    if (cnt && lane == 0) listAt = atomicAdd(a.count, cnt);
    listAt = __builtin_amdgcn_readfirstlane(listAt);
  }

  for (int item = first; item < a.n; item += step)
  {
    const vvcgpu_intra_desc p = a.preds[item];
    const RcDesc t = a.tus[item];
    const ItqDq q = a.dq[item];
    int mode; bool filt;
    if (!itq_resolve(a, p, t, q, mode, filt))                             // skipped: the markers, nothing else
    {
      if (lane == 0) { a.absSum[item] = 0xFFFFFFFFu; a.numSig[item] = 0xFFFFFFFFu; a.dist[item] = ~0ull; a.modeOut[item] = -1; }
      continue;
    }
    const int w = t.w, h = t.h, lw = ilog2(w), samples = w * h;
    itq_predict(a, p, t, mode, filt, l, lane);
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
      vvcgpu_depquant_desc r;
      r.coeff_off = r.level_off = t.level_off;
      r.lambda = q.lambda; r.qp = t.qp; r.rates_idx = q.rates_idx; r.w = (int16_t)w; r.h = (int16_t)h; r.luma = q.luma;
      r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
      a.recs[item] = r;
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
    iq_transform<RC_FWD>(l.dS, l.tile, nullptr, a.coef, a.bd, tab, tb, fbScr, lane);
    wave_sync();                                                          // the tile and the descriptor are free again
  }
}

__global__ __launch_bounds__(256) void intra_tu_dq_trellis_kernel(const TCoeff* __restrict__ coeffBase, TCoeff* __restrict__ levelBase,
                                                                  const vvcgpu_depquant_desc* __restrict__ descs, const int* __restrict__ list,
                                                                  const int* __restrict__ count,
                                                                  const vvcgpu_dq_rates* __restrict__ ratesBase, int bd, unsigned* __restrict__ absSumOut,
                                                                  unsigned* __restrict__ wsDec, unsigned char* __restrict__ wsCtx, VvcTrTables tb)
{
  const int n = *count;                                                   // the served items of the call, counted by the front
  if ((int)blockIdx.x * 64 >= n) return;
  iq_trellis<true>(coeffBase, levelBase, descs, list, n, ratesBase, bd, absSumOut, wsDec, wsCtx, tb);
}

__global__ __launch_bounds__(ITQ_THREADS, 1) void intra_tu_dq_back_kernel(const ItqArgs a, const VvcTrTables tb)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const _Float16* const tab = itq_load_tables(smem, a.image, tid);
  const ItqLds l = itq_lds(smem, wave);
  int* const fbScr = a.fbScratch + ((size_t)blockIdx.x * ITQ_WAVES + wave) * ITQ_FB_INTS;

  for (int item = (int)blockIdx.x + (int)gridDim.x * wave; item < a.n; item += (int)gridDim.x * ITQ_WAVES)
  {
    const vvcgpu_intra_desc p = a.preds[item];
    const RcDesc t = a.tus[item];
    int mode; bool filt;
    if (!itq_resolve(a, p, t, a.dq[item], mode, filt)) continue;          // (the front wrote the markers)
    const int w = t.w, h = t.h, lw = ilog2(w), samples = w * h;
    // the tile is where the body leaves resi': at 0, or -- a shape with a side of at most 8 (at most 512 samples) has the integer body's two buffers
    // at 1024 and 2048 -- at 3072
    short* const backT = (w <= 8 || h <= 8) ? l.tile + 3072 : l.tile;
    const bool coded = a.absSum[item] != 0u;                              // all levels zero: resi' is zero (piResi.fill(0), :1293)
    Pel* const rec = a.rec + t.rec_off;
    if (coded)
    {
      if (lane == 0) *l.dS = itq_desc(t);
      const unsigned short* const scan = tb.scan + tb.scanOff[(lw - 1) * 6 + (ilog2(h) - 1)];
      iq_dequant(a.level + t.level_off, a.coef + t.level_off, w, h, t.qp, a.bd, scan, lane);
      itq_global_sync();
      iq_transform<RC_INV>(l.dS, l.tile, backT, a.coef, a.bd, tab, tb, fbScr, lane);
      wave_sync();
    }
    // clip(pred + resi') to rec_base, xGetSSE(org, rec), the non-zero levels
    const Pel* org = a.org + t.org_off;
    const TCoeff* level = a.level + t.level_off;
    const Pel* pred = a.park + t.level_off;                               // as the front formed it
    unsigned long long sse = 0ull;                                        // 64 x 64 x 1023^2 is beyond 2^31
    int nz = 0;
    for (int e = lane; e < samples; e += 64)
    {
      const int r = e >> lw, x = e & (w - 1);
      const int rc = clip3(a.cmin, a.cmax, (int)pred[e] + (coded ? (int)backT[e] : 0));
      const unsigned df = (unsigned)abs((int)org[(ptrdiff_t)r * t.org_stride + x] - rc);
      sse += (unsigned long long)(df * df);
      nz += level[e] != 0;
      rec[(ptrdiff_t)r * t.rec_stride + x] = (short)rc;
    }
    sse = group_sum_u64<64>(sse);
    nz = wave_sum_i32(nz);
    if (lane == 0) { a.dist[item] = sse; a.numSig[item] = (unsigned)nz; }
    wave_sync();                                                          // the tile and the descriptor are free again
  }
}

}  // namespace

extern "C" {

size_t vvcgpu_intra_tu_code_dq_workspace_bytes(size_t level_extent, int n)
{
  const size_t c = iq_extent16(level_extent);
  // the coefficients, the trellis decisions and level histories, the parked predictions (all indexed by the item's level offset), per item a trellis record and a list entry
  return c * sizeof(TCoeff) + tq_dec_bytes(c) + tq_ctx_bytes(c) + c * sizeof(Pel) + (size_t)(n > 0 ? n : 0) * (sizeof(vvcgpu_depquant_desc) + sizeof(int)) + IQ_WS_SLACK;
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
  VVC_CHECK_ARG((flags & ~(VVCGPU_INTRA_TU_WRITE_PRED | VVCGPU_INTRA_TU_NO_SMOOTHING)) == 0, "%s: unknown flags 0x%x", name, flags);
  VVC_CHECK_ARG(pred_base || !(flags & VVCGPU_INTRA_TU_WRITE_PRED), "%s: null pointer (pred_base with VVCGPU_INTRA_TU_WRITE_PRED)", name);
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "%s: clip range %d..%d", name, clp_min, clp_max);
  VVC_CHECK_ARG(((uintptr_t)preds & 15) == 0 && ((uintptr_t)tus & 15) == 0 && ((uintptr_t)dq & 7) == 0,
                "%s: descriptor arrays must be 16-byte, dq array 8-byte aligned", name);
  VVC_CHECK_ARG(n_rates > 0, "%s: n_rates %d", name, n_rates);
  VVC_CHECK_ARG(level_extent >= 16 && level_extent < ((size_t)1 << 40), "%s: level_extent %zu", name, level_extent);
  VVC_CHECK_ARG(ws_bytes >= vvcgpu_intra_tu_code_dq_workspace_bytes(level_extent, n) && ((uintptr_t)ws & 15) == 0,
                "%s: workspace of %zu bytes for a level extent of %zu and %d items is too small (need %zu) or unaligned", name, ws_bytes, level_extent, n,
                vvcgpu_intra_tu_code_dq_workspace_bytes(level_extent, n));
  if (quantiser != VVCGPU_INTRA_TU_Q_DEPQUANT) { vvcgpu_set_error("%s: quantiser %d is not served", name, quantiser); return VVCGPU_E_UNSUPPORTED; }
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("%s: bit depth %d outside 8..10", name, bit_depth); return VVCGPU_E_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  VvcTrTables tb; const _Float16* image = nullptr;
  const int rt = vvcgpu_tr_images(&tb, &image);
  if (rt) return rt;
  const int cap = vvcgpu_cu_count(), wgs = n < cap ? n : cap;             // (the items are dealt to the workgroups first, then to their wavefronts: a short list spreads over the compute units)
  VVC_HIP(vvc_allow_lds(intra_tu_dq_front_kernel, ITQ_LDS_BYTES));
  VVC_HIP(vvc_allow_lds(intra_tu_dq_back_kernel, ITQ_LDS_BYTES));
  VVC_HIP(vvc_allow_lds(intra_tu_dq_trellis_kernel, TQ_LDS_BYTES));
  int cur = 0;
  int* counters = vvcgpu_counters(st, &cur);                              // the list's length: zero on entry, the front clears the other set
  if (!counters) return VVCGPU_E_DEVICE;
  VvcScratch sc(st);
  int* fbScratch = sc.take<int>((size_t)wgs * ITQ_WAVES * ITQ_FB_INTS);   // touched only for an item outside the matrix-core range
  if (!fbScratch) { vvcgpu_counters_failed(st); return VVCGPU_E_DEVICE; }
  // the workspace as vvcgpu_intra_tu_code_dq_workspace_bytes lays it out
  const size_t c = iq_extent16(level_extent);
  unsigned char* const w8 = static_cast<unsigned char*>(ws);
  TCoeff* coef = reinterpret_cast<TCoeff*>(w8);
  unsigned* dec = reinterpret_cast<unsigned*>(w8 + c * sizeof(TCoeff));
  unsigned char* ctx = w8 + c * sizeof(TCoeff) + tq_dec_bytes(c);
  Pel* park = reinterpret_cast<Pel*>(w8 + c * sizeof(TCoeff) + tq_dec_bytes(c) + tq_ctx_bytes(c));
  vvcgpu_depquant_desc* recs = reinterpret_cast<vvcgpu_depquant_desc*>(w8 + c * sizeof(TCoeff) + tq_dec_bytes(c) + tq_ctx_bytes(c) + c * sizeof(Pel));
  ItqArgs a;
  a.refs = refs_base; a.preds = preds; a.org = org_base; a.pred = pred_base; a.rec = rec_base; a.level = level_base; a.tus = tus; a.dq = dq; a.modeList = mode_list;
  a.absSum = abs_sum; a.numSig = num_sig; a.dist = reinterpret_cast<unsigned long long*>(dist); a.modeOut = mode_out; a.fbScratch = fbScratch; a.image = image;
  a.coef = coef; a.park = park; a.recs = recs; a.list = reinterpret_cast<int*>(recs + (size_t)n);
  a.count = counters + VVC_CTR_INTS * cur; a.nextCounters = counters + VVC_CTR_INTS * (cur ^ 1); a.levelExtent = (long long)level_extent;
  a.n = n; a.nRates = n_rates; a.writePred = (flags & VVCGPU_INTRA_TU_WRITE_PRED) ? 1 : 0; a.noSmoothing = (flags & VVCGPU_INTRA_TU_NO_SMOOTHING) ? 1 : 0;
  a.bd = bit_depth; a.cmin = clp_min; a.cmax = clp_max;
  hipLaunchKernelGGL(intra_tu_dq_front_kernel, dim3(wgs), dim3(ITQ_THREADS), ITQ_LDS_BYTES, st, a, tb);
  VVC_LAUNCH_CHECK_COUNTERS(st);
  hipLaunchKernelGGL(intra_tu_dq_trellis_kernel, dim3(cdiv(n, 64)), dim3(256), TQ_LDS_BYTES, st, coef, level_base, recs, a.list, a.count, rates, bit_depth,
                     abs_sum, dec, ctx, tb);
  VVC_LAUNCH_CHECK_COUNTERS(st);
  hipLaunchKernelGGL(intra_tu_dq_back_kernel, dim3(wgs), dim3(ITQ_THREADS), ITQ_LDS_BYTES, st, a, tb);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
