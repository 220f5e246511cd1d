// dqpass_dev.h -- what the RD pass entries under DepQuant 1 share around the trellis of depquant_dev.h, stated once for interresidq.hip
// (vvcgpu_inter_resi_code_dq_batch), intratudq.hip (vvcgpu_intra_tu_code_dq_batch) and intrachromadq.hip (vvcgpu_intra_chroma_code_dq_batch).
// Device side: the transform bodies of resichain_dev.h as real calls on a wavefront's LDS tile (forward into the coefficient workspace, inverse out of
// it), the trellis record of an item and its wavefront's run in the work list, the dependent de-quantiser of one TU by one wavefront, the way of a coded
// item's levels back to resi', and the closing loop over a parked prediction.  Host side: the workspace's layout, the checks of the arguments that the
// three entries have alike, and their set-up.  A front kernel stages the residual in the tile and runs iq_transform<RC_FWD>, the trellis is
// vvcgpu_depquant_listed_launch (depquant.hip), a back kernel runs iq_decode (iq_dequant, iq_transform<RC_INV>); the item walk around them is each
// file's own.  The transform-skip candidate of a 4x4 block takes iq_ts_forward / iq_ts_inverse in the transforms' place.
#pragma once
#include "common.h"
#include "depquant_dev.h"
#include "dist_dev.h"
#include "mfma_tr.h"
#include "quant_dev.h"
#include "resichain_dev.h"

namespace {

typedef vvcgpu_inter_resi_dq IqDq;                                        // the quantiser record of an item, the same struct in the three entries
constexpr int IQ_TAB_BYTES = RC_TAB_HALVES * 2;                           // the f16 matrices of the matrix-core bodies
constexpr int IQ_FB_INTS = 2 * 4096;                                      // global scratch per wavefront: the integer body's two buffers for an item outside the matrix-core range
constexpr size_t IQ_WS_SLACK = 4096 * sizeof(TCoeff) + 256;               // a quad of the trellis that walks along with a larger TU of its wavefront reads up to 4095 coefficients past its own

// The caller's workspace, stated once for the *_workspace_bytes functions and the entries.  Indexed by an item's level offset: the coefficients (at 0),
// the trellis' decisions and level histories and -- parked: the intra entries -- the predictions as the front formed them; behind them a trellis record
// and a work list entry for each of `records` records.  Byte offsets; the level extent counts in whole 16s.
struct IqLayout { size_t dec, ctx, park, recs, list, bytes; };
inline IqLayout iq_layout(size_t level_extent, int n, int recordsPerItem, bool parked)
{
  const size_t c = (level_extent + 15) & ~(size_t)15, records = (size_t)(n > 0 ? n : 0) * recordsPerItem;
  IqLayout l;
  l.dec = c * sizeof(TCoeff);
  l.ctx = l.dec + tq_dec_bytes(c);
  l.park = l.ctx + tq_ctx_bytes(c);
  l.recs = l.park + (parked ? c * sizeof(Pel) : 0);
  l.list = l.recs + records * sizeof(vvcgpu_depquant_desc);
  l.bytes = l.list + records * sizeof(int) + IQ_WS_SLACK;
  return l;
}
template <class T> inline T* iq_at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<unsigned char*>(ws) + off); }

// the transform bodies as real calls (the descriptor and the tile are the wavefront's, in LDS)
template <int W, int H, int MODE>
__device__ __noinline__ bool iq_tu_mfma_call(const RcDesc* dS, const Pel* tile, Pel* __restrict__ outBase, TCoeff* __restrict__ coefBase, int bd, const _Float16* tab,
                                             const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff, int lane)
{
  RC_IS_LDS(dS); RC_IS_LDS(tile); RC_IS_LDS(tab);
  return rc_tu_mfma<W, H, MODE>(*dS, tile, tile, outBase, coefBase, nullptr, 0, bd, 0, 0, tab, dqInv, scanOff, lane);
}
template <int MODE>
__device__ __noinline__ void iq_tu_generic_call(const RcDesc* dS, const Pel* tile, Pel* __restrict__ outBase, TCoeff* __restrict__ coefBase, int bd,
                                                const int* __restrict__ tr32, const unsigned short* __restrict__ dqInv, const int* __restrict__ scanOff,
                                                int* bufA, int* bufB, int lane)
{
  rc_tu_generic<MODE>(*dS, tile, tile, outBase, coefBase, nullptr, 0, bd, 0, 0, tr32, dqInv, scanOff, bufA, bufB, lane, nullptr);
}
// one TU through the forward (MODE RC_FWD: tile -> coefficients) or the inverse transform (RC_INV: coefficients -> outBase + rec_off)
template <int MODE>
__device__ __forceinline__ void iq_transform(const RcDesc* dS, short* resiT, Pel* outBase, TCoeff* coefBase, int bd, const _Float16* tab, const VvcTrTables& tb,
                                             int* fbScr, int lane)
{
  const int w = dS->w, h = dS->h;
  if (w <= 8 || h <= 8)                                                   // at most 512 samples: the integer body, its two buffers behind them in the tile
  {
    iq_tu_generic_call<MODE>(dS, resiT, outBase, coefBase, bd, tb.tr32, tb.dqInv, tb.scanOff, reinterpret_cast<int*>(resiT + 1024), reinterpret_cast<int*>(resiT + 2048), lane);
    return;
  }
  bool done = true;
#define IQ_MF(W_, H_) case ((W_) << 8) | (H_): done = iq_tu_mfma_call<W_, H_, MODE>(dS, resiT, outBase, coefBase, bd, tab, tb.dqInv, tb.scanOff, lane); break;
  switch ((w << 8) | h)
  {
  IQ_MF(16, 16) IQ_MF(16, 32) IQ_MF(16, 64) IQ_MF(32, 16) IQ_MF(32, 32) IQ_MF(32, 64) IQ_MF(64, 16) IQ_MF(64, 32) IQ_MF(64, 64)
  default: break;
  }
#undef IQ_MF
  if (!done)                                                              // samples outside the bit depth (out of contract): exact all the same
    iq_tu_generic_call<MODE>(dS, resiT, outBase, coefBase, bd, tb.tr32, tb.dqInv, tb.scanOff, fbScr, fbScr + 4096, lane);
}

// the trellis record of a w x h block whose coefficients and levels lie at `off`
__device__ __forceinline__ vvcgpu_depquant_desc iq_record(int64_t off, int qp, int w, int h, const IqDq& q, int luma)
{
  vvcgpu_depquant_desc r;
  r.coeff_off = r.level_off = off;
  r.lambda = q.lambda; r.qp = qp; r.rates_idx = q.rates_idx; r.w = (int16_t)w; r.h = (int16_t)h; r.luma = (int8_t)luma;
  r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
  return r;
}
// The wavefront's run in the trellis' work list, of as many entries as its lanes have counted served records (cnt) -> the run's first index.  The
// records are counted first so that the counter sees one atomic add per wavefront (one per item, 94 000 on one address for the inter pass on the 4K
// list, took 0.9 ms)
__device__ __forceinline__ int iq_reserve(int* count, int cnt, int lane)
{
  int listAt = 0;
  cnt = wave_sum(cnt);
  if (cnt && lane == 0) listAt = atomicAdd(count, cnt);
  return __builtin_amdgcn_readfirstlane(listAt);
}

// DQIntern::Quantizer::dequantBlock (DepQuant.cpp:708-785) of one TU by the wavefront: levels -> coefficients, both w x h with row pitch w.  The 4-state
// machine is linear over GF(2) (transform.hip, dq_group): with steps counted from the END of the scan, the state bit that enters the reconstruction of
// step t is the xor of the level parities of the earlier steps of the other step parity.  A lane takes a run of consecutive steps, folds its parities by
// step parity, a ballot gives the prefix over the lanes in front of it, a second pass reconstructs.
__device__ __forceinline__ void iq_dequant(const TCoeff* __restrict__ level, TCoeff* __restrict__ coef, int w, int h, int qp, int bd,
                                           const unsigned short* __restrict__ scan, int lane)
{
  const int lw = ilog2(w), lh = ilog2(h), cnt = w * h;
  const VqInv dep = vq_inv(qp + 1, vq_transform_shift(bd, lw, lh), vq_sqrt2(lw, lh));      // scale and shift of qp + 1 with one more bit (:758-759)
  int shift = dep.rightShift + 1;
  long long scale = dep.scale;
  if (shift < 0) { scale <<= -shift; shift = 0; }
  const long long add = (1ll << shift) >> 1;
  const int C = cnt >= 64 ? cnt >> 6 : 1, t0 = lane * C, t1 = min(t0 + C, cnt);
  int a0 = 0, a1 = 0;
  for (int t = t0; t < t1; t++)
  {
    const int lv = level[scan[cnt - 1 - t]];
    if (t & 1) a1 ^= lv; else a0 ^= lv;
  }
  const unsigned long long B0 = __builtin_amdgcn_ballot_w64((a0 & 1) != 0), B1 = __builtin_amdgcn_ballot_w64((a1 & 1) != 0);
  const unsigned long long below = (1ull << lane) - 1ull;
  int x0 = (int)__popcll(B0 & below) & 1, x1 = (int)__popcll(B1 & below) & 1;
  for (int t = t0; t < t1; t++)
  {
    const int pos = scan[cnt - 1 - t], lv = level[pos], hi = (t & 1) ? x0 : x1;
    int v = 0;
    if (lv != 0)
    {
      const int qIdx = 2 * lv + (lv > 0 ? -hi : hi);
      v = (int)min(max(((long long)qIdx * scale + add) >> shift, -(1ll << 15)), (1ll << 15) - 1);
    }
    coef[pos] = v;
    if (t & 1) x1 ^= lv & 1; else x0 ^= lv & 1;
  }
}

// The transform-skip candidate of a 4x4 block (TU::hasTransformSkipFlag with Log2MaxTransformSkipBlockSize 2; rotation and RDPCM are range extensions,
// off): TrQuant::transformNxN hands the scaled residual to the same DepQuant::quant, and dequantBlock does not look at tu.transformSkip without extended
// precision, so only the scaling around the trellis differs.  The shift is getTransformShift of the shape, 15 - bd - 2 (3 at 10 bits, 5 at 8); 4x4 needs
// no needsBlockSizeTrafoScale.  Sixteen lanes, an element each.
__device__ __forceinline__ int iq_ts_shift(int bd) { return 15 - bd - 2; }
// xTransformSkip (TrQuant.cpp:1140-1148): the residual, contiguous in the tile -> the sixteen coefficients
__device__ __forceinline__ void iq_ts_forward(const short* resiT, TCoeff* __restrict__ coef, int bd, int lane)
{
  if (lane < 16) coef[lane] = (int)resiT[lane] * (1 << iq_ts_shift(bd));
}
// xITransformSkip (TrQuant.cpp:823-833): the sixteen de-quantised coefficients -> resi' in backT
__device__ __forceinline__ void iq_ts_inverse(const TCoeff* __restrict__ coef, short* backT, int bd, int lane)
{
  const int shift = iq_ts_shift(bd);
  if (lane < 16) backT[lane] = (short)((coef[lane] + (1 << (shift - 1))) >> shift);
}

// Where the inverse body leaves resi' of a wavefront that keeps nothing else in its tile: at 0, or -- a shape with a side of at most 8 (at most 512
// samples) has the integer body's two buffers at 1024 and 2048 -- at 3072
__device__ __forceinline__ short* iq_back_tile(short* tile, int w, int h) { return (w <= 8 || h <= 8) ? tile + 3072 : tile; }
// The levels of a coded item (abs_sum != 0) back to resi' in backT: the dependent de-quantiser into the coefficient workspace, then the inverse
// transform.  d: the item's chain descriptor, put into the wavefront's dS (LDS) for the bodies.  tskip: the item is the transform-skip candidate of a
// 4x4 block -- the same de-quantiser, then the scaling back in place of the inverse transform
__device__ __forceinline__ void iq_decode(const RcDesc& d, RcDesc* dS, short* tile, short* backT, const TCoeff* level, TCoeff* coef, int bd, const _Float16* tab,
                                          const VvcTrTables& tb, int* fbScr, int lane, bool tskip = false)
{
  if (lane == 0) *dS = d;
  const unsigned short* const scan = tb.scan + tb.scanOff[(ilog2(d.w) - 1) * 6 + (ilog2(d.h) - 1)];
  iq_dequant(level + d.level_off, coef + d.level_off, d.w, d.h, d.qp, bd, scan, lane);
  wave_global_sync();
  if (tskip) iq_ts_inverse(coef + d.level_off, backT, bd, lane);
  else iq_transform<RC_INV>(dS, tile, backT, coef, bd, tab, tb, fbScr, lane);
  wave_sync();
}
// The closing loop of an intra item: clip(parked pred + resi') to rec (rows recStride apart), with resi' in backT if the item is coded and zero if not
// (piResi.fill(0)) -> xGetSSE(org, rec) and, if level is not null, the number of its non-zero levels; both summed over the wavefront
__device__ __forceinline__ unsigned long long iq_close(const Pel* org, ptrdiff_t orgStride, const Pel* pred, const short* backT, bool coded, Pel* rec,
                                                       ptrdiff_t recStride, const TCoeff* level, int w, int samples, int cmin, int cmax, int lane, int* numSig)
{
  const int lw = ilog2(w);
  unsigned long long sse = 0ull;                                          // 64 x 64 x 1023^2 is beyond 2^31
  int nz = 0;
  for (int e = lane; e < samples; e += 64)
  {
    const int r = e >> lw, x = e & (w - 1);
    const int rc = clip3(cmin, cmax, (int)pred[e] + (coded ? (int)backT[e] : 0));
    const unsigned df = (unsigned)abs((int)org[r * orgStride + x] - rc);
    sse += (unsigned long long)(df * df);
    if (level) nz += level[e] != 0;
    rec[r * recStride + x] = (short)rc;
  }
  if (level) *numSig = wave_sum(nz);
  return group_sum<64>(sse);
}

// ---- host side of the three entries.  `name` is the entry's name as the error text starts with it; a check returns VVCGPU_OK or the error code with the
// text set.  The checks every entry makes behind its own, in the order in which a call with several faults reports them: n_rates, level_extent, the
// workspace (need: bytes of the entry's iq_layout; unit: what n counts in its text), the quantiser (served: it is the entry's DEPQUANT value), bit depth
inline int iq_check_frame(const char* name, int n, const char* unit, int n_rates, size_t level_extent, const void* ws, size_t ws_bytes, size_t need,
                          int quantiser, bool served, int bit_depth)
{
  VVC_CHECK_ARG(n_rates > 0, "%s: n_rates %d", name, n_rates);
  VVC_CHECK_ARG(level_extent >= 16 && level_extent < ((size_t)1 << 40), "%s: level_extent %zu", name, level_extent);
  VVC_CHECK_ARG(ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
                "%s: workspace of %zu bytes for a level extent of %zu and %d %s is too small (need %zu) or unaligned", name, ws_bytes, level_extent, n, unit, need);
  if (!served) { vvcgpu_set_error("%s: quantiser %d is not served", name, quantiser); return VVCGPU_E_UNSUPPORTED; }
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("%s: bit depth %d outside 8..10", name, bit_depth); return VVCGPU_E_UNSUPPORTED; }
  return VVCGPU_OK;
}
// What an entry's launches need besides its own arguments: the tables and the f16 image, the call's counter set (count: the work list's length, zero on
// entry; the front kernel clears nextCounters, the set of the next call on the stream) and IQ_FB_INTS of global scratch for each of fbWaves wavefronts
// (touched only for an item outside the matrix-core range).  A failure behind the counters reports their set.
struct IqSetup { VvcTrTables tb; const _Float16* image; int* count; int* nextCounters; int* fbScratch; };
inline int iq_setup(hipStream_t st, VvcScratch& sc, size_t fbWaves, IqSetup& s)
{
  if (const int rt = vvcgpu_tr_images(&s.tb, &s.image)) return rt;
  int cur = 0;
  int* const counters = vvcgpu_counters(st, &cur);
  if (!counters) return VVCGPU_E_DEVICE;
  s.count = counters + VVC_CTR_INTS * cur; s.nextCounters = counters + VVC_CTR_INTS * (cur ^ 1);
  s.fbScratch = sc.take<int>(fbWaves * IQ_FB_INTS);
  if (!s.fbScratch) { vvcgpu_counters_failed(st); return VVCGPU_E_DEVICE; }
  return VVCGPU_OK;
}

}  // namespace
