// unipredme.hip -- the whole uni-predictive stage of the translational inter search of a PU (vvcgpu_unipred_me_batch) for gfx950.
//
// Reference behaviour reproduced (bit-exact, the double arithmetic of the costs included): the uni-predictive loop of InterSearch::predInterSearch
// (EncoderLib/InterSearch.cpp:877-964) with xEstimateMvPredAMVP (:1443-1483, bFilled = true) / xGetTemplateCost (:1606-1642), xMotionEstimation
// (bBi = false, :1668-1816): xTZSearch (:1971-2252; tz_dev.h) and xPatternSearchFracDIF (:2503-2552; frac_dev.h), and xCheckBestMVP (:1537-1603;
// me_dev.h); the mvd_l1_zero preparation of the bi-predictive stage (:1009-1023, :1038) for the out-items.
//
// Design: the (list, reference index) searches of a PU depend on each other only through the list-1 shortcut and the final comparisons, and one TZ
// search is a chain of about 20 dependent rounds, so the unit of ownership is the SEARCH: launch 1 gives each of the n x (n_ref[0] + n_ref[1])
// searches an owner -- one wavefront up to UP_WAVE_MAX samples, the workgroup's four above (the owner model: owner_dev.h and docs/KERNELS.md, "Owners
// of the whole-PU entries") -- which chooses the AMVP
// predictor (prediction of each candidate straight into its SAD against the original in LDS, never stored), runs the TZ state machine as a team
// (the sub-sampled original as packed pairs in the work area), the fractional refinement (window, first-stage plane and candidate block in the same
// work area) and xCheckBestMVP, and writes its record into the PU's result.  A list-1 reference that takes list 0's vector only chooses its
// predictor.  Launch 2, one lane per PU, walks the records in the reference's order: the list-1 shortcut, bestBiP*, keep-if-strictly-better, the
// valid-list-1 record, the out-item for vvcgpu_bipred_me_batch, and everything a skipped item gets.  Control flow is uniform per owner.
// AMVR passes (cfg.imv = 1, 2; its own instantiation of launch 1, chosen by the host): imvShift = imv << 1 in the TZ cost, xPatternSearchIntRefine
// (:2408-2500; me_imv_refine of me_dev.h) for the fractional refinement and its cost, no xCheckBestMVP (:1543-1546), the shortcut's vector bits with
// >> imvShift (:916).
#include "common.h"
#include "frac_dev.h"
#include "me_dev.h"
#include "tz_dev.h"
#include "pu_entry_host.h"

namespace {

constexpr int UP_WAVE_MAX = 1024;                       // samples a wavefront owns
constexpr int UP_SEG = 64 * TZ_SEG_REGS + 4;            // dwords of one wavefront's raster chunk
constexpr int UP_HDR = 1024;                            // bytes in front of the raster chunks: see up_lds

inline __host__ __device__ int up_hdr_bytes(int nt) { return UP_HDR + (nt >> 6) * UP_SEG * 4; }
// the work area holds the fractional refinement's three buffers (the first pass of a prediction, w x (h + 7), and the packed original of the integer
// search, at most w x h, are smaller)
inline __host__ __device__ int up_lds_bytes(int w, int h, int nt) { return up_hdr_bytes(nt) + 2 * (frac_r8(w * h) + frac_work_shorts(w, h)); }

struct UpLds : FracOwnerLds       // frac_dev.h: bytes 0..575 of the header; F.org = the original
{
  unsigned long long* keyL;       // bytes 576..607: the wavefronts' keys of a TZ round
  int* negL;                      // bytes 608..623
  unsigned long long* part;       // bytes 640..671: the wavefronts' partial SADs of a candidate's prediction
  unsigned* seg;                  // UP_HDR ..: one raster chunk per wavefront
};
static_assert(FRAC_HDR == 576 && 640 + 4 * 8 <= UP_HDR && UP_HDR % 16 == 0, "header layout");

template <int NT> __device__ __forceinline__ UpLds up_lds(unsigned char* base, int w, int h)
{
  UpLds L;
  frac_owner_lds(L, base, up_hdr_bytes(NT), w, h);
  L.keyL = reinterpret_cast<unsigned long long*>(base + FRAC_HDR);
  L.negL = reinterpret_cast<int*>(base + 608);
  L.part = reinterpret_cast<unsigned long long*>(base + 640);
  L.seg = reinterpret_cast<unsigned*>(base + UP_HDR);
  return L;
}

__device__ __forceinline__ bool up_item_ok(const vvcgpu_unipred_me_item& it, const vvcgpu_unipred_me_cfg& c)
{
  const int w = it.w, h = it.h;
  if (!pu_side_pow2_ok(w) || !pu_side_pow2_ok(h) || w > c.max_cu_w || h > c.max_cu_h || w > c.max_pu_w || h > c.max_pu_h) return false;
  if (it.pos_x < 0 || it.pos_y < 0 || it.pos_x > c.pic_w - w || it.pos_y > c.pic_h - h) return false;
  if (it.sub_shift < 0 || it.sub_shift > 1 || (h >> it.sub_shift) == 0 || it.org_stride <= 0) return false;
  if ((it.tz_flags & ~VVCGPU_TZ_EXTENDED) != 0) return false;
  for (int l = 0; l < 2; l++)
    for (int r = 0; r < c.n_ref[l]; r++)
    {
      const vvcgpu_unipred_me_ref& a = it.ref[l][r];
      if (a.num_cand < 1 || a.num_cand > 2 || a.flags < 0 || a.flags > (VVCGPU_UNIPRED_PRED2 | VVCGPU_UNIPRED_CACHED)) return false;
    }
  return true;
}

__device__ __forceinline__ bool up_shortcut(const vvcgpu_unipred_me_cfg& c, int list, int r) { return list == 1 && c.fast_me_gen_b_low_delay && c.list1_to_list0[r] >= 0; }

// one (list, reference index) search of a PU by NT lanes
template <int NT, bool IMV>
__device__ __forceinline__ void up_search(const vvcgpu_unipred_me_item* __restrict__ itp, const vvcgpu_unipred_me_cfg& c, const Pel* __restrict__ orgBase,
                                          unsigned char* base, int list, int r, vvcgpu_unipred_me_search* out, int tid)
{
  constexpr int TEAM = NT >> 6;
  MePu u;
  u.w = itp->w; u.h = itp->h; u.lgW = ilog2(u.w); u.posX = itp->pos_x; u.posY = itp->pos_y; u.subShift = itp->sub_shift;
  u.org = orgBase + itp->org_off; u.os = itp->org_stride;
  u.horMax = (c.pic_w + 8 - u.posX - 1) << 2; u.horMin = (-c.max_cu_w - 8 - u.posX + 1) << 2;
  u.verMax = (c.pic_h + 8 - u.posY - 1) << 2; u.verMin = (-c.max_cu_h - 8 - u.posY + 1) << 2;
  const int w = u.w, h = u.h, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const UpLds L = up_lds<NT>(base, w, h);
  const vvcgpu_unipred_me_ref& a = itp->ref[list][r];
  const Pel* plane = c.ref_planes[c.ref_plane[list][r]];

  for (int i = tid; i < w * h; i += NT) L.F.org[i] = u.org[(ptrdiff_t)(i >> u.lgW) * u.os + (i & (w - 1))];
  owner_sync<NT>();

  // xEstimateMvPredAMVP (bFilled): template cost of every candidate, the best by '>' in candidate order
  unsigned long long tmpl[2] = { 0ull, 0ull }, bestTmpl = ~0ull;
  int mvpIdx = 0;
#pragma unroll
  for (int i = 0; i < 2; i++)
  {
    if (i >= a.num_cand) break;
    unsigned sad = 0;
    me_pred_uni<NT>(u, plane, c.ref_stride, c.bit_depth, c.clp_min, c.clp_max, a.mv_cand[i][0], a.mv_cand[i][1], L.work, tid,
                    [&](int k, int, int, int v) { sad += (unsigned)abs((int)L.F.org[k] - v); });
    tmpl[i] = owner_sum<NT>(sad, L.part, tid) + rd_getcost(c.lambda, c.mvp_idx_cost[i]);
    if (bestTmpl > tmpl[i]) { bestTmpl = tmpl[i]; mvpIdx = i; }
  }
  int predX = a.mv_cand[mvpIdx][0], predY = a.mv_cand[mvpIdx][1];
  unsigned bits = itp->mb_bits[list] + pu_ref_bits(c.n_ref[list], r) + c.mvp_idx_cost[mvpIdx];

  if (up_shortcut(c, list, r))                                           // list 0's vector: the decision step finishes this record
  {
    if (tid == 0)
    {
      vvcgpu_unipred_me_search o;
      o.mv[0] = o.mv[1] = o.int_mv[0] = o.int_mv[1] = 0; o.mvp_idx = mvpIdx; o.bits = bits; o.cost = 0; o.tmpl_cost[0] = tmpl[0]; o.tmpl_cost[1] = tmpl[1];
      *out = o;
    }
    return;
  }

  // xTZSearch: the normal path starts at the predictor, the cached-start path at the block cache's vector with the fast settings
  int ix, iy;
  {
    TzTeam<TEAM> s;
    s.org = u.org; s.ref = plane; s.os = u.os; s.rs = c.ref_stride;
    s.w = w; s.h = h; s.subShift = u.subShift; s.refX = u.posX; s.refY = u.posY;
    s.rx0 = -(c.max_cu_w + 14); s.ry0 = -(c.max_cu_h + 14); s.rx1 = c.pic_w + c.max_cu_w + 14 - w; s.ry1 = c.pic_h + c.max_cu_h + 14 - h;
    s.horMax = u.horMax; s.horMin = u.horMin; s.verMax = u.verMax; s.verMin = u.verMin;
    s.lambda = c.lambda; s.predHor = predX; s.predVer = predY; s.costScale = 2; s.imvShift = IMV ? c.imv << 1 : 0;
    s.tl = tid;
    int LX = 1; while (4 * LX < w) LX <<= 1;
    s.LX = LX;
    s.keyL = L.keyL;
    s.segL = L.seg + wave * UP_SEG;
    tz_stage_org<TEAM>(s, reinterpret_cast<unsigned*>(L.work), (w * h) >> 1, L.negL);
    s.bestSad = ~0ull >> 16; s.bestX = s.bestY = 0; s.bestDist = 0; s.bestRound = 0; s.pointNr = 0;
    s.sr = TzRange{ 0, 0, 0, 0 };
    const bool cached = (a.flags & VVCGPU_UNIPRED_CACHED) != 0;
    const int flags = cached ? VVCGPU_TZ_FAST : (itp->tz_flags & VVCGPU_TZ_EXTENDED) | ((a.flags & VVCGPU_UNIPRED_PRED2) ? VVCGPU_TZ_PRED2 : 0);
    tz_machine<TEAM>(s, flags, c.search_range[list][r], c.first_search_stop, cached ? a.cached_mv[0] << 2 : predX, cached ? a.cached_mv[1] << 2 : predY,
                     a.pred2[0], a.pred2[1], false, [](const TzRound&, const TzRange&, int) { return false; });
    ix = s.bestX; iy = s.bestY;
  }
  owner_sync<NT>();                                                      // the packed original's last readers are done

  int mvX, mvY;
  unsigned long long cost;
  if (IMV)                                                               // xPatternSearchIntRefine around (ix, iy); no xCheckBestMVP (:1543-1546)
    me_imv_refine<NT>(u, L.F.org, plane, c.ref_stride, c.use_hadamard, 1.0, c.lambda, c.imv << 1, a.mv_cand, a.num_cand, c.mvp_idx_cost,
                      reinterpret_cast<unsigned long long*>(L.work), ix, iy, mvX, mvY, predX, predY, mvpIdx, bits, cost, tid);
  else                                                                   // xPatternSearchFracDIF around (ix, iy)
  {
    const int wp = w + 10;
    {
      const Pel* r0 = plane + (ptrdiff_t)(u.posY + iy - 4) * c.ref_stride + u.posX + ix - 4;
      for (int i = tid; i < (w + 9) * (h + 9); i += NT) { const int y = i / (w + 9), x = i - y * (w + 9); L.F.win[y * wp + x] = r0[(ptrdiff_t)y * c.ref_stride + x]; }
    }
    vvcgpu_mvcost mc;
    mc.lambda = c.lambda; mc.pred_hor = predX; mc.pred_ver = predY; mc.cost_scale = 0; mc.imv_shift = 0;
    frac_refine_pu(L.F, w, h, wp, c.bit_depth, c.clp_min, c.clp_max, c.use_hadamard, mc, ix, iy, true, tid, NT, L.fres);
    owner_sync<NT>();
    mvX = (ix << 2) + (L.fres->half_x << 1) + L.fres->qter_x; mvY = (iy << 2) + (L.fres->half_y << 1) + L.fres->qter_y;
    const unsigned mvBits = me_mvbits(predX, predY, 0, mvX, mvY);
    bits += mvBits;
    cost = (unsigned long long)(floor(1.0 * ((double)L.fres->cost - (double)rd_getcost(c.lambda, mvBits))) + (double)rd_getcost(c.lambda, bits));
    me_check_best_mvp(a.mv_cand, a.num_cand, c.mvp_idx_cost, c.lambda, mvX, mvY, predX, predY, mvpIdx, bits, cost);
  }
  if (tid == 0)
  {
    vvcgpu_unipred_me_search o;
    o.mv[0] = mvX; o.mv[1] = mvY; o.int_mv[0] = ix; o.int_mv[1] = iy; o.mvp_idx = mvpIdx; o.bits = bits; o.cost = cost;
    o.tmpl_cost[0] = tmpl[0]; o.tmpl_cost[1] = tmpl[1];
    *out = o;
  }
}

// IMV: an AMVR pass (cfg.imv != 0); its own instantiation, so that the quarter-sample pass keeps its registers
template <bool IMV>
__global__ __launch_bounds__(256) void unipred_search_kernel(const Pel* __restrict__ orgBase, const vvcgpu_unipred_me_item* __restrict__ items, int n,
                                                             const vvcgpu_unipred_me_cfg c, int waveBytes, vvcgpu_unipred_me_result* __restrict__ results)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = c.n_ref[0] + c.n_ref[1];
  const OwnerSlot o = owner_slot(n * S, wave);                          // unit = search k of PU b
  if (o.leave) return;
  const int b = o.unit / S, k = o.unit - b * S, list = k >= c.n_ref[0] ? 1 : 0, r = list ? k - c.n_ref[0] : k;
  const vvcgpu_unipred_me_item* it = items + b;
  if (!up_item_ok(*it, c)) return;                                       // the decision step writes the sentinel
  if ((it->w * it->h <= UP_WAVE_MAX) != o.waveOwner) return;               // the other kind of owner serves this item
  if (o.waveOwner) up_search<64, IMV>(it, c, orgBase, smem + (size_t)wave * waveBytes, list, r, &results[b].s[list][r], lane);
  else up_search<256, IMV>(it, c, orgBase, smem, list, r, &results[b].s[list][r], tid);
}

// per PU: the records of its searches in the reference's order (:877-964) -> the result and the out-item
__global__ __launch_bounds__(256) void unipred_decide_kernel(const vvcgpu_unipred_me_item* __restrict__ items, int n, const vvcgpu_unipred_me_cfg c,
                                                             vvcgpu_unipred_me_result* __restrict__ results, vvcgpu_bipred_me_item* __restrict__ outItems)
{
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  const vvcgpu_unipred_me_item& it = items[b];
  vvcgpu_unipred_me_result* R = results + b;
  if (!up_item_ok(it, c))
  {
    vvcgpu_unipred_me_result z;
    memset(&z, 0, sizeof(z));
    z.cost[0] = z.cost[1] = ~0ull;
    *R = z;
    if (outItems) { vvcgpu_bipred_me_item zi; memset(&zi, 0, sizeof(zi)); outItems[b] = zi; }
    return;
  }
  unsigned long long uiCost[2] = { ~0ull, ~0ull }, costL0[VVCGPU_UNIPRED_ME_MAX_REFS], bestBiPDist = ~0ull, costValid = ~0ull;
  unsigned uiBits[2] = { 0u, 0u }, bitsL0[VVCGPU_UNIPRED_ME_MAX_REFS], bitsValid = 0xFFFFFFFFu;
  int refIdx[2] = { 0, 0 }, mv[2][2] = { { 0, 0 }, { 0, 0 } }, bestBiPRef = 0, bestBiPMvp = 0, refValid = 0, mvValid[2] = { 0, 0 };
  for (int list = 0; list < 2; list++)
    for (int r = 0; r < VVCGPU_UNIPRED_ME_MAX_REFS; r++)
    {
      vvcgpu_unipred_me_search s;
      if (r >= c.n_ref[list]) { memset(&s, 0, sizeof(s)); R->s[list][r] = s; continue; }
      s = R->s[list][r];
      const vvcgpu_unipred_me_ref& a = it.ref[list][r];
      const int amvpIdx = (a.num_cand > 1 && s.tmpl_cost[0] > s.tmpl_cost[1]) ? 1 : 0;       // xEstimateMvPredAMVP's choice
      if (c.mvd_l1_zero && list == 1 && s.tmpl_cost[amvpIdx] < bestBiPDist) { bestBiPDist = s.tmpl_cost[amvpIdx]; bestBiPMvp = amvpIdx; bestBiPRef = r; }
      if (up_shortcut(c, list, r))                                       // :905-922, then xCheckBestMVP
      {
        const int k = c.list1_to_list0[r];
        int mvpIdx = s.mvp_idx, predX = a.mv_cand[mvpIdx][0], predY = a.mv_cand[mvpIdx][1];
        s.mv[0] = R->s[0][k].mv[0]; s.mv[1] = R->s[0][k].mv[1];
        unsigned long long cost = costL0[k];
        cost -= rd_getcost(c.lambda, bitsL0[k]);
        unsigned bits = s.bits + me_mvbits_imv(predX, predY, 0, c.imv << 1, s.mv[0], s.mv[1]);
        cost += rd_getcost(c.lambda, bits);
        if (c.imv == 0) me_check_best_mvp(a.mv_cand, a.num_cand, c.mvp_idx_cost, c.lambda, s.mv[0], s.mv[1], predX, predY, mvpIdx, bits, cost);
        s.mvp_idx = mvpIdx; s.bits = bits; s.cost = cost;
        R->s[list][r] = s;
      }
      if (list == 0) { costL0[r] = s.cost; bitsL0[r] = s.bits; }
      if (s.cost < uiCost[list]) { uiCost[list] = s.cost; uiBits[list] = s.bits; mv[list][0] = s.mv[0]; mv[list][1] = s.mv[1]; refIdx[list] = r; }
      if (list == 1 && s.cost < costValid && c.list1_to_list0[r] < 0) { costValid = s.cost; bitsValid = s.bits; mvValid[0] = s.mv[0]; mvValid[1] = s.mv[1]; refValid = r; }
    }
  for (int l = 0; l < 2; l++) { R->ref_idx[l] = refIdx[l]; R->mv[l][0] = mv[l][0]; R->mv[l][1] = mv[l][1]; R->cost[l] = uiCost[l]; R->bits[l] = uiBits[l]; }
  R->best_bip_ref_idx_l1 = bestBiPRef; R->best_bip_mvp_l1 = bestBiPMvp; R->best_bip_dist = bestBiPDist;
  R->valid_l1_ref_idx = refValid; R->valid_l1_mv[0] = mvValid[0]; R->valid_l1_mv[1] = mvValid[1]; R->valid_l1_bits = bitsValid; R->valid_l1_cost = costValid;
  if (!outItems) return;

  vvcgpu_bipred_me_item o;
  memset(&o, 0, sizeof(o));
  o.pos_x = it.pos_x; o.pos_y = it.pos_y; o.w = it.w; o.h = it.h; o.sub_shift = it.sub_shift; o.org_off = it.org_off; o.org_stride = it.org_stride;
  for (int l = 0; l < 2; l++)
  {
    o.n_ref[l] = c.n_ref[l]; o.ref_idx[l] = refIdx[l]; o.mv[l][0] = mv[l][0]; o.mv[l][1] = mv[l][1]; o.cost[l] = uiCost[l]; o.bits[l] = uiBits[l];
    for (int r = 0; r < c.n_ref[l]; r++)
    {
      const vvcgpu_unipred_me_ref& a = it.ref[l][r];
      vvcgpu_bipred_me_ref& q = o.ref[l][r];
      q.plane = c.ref_plane[l][r]; q.mv[0] = R->s[l][r].mv[0]; q.mv[1] = R->s[l][r].mv[1];
      for (int i = 0; i < 2; i++) { q.mv_cand[i][0] = a.mv_cand[i][0]; q.mv_cand[i][1] = a.mv_cand[i][1]; }
      q.num_cand = a.num_cand; q.mvp_idx = (int16_t)R->s[l][r].mvp_idx;
    }
  }
  for (int i = 0; i < 3; i++) o.mb_bits[i] = it.mb_bits[i];
  if (c.mvd_l1_zero && c.n_ref[1] > 0)                                   // :1009-1023, :1038
  {
    vvcgpu_bipred_me_ref& q = o.ref[1][bestBiPRef];
    q.mvp_idx = (int16_t)bestBiPMvp;
    q.mv[0] = q.mv_cand[bestBiPMvp][0]; q.mv[1] = q.mv_cand[bestBiPMvp][1];
    o.mv[1][0] = q.mv[0]; o.mv[1][1] = q.mv[1]; o.ref_idx[1] = bestBiPRef;
  }
  outItems[b] = o;
}

// the launch's LDS (cfg checked, max_pu set)
PuOwnerLds up_owner_lds(const vvcgpu_unipred_me_cfg& c) { return pu_owner_lds(4, c.max_pu_w, c.max_pu_h, UP_WAVE_MAX, up_lds_bytes); }

}  // namespace

extern "C" int vvcgpu_unipred_me_batch(const vvc_pel* org_base, const vvcgpu_unipred_me_item* items, int n, const vvcgpu_unipred_me_cfg* cfg_host,
                                       vvcgpu_unipred_me_result* results, vvcgpu_bipred_me_item* bipred_items_out, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "unipred_me_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org_base && items && cfg_host && results, "unipred_me_batch: null pointer");
  vvcgpu_unipred_me_cfg c = *cfg_host;
  if (const int rc = pu_check_frame("unipred_me_batch", c, VVCGPU_UNIPRED_ME_MAX_PLANES)) return rc;
  const auto searchRangeOk = [&](int l, int r)
  {
    VVC_CHECK_ARG(c.search_range[l][r] >= 1 && c.search_range[l][r] <= 256, "unipred_me_batch: search_range[%d][%d] %d outside 1..256", l, r, c.search_range[l][r]);
    return VVCGPU_OK;
  };
  if (const int rc = pu_check_lists("unipred_me_batch", c, VVCGPU_UNIPRED_ME_MAX_REFS, searchRangeOk)) return rc;
  if (const int rc = pu_check_imv("unipred_me_batch", c)) return rc;
  if (const int rc = pu_check_tail("unipred_me_batch", c, n, 1 << 27, pu_side_pow2_ok, "4, 8, .. 128")) return rc;
  const PuOwnerLds L = up_owner_lds(c);
  const int total = n * (c.n_ref[0] + c.n_ref[1]);
  hipStream_t st = (hipStream_t)stream;
  const auto search = c.imv ? unipred_search_kernel<true> : unipred_search_kernel<false>;
  VVC_HIP(vvc_allow_lds(search, L.lds));
  hipLaunchKernelGGL(search, dim3(pu_owner_grid(total, L.groupBytes != 0)), dim3(256), L.lds, st, org_base, items, n, c, L.waveBytes, results);
  VVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(unipred_decide_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, items, n, c, results, bipred_items_out);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
