// affine_unipredme.hip -- the whole uni-predictive stage of the affine inter search of a PU (vvcgpu_affine_unipred_me_batch) for gfx950.
//
// Reference behaviour reproduced (bit-exact, the double arithmetic of the costs included): the uni-predictive part of
// InterSearch::xPredAffineInterSearch (EncoderLib/InterSearch.cpp:2651-2814) with xEstimateAffineAMVP (:3745-3794, the caller's candidates) /
// xGetAffineTemplateCost (:1645-1665, bi = false), the start vectors of :2681-2727 with the 4-to-6-parameter inheritance of :2700-2706,
// xAffineMotionEstimation (bBi = false, :3286-3743; afm_dev.h), xCheckBestAffineMVP (:3181-3284; afm_dev.h), the list-1 shortcut (:2740-2774), the
// records of :2788-2812 and the mvd_l1_zero preparation of the bi-predictive stage (:2840-2853) for the out-items.
//
// Design: the shape of unipredme.hip.  The (list, reference index) searches of a PU depend on each other only through the list-1 shortcut and the
// final comparisons, and one gradient search is a chain of dependent predictions, so the unit of ownership is the SEARCH: launch 1 gives each of the
// n x (n_ref[0] + n_ref[1]) searches an owner -- one wavefront up to AFI_WAVE_MAX samples, the workgroup's four above (the owner model: owner_dev.h
// and docs/KERNELS.md, "Owners of the whole-PU entries").  The owner forms every template-cost prediction (each candidate, the translational start,
// the inherited start) in the prediction tile of afm_dev.h and reduces its SAD against the original straight from that tile (nothing is written out),
// chooses the start vectors, runs the gradient search of afm_dev.h unchanged and xCheckBestAffineMVP, and writes its record into the PU's result.  A
// search that takes list 0's vectors, or that a 6-parameter PU skips, only chooses its predictor.  Launch 2, one lane per PU, walks the records in the
// reference's order: the list-1 shortcut with its xCheckBestAffineMVP, bestBiP*, keep-if-strictly-better, the valid-list-1 record, the out-item for
// vvcgpu_affine_bipred_me_batch, and everything a skipped item gets.  Control flow is uniform per owner.  Dynamic LDS, sized on the host from
// cfg.max_pu_w / max_pu_h.
#include "common.h"
#include "afm_dev.h"
#include "pu_entry_host.h"

namespace {

typedef AfmHdr<0> AupHdr;                  // the header of afm_dev.h with no state of the entry's own
static_assert(AupHdr::WAVE == 752 && AupHdr::GROUP == 3888, "header sizes");

__device__ __forceinline__ bool aup_item_ok(const vvcgpu_affine_unipred_item& it, const vvcgpu_affine_unipred_cfg& c)
{
  const int w = it.w, h = it.h;
  if (!pu_side_affine_ok(w) || !pu_side_affine_ok(h) || w > c.max_cu_w || h > c.max_cu_h || w > c.max_pu_w || h > c.max_pu_h) return false;
  if (it.pos_x < 0 || it.pos_y < 0 || it.pos_x > c.pic_w - w || it.pos_y > c.pic_h - h || it.org_stride <= 0) return false;
  for (int l = 0; l < 2; l++)
  {
    if (c.n_ref[l] > 0 && (it.only_ref[l] < -1 || it.only_ref[l] >= c.n_ref[l])) return false;
    for (int r = 0; r < c.n_ref[l]; r++)
      if (it.ref[l][r].num_cand < 1 || it.ref[l][r].num_cand > 2) return false;
  }
  return true;
}

// :2673: a 6-parameter PU searches only the reference index its 4-parameter search chose
__device__ __forceinline__ bool aup_skipped(const vvcgpu_affine_unipred_item& it, int list, int r) { return it.six_param != 0 && it.only_ref[list] != r; }
// :2740-2746
__device__ __forceinline__ bool aup_shortcut(const vvcgpu_affine_unipred_item& it, const vvcgpu_affine_unipred_cfg& c, int list, int r)
{
  return list == 1 && c.fast_me_gen_b_low_delay && c.list1_to_list0[r] >= 0 && (it.six_param == 0 || c.list1_to_list0[r] == it.only_ref[0]);
}
// Mv::roundMV2SignalPrecision of a 1/16-unit component (Mv.h:242-257)
__device__ __forceinline__ int aup_round_signal(int v) { return (v >= 0 ? (v + 2) >> 2 : -((-v + 2) >> 2)) * 4; }

// xGetAffineTemplateCost without its getCost term: xPredAffineBlk of `mv` into the tile, the SAD against the original from the tile
template <int NT>
__device__ __forceinline__ unsigned long long aup_template_sad(const AfmPu& u, const Pel* __restrict__ org, const int (&mv)[3][2], const AfmLds& L, int tid)
{
  afm_predict<NT>(u, mv, L.predL, L.tmpW, tid);
  owner_sync<NT>();
  const int lgW = ilog2(u.w), pixels = u.w * u.h;
  unsigned sad = 0;
  for (int i = tid; i < pixels; i += NT) sad += (unsigned)abs((int)org[(ptrdiff_t)(i >> lgW) * u.os + (i & (u.w - 1))] - (int)L.predL[i]);
  const unsigned long long s = owner_sum<NT>(sad, L.distW, tid);
  if (NT == 64) owner_sync<64>();                                        // the tile is written again by the next prediction (NT = 256: the sum's barriers)
  return s;
}

// one (list, reference index) search of a PU by NT lanes
template <int NT>
__device__ __forceinline__ void aup_search(const vvcgpu_affine_unipred_item* __restrict__ itp, const vvcgpu_affine_unipred_cfg& c, const Pel* __restrict__ orgBase,
                                           const AfmLds& L, int list, int r, vvcgpu_affine_unipred_search* out, int tid)
{
  AfmPu u;
  const bool six = itp->six_param != 0;
  afm_set_pu(u, itp->pos_x, itp->pos_y, itp->w, itp->h, six, c.pic_w, c.pic_h, c.max_cu_w, c.max_cu_h, c.bit_depth, c.clp_min, c.clp_max);
  u.os = itp->org_stride; u.rs = c.ref_stride;
  u.ref = c.ref_planes[c.ref_plane[list][r]] + (ptrdiff_t)u.posY * c.ref_stride + u.posX;
  const Pel* org = orgBase + itp->org_off;
  const vvcgpu_affine_unipred_ref& a = itp->ref[list][r];

  const bool skipped = aup_skipped(*itp, list, r), shortcut = !skipped && aup_shortcut(*itp, c, list, r);
  int four[3][2];                                                        // :2696-2706: the inherited 4-parameter result of a 6-parameter PU
  four[0][0] = a.mv4[0][0]; four[0][1] = a.mv4[0][1]; four[1][0] = a.mv4[1][0]; four[1][1] = a.mv4[1][1];
  {
    const int sh = 7 + ilog2(u.h) - ilog2(u.w);                          // 4..10
    const int vx2 = (int)(((unsigned)four[0][0] << 7) - ((unsigned)(four[1][1] - four[0][1]) << sh)) >> 7;
    const int vy2 = (int)(((unsigned)four[0][1] << 7) + ((unsigned)(four[1][0] - four[0][0]) << sh)) >> 7;
    four[2][0] = aup_round_signal(vx2); four[2][1] = aup_round_signal(vy2);
  }

  // the template costs, one prediction after the other through one body: candidate 0, candidate 1 (xEstimateAffineAMVP: the best by '>' in
  // candidate order), then for a search the translational result (:2681-2692) and, for a 6-parameter PU, the inherited result (:2693-2717)
  unsigned long long tm0 = 0, tm1 = 0, startCost = 0, inheritCost = 0, biPDist = ~0ull;
  int mvpIdx = 0;
  const int nT = (skipped || shortcut) ? 2 : (six ? 4 : 3);
#pragma unroll 1
  for (int t = 0; t < nT; t++)
  {
    if (t == 1 && a.num_cand < 2) continue;
    int tv[3][2];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int d = 0; d < 2; d++) tv[k][d] = t < 2 ? a.mv_cand[t][k][d] : t == 2 ? a.hevc_mv[d] : four[k][d];
    const unsigned long long v = aup_template_sad<NT>(u, org, tv, L, tid) + rd_getcost(c.lambda, c.mvp_idx_cost[t < 2 ? t : mvpIdx]);
    if (t < 2)
    {
      if (t == 0) tm0 = v; else tm1 = v;
      if (biPDist > v) { biPDist = v; mvpIdx = t; }
    }
    else if (t == 2) startCost = v;
    else inheritCost = v;
  }
  vvcgpu_affine_unipred_search o;
  memset(&o, 0, sizeof(o));
  o.tmpl_cost[0] = tm0; o.tmpl_cost[1] = tm1; o.mvp_idx = mvpIdx;
  if (skipped)                                                           // :2673-2677: the predictor choice is all that is kept
  {
    if (tid == 0) *out = o;
    return;
  }
  unsigned bits = itp->mb_bits[list] + pu_ref_bits(c.n_ref[list], r) + c.mvp_idx_cost[mvpIdx];
  if (shortcut)                                                          // list 0's vectors: the decision step finishes this record
  {
    o.bits = bits; o.searched = 2;
    if (tid == 0) *out = o;
    return;
  }

  // :2709-2727: the inherited vectors on strict '<', then that start when its cost is < biPDistTemp, otherwise the predictor
  const bool inherit = six && inheritCost < startCost;
  const int sel = (inherit ? inheritCost : startCost) < biPDist ? (inherit ? 2 : 1) : 0;
  o.start_cost = startCost; o.inherit_cost = inheritCost; o.start = sel;
  int pred[3][2], start[3][2];
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int d = 0; d < 2; d++)
    {
      pred[k][d] = a.mv_cand[mvpIdx][k][d];
      start[k][d] = sel == 0 ? pred[k][d] : sel == 1 ? a.hevc_mv[d] : four[k][d];
    }

  int mv[3][2];
  unsigned steps;
  unsigned long long cost;
  afm_search_body<NT, const Pel*>(u, org, c.lambda, false, c.affine_type, bits, pred, start, L, nullptr, tid, mv, bits, cost, steps);
  afm_check_best_mvp(a.mv_cand, a.num_cand, c.mvp_idx_cost, c.lambda, u.nmv, mv, pred, mvpIdx, bits, cost);
  if (tid == 0)
  {
#pragma unroll
    for (int k = 0; k < 3; k++) { o.mv[k][0] = mv[k][0]; o.mv[k][1] = mv[k][1]; }
    o.mvp_idx = mvpIdx; o.bits = bits; o.cost = cost; o.steps = steps; o.searched = 1;
    *out = o;
  }
}

__global__ __launch_bounds__(256) void affine_unipred_search_kernel(const Pel* __restrict__ orgBase, const vvcgpu_affine_unipred_item* __restrict__ items, int n,
                                                                    const vvcgpu_affine_unipred_cfg c, int waveBytes,
                                                                    vvcgpu_affine_unipred_result* __restrict__ results)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform for the compiler too
  const int S = c.n_ref[0] + c.n_ref[1];
  const OwnerSlot o = owner_slot(n * S, wave);                          // unit = search k of PU b
  if (o.leave) return;
  const int b = o.unit / S, k = o.unit - b * S, list = k >= c.n_ref[0] ? 1 : 0, r = list ? k - c.n_ref[0] : k;
  const vvcgpu_affine_unipred_item* it = items + b;
  if (!aup_item_ok(*it, c)) return;                                      // the decision step writes the sentinel
  if ((it->w * it->h <= AFI_WAVE_MAX) != o.waveOwner) return;              // the other kind of owner serves this item
  if (o.waveOwner) aup_search<64>(it, c, orgBase, afm_lds<64, 0>(smem + (size_t)wave * waveBytes, 0), list, r, &results[b].s[list][r], lane);
  else aup_search<256>(it, c, orgBase, afm_lds<256, 0>(smem, wave), list, r, &results[b].s[list][r], tid);
}

// per PU: the records of its searches in the reference's order (:2651-2814) -> the result and the out-item
__global__ __launch_bounds__(256) void affine_unipred_decide_kernel(const vvcgpu_affine_unipred_item* __restrict__ items, int n, const vvcgpu_affine_unipred_cfg c,
                                                                    vvcgpu_affine_unipred_result* __restrict__ results,
                                                                    vvcgpu_affine_bipred_item* __restrict__ outItems)
{
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  const vvcgpu_affine_unipred_item& it = items[b];
  vvcgpu_affine_unipred_result* R = results + b;
  if (!aup_item_ok(it, c))
  {
    zero_record(R);
    R->cost[0] = R->cost[1] = ~0ull;
    if (outItems) zero_record(outItems + b);
    return;
  }
  const int nmv = it.six_param ? 3 : 2;
  unsigned long long uiCost[2] = { ~0ull, ~0ull }, bestBiPDist = ~0ull, costValid = ~0ull;
  unsigned uiBits[2] = { 0u, 0u }, bitsValid = 0xFFFFFFFFu;
  int refIdx[2] = { 0, 0 }, bestBiPRef = 0, bestBiPMvp = 0, refValid = 0;
  bool found[2] = { false, false }, foundValid = false;
  for (int list = 0; list < 2; list++)
    for (int r = 0; r < VVCGPU_AFFINE_UNIPRED_MAX_REFS; r++)
    {
      vvcgpu_affine_unipred_search s;
      if (r >= c.n_ref[list]) { zero_record(&R->s[list][r]); continue; }
      s = R->s[list][r];
      if (s.searched == 0) continue;                                     // :2673-2677, before the bestBiP* update
      const vvcgpu_affine_unipred_ref& a = it.ref[list][r];
      const int amvpIdx = (a.num_cand > 1 && s.tmpl_cost[0] > s.tmpl_cost[1]) ? 1 : 0;       // xEstimateAffineAMVP's choice
      if (c.mvd_l1_zero && list == 1 && s.tmpl_cost[amvpIdx] < bestBiPDist) { bestBiPDist = s.tmpl_cost[amvpIdx]; bestBiPMvp = amvpIdx; bestBiPRef = r; }
      if (s.searched == 2)                                               // :2747-2774, then xCheckBestAffineMVP
      {
        const vvcgpu_affine_unipred_search& s0 = R->s[0][c.list1_to_list0[r]];
        int mvpIdx = s.mvp_idx, pred[3][2], mv[3][2];
#pragma unroll
        for (int k = 0; k < 3; k++) { pred[k][0] = a.mv_cand[mvpIdx][k][0]; pred[k][1] = a.mv_cand[mvpIdx][k][1]; mv[k][0] = s0.mv[k][0]; mv[k][1] = s0.mv[k][1]; }
        unsigned long long cost = s0.cost;
        cost -= rd_getcost(c.lambda, s0.bits);
        unsigned bits = afm_bits(s.bits, pred, nmv, mv);
        cost += rd_getcost(c.lambda, bits);
        afm_check_best_mvp(a.mv_cand, a.num_cand, c.mvp_idx_cost, c.lambda, nmv, mv, pred, mvpIdx, bits, cost);
#pragma unroll
        for (int k = 0; k < 3; k++) { s.mv[k][0] = mv[k][0]; s.mv[k][1] = mv[k][1]; }
        s.mvp_idx = mvpIdx; s.bits = bits; s.cost = cost;
        R->s[list][r] = s;
      }
      if (s.cost < uiCost[list]) { uiCost[list] = s.cost; uiBits[list] = s.bits; refIdx[list] = r; found[list] = true; }
      if (list == 1 && s.cost < costValid && c.list1_to_list0[r] < 0) { costValid = s.cost; bitsValid = s.bits; refValid = r; foundValid = true; }
    }
  for (int l = 0; l < 2; l++)
  {
    R->ref_idx[l] = refIdx[l]; R->cost[l] = uiCost[l]; R->bits[l] = uiBits[l];
    for (int k = 0; k < 3; k++) { R->mv[l][k][0] = found[l] ? R->s[l][refIdx[l]].mv[k][0] : 0; R->mv[l][k][1] = found[l] ? R->s[l][refIdx[l]].mv[k][1] : 0; }
  }
  R->best_bip_ref_idx_l1 = bestBiPRef; R->best_bip_mvp_l1 = bestBiPMvp; R->best_bip_dist = bestBiPDist;
  R->valid_l1_ref_idx = refValid; R->valid_l1_bits = bitsValid; R->valid_l1_cost = costValid;
  for (int k = 0; k < 3; k++) { R->valid_l1_mv[k][0] = foundValid ? R->s[1][refValid].mv[k][0] : 0; R->valid_l1_mv[k][1] = foundValid ? R->s[1][refValid].mv[k][1] : 0; }
  if (!outItems) return;

  vvcgpu_affine_bipred_item* o = outItems + b;                           // every byte of the record is written
  o->pos_x = it.pos_x; o->pos_y = it.pos_y; o->w = it.w; o->h = it.h; o->six_param = it.six_param; o->reserved0 = 0;
  o->org_off = it.org_off; o->org_stride = it.org_stride; o->reserved1 = 0; o->reserved2 = 0;
  for (int i = 0; i < 3; i++) o->mb_bits[i] = it.mb_bits[i];
  for (int l = 0; l < 2; l++)
  {
    o->n_ref[l] = c.n_ref[l]; o->ref_idx[l] = refIdx[l]; o->cost[l] = uiCost[l]; o->bits[l] = uiBits[l]; o->only_ref[l] = it.only_ref[l];
    for (int k = 0; k < 3; k++) { o->mv[l][k][0] = R->mv[l][k][0]; o->mv[l][k][1] = R->mv[l][k][1]; }
    for (int r = 0; r < VVCGPU_AFFINE_BIPRED_MAX_REFS; r++)
    {
      vvcgpu_affine_bipred_ref q;
      memset(&q, 0, sizeof(q));
      if (r < c.n_ref[l])
      {
        const vvcgpu_affine_unipred_ref& a = it.ref[l][r];
        q.plane = c.ref_plane[l][r]; q.num_cand = a.num_cand; q.mvp_idx = (int16_t)R->s[l][r].mvp_idx;
        for (int k = 0; k < 3; k++)
        {
          q.mv[k][0] = R->s[l][r].mv[k][0]; q.mv[k][1] = R->s[l][r].mv[k][1];
          for (int i = 0; i < 2; i++) { q.mv_cand[i][k][0] = a.mv_cand[i][k][0]; q.mv_cand[i][k][1] = a.mv_cand[i][k][1]; }
        }
        if (c.mvd_l1_zero && l == 1 && r == bestBiPRef)                  // :2840-2853
        {
          q.mvp_idx = (int16_t)bestBiPMvp;
          for (int k = 0; k < 3; k++)
          {
            q.mv[k][0] = a.mv_cand[bestBiPMvp][k][0]; q.mv[k][1] = a.mv_cand[bestBiPMvp][k][1];
            o->mv[1][k][0] = q.mv[k][0]; o->mv[1][k][1] = q.mv[k][1];
          }
          o->ref_idx[1] = bestBiPRef;
        }
      }
      o->ref[l][r] = q;
    }
  }
}

// the launch's LDS (cfg checked, max_pu set): an owner's header and its tile
PuOwnerLds aup_owner_lds(const vvcgpu_affine_unipred_cfg& c)
{
  return pu_owner_lds(16, c.max_pu_w, c.max_pu_h, AFI_WAVE_MAX, [](int w, int h, int nt) { return AupHdr::bytes(nt, w * h * (int)sizeof(Pel)); });
}

}  // namespace

extern "C" int vvcgpu_affine_unipred_me_batch(const vvc_pel* org_base, const vvcgpu_affine_unipred_item* items, int n, const vvcgpu_affine_unipred_cfg* cfg_host,
                                              vvcgpu_affine_unipred_result* results, vvcgpu_affine_bipred_item* bipred_items_out, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "affine_unipred_me_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org_base && items && cfg_host && results, "affine_unipred_me_batch: null pointer");
  vvcgpu_affine_unipred_cfg c = *cfg_host;
  if (const int rc = pu_check_frame("affine_unipred_me_batch", c, 16)) return rc;
  if (const int rc = pu_check_lists("affine_unipred_me_batch", c, VVCGPU_AFFINE_UNIPRED_MAX_REFS, [](int, int) { return VVCGPU_OK; })) return rc;
  const int S = c.n_ref[0] + c.n_ref[1];
  if (const int rc = pu_check_tail("affine_unipred_me_batch", c, n, (1 << 27) / S, pu_side_affine_ok, "16, 32, 64, 128")) return rc;
  const PuOwnerLds L = aup_owner_lds(c);
  const int total = n * S;
  hipStream_t st = (hipStream_t)stream;
  VVC_HIP(vvc_allow_lds(affine_unipred_search_kernel, L.lds));
  hipLaunchKernelGGL(affine_unipred_search_kernel, dim3(pu_owner_grid(total, L.groupBytes != 0)), dim3(256), L.lds, st, org_base, items, n, c, L.waveBytes, results);
  VVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(affine_unipred_decide_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, items, n, c, results, bipred_items_out);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
