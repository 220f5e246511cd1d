// affine_bipredme.hip -- the whole affine bi-predictive search of a PU in one launch (vvcgpu_affine_bipred_me_batch) for gfx950.
//
// Reference behaviour reproduced (bit-exact, the double arithmetic included): the bi-predictive part of InterSearch::xPredAffineInterSearch
// (EncoderLib/InterSearch.cpp:2823-2997) with xAffineMotionEstimation(bBi = true) (:3286-3743; afm_dev.h), xCheckBestAffineMVP (:3181-3284) and the
// luma motionCompensation of an affine PU: InterPrediction::xPredInterUni (CommonLib/InterPrediction.cpp:377-407) on the control-point vectors that
// PU::setAllAffineMv leaves in the corners of the motion buffer (UnitTools.cpp:2319-2330; no clipMv of them), xPredAffineBlk (:550-722) with
// bi = false; PelBuf::removeHighFreq (Buffer.h:389-416); RdCost::getBitsOfVectorWithPredictor / getCost (RdCost.h:172-199).
//
// Design: the owner of a PU -- one wavefront up to AFI_WAVE_MAX samples, the workgroup's four above -- carries it through every iteration (the owner
// model: owner_dev.h and docs/KERNELS.md, "Owners of the whole-PU entries").  Per owner LDS holds two Pel tiles: the prediction tile of the search
// (afm_dev.h) and the search key.  What an iteration needs of the lists' predictions is only the OTHER list's, and only to form the key 2 org -
// otherPred: it is formed in the prediction tile when the iteration starts (the reference forms it at :2913-2920 and again after each acceptance,
// :2970-2977, which the iteration never reads) and turned into the key in the second tile; every search of the iteration then reads the key where
// afm_dev.h's passes read an original, through an LDS-qualified pointer.  Dynamic LDS, sized on the host from cfg.max_pu_w / max_pu_h.  Control flow
// is uniform per owner: every lane computes the same scalar state; the per-(list, reference) state that is indexed dynamically (cMvTemp, aaiMvpIdxBi,
// cMvPredBi) lives in LDS.
#include "common.h"
#include "afm_dev.h"
#include "pu_entry_host.h"

namespace {

constexpr int ABP_ST = 13;                 // ints of state per (list, reference): cMvTemp[3][2], aaiMvpIdxBi, cMvPredBi[3][2]
constexpr int ABP_ST_BYTES = 2 * VVCGPU_AFFINE_BIPRED_MAX_REFS * ABP_ST * 4;
typedef AfmHdr<ABP_ST_BYTES> AbpHdr;       // the header of afm_dev.h with the state block behind the equation sums
static_assert(AbpHdr::WAVE == 1168 && AbpHdr::GROUP == 4304, "header sizes");

struct AbpLds
{
  AfmLds A;          // predL: the first tile
  Pel* key;          // the second tile
  int* st;           // [2][4][ABP_ST]
};

template <int NT>
__device__ __forceinline__ AbpLds abp_lds(unsigned char* base, int wave, int pixels)
{
  AbpLds L;
  L.A = afm_lds<NT, ABP_ST_BYTES>(base, wave);
  L.st = reinterpret_cast<int*>(base + AFM_OFF_STATE);
  L.key = L.A.predL + pixels;
  return L;
}

// xCheckBestAffineMVP (afm_dev.h) with the candidate set of the record `a`
__device__ __forceinline__ void abp_check_best_mvp(const vvcgpu_affine_bipred_ref& a, const vvcgpu_affine_bipred_cfg& c, int nmv, const int (&mv)[3][2],
                                                   int (&pred)[3][2], int& mvpIdx, unsigned& bits, unsigned long long& cost)
{
  afm_check_best_mvp(a.mv_cand, a.num_cand, c.mvp_idx_cost, c.lambda, nmv, mv, pred, mvpIdx, bits, cost);
}

template <int NT>
__device__ __forceinline__ void abp_search(const vvcgpu_affine_bipred_item* __restrict__ itp, const vvcgpu_affine_bipred_cfg& c, const Pel* __restrict__ orgBase,
                                           const AbpLds& L, vvcgpu_affine_bipred_result* res, vvcgpu_affine_bipred_step* trace, int tid)
{
  AfmPu u;
  const bool six = itp->six_param != 0;
  afm_set_pu(u, itp->pos_x, itp->pos_y, itp->w, itp->h, six, c.pic_w, c.pic_h, c.max_cu_w, c.max_cu_h, c.bit_depth, c.clp_min, c.clp_max);
  u.os = u.w; u.rs = c.ref_stride;                                         // the original of every search is the key: pitch w
  const Pel* org = orgBase + itp->org_off;
  const int os = itp->org_stride, pixels = u.w * u.h;
  const ptrdiff_t puOff = (ptrdiff_t)u.posY * c.ref_stride + u.posX;
  const int nRef[2] = { itp->n_ref[0], itp->n_ref[1] };
  const int onlyRef[2] = { six ? itp->only_ref[0] : -1, six ? itp->only_ref[1] : -1 };      // :2936-2941: a 6-parameter PU only
  const unsigned long long uniCost[2] = { itp->cost[0], itp->cost[1] };
  const unsigned mbBits2 = itp->mb_bits[2];
  int refBi[2] = { itp->ref_idx[0], itp->ref_idx[1] };

  if (tid < 2 * VVCGPU_AFFINE_BIPRED_MAX_REFS)
  {
    const vvcgpu_affine_bipred_ref& a = itp->ref[tid >> 2][tid & 3];
    const int k = a.mvp_idx & 1;
    int* s = L.st + tid * ABP_ST;
    const bool fixed = c.mvd_l1_zero && tid == 4 + refBi[1];               // :2847-2853: list 1 stays on its predictor
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
      s[2 * i] = fixed ? a.mv_cand[k][i][0] : a.mv[i][0]; s[2 * i + 1] = fixed ? a.mv_cand[k][i][1] : a.mv[i][1];
      s[7 + 2 * i] = a.mv_cand[k][i][0]; s[8 + 2 * i] = a.mv_cand[k][i][1];
    }
    s[6] = k;
  }
  owner_sync<NT>();

  int mvBi[2][3][2];
#pragma unroll
  for (int l = 0; l < 2; l++)
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
      const bool fixed = c.mvd_l1_zero && l == 1;
      const int* s = L.st + (4 + refBi[1]) * ABP_ST;
      mvBi[l][i][0] = fixed ? s[2 * i] : itp->mv[l][i][0]; mvBi[l][i][1] = fixed ? s[2 * i + 1] : itp->mv[l][i][1];
    }
  unsigned motBits[2];
  motBits[0] = itp->bits[0] - itp->mb_bits[0];
  if (c.mvd_l1_zero) motBits[1] = itp->mb_bits[1] + pu_ref_bits(nRef[1], refBi[1]) + c.mvp_idx_cost[L.st[(4 + refBi[1]) * ABP_ST + 6]];        // :2864-2874
  else motBits[1] = itp->bits[1] - itp->mb_bits[1];
  unsigned bits2 = mbBits2 + motBits[0] + motBits[1];
  unsigned long long costBi = ~0ull;
  unsigned calls = 0, closing = 0;

  for (int iter = 0; iter < c.num_iter; iter++)
  {
    int list = iter & 1;
    if (c.pick_list_by_cost) list = uniCost[0] <= uniCost[1] ? 1 : 0;
    else if (iter == 0) list = 0;
    if (c.mvd_l1_zero) list = 0;
    const int other = 1 - list;
    // the other list's prediction into the first tile, the key from it into the second
    u.ref = c.ref_planes[itp->ref[other][refBi[other]].plane] + puOff;
    afm_predict<NT>(u, mvBi[other], L.A.predL, L.A.tmpW, tid);
    owner_sync<NT>();
    for (int i = tid; i < pixels; i += NT)
    {
      const int y = i / u.w, x = i - y * u.w;
      const int k2 = 2 * (int)org[(ptrdiff_t)y * os + x] - (int)L.A.predL[i];
      L.key[i] = (Pel)(c.clip_for_bipred_me ? clip3(c.clp_min, c.clp_max, k2) : k2);
    }
    owner_sync<NT>();

    bool changed = false;
    for (int r = 0; r < nRef[list]; r++)
    {
      if (onlyRef[list] >= 0 && onlyRef[list] != r) continue;
      const vvcgpu_affine_bipred_ref& a = itp->ref[list][r];
      int* s = L.st + (list * 4 + r) * ABP_ST;
      int start[3][2], pred[3][2], mv[3][2];
#pragma unroll
      for (int i = 0; i < 3; i++) { start[i][0] = s[2 * i]; start[i][1] = s[2 * i + 1]; pred[i][0] = s[7 + 2 * i]; pred[i][1] = s[8 + 2 * i]; }
      int mvpIdx = s[6];
      unsigned bitsT = mbBits2 + motBits[other] + pu_ref_bits(nRef[list], r) + c.mvp_idx_cost[mvpIdx];      // :2944-2953
      u.ref = c.ref_planes[a.plane] + puOff;
      unsigned steps;
      unsigned long long costT;
      afm_search_body<NT, AfiLdsPel>(u, (AfiLdsPel)L.key, c.lambda, true, c.affine_type, bitsT, pred, start, L.A, nullptr, tid, mv, bitsT, costT, steps);
      abp_check_best_mvp(a, c, u.nmv, mv, pred, mvpIdx, bitsT, costT);
      owner_sync<NT>();                                                    // every lane has read st
      if (tid == 0)
      {
#pragma unroll
        for (int i = 0; i < 3; i++) { s[2 * i] = mv[i][0]; s[2 * i + 1] = mv[i][1]; s[7 + 2 * i] = pred[i][0]; s[8 + 2 * i] = pred[i][1]; }
        s[6] = mvpIdx;
      }
      const bool accepted = costT < costBi;
      if (trace && tid == 0)
      {
        vvcgpu_affine_bipred_step t;
        t.list = list; t.ref = r;
#pragma unroll
        for (int i = 0; i < 3; i++) { t.mv[i][0] = mv[i][0]; t.mv[i][1] = mv[i][1]; }
        t.steps = steps; t.bits = bitsT; t.mvp_idx = mvpIdx; t.accepted = accepted ? 1 : 0; t.cost = costT;
        trace[calls] = t;
      }
      calls++;
      if (accepted)
      {
        changed = true;
#pragma unroll
        for (int i = 0; i < 3; i++) { mvBi[list][i][0] = mv[i][0]; mvBi[list][i][1] = mv[i][1]; }
        refBi[list] = r;
        costBi = costT;
        motBits[list] = bitsT - mbBits2 - motBits[other];
        bits2 = bitsT;
      }
      owner_sync<NT>();                                                    // st is written before anyone reads it again
    }
    if (!changed)
    {
      if (costBi <= uniCost[0] && costBi <= uniCost[1])
      {
        closing = 1;
        for (int l = 0; l < (c.mvd_l1_zero ? 1 : 2); l++)                   // :2985-2992: each with the candidate set of the list it checks
        {
          int* s = L.st + (l * 4 + refBi[l]) * ABP_ST;
          int pred[3][2];
#pragma unroll
          for (int i = 0; i < 3; i++) { pred[i][0] = s[7 + 2 * i]; pred[i][1] = s[8 + 2 * i]; }
          int mvpIdx = s[6];
          abp_check_best_mvp(itp->ref[l][refBi[l]], c, u.nmv, mvBi[l], pred, mvpIdx, bits2, costBi);
          owner_sync<NT>();
          if (tid == 0)
          {
#pragma unroll
            for (int i = 0; i < 3; i++) { s[7 + 2 * i] = pred[i][0]; s[8 + 2 * i] = pred[i][1]; }
            s[6] = mvpIdx;
          }
          owner_sync<NT>();
        }
      }
      break;
    }
  }
  if (tid == 0)
  {
    vvcgpu_affine_bipred_result o;
    for (int l = 0; l < 2; l++)
    {
      const int* s = L.st + (l * 4 + refBi[l]) * ABP_ST;
#pragma unroll
      for (int i = 0; i < 3; i++)
      {
        o.mv[l][i][0] = mvBi[l][i][0]; o.mv[l][i][1] = mvBi[l][i][1];
        o.mvp[l][i][0] = s[7 + 2 * i]; o.mvp[l][i][1] = s[8 + 2 * i];
      }
      o.ref_idx[l] = refBi[l]; o.mvp_idx[l] = s[6]; o.mot_bits[l] = motBits[l];
    }
    o.bits = bits2; o.me_calls = calls; o.closing = closing; o.reserved = 0; o.cost = costBi;
    *res = o;
    if (trace)
      for (unsigned k = calls; k < VVCGPU_AFFINE_BIPRED_MAX_STEPS; k++) zero_record(trace + k);
  }
}

__device__ __forceinline__ bool abp_item_ok(const vvcgpu_affine_bipred_item& it, const vvcgpu_affine_bipred_cfg& c)
{
  const int w = it.w, h = it.h;
  if (!pu_side_affine_ok(w) || !pu_side_affine_ok(h) || w > c.max_cu_w || h > c.max_cu_h || w > c.max_pu_w || h > c.max_pu_h) return false;
  if (it.pos_x < 0 || it.pos_y < 0 || it.pos_x > c.pic_w - w || it.pos_y > c.pic_h - h || it.org_stride <= 0) return false;
  for (int l = 0; l < 2; l++)
  {
    const int n = it.n_ref[l];
    if (n < 1 || n > VVCGPU_AFFINE_BIPRED_MAX_REFS || it.ref_idx[l] < 0 || it.ref_idx[l] >= n || it.only_ref[l] < -1 || it.only_ref[l] >= n) return false;
    for (int r = 0; r < n; r++)
    {
      const vvcgpu_affine_bipred_ref& a = it.ref[l][r];
      if (a.plane < 0 || a.plane >= c.n_planes || a.num_cand < 1 || a.num_cand > 2 || a.mvp_idx < 0 || a.mvp_idx >= a.num_cand) return false;
    }
  }
  return true;
}

__global__ __launch_bounds__(256) void affine_bipred_me_kernel(const Pel* __restrict__ orgBase, const vvcgpu_affine_bipred_item* __restrict__ items, int n,
                                                               const vvcgpu_affine_bipred_cfg c, int waveBytes,
                                                               vvcgpu_affine_bipred_result* __restrict__ results,
                                                               vvcgpu_affine_bipred_step* __restrict__ trace)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform for the compiler too
  const OwnerSlot o = owner_slot(n, wave);
  if (o.leave) return;
  const int b = o.unit;
  const vvcgpu_affine_bipred_item* it = items + b;
  vvcgpu_affine_bipred_step* tr = trace ? trace + (size_t)b * VVCGPU_AFFINE_BIPRED_MAX_STEPS : nullptr;
  if (!abp_item_ok(*it, c))                                              // outside the contract: nothing is read or predicted
  {
    if (!o.waveOwner) owner_write_sentinel(results + b, tr, VVCGPU_AFFINE_BIPRED_MAX_STEPS, tid);
    return;
  }
  if ((it->w * it->h <= AFI_WAVE_MAX) != o.waveOwner) return;            // the other kind of owner serves this item
  if (o.waveOwner) abp_search<64>(it, c, orgBase, abp_lds<64>(smem + (size_t)wave * waveBytes, 0, it->w * it->h), results + b, tr, lane);
  else abp_search<256>(it, c, orgBase, abp_lds<256>(smem, wave, it->w * it->h), results + b, tr, tid);
}

// the launch's LDS (cfg checked, max_pu set): an owner's header and two tiles
PuOwnerLds abp_owner_lds(const vvcgpu_affine_bipred_cfg& c)
{
  return pu_owner_lds(16, c.max_pu_w, c.max_pu_h, AFI_WAVE_MAX, [](int w, int h, int nt) { return AbpHdr::bytes(nt, 2 * w * h * (int)sizeof(Pel)); });
}

}  // namespace

extern "C" int vvcgpu_affine_bipred_me_batch(const vvc_pel* org_base, const vvcgpu_affine_bipred_item* items, int n, const vvcgpu_affine_bipred_cfg* cfg_host,
                                             vvcgpu_affine_bipred_result* results, vvcgpu_affine_bipred_step* trace, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "affine_bipred_me_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org_base && items && cfg_host && results, "affine_bipred_me_batch: null pointer");
  vvcgpu_affine_bipred_cfg c = *cfg_host;
  if (const int rc = pu_check_frame("affine_bipred_me_batch", c, 16)) return rc;
  VVC_CHECK_ARG(c.num_iter == 1 || c.num_iter == 4, "affine_bipred_me_batch: num_iter %d (4 or 1)", c.num_iter);
  if (const int rc = pu_check_tail("affine_bipred_me_batch", c, n, 1 << 28, pu_side_affine_ok, "16, 32, 64, 128")) return rc;
  const PuOwnerLds L = abp_owner_lds(c);
  VVC_HIP(vvc_allow_lds(affine_bipred_me_kernel, L.lds));
  hipLaunchKernelGGL(affine_bipred_me_kernel, dim3(pu_owner_grid(n, true)), dim3(256), L.lds, (hipStream_t)stream, org_base, items, n, c, L.waveBytes, results,
                     trace);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
