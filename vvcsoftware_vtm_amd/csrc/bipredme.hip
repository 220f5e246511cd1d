// bipredme.hip -- the whole bi-predictive refinement of a PU in one launch (vvcgpu_bipred_me_batch) for gfx950.
//
// Reference behaviour reproduced (bit-exact, the double arithmetic of the cost included): the loop of InterSearch::predInterSearch
// (EncoderLib/InterSearch.cpp:1058-1164) with xMotionEstimation(bBi = true) (:1668-1816): removeHighFreq (Buffer.h:389-416), xSetSearchRange (:1820-1854),
// xPatternSearch (:1887-1941), xPatternSearchFracDIF (:2503-2552; frac_dev.h), and xCheckBestMVP (:1537-1603; me_dev.h); motionCompensation -> xPredInterUni ->
// xPredInterBlk (CommonLib/InterPrediction.cpp:480-547) with InterpolationFilter::filter / filterCopy (InterpolationFilter.cpp:205-379), clipMv
// (Mv.cpp:64-80) -- the prediction body is me_pred_uni of me_dev.h --, Mv::divideByPowerOf2 (Mv.h:142-151, ME_ENABLE_ROUNDING_OF_MVS), RdCost::getBitsOfVectorWithPredictor / getCost (RdCost.h:172-199).
//
// Design: the owner of a PU -- one wavefront up to BP_WAVE_MAX samples, the workgroup's four above -- carries it through every iteration (the owner
// model: owner_dev.h and docs/KERNELS.md, "Owners of the whole-PU entries").  What an iteration needs of the lists' predictions is only the OTHER
// list's, and only to form the search key 2 org - otherPred, so the prediction goes from the interpolation straight into the key and is never stored:
// per owner LDS holds the key (w x h), and a work area that is in turn the first-pass plane of the interpolation, the reference window of the integer
// search (block + range each way) and the window, first-stage plane and candidate block of the fractional refinement.  Dynamic LDS, sized on the host
// from cfg.max_pu_w / max_pu_h.  The integer search gives every position to a group of 1..64 lanes (a quarter of the block's sampled pixels each at
// most), so that no sum crosses a wavefront; the arg-min keeps (cost, scan index) pairs, which is the strict '<' of the y-outer, x-inner scan.
//  Control flow is uniform per owner: every lane computes the same scalar state; the per-(list, reference) state that is indexed dynamically
// (cMvTemp, aaiMvpIdxBi, cMvPredBi) lives in LDS.
// AMVR passes (cfg.imv = 1, 2; their own instantiation of the kernel, chosen by the host): xPatternSearch takes its vector bits with >> imvShift
// (:1913), xPatternSearchIntRefine (:2408-2500; me_imv_refine of me_dev.h) with half weight on the key replaces the fractional refinement and its
// cost, and no xCheckBestMVP runs (:1543-1546).
#include "common.h"
#include "frac_dev.h"
#include "me_dev.h"
#include "pu_entry_host.h"

namespace {

constexpr int BP_WAVE_MAX = 1024;          // samples a wavefront owns
constexpr int BP_HDR = 1024;               // bytes in front of an owner's key: see BpLds
constexpr int BP_ST = 5;                   // ints of state per (list, reference): cMvTemp (2), aaiMvpIdxBi, cMvPredBi (2)

// shorts of the work area: the fractional refinement's three buffers, or the search window
inline __host__ __device__ int bp_work_shorts(int w, int h, int range)
{
  const int frac = frac_work_shorts(w, h), srch = frac_r8((w + 2 * range) * (h + 2 * range));
  return frac > srch ? frac : srch;
}
inline __host__ __device__ int bp_lds_bytes(int w, int h, int range) { return BP_HDR + 2 * (frac_r8(w * h) + bp_work_shorts(w, h, range)); }

struct BpLds : FracOwnerLds       // frac_dev.h: bytes 0..575 of the header; F.org = the key
{
  int* st;                        // bytes 576..735: [2][4][BP_ST]
  unsigned long long* sb;         // bytes 736..799: the wavefronts' best (cost, scan index << 32 | sad) of the integer search
};
constexpr int BP_OFF_SB = FRAC_HDR + 2 * VVCGPU_BIPRED_ME_MAX_REFS * BP_ST * 4;
static_assert(BP_OFF_SB == 736 && BP_OFF_SB % 8 == 0 && BP_OFF_SB + 4 * 2 * 8 <= BP_HDR && BP_HDR % 16 == 0, "header layout");

// motionCompensation (luma, uni; me_dev.h) of the quarter-unit vector (mvX, mvY) against `ref` (sample (0, 0) of the picture), and the key from it:
// key = 2 org - pred, clipped when cfg.clip_for_bipred_me.  tmp: w x (h + 7) shorts.
template <int NT>
__device__ __forceinline__ void bp_key(const MePu& u, const vvcgpu_bipred_me_cfg& c, const Pel* __restrict__ ref, int mvX, int mvY, short* key, short* tmp, int tid)
{
  me_pred_uni<NT>(u, ref, c.ref_stride, c.bit_depth, c.clp_min, c.clp_max, mvX, mvY, tmp, tid, [&](int i, int y, int x, int v)
  {
    const int k2 = 2 * (int)u.org[(ptrdiff_t)y * u.os + x] - v;
    key[i] = (short)(c.clip_for_bipred_me ? clip3(c.clp_min, c.clp_max, k2) : k2);
  });
}

// xPatternSearch over [left, left + nx) x [top, top + ny) (integer vectors), the vector bits taken with >> sh (imvShift, :1913); sw = the window
// (pitch swp), its sample (0, 0) = the block at (left, top)
template <int NT>
__device__ __forceinline__ void bp_int_search(const MePu& u, const BpLds& L, const short* sw, int swp, int left, int top, int nx, int ny, double lambda,
                                              int predH, int predV, int sh, int tid, int& bx, int& by)
{
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = NT >> 6;
  const int hs = u.h >> u.subShift, n = u.w * hs;                         // sampled pixels: a power of two
  const int S = min(64, max(1, n >> 2)), lgS = ilog2(S), G = 64 >> lgS;
  const int grp = lane >> lgS, s = lane & (S - 1);
  const int P = nx * ny;
  unsigned long long bestC = ~0ull;
  unsigned bestP = 0xFFFFFFFFu;
  for (int p0 = wave * G; p0 < P; p0 += nw * G)
  {
    const int p = p0 + grp;
    const bool act = p < P;
    const int j = act ? p / nx : 0, i = act ? p - j * nx : 0;
    const short* cur = sw + j * swp + i;
    unsigned sum = 0;
    for (int k = s; k < n; k += S)
    {
      const int row = k >> u.lgW, x = k & (u.w - 1), y = row << u.subShift;
      sum += (unsigned)abs((int)L.F.org[y * u.w + x] - (int)cur[y * swp + x]);
    }
    for (int o = 1; o < S; o <<= 1) sum += __shfl_xor(sum, o);
    if (act)
    {
      const unsigned long long cost = (unsigned long long)(sum << u.subShift) + rd_getcost(lambda, me_mvbits_imv(predH, predV, 2, sh, left + i, top + j));
      if (cost < bestC) { bestC = cost; bestP = (unsigned)p; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    const unsigned long long oc = __shfl_xor(bestC, o);
    const unsigned op = __shfl_xor(bestP, o);
    if (oc < bestC || (oc == bestC && op < bestP)) { bestC = oc; bestP = op; }
  }
  if (NT == 256)
  {
    if (lane == 0) { L.sb[2 * wave] = bestC; L.sb[2 * wave + 1] = bestP; }
    __syncthreads();
    bestC = L.sb[0]; bestP = (unsigned)L.sb[1];
#pragma unroll
    for (int k = 1; k < 4; k++)
    {
      const unsigned long long oc = L.sb[2 * k];
      const unsigned op = (unsigned)L.sb[2 * k + 1];
      if (oc < bestC || (oc == bestC && op < bestP)) { bestC = oc; bestP = op; }
    }
    __syncthreads();                                                     // sb is written again by the next search
  }
  const int j = (int)bestP / nx;
  bx = left + (int)bestP - j * nx; by = top + j;
}

// IMV: an AMVR pass (cfg.imv != 0): xPatternSearchIntRefine for the fractional step, no xCheckBestMVP
template <int NT, bool IMV>
__device__ __forceinline__ void bp_search(const vvcgpu_bipred_me_item* __restrict__ itp, const vvcgpu_bipred_me_cfg& c, const Pel* __restrict__ orgBase,
                                          const BpLds& L, vvcgpu_bipred_me_result* res, vvcgpu_bipred_me_step* trace, int tid)
{
  MePu u;
  u.w = itp->w; u.h = itp->h; u.lgW = ilog2(u.w); u.posX = itp->pos_x; u.posY = itp->pos_y; u.subShift = itp->sub_shift;
  u.org = orgBase + itp->org_off; u.os = itp->org_stride;
  u.horMax = (c.pic_w + 8 - u.posX - 1) << 2; u.horMin = (-c.max_cu_w - 8 - u.posX + 1) << 2;
  u.verMax = (c.pic_h + 8 - u.posY - 1) << 2; u.verMin = (-c.max_cu_h - 8 - u.posY + 1) << 2;
  const int w = u.w, h = u.h, R = c.bipred_search_range, sh = IMV ? c.imv << 1 : 0;
  const int nRef[2] = { itp->n_ref[0], itp->n_ref[1] };
  const unsigned long long uniCost[2] = { itp->cost[0], itp->cost[1] };
  const unsigned mbBits2 = itp->mb_bits[2];

  if (tid < 2 * VVCGPU_BIPRED_ME_MAX_REFS)
  {
    const vvcgpu_bipred_me_ref& a = itp->ref[tid >> 2][tid & 3];
    const int k = a.mvp_idx & 1;
    int* s = L.st + tid * BP_ST;
    s[0] = a.mv[0]; s[1] = a.mv[1]; s[2] = k; s[3] = a.mv_cand[k][0]; s[4] = a.mv_cand[k][1];
  }
  owner_sync<NT>();

  int mvBi[2][2] = { { itp->mv[0][0], itp->mv[0][1] }, { itp->mv[1][0], itp->mv[1][1] } };
  int refBi[2] = { itp->ref_idx[0], itp->ref_idx[1] };
  unsigned motBits[2];
  motBits[0] = itp->bits[0] - itp->mb_bits[0];
  if (c.mvd_l1_zero) motBits[1] = itp->mb_bits[1] + pu_ref_bits(nRef[1], refBi[1]) + c.mvp_idx_cost[L.st[(4 + refBi[1]) * BP_ST + 2]];     // :1024-1036
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
    bp_key<NT>(u, c, c.ref_planes[itp->ref[other][refBi[other]].plane], mvBi[other][0], mvBi[other][1], L.F.org, L.work, tid);

    bool changed = false;
    for (int r = 0; r < nRef[list]; r++)
    {
      const vvcgpu_bipred_me_ref& a = itp->ref[list][r];
      int* s = L.st + (list * 4 + r) * BP_ST;
      int mvpIdx = s[2], predX = s[3], predY = s[4];
      unsigned bitsT = mbBits2 + motBits[other] + pu_ref_bits(nRef[list], r) + c.mvp_idx_cost[mvpIdx];
      const Pel* ref = c.ref_planes[a.plane] + (ptrdiff_t)u.posY * c.ref_stride + u.posX;
      // xSetSearchRange around cMvTemp[list][r]
      const int cx = min(u.horMax, max(u.horMin, s[0])), cy = min(u.verMax, max(u.verMin, s[1]));
      const int left = (min(u.horMax, max(u.horMin, cx - (R << 2))) + 2) >> 2, right = (min(u.horMax, max(u.horMin, cx + (R << 2))) + 2) >> 2;
      const int top = (min(u.verMax, max(u.verMin, cy - (R << 2))) + 2) >> 2, bottom = (min(u.verMax, max(u.verMin, cy + (R << 2))) + 2) >> 2;
      const int nx = right - left + 1, ny = bottom - top + 1;              // 1 .. 2 R + 1 each
      const int swp = w + nx - 1, swr = h + ny - 1;
      owner_sync<NT>();                                                   // the work area's last readers are done
      {
        const Pel* r0 = ref + (ptrdiff_t)top * c.ref_stride + left;
        for (int i = tid; i < swp * swr; i += NT) { const int y = i / swp, x = i - y * swp; L.work[i] = r0[(ptrdiff_t)y * c.ref_stride + x]; }
      }
      owner_sync<NT>();
      int ix, iy;
      bp_int_search<NT>(u, L, L.work, swp, left, top, nx, ny, c.lambda, predX, predY, sh, tid, ix, iy);
      owner_sync<NT>();
      int mvX, mvY;
      unsigned long long costT;
      if (IMV)                                                            // xPatternSearchIntRefine around (ix, iy), half weight on the key
        me_imv_refine<NT>(u, L.F.org, c.ref_planes[a.plane], c.ref_stride, c.use_hadamard, 0.5, c.lambda, sh, a.mv_cand, a.num_cand, c.mvp_idx_cost,
                          reinterpret_cast<unsigned long long*>(L.work), ix, iy, mvX, mvY, predX, predY, mvpIdx, bitsT, costT, tid);
      else                                                                // xPatternSearchFracDIF around (ix, iy)
      {
        const int wp = w + 10;
        {
          const Pel* r0 = ref + (ptrdiff_t)(iy - 4) * c.ref_stride + ix - 4;
          for (int i = tid; i < (w + 9) * (h + 9); i += NT) { const int y = i / (w + 9), x = i - y * (w + 9); L.F.win[y * wp + x] = r0[(ptrdiff_t)y * c.ref_stride + x]; }
        }
        vvcgpu_mvcost mc;
        mc.lambda = c.lambda; mc.pred_hor = predX; mc.pred_ver = predY; mc.cost_scale = 0; mc.imv_shift = 0;
        frac_refine_pu(L.F, w, h, wp, c.bit_depth, c.clp_min, c.clp_max, c.use_hadamard, mc, ix, iy, true, tid, NT, L.fres);
        owner_sync<NT>();
        mvX = (ix << 2) + (L.fres->half_x << 1) + L.fres->qter_x; mvY = (iy << 2) + (L.fres->half_y << 1) + L.fres->qter_y;
        const unsigned mvBits = me_mvbits(predX, predY, 0, mvX, mvY);
        bitsT += mvBits;
        costT = (unsigned long long)(floor(0.5 * ((double)L.fres->cost - (double)rd_getcost(c.lambda, mvBits))) + (double)rd_getcost(c.lambda, bitsT));
        me_check_best_mvp(a.mv_cand, a.num_cand, c.mvp_idx_cost, c.lambda, mvX, mvY, predX, predY, mvpIdx, bitsT, costT);
      }
      owner_sync<NT>();                                                   // every lane has read st and fres
      if (tid == 0) { s[0] = mvX; s[1] = mvY; s[2] = mvpIdx; s[3] = predX; s[4] = predY; }
      const bool accepted = costT < costBi;
      if (trace && tid == 0)
      {
        vvcgpu_bipred_me_step t;
        t.list = list; t.ref = r; t.int_mv[0] = ix; t.int_mv[1] = iy; t.mv[0] = mvX; t.mv[1] = mvY; t.bits = bitsT; t.mvp_idx = mvpIdx;
        t.accepted = accepted ? 1 : 0; t.reserved = 0; t.cost = costT;
        trace[calls] = t;
      }
      calls++;
      if (accepted)
      {
        changed = true;
        mvBi[list][0] = mvX; mvBi[list][1] = mvY; refBi[list] = r;
        costBi = costT;
        motBits[list] = bitsT - mbBits2 - motBits[other];
        bits2 = bitsT;
      }
    }
    owner_sync<NT>();
    if (!changed)
    {
      if (costBi <= uniCost[0] && costBi <= uniCost[1])
      {
        closing = 1;
        // amvp[eRefPicList]: list 0's is the set just copied for iRefIdxBi[0]; list 1's is, at the first check, the one the loop above copied last
        if (!IMV)                                                         // an AMVR pass: xCheckBestMVP returns at once (:1543-1546)
        {
          const vvcgpu_bipred_me_ref& a = list == 0 ? itp->ref[0][refBi[0]] : itp->ref[1][nRef[1] - 1];
          int* s = L.st + refBi[0] * BP_ST;
          int mvpIdx = s[2], predX = s[3], predY = s[4];
          me_check_best_mvp(a.mv_cand, a.num_cand, c.mvp_idx_cost, c.lambda, mvBi[0][0], mvBi[0][1], predX, predY, mvpIdx, bits2, costBi);
          owner_sync<NT>();
          if (tid == 0) { s[2] = mvpIdx; s[3] = predX; s[4] = predY; }
          owner_sync<NT>();
        }
        if (!IMV && !c.mvd_l1_zero)
        {
          const vvcgpu_bipred_me_ref& a = list == 0 ? itp->ref[0][refBi[0]] : itp->ref[1][refBi[1]];
          int* s = L.st + (4 + refBi[1]) * BP_ST;
          int mvpIdx = s[2], predX = s[3], predY = s[4];
          me_check_best_mvp(a.mv_cand, a.num_cand, c.mvp_idx_cost, c.lambda, mvBi[1][0], mvBi[1][1], predX, predY, mvpIdx, bits2, costBi);
          owner_sync<NT>();
          if (tid == 0) { s[2] = mvpIdx; s[3] = predX; s[4] = predY; }
          owner_sync<NT>();
        }
      }
      break;
    }
  }
  if (tid == 0)
  {
    vvcgpu_bipred_me_result o;
    for (int l = 0; l < 2; l++)
    {
      const int* s = L.st + (l * 4 + refBi[l]) * BP_ST;
      o.mv[l][0] = mvBi[l][0]; o.mv[l][1] = mvBi[l][1]; o.ref_idx[l] = refBi[l];
      o.mvp_idx[l] = s[2]; o.mvp[l][0] = s[3]; o.mvp[l][1] = s[4];
      o.mot_bits[l] = motBits[l];
    }
    o.bits = bits2; o.me_calls = calls; o.closing = closing; o.reserved = 0; o.cost = costBi;
    *res = o;
    if (trace)
      for (unsigned k = calls; k < VVCGPU_BIPRED_ME_MAX_STEPS; k++) zero_record(trace + k);
  }
}

__device__ __forceinline__ bool bp_item_ok(const vvcgpu_bipred_me_item& it, const vvcgpu_bipred_me_cfg& c)
{
  const int w = it.w, h = it.h;
  if (!pu_side_pow2_ok(w) || !pu_side_pow2_ok(h) || w > c.max_cu_w || h > c.max_cu_h || w > c.max_pu_w || h > c.max_pu_h) return false;
  if (it.pos_x < 0 || it.pos_y < 0 || it.pos_x > c.pic_w - w || it.pos_y > c.pic_h - h) return false;
  if (it.sub_shift < 0 || it.sub_shift > 1 || (h >> it.sub_shift) == 0 || it.org_stride <= 0) return false;
  for (int l = 0; l < 2; l++)
  {
    const int n = it.n_ref[l];
    if (n < 1 || n > VVCGPU_BIPRED_ME_MAX_REFS || it.ref_idx[l] < 0 || it.ref_idx[l] >= n) return false;
    for (int r = 0; r < n; r++)
    {
      const vvcgpu_bipred_me_ref& a = it.ref[l][r];
      if (a.plane < 0 || a.plane >= c.n_planes || a.num_cand < 1 || a.num_cand > 2 || a.mvp_idx < 0 || a.mvp_idx >= a.num_cand) return false;
    }
  }
  return true;
}

__device__ __forceinline__ BpLds bp_lds(unsigned char* base, int w, int h)
{
  BpLds L;
  frac_owner_lds(L, base, BP_HDR, w, h);
  L.st = reinterpret_cast<int*>(base + FRAC_HDR);
  L.sb = reinterpret_cast<unsigned long long*>(base + BP_OFF_SB);
  return L;
}

template <bool IMV>
__global__ __launch_bounds__(256) void bipred_me_kernel(const Pel* __restrict__ orgBase, const vvcgpu_bipred_me_item* __restrict__ items, int n,
                                                        const vvcgpu_bipred_me_cfg c, int waveBytes, vvcgpu_bipred_me_result* __restrict__ results,
                                                        vvcgpu_bipred_me_step* __restrict__ trace)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform for the compiler too: item fields and loop state in scalar registers
  const OwnerSlot o = owner_slot(n, wave);
  if (o.leave) return;
  const int b = o.unit;
  const vvcgpu_bipred_me_item* it = items + b;
  vvcgpu_bipred_me_step* tr = trace ? trace + (size_t)b * VVCGPU_BIPRED_ME_MAX_STEPS : nullptr;
  if (!bp_item_ok(*it, c))                                               // outside the contract: nothing is read or predicted
  {
    if (!o.waveOwner) owner_write_sentinel(results + b, tr, VVCGPU_BIPRED_ME_MAX_STEPS, tid);
    return;
  }
  if ((it->w * it->h <= BP_WAVE_MAX) != o.waveOwner) return;             // the other kind of owner serves this item
  if (o.waveOwner) bp_search<64, IMV>(it, c, orgBase, bp_lds(smem + (size_t)wave * waveBytes, it->w, it->h), results + b, tr, lane);
  else bp_search<256, IMV>(it, c, orgBase, bp_lds(smem, it->w, it->h), results + b, tr, tid);
}

// the launch's LDS (cfg checked, max_pu set)
PuOwnerLds bp_owner_lds(const vvcgpu_bipred_me_cfg& c)
{
  return pu_owner_lds(4, c.max_pu_w, c.max_pu_h, BP_WAVE_MAX, [&](int w, int h, int) { return bp_lds_bytes(w, h, c.bipred_search_range); });
}

}  // namespace

extern "C" int vvcgpu_bipred_me_batch(const vvc_pel* org_base, const vvcgpu_bipred_me_item* items, int n, const vvcgpu_bipred_me_cfg* cfg_host,
                                      vvcgpu_bipred_me_result* results, vvcgpu_bipred_me_step* trace, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "bipred_me_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org_base && items && cfg_host && results, "bipred_me_batch: null pointer");
  vvcgpu_bipred_me_cfg c = *cfg_host;
  if (const int rc = pu_check_frame("bipred_me_batch", c, VVCGPU_BIPRED_ME_MAX_PLANES)) return rc;
  VVC_CHECK_ARG(c.bipred_search_range >= 1 && c.bipred_search_range <= 8, "bipred_me_batch: bipred_search_range %d outside 1..8", c.bipred_search_range);
  VVC_CHECK_ARG(c.num_iter == 1 || c.num_iter == 4, "bipred_me_batch: num_iter %d (4 or 1)", c.num_iter);
  if (const int rc = pu_check_imv("bipred_me_batch", c)) return rc;
  if (const int rc = pu_check_tail("bipred_me_batch", c, n, 1 << 28, pu_side_pow2_ok, "4, 8, .. 128")) return rc;
  const PuOwnerLds L = bp_owner_lds(c);
  const auto kernel = c.imv ? bipred_me_kernel<true> : bipred_me_kernel<false>;
  VVC_HIP(vvc_allow_lds(kernel, L.lds));
  hipLaunchKernelGGL(kernel, dim3(pu_owner_grid(n, true)), dim3(256), L.lds, (hipStream_t)stream, org_base, items, n, c, L.waveBytes, results, trace);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
