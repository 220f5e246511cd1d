// tzsearch.hip -- integer-sample TZ search of whole PUs (next row N2) for gfx950.
//
// Reference behaviour reproduced (bit-exact position, cost and SAD):
//   InterSearch::xTZSearch               EncoderLib/InterSearch.cpp:1971-2252
//   InterSearch::xTZSearchHelp           :249-343 (subShiftMode 0/2 branch)
//   InterSearch::xTZ2PointSearch         :349-374
//   InterSearch::xTZ8PointDiamondSearch  :431-632
//   InterSearch::xSetSearchRange         :1820-1853,  clipMv CommonLib/Mv.cpp:64-80,  Mv::divideByPowerOf2 Mv.h:142-151
//   RdCost::getCostOfVectorWithPredictor CommonLib/RdCost.h:172-199
//
// Design: the search is a short, data-dependent chain of "rounds" (one probe, a diamond of <= 16 probes, two neighbours, a
// raster of up to ~1500 probes).  A team of lanes -- one wavefront (TEAM 1, small PUs) or one workgroup of four (TEAM 4, large
// PUs) -- owns one PU and keeps the whole search state uniform; within a round the probes are independent, so the team
// evaluates them together: the (sub-sampled) original block sits in LDS as packed pairs, LX = w / 4 lanes span a row with one
// 4-sample quad each (8-byte LDS read, aligned dword reads of the reference row + v_alignbit for odd positions, two
// v_sad_u16), RP lane groups split the rows when a round has few probes, and the remaining lanes take further probes.  A
// round then is a 64-bit min over  cost << 16 | visiting index  -- the reference's strict '<' in visiting order.
// PUs of any size mix in one launch; blocks that do not fit the team's LDS slice fall back to sample-wise reads.
#include "common.h"
#include "tz_dev.h"

namespace {

// state of a PU whose raster stage runs as its own launch (split form, see vvcgpu_tz_search_batch)
struct TzSave { unsigned long long bestSad; int bestX, bestY; unsigned bestDist, bestRound; int pointNr, deferred; int left, top, right, bottom; int x0, y0, nx, ny; int reserved; int pad; };

template <int TEAM>
__global__ __launch_bounds__(256) void tz_search_kernel(const Pel* __restrict__ org, int os, const Pel* __restrict__ ref, int rs,
                                                        const vvcgpu_tz_pu* __restrict__ pus, int n, vvcgpu_tz_cfg cfg,
                                                        vvcgpu_search_best* __restrict__ results, int ldsDwords, int phase, TzSave* __restrict__ save,
                                                        vvcgpu_search_blk* __restrict__ rblk, VvcRasterPer* __restrict__ rper,
                                                        const vvcgpu_search_best* __restrict__ rbest)
{
  extern __shared__ __attribute__((aligned(16))) unsigned orgL[];          // ldsDwords dwords: the sub-sampled original block(s) of the team
  __shared__ unsigned long long keyL[4];
  __shared__ int negL[4];
  __shared__ unsigned segS[4][64 * TZ_SEG_REGS + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = __builtin_amdgcn_readfirstlane(TEAM == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wave);
  if (b >= n) return;                                          // TEAM 4: the whole workgroup leaves; TEAM 1: no barrier is used
  const vvcgpu_tz_pu pu = pus[b];
  if (phase == 2 && !save[b].deferred) return;                 // finished in the first launch (team-uniform)

  TzTeam<TEAM> s;
  s.org = org + (ptrdiff_t)pu.org_y * os + pu.org_x; s.ref = ref; s.os = os; s.rs = rs;
  s.w = pu.w; s.h = pu.h; s.subShift = pu.sub_shift; s.refX = pu.ref_x; s.refY = pu.ref_y;
  s.rx0 = cfg.ref_x0; s.ry0 = cfg.ref_y0; s.rx1 = cfg.ref_x1 - pu.w; s.ry1 = cfg.ref_y1 - pu.h;
  s.horMax = (cfg.pic_w + 8 - pu.pos_x - 1) << 2; s.horMin = (-cfg.max_cu_w - 8 - pu.pos_x + 1) << 2;
  s.verMax = (cfg.pic_h + 8 - pu.pos_y - 1) << 2; s.verMin = (-cfg.max_cu_h - 8 - pu.pos_y + 1) << 2;
  s.lambda = cfg.lambda; s.predHor = pu.pred_hor; s.predVer = pu.pred_ver; s.costScale = cfg.cost_scale; s.imvShift = cfg.imv_shift;
  s.tl = TEAM == 4 ? (int)threadIdx.x : lane;
  int LX = 1; while (4 * LX < pu.w) LX <<= 1;                 // quads along a row, rounded up to a power of two (w <= 128 -> LX <= 32)
  s.LX = LX;
  s.keyL = keyL;
  s.segL = segS[wave];

  // the sub-sampled original block -> LDS as packed pairs (w is a multiple of 4: VVC block widths are 4, 8, 12, 16, 24, ...)
  {
    const int slice = TEAM == 4 ? ldsDwords : ldsDwords / 4;
    tz_stage_org<TEAM>(s, orgL + (TEAM == 4 ? 0 : wave * slice), slice, negL);
  }

  const int range = pu.reserved[0] > 0 ? min(pu.reserved[0], cfg.search_range) : cfg.search_range;   // per-PU range (the adaptive search range is per reference picture), never beyond cfg.search_range: the split form sizes its raster launch from that
  s.bestSad = ~0ull >> 16; s.bestX = s.bestY = 0; s.bestDist = 0; s.bestRound = 0; s.pointNr = 0;
  s.sr = TzRange{ 0, 0, 0, 0 };
  if (phase == 2)
  {
    // resume behind the raster stage: the state of the first launch, then the raster launch's best candidate under the round rule
    // (strictly better than what the earlier rounds found; the raster's own ties were resolved in visiting order by its key)
    const TzSave sv = save[b];
    s.bestSad = sv.bestSad; s.bestX = sv.bestX; s.bestY = sv.bestY; s.bestDist = sv.bestDist; s.bestRound = sv.bestRound; s.pointNr = sv.pointNr;
    s.sr.left = sv.left; s.sr.top = sv.top; s.sr.right = sv.right; s.sr.bottom = sv.bottom;
    const unsigned long long key = rbest[b].cost;
    if (key != ~0ull && (key >> 24) < s.bestSad)
    {
      const int idx = (int)(key & 0xFFFFFFu), j = idx / sv.nx, i = idx - j * sv.nx;
      s.bestSad = key >> 24; s.bestX = sv.x0 + 5 * i; s.bestY = sv.y0 + 5 * j; s.bestDist = 5u; s.bestRound = 0; s.pointNr = 0;
    }
  }
  // first launch of the split form: a plain step-5 raster whose every probe lies inside the readable rectangle (no clamping of the
  // block origin) is left to the raster launch; this PU resumes behind it in the third launch
  // (the raster kernel stages whole 16-byte words of the window rows: 8 samples of slack on both sides)
  auto defer = [&](const TzRound& R, const TzRange& l, int ny) -> bool
  {
    if (!(phase == 1 && R.d == 5 && R.nx <= 40 && ny <= 40 && pu.w == (cfg.uniform_pu & 0xFFFF) && pu.h == ((cfg.uniform_pu >> 16) & 0xFFFF) && pu.sub_shift == 1 &&
          s.refX + l.left - 8 >= s.rx0 && s.refX + l.left + (R.nx - 1) * 5 + 8 <= s.rx1 && s.refY + l.top >= s.ry0 && s.refY + l.top + (ny - 1) * 5 <= s.ry1))
      return false;
    if (s.tl == 0)
    {
      TzSave sv;
      sv.bestSad = s.bestSad; sv.bestX = s.bestX; sv.bestY = s.bestY; sv.bestDist = s.bestDist; sv.bestRound = s.bestRound; sv.pointNr = s.pointNr;
      sv.left = s.sr.left; sv.top = s.sr.top; sv.right = s.sr.right; sv.bottom = s.sr.bottom;
      sv.x0 = l.left; sv.y0 = l.top; sv.nx = R.nx; sv.ny = ny; sv.deferred = 1; sv.reserved = 0;
      save[b] = sv;
      rblk[b] = vvcgpu_search_blk{ pu.org_x, pu.org_y, pu.ref_x, pu.ref_y };       // reference position of the zero vector, as in vvcgpu_sad_search
      rper[b] = VvcRasterPer{ 1, R.nx, ny, l.left, l.top, pu.pred_hor, pu.pred_ver, 0 };
    }
    return true;
  };
  if (!tz_machine<TEAM>(s, pu.flags, range, cfg.first_search_stop, pu.start_x, pu.start_y, pu.pred2_x, pu.pred2_y, phase == 2, defer)) return;

  if (s.tl == 0)
  {
    vvcgpu_search_best r;
    r.x = s.bestX; r.y = s.bestY; r.cost = s.bestSad; r.sad = s.bestSad - s.mvcost(s.bestX, s.bestY);
    results[b] = r;
    if (phase == 1) { save[b].deferred = 0; rper[b].active = 0; rblk[b] = vvcgpu_search_blk{ pu.org_x, pu.org_y, pu.ref_x, pu.ref_y }; }
  }
}

// TZ results -> the block list of the fractional refinement (reference block displaced by the integer MV, :1816) + per-PU predictors
__global__ __launch_bounds__(256) void tz_to_frac_kernel(const vvcgpu_tz_pu* __restrict__ pus, const vvcgpu_search_best* __restrict__ best, int n,
                                                         vvcgpu_frac_blk* __restrict__ blk, int* __restrict__ preds)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const vvcgpu_tz_pu p = pus[i];
  const int bx = best[i].x, by = best[i].y;
  vvcgpu_frac_blk f;
  f.org_x = p.org_x; f.org_y = p.org_y; f.ref_x = p.ref_x + bx; f.ref_y = p.ref_y + by; f.mv_x = bx; f.mv_y = by;
  blk[i] = f;
  preds[2 * i] = p.pred_hor; preds[2 * i + 1] = p.pred_ver;
}

}  // namespace

// the body of vvcgpu_tz_search_batch, claiming from the caller's scope (vvcgpu_me_batch: one scope for the whole chain)
static int tz_search(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_tz_pu* pus, int n,
                     const vvcgpu_tz_cfg* cfg_host, vvcgpu_search_best* results, void* stream, VvcScratch& sc)
{
  VVC_CHECK_ARG(n >= 0, "tz_search_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org && ref && pus && cfg_host && results, "tz_search_batch: null pointer");
  const vvcgpu_tz_cfg c = *cfg_host;
  VVC_CHECK_ARG(org_stride > 0 && ref_stride > 0, "tz_search_batch: strides %d %d", org_stride, ref_stride);
  VVC_CHECK_ARG(c.search_range >= 1 && c.search_range <= 512, "tz_search_batch: search_range %d", c.search_range);
  VVC_CHECK_ARG(c.cost_scale >= 0 && c.cost_scale <= 4 && c.imv_shift >= 0 && c.imv_shift <= 4, "tz_search_batch: cost_scale %d imv_shift %d",
                c.cost_scale, c.imv_shift);
  VVC_CHECK_ARG(c.lambda >= 0.0 && c.lambda < 1048576.0, "tz_search_batch: lambda out of range");
  VVC_CHECK_ARG(c.pic_w > 0 && c.pic_h > 0 && c.max_cu_w > 0 && c.max_cu_h > 0, "tz_search_batch: picture geometry");
  VVC_CHECK_ARG(c.ref_x1 - c.ref_x0 >= 128 && c.ref_y1 - c.ref_y0 >= 128 && c.ref_x0 >= 0 && c.ref_y0 >= 0 && c.ref_x1 <= ref_stride,
                "tz_search_batch: readable rectangle [%d,%d)x[%d,%d) (stride %d) must hold a 128x128 block", c.ref_x0, c.ref_x1, c.ref_y0, c.ref_y1,
                ref_stride);
  hipStream_t st = (hipStream_t)stream;
  // LDS for the teams' original blocks: 32 KB serve any PU (8 KB per wavefront: 64x128 sub-sampled; one workgroup per PU: 128x128); with the
  // caller's word that the PUs are w x h the allocation shrinks to what they need (16x16: 1 KB per workgroup), which doubles the resident
  // wavefronts of this latency-bound kernel (a PU that is larger after all reads its block sample-wise: correct, slower)
  int ldsDwords = TZ_LDS_DWORDS;
  {
    const int uw0 = c.uniform_pu & 0xFFFF, uh0 = (c.uniform_pu >> 16) & 0xFFFF;
    if (c.uniform_pu != 0 && uw0 >= 4 && uh0 >= 4 && uw0 <= 128 && uh0 <= 128)
    {
      const int per = (((uh0 >> 1) * (uw0 >> 1)) + 63) & ~63;
      ldsDwords = c.wg_per_pu ? per : 4 * per;
      if (ldsDwords > TZ_LDS_DWORDS) ldsDwords = TZ_LDS_DWORDS;
    }
  }
  auto launch = [&](int phase, TzSave* save, vvcgpu_search_blk* rblk, VvcRasterPer* rper, const vvcgpu_search_best* rbest)
  {
    if (c.wg_per_pu)
      hipLaunchKernelGGL(tz_search_kernel<4>, dim3(n), dim3(256), (size_t)ldsDwords * 4, st, org, org_stride, ref, ref_stride, pus, n, c, results, ldsDwords, phase, save, rblk, rper, rbest);
    else
      hipLaunchKernelGGL(tz_search_kernel<1>, dim3((n + 3) / 4), dim3(256), (size_t)ldsDwords * 4, st, org, org_stride, ref, ref_stride, pus, n, c, results, ldsDwords, phase, save, rblk, rper, rbest);
  };
  // Split form (cfg.uniform_pu = h << 16 | w: the caller states that EVERY PU of the batch is w x h with 2:1 row sub-sampling): the raster stage,
  // 86 % of the probes of a search that enters it, runs as the quad raster kernel of sadsearch.hip between two launches of the state machine --
  // the in-kernel raster round works one wavefront per PU at ~8 % of the v_sad_u16 issue rate, the raster kernel at ~60 %.
  const int uw = c.uniform_pu & 0xFFFF, uh = (c.uniform_pu >> 16) & 0xFFFF;
  const int gridMax = (2 * c.search_range) / 5 + 1;
  if (c.uniform_pu != 0 && (uw == 16 || uw == 32 || uw == 64) && (uh == 16 || uh == 32 || uh == 64) && gridMax <= 40 &&
      (org_stride & 1) == 0 && (ref_stride & 7) == 0 && ((uintptr_t)org & 3) == 0 && ((uintptr_t)ref & 15) == 0)
  {
    TzSave* save = sc.take<TzSave>(n);
    vvcgpu_search_best* rbest = sc.take<vvcgpu_search_best>(n);
    VvcRasterPer* rper = sc.take<VvcRasterPer>(n);
    vvcgpu_search_blk* rblk = sc.take<vvcgpu_search_blk>(n);
    unsigned* packed = sc.take<unsigned>((size_t)n * 2 * (uh >> 1) * (uw >> 1));
    if (!save || !rbest || !rper || !rblk || !packed) return VVCGPU_E_DEVICE;
    launch(1, save, rblk, rper, nullptr);
    VVC_LAUNCH_CHECK();
    vvcgpu_mvcost mv;
    mv.lambda = c.lambda; mv.pred_hor = 0; mv.pred_ver = 0; mv.cost_scale = c.cost_scale; mv.imv_shift = c.imv_shift;
    const int rc = vvcgpu_raster_per_block_launch(org, org_stride, ref, ref_stride, rblk, rper, n, uw, uh, 1, gridMax, gridMax, &mv, rbest, packed, st);
    if (rc != VVCGPU_OK) return rc;
    launch(2, save, rblk, rper, rbest);
    VVC_LAUNCH_CHECK();
    return VVCGPU_OK;
  }
  launch(0, nullptr, nullptr, nullptr, nullptr);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

extern "C" {

int vvcgpu_tz_search_batch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride,
                           const vvcgpu_tz_pu* pus, int n, const vvcgpu_tz_cfg* cfg_host,
                           vvcgpu_search_best* results, void* stream)
{
  VvcScratch sc((hipStream_t)stream);
  return tz_search(org, org_stride, ref, ref_stride, pus, n, cfg_host, results, stream, sc);
}

int vvcgpu_me_batch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_tz_pu* pus, int n, int w, int h,
                    const vvcgpu_tz_cfg* cfg_host, int bit_depth, int clp_min, int clp_max, int use_hadamard,
                    vvcgpu_search_best* int_results, vvcgpu_frac_result* frac_results, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "me_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(cfg_host && int_results && frac_results, "me_batch: null pointer");
  vvcgpu_tz_cfg cfgu = *cfg_host;
  if (cfgu.uniform_pu == 0 && (w == 16 || w == 32 || w == 64) && (h == 16 || h == 32 || h == 64)) cfgu.uniform_pu = (h << 16) | w;   // the chain's PUs are w x h
  hipStream_t st = (hipStream_t)stream;
  VvcScratch sc(st);
  int rc = tz_search(org, org_stride, ref, ref_stride, pus, n, &cfgu, int_results, stream, sc);
  if (rc != VVCGPU_OK) return rc;
  vvcgpu_frac_blk* blk = sc.take<vvcgpu_frac_blk>(n);
  int* preds = sc.take<int>(2 * (size_t)n);
  if (!blk || !preds) return VVCGPU_E_DEVICE;
  hipLaunchKernelGGL(tz_to_frac_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, pus, int_results, n, blk, preds);
  VVC_LAUNCH_CHECK();
  vvcgpu_mvcost mv;
  mv.lambda = cfg_host->lambda; mv.pred_hor = 0; mv.pred_ver = 0; mv.cost_scale = 0; mv.imv_shift = 0;
  return vvcgpu_frac_refine_launch(org, org_stride, ref, ref_stride, blk, n, w, h, bit_depth, clp_min, clp_max, use_hadamard, &mv, preds,
                                   frac_results, stream);
}

}  // extern "C"
