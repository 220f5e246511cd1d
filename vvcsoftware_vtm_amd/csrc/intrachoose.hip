// intrachoose.hip -- vvcgpu_intra_luma_choose_batch and vvcgpu_intra_chroma_choose_batch: the cost compares of the intra RD loops over the outputs of
// the pixel passes and of vvcgpu_resi_rate_batch, and the commit of the winner (reconstruction, levels, context row), one launch each.
//
// Reference behaviour reproduced (bit-exact, the host's doubles included):
//   IntraSearch::estIntraPredLumaQT, the mode loop                                               EncoderLib/IntraSearch.cpp:637-697
//   IntraSearch::xRecurIntraCodingLumaQT, the transform loop                                     EncoderLib/IntraSearch.cpp:1429-1588
//   IntraSearch::estIntraPredChromaQT, the mode loop and the copies behind it                    EncoderLib/IntraSearch.cpp:773-847
//   IntraSearch::xGetIntraFracBitsQT as a sum of distinct contexts' bits                         EncoderLib/IntraSearch.cpp:1047-1128
//   RdCost::calcRdCost (a multiply, then an add), RdCost::getDistPart                            CommonLib/RdCost.cpp, RdCost.h:406-409
//
// Design (docs/KERNELS.md, "The intra compares"): a wavefront takes a PU.  Its lanes form the costs of the candidates (at most 80: two per lane) and
// lay them into LDS; lane 0 walks the two ordered loops over them exactly as the host does, ties included; all 64 lanes then copy the winner, a row
// at a time in the widest word that source and destination row are both aligned to.  The grid may be smaller than the list.
#include "common.h"
#include "intrachoose_dev.h"

static_assert(sizeof(vvcgpu_intra_choose_pu) == 96 && sizeof(vvcgpu_intra_choose_result) == 48, "descriptor layouts");
static_assert(sizeof(vvcgpu_intra_chroma_choose_pu) == 160 && sizeof(vvcgpu_intra_chroma_choose_result) == 48, "descriptor layouts");

namespace {

struct LcArgs
{
  const vvcgpu_intra_choose_pu* pus; const vvcgpu_resi_chain_desc* tus; const unsigned* absSum; const unsigned* numSig; const unsigned long long* dist;
  const int* modeOut; const unsigned long long* frac; double scale; const Pel* rec; const TCoeff* level; const unsigned char* ctxOut; Pel* recDst;
  TCoeff* levelDst; unsigned char* ctxBest; unsigned long long* candCost; vvcgpu_intra_choose_result* result; int nPu, n;
};

__global__ __launch_bounds__(IC_THREADS) void intra_luma_choose_kernel(const LcArgs a)
{
  __shared__ double costS[IC_WAVES][IC_MAX_CAND];
  __shared__ unsigned char codeS[IC_WAVES][IC_MAX_CAND];                  // IC_VALID | IC_CBF | IC_TS | IC_PASSED
  __shared__ int bestS[IC_WAVES];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double* const cost = costS[wave];
  unsigned char* const code = codeS[wave];

  for (int p = (int)blockIdx.x * IC_WAVES + wave; p < a.nPu; p += (int)gridDim.x * IC_WAVES)
  {
    const vvcgpu_intra_choose_pu* const up = a.pus + p;                   // (indexed members are read where they lie: no private copy of the arrays)
    const vvcgpu_intra_choose_pu u = *up;
    const int nm = u.n_modes, nt = u.n_tr, nc = nm * nt;
    bool ok = nm >= 1 && nm <= 16 && nt >= 1 && nt <= 5 && u.cand_first >= 0 && (long long)u.cand_first + nm * nt <= (long long)a.n;
    ok = ok && (u.flags & ~7) == 0 && (u.reserved[0] | u.reserved[1]) == 0;
    int w = 0, h = 0;
    if (ok)
    {
      w = a.tus[u.cand_first].w; h = a.tus[u.cand_first].h;
      ok = side_ok(w, 4) && side_ok(h, 4);
      bool same = true;
      for (int c = lane; c < nc; c += 64) same = same && a.tus[u.cand_first + c].w == w && a.tus[u.cand_first + c].h == h;
      ok = ok && __ballot(!same) == 0ull;
    }
    int best = -1;
    if (ok)
    {
      const bool emtFlag = u.flags & VVCGPU_INTRA_CHOOSE_EMT_FLAG, tsLast = u.flags & VVCGPU_INTRA_CHOOSE_TS_LAST;
      // ---- lanes as candidates: bits and cost
      for (int c = lane; c < nc; c += 64)
      {
        const int j = u.cand_first + c, t = c % nt;
        const unsigned s = a.absSum[j];
        const unsigned long long fb = a.frac[j];
        const bool cbf = s > 0u, valid = s != 0xFFFFFFFFu && (!cbf || fb != ~0ull), ts = tsLast && t == nt - 1;
        const int mode = a.modeOut[j];
        const int cls = mode == u.mpm[0] ? 0 : mode == u.mpm[1] ? 1 : mode == u.mpm[2] ? 2 : 3;
        const unsigned long long bits = up->mode_bits[cls] + up->cbf_bits[cbf ? 1 : 0] + (cbf ? u.emt_cu_bits + fb : 0ull);
        const bool forbidden = (ts && !cbf) || (emtFlag && t > 0 && !ts && a.numSig[j] <= IC_EMT_SIG_NUM_THR);    // :1501-1502
        cost[c] = forbidden ? RD_MAX_DOUBLE : rd_cost(a.scale, a.dist[j], bits);
        code[c] = (unsigned char)((valid ? IC_VALID : 0) | (cbf ? IC_CBF : 0) | (ts ? IC_TS : 0));
      }
      wave_sync();
      // ---- lane 0 as the host: the transform loop inside the mode loop
      if (lane == 0)
      {
        const bool fastEmt = u.flags & VVCGPU_INTRA_CHOOSE_FAST_EMT;
        double bestCost = RD_MAX_DOUBLE;
        for (int m = 0; m < nm; m++)
        {
          const int c0 = m * nt;
          if (!(code[c0] & IC_VALID)) { for (int t = 0; t < nt; t++) code[c0 + t] |= IC_PASSED; continue; }
          double single = RD_MAX_DOUBLE;
          int bt = -1;
          bool cbfBest = false;
          for (int t = 0; t < nt; t++)
          {
            const unsigned cd = code[c0 + t];
            if (!(cd & IC_VALID) || (fastEmt && t > 0 && !(cd & IC_TS) && !cbfBest)) { code[c0 + t] = (unsigned char)(cd | IC_PASSED); continue; }   // :1449
            const double cs = cost[c0 + t];
            if (cs < single) { single = cs; bt = c0 + t; cbfBest = cd & IC_CBF; }                                     // :1524
          }
          if (bt >= 0 && single < bestCost) { bestCost = single; best = bt; }                                         // :664
        }
        bestS[wave] = best;
      }
      wave_sync();
      best = bestS[wave];
      for (int c = lane; c < nc; c += 64)
        a.candCost[u.cand_first + c] = (code[c] & IC_PASSED) ? VVCGPU_INTRA_CHOOSE_PASSED : (unsigned long long)__double_as_longlong(cost[c]);
    }
    // ---- the result and the commit
    vvcgpu_intra_choose_result r;
    r.best_cand = -1; r.best_mode = -1; r.best_tr = -1; r.cbf = 0; r.dist = ~0ull; r.bits = ~0ull; r.cost = RD_MAX_DOUBLE; r.reserved = 0;
    if (best >= 0)
    {
      const int j = u.cand_first + best;
      const bool cbf = code[best] & IC_CBF;
      const int mode = a.modeOut[j];
      const int cls = mode == u.mpm[0] ? 0 : mode == u.mpm[1] ? 1 : mode == u.mpm[2] ? 2 : 3;
      r.best_cand = j; r.best_mode = mode; r.best_tr = best % nt; r.cbf = cbf ? 1 : 0; r.dist = a.dist[j];
      r.bits = up->mode_bits[cls] + up->cbf_bits[cbf ? 1 : 0] + (cbf ? u.emt_cu_bits + a.frac[j] : 0ull);
      r.cost = cost[best];
      const vvcgpu_resi_chain_desc t = a.tus[j];
      ic_copy_block(a.rec + t.rec_off, t.rec_stride, a.recDst + u.rec_dst_off, u.rec_dst_stride, w, h, lane);
      ic_copy_levels(a.level + t.level_off, a.levelDst + u.level_dst_off, w * h, lane);
      if (a.ctxOut) ic_copy_row(a.ctxOut + (size_t)j * VVCGPU_RESI_RATE_CTX_BYTES, a.ctxBest + (size_t)p * VVCGPU_RESI_RATE_CTX_BYTES, lane);
    }
    if (lane == 0) a.result[p] = r;
    wave_sync();                                                          // the costs and codes are free again
  }
}

struct CcArgs
{
  const vvcgpu_intra_chroma_choose_pu* cpus; const vvcgpu_intra_chroma_pu* pus; const unsigned* absSum; const unsigned long long* dist;
  const unsigned long long* fracCb; const unsigned long long* fracCr; double scale; const Pel* rec; const TCoeff* level; const unsigned char* ctxOut;
  Pel* recDst; TCoeff* levelDst; unsigned char* ctxBest; unsigned long long* slotCost; vvcgpu_intra_chroma_choose_result* result; int n;
};

__global__ __launch_bounds__(IC_THREADS) void intra_chroma_choose_kernel(const CcArgs a)
{
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int p = (int)blockIdx.x * IC_WAVES + wave; p < a.n; p += (int)gridDim.x * IC_WAVES)
  {
    const vvcgpu_intra_chroma_choose_pu* const up = a.cpus + p;           // (indexed members are read where they lie: no private copy of the arrays)
    const vvcgpu_intra_chroma_pu* const qp = a.pus + p;
    const vvcgpu_intra_chroma_choose_pu u = *up;
    const vvcgpu_intra_chroma_pu q = *qp;
    const int w = q.w, h = q.h;
    const bool ok = side_ok(w, 2) && side_ok(h, 2) && (u.reserved[0] | u.reserved[1] | u.reserved[2]) == 0;
    // ---- lanes 0..5 as slots
    const int k = lane < 6 ? lane : 5;
    const size_t o = 12 * (size_t)p + 2 * k;
    const unsigned sCb = a.absSum[o], sCr = a.absSum[o + 1];
    const bool cbfCb = sCb > 0u, cbfCr = sCr > 0u;
    const unsigned long long fCb = a.fracCb[o], fCr = a.fracCr[o + 1];
    const bool cand = ok && lane < 6 && qp->mode[k] != -1 && sCb != 0xFFFFFFFFu && sCr != 0xFFFFFFFFu && (!cbfCb || fCb != ~0ull) && (!cbfCr || fCr != ~0ull);
    const unsigned long long bits = up->mode_bits[k] + up->cbf_cb_bits[cbfCb ? 1 : 0] + up->cbf_cr_bits[2 * (cbfCb ? 1 : 0) + (cbfCr ? 1 : 0)]
                                    + (cbfCb ? fCb : 0ull) + (cbfCr ? fCr : 0ull);
    const unsigned long long dist = rd_weighted(u.dist_weight[0], a.dist[o]) + rd_weighted(u.dist_weight[1], a.dist[o + 1]);
    const double cost = rd_cost(a.scale, dist, bits);
    if (lane < 6) a.slotCost[6 * (size_t)p + k] = cand ? (unsigned long long)__double_as_longlong(cost) : VVCGPU_INTRA_CHOOSE_PASSED;
    // ---- the ordered loop of :773-826 over the six lanes' values
    const unsigned long long cands = __ballot(cand);
    int best = -1;
    double bestCost = RD_MAX_DOUBLE;
    for (int s = 0; s < 6; s++)
    {
      const double cs = __shfl(cost, s);
      if (((cands >> s) & 1ull) && cs < bestCost) { bestCost = cs; best = s; }                                          // :803
    }
    vvcgpu_intra_chroma_choose_result r;
    r.best_slot = -1; r.best_mode = -1; r.cbf[0] = 0; r.cbf[1] = 0; r.dist = ~0ull; r.bits = ~0ull; r.cost = RD_MAX_DOUBLE; r.reserved = 0;
    if (best >= 0)
    {
      r.best_slot = best; r.best_mode = qp->mode[best]; r.cbf[0] = __shfl((int)cbfCb, best); r.cbf[1] = __shfl((int)cbfCr, best);
      r.dist = __shfl(dist, best); r.bits = __shfl(bits, best); r.cost = bestCost;
      const int area = w * h;
#pragma unroll
      for (int c = 0; c < 2; c++)
      {
        const long long blk = (long long)(2 * best + c) * area;
        ic_copy_block(a.rec + q.cand_off + blk, w, a.recDst + u.rec_dst_off[c], u.rec_dst_stride, w, h, lane);
        ic_copy_levels(a.level + q.level_off + blk, a.levelDst + u.level_dst_off[c], area, lane);
      }
      if (a.ctxOut)
        ic_copy_row(a.ctxOut + (12 * (size_t)p + 2 * best + 1) * VVCGPU_RESI_RATE_CTX_BYTES, a.ctxBest + (size_t)p * VVCGPU_RESI_RATE_CTX_BYTES, lane);
    }
    if (lane == 0) a.result[p] = r;
  }
}

inline bool ic_aligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) == 0; }

}  // namespace

extern "C" int vvcgpu_intra_luma_choose_batch(const struct vvcgpu_intra_choose_pu* pus, int n_pu, const vvcgpu_resi_chain_desc* tus, int n,
                                              const uint32_t* abs_sum, const uint32_t* num_sig, const uint64_t* dist, const int32_t* mode_out,
                                              const uint64_t* frac_bits, double dist_scale, const vvc_pel* rec_base, const vvc_coef* level_base,
                                              const uint8_t* ctx_out, vvc_pel* rec_dst_base, vvc_coef* level_dst_base, uint8_t* ctx_best,
                                              double* cand_cost, struct vvcgpu_intra_choose_result* result, void* stream)
{
  const char* name = "intra_luma_choose_batch";
  VVC_CHECK_ARG(n_pu >= 0 && n >= 0, "%s: n_pu %d, n %d", name, n_pu, n);
  if (n_pu == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(pus && tus && abs_sum && num_sig && dist && mode_out && frac_bits && rec_base && level_base && rec_dst_base && level_dst_base && cand_cost
                && result, "%s: null pointer", name);
  VVC_CHECK_ARG((ctx_out != nullptr) == (ctx_best != nullptr), "%s: ctx_out and ctx_best go together", name);
  VVC_CHECK_ARG(ic_aligned(pus, 15) && ic_aligned(tus, 15) && ic_aligned(result, 15), "%s: pus, tus and result must be 16-byte aligned", name);
  VVC_CHECK_ARG(ic_aligned(dist, 7) && ic_aligned(frac_bits, 7) && ic_aligned(cand_cost, 7) && ic_aligned(abs_sum, 3) && ic_aligned(num_sig, 3)
                && ic_aligned(mode_out, 3), "%s: misaligned array", name);
  LcArgs a;
  a.pus = pus; a.tus = tus; a.absSum = abs_sum; a.numSig = num_sig; a.dist = reinterpret_cast<const unsigned long long*>(dist); a.modeOut = mode_out;
  a.frac = reinterpret_cast<const unsigned long long*>(frac_bits); a.scale = dist_scale; a.rec = rec_base; a.level = level_base; a.ctxOut = ctx_out;
  a.recDst = rec_dst_base; a.levelDst = level_dst_base; a.ctxBest = ctx_best; a.candCost = reinterpret_cast<unsigned long long*>(cand_cost);
  a.result = result; a.nPu = n_pu; a.n = n;
  hipLaunchKernelGGL(intra_luma_choose_kernel, dim3(vvc_grid_cap(n_pu, IC_WAVES, 8)), dim3(IC_THREADS), 0, (hipStream_t)stream, a);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

extern "C" int vvcgpu_intra_chroma_choose_batch(const struct vvcgpu_intra_chroma_choose_pu* cpus, const vvcgpu_intra_chroma_pu* pus, int n,
                                                const uint32_t* abs_sum, const uint64_t* dist, const uint64_t* frac_bits_cb, const uint64_t* frac_bits_cr,
                                                double dist_scale, const vvc_pel* cand_rec_base, const vvc_coef* level_base, const uint8_t* ctx_out,
                                                vvc_pel* rec_dst_base, vvc_coef* level_dst_base, uint8_t* ctx_best, double* slot_cost,
                                                struct vvcgpu_intra_chroma_choose_result* result, void* stream)
{
  const char* name = "intra_chroma_choose_batch";
  VVC_CHECK_ARG(n >= 0 && n <= 0x7FFFFFFF / 12, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(cpus && pus && abs_sum && dist && frac_bits_cb && frac_bits_cr && cand_rec_base && level_base && rec_dst_base && level_dst_base && slot_cost
                && result, "%s: null pointer", name);
  VVC_CHECK_ARG((ctx_out != nullptr) == (ctx_best != nullptr), "%s: ctx_out and ctx_best go together", name);
  VVC_CHECK_ARG(ic_aligned(cpus, 15) && ic_aligned(pus, 15) && ic_aligned(result, 15), "%s: cpus, pus and result must be 16-byte aligned", name);
  VVC_CHECK_ARG(ic_aligned(dist, 7) && ic_aligned(frac_bits_cb, 7) && ic_aligned(frac_bits_cr, 7) && ic_aligned(slot_cost, 7) && ic_aligned(abs_sum, 3),
                "%s: misaligned array", name);
  CcArgs a;
  a.cpus = cpus; a.pus = pus; a.absSum = abs_sum; a.dist = reinterpret_cast<const unsigned long long*>(dist);
  a.fracCb = reinterpret_cast<const unsigned long long*>(frac_bits_cb); a.fracCr = reinterpret_cast<const unsigned long long*>(frac_bits_cr);
  a.scale = dist_scale; a.rec = cand_rec_base; a.level = level_base; a.ctxOut = ctx_out; a.recDst = rec_dst_base; a.levelDst = level_dst_base;
  a.ctxBest = ctx_best; a.slotCost = reinterpret_cast<unsigned long long*>(slot_cost); a.result = result; a.n = n;
  hipLaunchKernelGGL(intra_chroma_choose_kernel, dim3(vvc_grid_cap(n, IC_WAVES, 8)), dim3(IC_THREADS), 0, (hipStream_t)stream, a);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
