// resirate.hip -- vvcgpu_resi_rate_batch: CABACWriter::residual_coding under the bit estimator for a list of level blocks, in one launch, and
// vvcgpu_inter_resi_choose_batch: the compare of xEstimateInterResidualQT over the outputs of the inter residual pass and of the former.
//
// Reference behaviour reproduced (bit-exact):
//   CABACWriter::residual_coding                                                                 EncoderLib/CABACWriter.cpp:1970-2087
//     transform_skip_flag :2090-2103, emt_tu_index :2106-2133, last_sig_coeff :2202-2255, residual_coding_subblock :2260-2383
//   CoeffCodingContext, initSubblock                                                             CommonLib/ContextModelling.cpp:217-393
//     sigCtxIdAbs, ctxOffsetAbs, GoRiceParAbs                                                    CommonLib/ContextModelling.h:135-220
//   BinProbModel_Std::estFracBitsUpdate, BitEstimatorBase::encodeBinsEP / encodeRemAbsEP         Contexts.h:91-96, BinEncoder.h:266-267, BinEncoder.cpp:452-503
//   InterSearch::xEstimateInterResidualQT, the compare                                           EncoderLib/InterSearch.cpp:4395-4568
//
// Design (docs/KERNELS.md, "The residual rate"): the bins of a block and the context of every bin follow from the levels alone, and the fractional
// bits are a sum, so only the bins of ONE context are ordered.  A wavefront takes an item and lays its levels (16 bits each) into LDS, finding
// scanPosLast, numSig and the significant groups on the way (the inverse scan of transform.hip).  Then, 64 scan positions at a time from the last
// one down: with lanes as scan positions it forms the template sums, the state of the dependent-quantisation automaton (a suffix composition of the
// parity maps), every position's bins and context offsets as one 18-bit record, and the bypass bits as a sum; with lanes as contexts it walks the
// records of the chunk (v_readlane, no LDS), every lane updating the states it owns.  The two model tables sit in LDS.
#include "common.h"
#include "resirate_dev.h"

static_assert(sizeof(vvcgpu_resi_rate_item) == 32 && sizeof(vvcgpu_inter_resi_item) == 80, "descriptor layouts");

namespace {

struct RrArgs
{
  const TCoeff* level; const RrItem* items; const unsigned* gate; const unsigned char* ctx; const unsigned* est; const unsigned char* nxt;
  unsigned long long* frac; unsigned* numSig; unsigned char* ctxOut; const unsigned short* scan; const unsigned short* inv; const int* scanOff;
  int n, nCtx;
};

// record of a scan position: sig context 0..59 | sig coded << 6 | non-zero << 7 | ctxOffsetAbs << 8 | par << 13 | gt1 << 14 | gt2 << 15; on the first
// position of a group also its flag << 16 | (sigRight | sigLower) << 17
#define RR_UPD(S, hit, bin) do { if (hit) { acc += estS[(S) ^ (bin)]; (S) = nxtS[((S) << 1) | (bin)]; } } while (0)

__device__ __forceinline__ bool rr_item_ok(const RrItem& t, int nCtx)
{
  bool ok = rr_side_ok(t.w) && rr_side_ok(t.h) && t.ctx_idx >= 0 && t.ctx_idx < nCtx && t.level_off >= 0;
  ok = ok && (t.luma | 1) == 1 && (t.dep_quant | 1) == 1 && (t.sign_hiding | 1) == 1 && t.ts_flag >= -1 && t.ts_flag <= 1;
  ok = ok && t.emt_idx >= -1 && t.emt_idx <= 3 && (t.emt_inter | 1) == 1 && (t.emt_thr | 1) == 1;
  int res = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) res |= t.reserved[i];
  return ok && res == 0;
}

__global__ __launch_bounds__(RR_THREADS) void resi_rate_kernel(const RrArgs a)
{
  __shared__ unsigned estS[128];
  __shared__ unsigned char nxtS[256];
  __shared__ short levS[RR_WAVES][RR_MAX_COEF];
  __shared__ __align__(4) unsigned char cgS[RR_WAVES][RR_MAX_GROUPS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < 128) estS[tid] = a.est[tid];
  nxtS[tid] = a.nxt[tid];
  __syncthreads();                                                        // the only workgroup barrier: below every wavefront walks its own items
  short* const lev = levS[wave];
  unsigned char* const cg = cgS[wave];
  const int b0 = rr_row_byte(0, lane), b1 = rr_row_byte(1, lane), b2 = rr_row_byte(2, lane);
  const int absCls = lane < 21 ? 0 : lane < 42 ? 1 : 2, absLane = lane - 21 * absCls;     // lane 63 (transform skip): 21, no offset

  for (int item = (int)blockIdx.x * RR_WAVES + wave; item < a.n; item += (int)gridDim.x * RR_WAVES)
  {
    const RrItem t = a.items[item];
    if ((a.gate && a.gate[item] == 0xFFFFFFFFu) || !rr_item_ok(t, a.nCtx))                   // skipped: the markers, nothing else
    {
      if (lane == 0) { a.frac[item] = ~0ull; a.numSig[item] = 0xFFFFFFFFu; }
      continue;
    }
    const int w = t.w, h = t.h, lw = ilog2(w), lh = ilog2(h), N = w * h;
    const int lg = ((w | h) & 3) ? 1 : 2, lcg = 2 * lg, CG = 1 << lcg, wg = w >> lg, hg = h >> lg;
    const int so = a.scanOff[(lw - 1) * 6 + lh - 1];
    const bool luma = t.luma != 0;
    const unsigned char* const row = a.ctx + (size_t)t.ctx_idx * VVCGPU_RESI_RATE_CTX_BYTES;
    unsigned s0 = row[b0] & 127u, s1 = row[b1] & 127u, s2 = row[b2] & 127u;
    unsigned long long acc = 0;                                           // fractional bits of the lane's contexts
    unsigned ep = 0;                                                      // bypass bins: uniform parts on lane 0, the remainders on their lanes

    // ---- the levels into LDS; scanPosLast, numSig and the significant groups
    reinterpret_cast<unsigned*>(cg)[lane] = 0u;
    wave_sync();
    int last = -1;
    unsigned numSig = 0;
    {
      const TCoeff* const src = a.level + t.level_off;
      for (int i = lane; i < N; i += 64)
      {
        const int v = clip3(-32767, 32767, src[i]);
        lev[i] = (short)v;
        if (v != 0)
        {
          last = max(last, (int)a.inv[so + i]);
          cg[((i >> lw) >> lg) * wg + ((i & (w - 1)) >> lg)] = 1;
        }
        numSig += (unsigned)__popcll(__ballot(v != 0));
      }
    }
    last = __builtin_amdgcn_readfirstlane(wave_max(last));
    numSig = (unsigned)__builtin_amdgcn_readfirstlane((int)numSig);
    wave_sync();

    if (last >= 0)
    {
      // ---- transform_skip_flag, last_sig_coeff, emt_tu_index
      if (t.ts_flag >= 0) RR_UPD(s1, lane == 63, (unsigned)t.ts_flag);
      {
        const int posL = a.scan[so + last], px = posL & (w - 1), py = posL >> lw;
        const int gx = rr_group_idx(px), gy = rr_group_idx(py), mx = rr_group_idx(w - 1), my = rr_group_idx(h - 1);
        // prefix_ctx[log2 side] = 0, 0, 0, 3, 6, 10, 15 (the luma table of the rectCUs branch); chroma: no offset, the shift Clip3(0, 2, side >> 3)
        const int pcX = lw < 3 ? 0 : lw == 3 ? 3 : lw == 4 ? 6 : lw == 5 ? 10 : 15, pcY = lh < 3 ? 0 : lh == 3 ? 3 : lh == 4 ? 6 : lh == 5 ? 10 : 15;
        const int oX = luma ? pcX : 0, oY = luma ? pcY : 0;
        const int shX = luma ? (lw + 1) >> 2 : min(2, w >> 3), shY = luma ? (lh + 1) >> 2 : min(2, h >> 3);
        const int nbX = gx + (gx < mx ? 1 : 0), nbY = gy + (gy < my ? 1 : 0);
        for (int i = 0; i < nbX; i++) RR_UPD(s2, lane == VVCGPU_RESI_RATE_LAST_X + oX + (i >> shX), (unsigned)(i < gx));
        for (int i = 0; i < nbY; i++) RR_UPD(s2, lane == VVCGPU_RESI_RATE_LAST_Y + oY + (i >> shY), (unsigned)(i < gy));
        if (lane == 0) ep += (unsigned)((gx > 3 ? (gx - 2) >> 1 : 0) + (gy > 3 ? (gy - 2) >> 1 : 0));
      }
      if (t.emt_idx >= 0 && (!t.emt_thr || numSig > 2u))
      {
        RR_UPD(s2, lane == 50 + 2 * t.emt_inter, (unsigned)(t.emt_idx & 1));
        RR_UPD(s2, lane == 51 + 2 * t.emt_inter, (unsigned)(t.emt_idx >> 1));
      }

      // ---- the sub-blocks, 64 scan positions at a time from the last one down
      const int lastSub = last >> lcg;
      unsigned dqState = 0;                                               // the automaton's state on entry of the chunk
      for (int c = last >> 6; c >= 0; c--)
      {
        // lanes are scan positions
        const int p = (c << 6) + lane;
        const bool inBlock = p < N && p <= last;
        const int pos = inBlock ? a.scan[so + p] : 0, x = pos & (w - 1), y = pos >> lw, diag = x + y;
        const int v = inBlock ? lev[pos] : 0, av = abs(v);
        const int sub = p >> lcg, cgIdx = (y >> lg) * wg + (x >> lg);
        const bool subSig = sub == 0 || sub == lastSub || cg[cgIdx] != 0;
        const bool processed = inBlock && subSig;
        int sumAbs = 0, numPos = 0, sumGr = 0;
        {
          const bool r1 = x < w - 1, r2 = x < w - 2, d1 = y < h - 1, d2 = y < h - 2;
          const int nb[5] = { r1 ? lev[pos + 1] : 0, r2 ? lev[pos + 2] : 0, (r1 && d1) ? lev[pos + w + 1] : 0, d1 ? lev[pos + w] : 0, d2 ? lev[pos + 2 * w] : 0 };
#pragma unroll
          for (int k = 0; k < 5; k++) { const int q = abs(nb[k]); sumAbs += min(4 - (q & 1), q); numPos += q != 0; sumGr += q - (q != 0); }
        }
        const unsigned long long nzb = __ballot(processed && v != 0);
        const unsigned subMask = (unsigned)(nzb >> (lane & ~(CG - 1))) & ((1u << CG) - 1u);                 // the non-zero positions of the lane's group
        const bool groupHead = (lane & (CG - 1)) == 0;
        const bool inferLast = p == last;
        const bool inferFirst = processed && sub != 0 && sub != lastSub && groupHead && subMask == 1u;
        // the automaton's state in front of the position: the maps of the positions coded before it in the chunk, composed, on the entry state
        unsigned state = 0;
        if (t.dep_quant)
        {
          unsigned g = processed ? ((v & 1) ? RR_DQ_ODD : RR_DQ_EVEN) : RR_DQ_ID;
#pragma unroll
          for (int d = 1; d < 64; d <<= 1)
          {
            unsigned o = (unsigned)__shfl_down((int)g, d);
            if (lane + d >= 64) o = RR_DQ_ID;
            g = rr_dq_compose(g, o);
          }
          unsigned e = (unsigned)__shfl_down((int)g, 1);
          if (lane == 63) e = RR_DQ_ID;
          state = (e >> (2 * dqState)) & 3u;
          dqState = (unsigned)__builtin_amdgcn_readfirstlane((int)((g >> (2 * dqState)) & 3u));
        }
        const int sigCtx = 20 * max(0, (int)state - 1) + min(sumAbs, 5) + (diag < 2 ? 6 : 0) + (luma && diag < 5 ? 6 : 0);
        // ctxOffsetAbs: from the template of the last sigCtxIdAbs -- the position's own, the next position's for an inferred first position of a
        // group, none (offset 0) for the last position of the block
        int tDiag = diag, tSum1 = sumAbs - numPos;
        const int nDiag = __shfl_down(tDiag, 1), nSum1 = __shfl_down(tSum1, 1);
        if (inferFirst) { tDiag = nDiag; tSum1 = nSum1; }
        int absOff = min(tSum1, 4) + 1 + (tDiag == 0 ? (luma ? 15 : 5) : luma ? (tDiag < 3 ? 10 : tDiag < 10 ? 5 : 0) : 0);
        if (inferLast) absOff = 0;
        unsigned rec = 0;
        if (processed)
        {
          const bool nz = v != 0;
          rec = (unsigned)sigCtx | ((!inferLast && !inferFirst) ? 1u << 6 : 0u) | (nz ? 1u << 7 : 0u);
          if (nz) rec |= (unsigned)absOff << 8 | (unsigned)((av - 1) & 1) << 13 | (av >= 3 ? 1u << 14 : 0u) | (av > 4 ? 1u << 15 : 0u);
          if (av > 4) ep += (unsigned)rr_rem_bins((unsigned)(av - 5) >> 1, rr_rice_par(min(sumGr, 31)));
        }
        if (groupHead && inBlock)                                         // the group's flag and its context: the flags of the groups right of and below it
        {
          const bool right = (x >> lg) + 1 < wg && cg[cgIdx + 1] != 0, lower = (y >> lg) + 1 < hg && cg[cgIdx + wg] != 0;
          rec |= (cg[cgIdx] != 0 ? 1u << 16 : 0u) | ((right || lower) ? 1u << 17 : 0u);
        }
        // signs: one per non-zero level, one less in a group that hides one (posLast - posFirst >= SBH_THRESHOLD)
        {
          const bool hides = t.sign_hiding && groupHead && subMask != 0u && (31 - __clz((int)subMask)) - (__ffs((int)subMask) - 1) >= 4;
          const unsigned long long hideMask = __ballot(hides);
          if (lane == 0) ep += (unsigned)__popcll(nzb) - (unsigned)__popcll(hideMask);
        }

        // lanes are contexts: the records of the chunk, from its last position down
        for (int sb = (64 >> lcg) - 1; sb >= 0; sb--)
        {
          const int base = sb << lcg, first = (c << 6) + base, subU = first >> lcg;
          if (first >= N || subU > lastSub) continue;
          if (subU > 0 && subU < lastSub)
          {
            const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)rec, base);
            const unsigned flag = (r0 >> 16) & 1u;
            RR_UPD(s0, lane == 60 + (int)((r0 >> 17) & 1u), flag);
            if (!flag) continue;
          }
          for (int j = base + CG - 1; j >= base; j--)
          {
            const unsigned r = (unsigned)__builtin_amdgcn_readlane((int)rec, j);
            if (r & (1u << 6)) RR_UPD(s0, lane == (int)(r & 63u), (r >> 7) & 1u);
            if (r & (1u << 7))
            {
              const bool hit = absLane == (int)((r >> 8) & 31u) && (absCls < 2 || (r & (1u << 14)));
              RR_UPD(s1, hit, (r >> (13 + absCls)) & 1u);
            }
          }
        }
      }
    }

    // ---- the sums and the row
    acc += (unsigned long long)ep << RR_SCALE_BITS;
    acc = wave_sum(acc);
    if (lane == 0) { a.frac[item] = acc; a.numSig[item] = numSig; }
    if (a.ctxOut)
    {
      unsigned char* const out = a.ctxOut + (size_t)item * VVCGPU_RESI_RATE_CTX_BYTES;
      out[b0] = (unsigned char)s0; out[b1] = (unsigned char)s1; out[b2] = (unsigned char)s2;
    }
    wave_sync();                                                       // the levels and the group flags are free again
  }
}

// ---- the compare ---------------------------------------------------------------------------------------------------------------------------------
struct RcArgs
{
  const vvcgpu_inter_resi_item* items; const unsigned* absSum; const unsigned long long* distResi; const unsigned long long* zeroDist;
  const unsigned long long* frac; const unsigned long long* cbfBits; const int* prev; const double* weight; double scale;
  int* slot; int* cbf; unsigned* absOut; unsigned long long* dist; unsigned long long* bits; double* minCost; int n;
};
struct RcPick { int slot, cbf; unsigned absSum; unsigned long long dist, bits; double cost; };

// :4395-4568 for item i with the previous component's cbf p; false: the item is skipped
__device__ bool rc_choose_one(const RcArgs& a, int i, int p, RcPick& best)
{
  unsigned long long trBits;
  __builtin_memcpy(&trBits, a.items[i].tr, 8);
  const size_t o = (size_t)VVCGPU_INTER_RESI_SLOTS * i;
  int lastUsed = -1;
  bool tsEarly = false;
#pragma unroll
  for (int k = 0; k < VVCGPU_INTER_RESI_SLOTS; k++)
  {
    const int code = (int)(signed char)(trBits >> (8 * k));
    if (code == -1) continue;
    if (lastUsed >= 0 && (int)(signed char)(trBits >> (8 * lastUsed)) == VVCGPU_INTER_RESI_TS) tsEarly = true;
    lastUsed = k;
  }
  const unsigned long long zd = a.zeroDist[i];
  auto cand = [&](int k) {
    const int code = (int)(signed char)(trBits >> (8 * k));
    const unsigned s = a.absSum[o + k];
    return code != -1 && s != 0xFFFFFFFFu && (s == 0u || a.frac[o + k] != ~0ull);
  };
  if (!cand(0) || zd == ~0ull || tsEarly) return false;
  const double weight = a.weight[i];
  const unsigned long long nonDist = rd_weighted(weight, zd), nonBits = a.cbfBits[4 * (size_t)i + 2 * p];
  const double nonCost = rd_cost(a.scale, nonDist, nonBits);
  double minCost = RD_MAX_DOUBLE;
  best.slot = -1;
  for (int k = 0; k < VVCGPU_INTER_RESI_SLOTS; k++)
  {
    if (!cand(k)) continue;
    const bool ts = (int)(signed char)(trBits >> (8 * k)) == VVCGPU_INTER_RESI_TS;
    unsigned s = a.absSum[o + k];
    unsigned long long bits, dist; double cost; int cbf;
    if (s > 0u)
    {
      bits = a.cbfBits[4 * (size_t)i + 2 * p + 1] + a.frac[o + k]; dist = rd_weighted(weight, a.distResi[o + k]); cbf = 1;
      cost = rd_cost(a.scale, dist, bits);
    }
    else if (ts) { bits = 0; dist = 0; cbf = 0; cost = RD_MAX_DOUBLE; }
    else { bits = nonBits; dist = nonDist; cbf = 0; cost = nonCost; }
    if (cost < minCost || (ts && cost == minCost))
    {
      if (k == 0 && (nonCost < cost || s == 0u)) { s = 0u; bits = nonBits; dist = nonDist; cbf = 0; cost = nonCost; }   // the forced null
      best.slot = k; best.cbf = cbf; best.absSum = s; best.dist = dist; best.bits = bits; best.cost = cost;
      minCost = cost;
    }
  }
  return best.slot >= 0;
}

__global__ __launch_bounds__(256) void inter_resi_choose_kernel(const RcArgs a)
{
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= a.n) return;
  RcPick best;
  bool ok = true;
  int p = 0;
  const int pv = a.prev[i];
  if (pv != -1)
  {
    ok = pv >= 0 && pv < a.n;
    if (ok) ok = rc_choose_one(a, pv, 0, best);
    if (ok) p = best.cbf;
  }
  if (ok) ok = rc_choose_one(a, i, p, best);
  if (!ok) { best.slot = -1; best.cbf = 0; best.absSum = 0xFFFFFFFFu; best.dist = ~0ull; best.bits = ~0ull; best.cost = RD_MAX_DOUBLE; }
  a.slot[i] = best.slot; a.cbf[i] = best.cbf; a.absOut[i] = best.absSum; a.dist[i] = best.dist; a.bits[i] = best.bits; a.minCost[i] = best.cost;
}

}  // namespace

extern "C" int vvcgpu_resi_rate_batch(const vvc_coef* level_base, const struct vvcgpu_resi_rate_item* items, int n, const uint32_t* gate,
                                      const uint8_t* ctx, int n_ctx, const uint32_t* est_bits, const uint8_t* next_state,
                                      uint64_t* frac_bits, uint32_t* num_sig, uint8_t* ctx_out, void* stream)
{
  const char* name = "resi_rate_batch";
  VVC_CHECK_ARG(n >= 0, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(level_base && items && ctx && est_bits && next_state && frac_bits && num_sig, "%s: null pointer", name);
  VVC_CHECK_ARG(n_ctx >= 1, "%s: n_ctx %d", name, n_ctx);
  VVC_CHECK_ARG(((uintptr_t)items & 7) == 0, "%s: item array must be 8-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  VvcTrTables tb;
  if (const int rt = vvcgpu_tr_tables(&tb)) return rt;
  RrArgs a;
  a.level = level_base; a.items = items; a.gate = gate; a.ctx = ctx; a.est = est_bits; a.nxt = next_state;
  a.frac = reinterpret_cast<unsigned long long*>(frac_bits); a.numSig = num_sig; a.ctxOut = ctx_out;
  a.scan = tb.scan; a.inv = tb.dqInv; a.scanOff = tb.scanOff; a.n = n; a.nCtx = n_ctx;
  hipLaunchKernelGGL(resi_rate_kernel, dim3(vvc_grid_cap(n, RR_WAVES, 8)), dim3(RR_THREADS), 0, st, a);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

extern "C" int vvcgpu_inter_resi_choose_batch(const vvcgpu_inter_resi_item* items, int n, const uint32_t* abs_sum, const uint64_t* dist_resi,
                                              const uint64_t* zero_dist, const uint64_t* frac_bits, const uint64_t* cbf_bits, const int32_t* prev,
                                              const double* dist_weight, double dist_scale, int32_t* slot, int32_t* cbf, uint32_t* abs_sum_out,
                                              uint64_t* dist, uint64_t* bits, double* min_cost, void* stream)
{
  const char* name = "inter_resi_choose_batch";
  VVC_CHECK_ARG(n >= 0, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(items && abs_sum && dist_resi && zero_dist && frac_bits && cbf_bits && prev && dist_weight && slot && cbf && abs_sum_out && dist && bits
                && min_cost, "%s: null pointer", name);
  VVC_CHECK_ARG(((uintptr_t)items & 15) == 0, "%s: item array must be 16-byte aligned", name);
  RcArgs a;
  a.items = items; a.absSum = abs_sum; a.distResi = reinterpret_cast<const unsigned long long*>(dist_resi);
  a.zeroDist = reinterpret_cast<const unsigned long long*>(zero_dist); a.frac = reinterpret_cast<const unsigned long long*>(frac_bits);
  a.cbfBits = reinterpret_cast<const unsigned long long*>(cbf_bits); a.prev = prev; a.weight = dist_weight; a.scale = dist_scale;
  a.slot = slot; a.cbf = cbf; a.absOut = abs_sum_out; a.dist = reinterpret_cast<unsigned long long*>(dist);
  a.bits = reinterpret_cast<unsigned long long*>(bits); a.minCost = min_cost; a.n = n;
  hipLaunchKernelGGL(inter_resi_choose_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
