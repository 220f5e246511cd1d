// dist.hip -- block distortion for gfx950: batched SAD / Hadamard-SATD / SSE (D1-D3) and the AMVR integer refinement.
// (The SAD search surface is sadsearch.hip.)
//
// Reference behaviour reproduced (bit-exact):
//   RdCost::xGetSAD*  CommonLib/RdCost.cpp:450-1000   (SIMD twins x86/RdCostX86.h:215-432; no early exit)
//   RdCost::xGetHADs  :2855-2974, xCalcHADs* :2205-2853 (rect tiles: (int)(sad / sqrt(128.0) * 2) in IEEE f64)
//   RdCost::xGetSSE*  :1820-2200
//   InterSearch::xPatternSearchIntRefine                              EncoderLib/InterSearch.cpp:2408-2501
//
// Design
//   * batch kernel: one 64-lane wave per descriptor.  SATD maps one tile ROW to one lane: the horizontal
//     Walsh-Hadamard runs in registers, the vertical one across lanes with xor-shuffles (no LDS), tiles of a
//     block are spread over the lane groups of the wave, partial sums are combined with wave shuffles.
#include "common.h"
#include "dist_dev.h"
#include "raster_dev.h"

namespace {

// four samples of a row; the widest load the address allows (a reference block sits at an arbitrary motion vector: any alignment occurs)
__device__ __forceinline__ void dist_load4(const Pel* p, int (&v)[4])
{
  const uintptr_t a = (uintptr_t)p;
  if ((a & 7) == 0) { const pel4 q = *reinterpret_cast<const pel4*>(p); v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3]; }
  else if ((a & 3) == 0)
  {
    const pel2 q0 = *reinterpret_cast<const pel2*>(p), q1 = *reinterpret_cast<const pel2*>(p + 2);
    v[0] = q0[0]; v[1] = q0[1]; v[2] = q1[0]; v[3] = q1[1];
  }
  else { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3]; }
}

// one descriptor by a group of G lanes (lane = index inside the group); the result is valid in every lane of the group
template <int G>
__device__ __forceinline__ unsigned long long dist_one(int kind, const vvcgpu_dist_desc& d, const Pel* __restrict__ orgBase, const Pel* __restrict__ curBase,
                                                       int lane, bool act, int hSel = 0)      // hSel: height of the whole block when d is a band of it (Hadamard tile choice)
{
  const Pel* org = orgBase + d.org_off;
  const Pel* cur = curBase + d.cur_off;
  const int w = act ? d.w : 0, h = act ? d.h : 0, os = d.org_stride, cs = d.cur_stride;
  unsigned long long res;
  int offset = 0;
  const int ssSad = (kind == 0 || kind == 3) ? d.sub_shift : 0;
  if (kind >= 3)                                          // D4: mean difference over the (sub-sampled, MR-SAD only) block, truncating division
  {
    const int rows = h >> ssSad;
    long long acc = 0;
    for (int idx = lane; idx < rows * w; idx += G)
    {
      const int r = idx / w, x = idx - r * w;
      acc += (int)org[(size_t)(r << ssSad) * os + x] - (int)cur[(size_t)(r << ssSad) * cs + x];
    }
    acc = (long long)group_sum<G>((unsigned long long)acc);
    offset = act ? (int)(Pel)(kind == 3 ? (int)acc / (w * rows) : (int)(acc / (long long)(w * h))) : 0;
  }
  if (kind == 1 || kind == 4)
  {
    res = satd_block<G>(org, os, cur, cs, w, h, lane, offset, hSel);
  }
  else
  {
    const int ss = ssSad;
    const int rows = h >> ss;
    unsigned long long acc = 0;
    if ((w & 3) == 0)
    {
      const int upr = w >> 2;                             // units of four samples per row
      for (int u = lane; u < rows * upr; u += G)
      {
        const int r = u / upr, x = (u - r * upr) << 2;
        int o[4], c[4];
        dist_load4(org + (size_t)(r << ss) * os + x, o);
        dist_load4(cur + (size_t)(r << ss) * cs + x, c);
#pragma unroll
        for (int k = 0; k < 4; k++) { const int df = o[k] - c[k] - offset; acc += kind == 2 ? (unsigned)(df * df) : (unsigned)abs(df); }
      }
    }
    else
    {
      for (int idx = lane; idx < rows * w; idx += G)
      {
        const int r = idx / w, x = idx - r * w;
        const int df = (int)org[(size_t)(r << ss) * os + x] - (int)cur[(size_t)(r << ss) * cs + x] - offset;
        acc += kind == 2 ? (unsigned)(df * df) : (unsigned)abs(df);
      }
    }
    res = group_sum<G>(acc) << ss;
  }
  return res;
}

// A workgroup takes up to 64 consecutive descriptors and BINS them first (one ballot of its first wave).  The reference encoder's calls are mostly
// narrow (tests/golden/trace_*.npz: 4- and 8-wide blocks are 80 % of the distortion calls): blocks of at most 128 samples run four side by side in a
// wave, 16 lanes each; larger ones take a whole wave each.  (Until round 4 a wave took four CONSECUTIVE descriptors and ran them side by side only
// when all four were small: on the real call mix most waves lost that form to one larger neighbour.)  HEAVY blocks (more than 2048 samples,
// SAD / Hadamard / SSE) are not computed here: one wave needs ~60 us for a 128 x 128 block, which was the run time of the whole launch on a real call
// mix -- they are listed, their result is zeroed, and dist_heavy_kernel splits each into bands of >= 16 rows over as many waves, summing with 64-bit atomics.
constexpr int DIST_HEAVY = 2048, DIST_WG_DESCS = 64;
__device__ __forceinline__ int dist_band_rows(int w) { return max(16, ((DIST_HEAVY / w) + 15) & ~15); }
__device__ __forceinline__ bool dist_is_heavy(int kind, int w, int h) { return kind <= 2 && w * h > DIST_HEAVY && (h & 15) == 0 && h <= 8 * dist_band_rows(w); }

__global__ __launch_bounds__(256) void dist_batch_kernel(int kind, const Pel* __restrict__ orgBase,
                                                         const Pel* __restrict__ curBase,
                                                         const vvcgpu_dist_desc* __restrict__ descs, int n, int perWg,
                                                         unsigned long long* __restrict__ out, int* __restrict__ heavyCount, int* __restrict__ heavyList,
                                                         int* __restrict__ nextCounters)
{
  if (blockIdx.x == 0 && threadIdx.x < VVC_CTR_INTS) nextCounters[threadIdx.x] = 0;       // the counter set of the next call on this stream (vvcgpu_counters)
  __shared__ unsigned char sList[DIST_WG_DESCS], mList[DIST_WG_DESCS];
  __shared__ int cntS, cntM;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int base = blockIdx.x * perWg;
  if (wave == 0)
  {
    const int di = base + lane;
    int w = 0, h = 0;
    if (lane < perWg && di < n) { w = descs[di].w; h = descs[di].h; }
    const int sz = w * h;
    // (a 16 x 16 Hadamard on 16 lanes takes two tile passes: slower than the whole wave)
    const bool on = lane < perWg && di < n, small = on && sz <= 128, heavy = on && dist_is_heavy(kind, w, h), med = on && !small && !heavy;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long ms = __builtin_amdgcn_ballot_w64(small), mm = __builtin_amdgcn_ballot_w64(med), mh = __builtin_amdgcn_ballot_w64(heavy);
    if (small) sList[__popcll(ms & below)] = (unsigned char)lane;
    if (med) mList[__popcll(mm & below)] = (unsigned char)lane;
    if (lane == 0) { cntS = (int)__popcll(ms); cntM = (int)__popcll(mm); }
    if (mh != 0ull)                                     // ONE atomic per workgroup (same-address atomics retire at ~12 ns each)
    {
      int b = 0;
      if (lane == 0) b = atomicAdd(heavyCount, (int)__popcll(mh));
      b = __builtin_amdgcn_readfirstlane(b);
      if (heavy) { out[di] = 0ull; heavyList[b + (int)__popcll(mh & below)] = di; }
    }
  }
  __syncthreads();
  const int nS = cntS, nM = cntM;
  for (int g0 = wave * 4; g0 < nS; g0 += 16)
  {
    const int k = g0 + (lane >> 4);
    const bool act = k < nS;
    const int di = base + sList[act ? k : g0];
    const vvcgpu_dist_desc mine = descs[di];
    const unsigned long long res = dist_one<16>(kind, mine, orgBase, curBase, lane & 15, act);
    if (act && (lane & 15) == 0) out[di] = res;
  }
  for (int k = wave; k < nM; k += 4)
  {
    const int di = base + __builtin_amdgcn_readfirstlane((int)mList[k]);
    const vvcgpu_dist_desc d = descs[di];
    const unsigned long long res = dist_one<64>(kind, d, orgBase, curBase, lane, true);
    if (lane == 0) out[di] = res;
  }
}

// one wave per (heavy block, band of rows); up to 8 bands per block (128 rows / 16)
__global__ __launch_bounds__(256) void dist_heavy_kernel(int kind, const Pel* __restrict__ orgBase, const Pel* __restrict__ curBase,
                                                         const vvcgpu_dist_desc* __restrict__ descs, unsigned long long* __restrict__ out,
                                                         const int* __restrict__ heavyCount, const int* __restrict__ heavyList)
{
  const int lane = threadIdx.x & 63;
  const int cnt = heavyCount[0], waves = gridDim.x * 4;
  for (int p = blockIdx.x * 4 + (threadIdx.x >> 6); p < cnt * 8; p += waves)
  {
    const int band = p / cnt, di = heavyList[p - band * cnt];           // band-major pairs (see if_heavy_kernel, interp.hip)
    vvcgpu_dist_desc d = descs[di];
    const int hFull = d.h, br = dist_band_rows(d.w), r0 = band * br;
    if (r0 >= hFull) continue;
    d.org_off += (int64_t)r0 * d.org_stride;
    d.cur_off += (int64_t)r0 * d.cur_stride;
    d.h = (int16_t)min(br, hFull - r0);
    const unsigned long long res = dist_one<64>(kind, d, orgBase, curBase, lane, true, hFull);
    if (lane == 0) atomicAdd(&out[di], res);
  }
}

// ---- AMVR integer refinement: InterSearch::xPatternSearchIntRefine (InterSearch.cpp:2408-2501) -------------------------------
// One wavefront per PU: the <= 18 (position, predictor) pairs are visited in the reference's order; each distortion is computed
// by the whole wavefront with the SATD / SAD code of vvcgpu_dist_batch.
__device__ __forceinline__ unsigned long long block_dist(bool had, const Pel* org, int os, const Pel* cur, int cs, int w, int h, int lane)
{
  if (had) return satd_block<64>(org, os, cur, cs, w, h, lane);
  unsigned long long acc = 0;
  for (int idx = lane; idx < h * w; idx += 64)
  {
    const int r = idx / w, x = idx - r * w;
    acc += (unsigned)abs((int)org[(size_t)r * os + x] - (int)cur[(size_t)r * cs + x]);
  }
  return wave_sum(acc);
}

__global__ __launch_bounds__(256) void imv_refine_kernel(const Pel* __restrict__ org, int os, const Pel* __restrict__ ref, int rs,
                                                         const vvcgpu_imv_pu* __restrict__ pus, int n, vvcgpu_tz_cfg cfg, int useHad, double weight,
                                                         vvcgpu_imv_result* __restrict__ results)
{
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= n) return;
  const vvcgpu_imv_pu p = pus[b];
  const int sh = cfg.imv_shift, mvOffset = 1 << sh;
  const int horMax = (cfg.pic_w + 8 - p.pos_x - 1) << 2, horMin = (-cfg.max_cu_w - 8 - p.pos_x + 1) << 2;
  const int verMax = (cfg.pic_h + 8 - p.pos_y - 1) << 2, verMin = (-cfg.max_cu_h - 8 - p.pos_y + 1) << 2;
  const int mvx = p.mv_x << 2, mvy = p.mv_y << 2;
  int baseX[2], baseY[2];
#pragma unroll
  for (int c = 0; c < 2; c++)
  {
    const int off = 1 << (sh - 1);
    baseX[c] = (((mvx - p.cand_x[c]) + off) >> sh) << sh;
    baseY[c] = (((mvy - p.cand_y[c]) + off) >> sh) << sh;
  }
  const Pel* o = org + (ptrdiff_t)p.org_y * os + p.org_x;
  unsigned long long bestDist = ~0ull, satd = 0;
  int bestX = mvx, bestY = mvy, bestIdx = p.mvp_idx, bestBits = 0;
  for (int pos = 0; pos < 9; pos++)
  {
    // testPos order: centre, then the 3 x 3 neighbourhood row by row in (x = -1, 0, 1) major order (:2429)
    const int q = pos == 0 ? 4 : (pos <= 4 ? pos - 1 : pos);       // index into the 3 x 3 grid, x-major
    const int dx = q / 3 - 1, dy = q % 3 - 1;
    int tx[2] = { 0, 0 }, ty[2] = { 0, 0 };
    for (int c = 0; c < p.num_cand; c++)
    {
      const int candX = c == 0 ? p.cand_x[0] : p.cand_x[1], candY = c == 0 ? p.cand_y[0] : p.cand_y[1];
      tx[c] = dx * mvOffset + (c == 0 ? baseX[0] : baseX[1]) + candX;
      ty[c] = dy * mvOffset + (c == 0 ? baseY[0] : baseY[1]) + candY;
      unsigned long long dist;
      if (c == 0 || tx[0] != tx[1] || ty[0] != ty[1])
      {
        const int cx = min(horMax, max(horMin, tx[c])), cy = min(verMax, max(verMin, ty[c]));
        const int px = min(max(p.ref_x + (cx >> 2), cfg.ref_x0), cfg.ref_x1 - p.w), py = min(max(p.ref_y + (cy >> 2), cfg.ref_y0), cfg.ref_y1 - p.h);
        const unsigned long long d = block_dist(useHad != 0, o, os, ref + (ptrdiff_t)py * rs + px, rs, p.w, p.h, lane);
        dist = satd = (unsigned long long)((double)d * weight);
      }
      else dist = satd;
      const unsigned mvBits = expgolomb_bits((tx[c] - candX) >> sh) + expgolomb_bits((ty[c] - candY) >> sh);
      const int iMvBits = (int)((c == 0 ? p.idx_cost[0] : p.idx_cost[1]) + mvBits);
      dist += (unsigned long long)(cfg.lambda * (double)mvBits);
      if (dist < bestDist) { bestDist = dist; bestX = tx[c]; bestY = ty[c]; bestIdx = c; bestBits = iMvBits; }
    }
  }
  if (lane == 0)
  {
    unsigned bits = p.bits - (p.mvp_idx == 0 ? p.idx_cost[0] : p.idx_cost[1]);
    bits += (unsigned)bestBits;
    vvcgpu_imv_result r;
    r.cost = bestDist - (unsigned long long)(cfg.lambda * (double)(unsigned)bestBits) + (unsigned long long)(cfg.lambda * (double)bits);
    const int candX = bestIdx == 0 ? p.cand_x[0] : p.cand_x[1], candY = bestIdx == 0 ? p.cand_y[0] : p.cand_y[1];
    bits += expgolomb_bits((bestX - candX) >> sh) + expgolomb_bits((bestY - candY) >> sh);
    r.mv_x = bestX; r.mv_y = bestY; r.mvp_idx = bestIdx; r.bits = bits;
    results[b] = r;
  }
}

}  // namespace

extern "C" {

int vvcgpu_dist_batch(int kind, const vvc_pel* org_base, const vvc_pel* cur_base, const vvcgpu_dist_desc* descs,
                      int n, int bit_depth, uint64_t* out, void* stream)
{
  VVC_CHECK_ARG(kind >= 0 && kind <= 4, "dist_batch: kind %d", kind);
  VVC_CHECK_ARG(n >= 0, "dist_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org_base && cur_base && descs && out, "dist_batch: null pointer");
  if (bit_depth > 10) { vvcgpu_set_error("dist_batch: bit depth %d > 10 is outside the precondition", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  VvcScratch sc(st);
  int* heavyList = sc.take<int>(n);
  if (!heavyList) return VVCGPU_E_DEVICE;
  int cur = 0;
  int* counters = vvcgpu_counters(st, &cur);                                  // zeroed counter for this call; the kernel clears the other set
  if (!counters) return VVCGPU_E_DEVICE;
  int perWg = DIST_WG_DESCS;                              // fewer descriptors per workgroup when 64 would leave compute units without one
  while (perWg > 16 && cdiv(n, perWg) < 4096) perWg >>= 1;
  hipLaunchKernelGGL(dist_batch_kernel, dim3(cdiv(n, perWg)), dim3(256), 0, st, kind, org_base, cur_base,
                     descs, n, perWg, reinterpret_cast<unsigned long long*>(out), counters + VVC_CTR_INTS * cur, heavyList, counters + VVC_CTR_INTS * (cur ^ 1));
  if (kind <= 2)                                                              // blocks of more than 2048 samples: bands over many waves (none: the launch leaves at once)
    hipLaunchKernelGGL(dist_heavy_kernel, dim3(n * 2 < 1024 ? (n * 2 > 0 ? n * 2 : 1) : 1024), dim3(256), 0, st, kind, org_base, cur_base, descs,
                       reinterpret_cast<unsigned long long*>(out), counters + VVC_CTR_INTS * cur, heavyList);
  VVC_LAUNCH_CHECK_COUNTERS(st);
  return VVCGPU_OK;
}

int vvcgpu_imv_refine_batch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_imv_pu* pus, int n,
                            const vvcgpu_tz_cfg* cfg_host, int use_hadamard, double weight, vvcgpu_imv_result* results, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "imv_refine_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org && ref && pus && cfg_host && results, "imv_refine_batch: null pointer");
  const vvcgpu_tz_cfg c = *cfg_host;
  VVC_CHECK_ARG(c.imv_shift >= 1 && c.imv_shift <= 6, "imv_refine_batch: imv_shift %d (2 = integer, 4 = four-sample resolution)", c.imv_shift);
  VVC_CHECK_ARG(c.lambda >= 0.0 && c.lambda < 1048576.0 && weight >= 0.0 && weight <= 16.0, "imv_refine_batch: lambda / weight out of range");
  VVC_CHECK_ARG(c.pic_w > 0 && c.pic_h > 0 && c.max_cu_w > 0 && c.max_cu_h > 0, "imv_refine_batch: picture geometry");
  VVC_CHECK_ARG(c.ref_x1 - c.ref_x0 >= 128 && c.ref_y1 - c.ref_y0 >= 128 && c.ref_x0 >= 0 && c.ref_y0 >= 0 && c.ref_x1 <= ref_stride,
                "imv_refine_batch: readable rectangle");
  hipLaunchKernelGGL(imv_refine_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, org, org_stride, ref, ref_stride, pus, n, c, use_hadamard,
                     weight, results);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
