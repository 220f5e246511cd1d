// mergecand.hip -- vvcgpu_merge_cand_batch: the first pass of the merge analysis of a CU for a list of independent PUs, in two launches.
//
// Reference behaviour reproduced (bit-exact, the doubles included):
//   EncCu::xCheckRDCostMerge2Nx2N, first pass          EncoderLib/EncCu.cpp:1537-1612
//   InterPrediction::motionCompensation / xSubPuMC      CommonLib/InterPrediction.cpp:265-345, 480-547 (through the bodies of mc_dev.h)
//   RdCost::xGetHADs / xGetSAD / xGetSSE               CommonLib/RdCost.cpp (through dist_dev.h)
//   updateCandList                                      CommonLib/UnitTools.h:190-223
//
// Design (docs/KERNELS.md, "The merge candidate pass"):
//   launch 1  one owner per CANDIDATE under the model of owner_dev.h: a wavefront owns a candidate whose luma block has at most 1024 samples, a
//             workgroup a larger one.  The owner first checks every descriptor of the candidate (a candidate outside the contract writes nothing but
//             its sentinels), then serves the components one after the other: the descriptors of the component are cut into bands of tile rows, the
//             bands are dealt to the owner's wavefronts, and every band is predicted by mc_generic_pu INTO THE OWNER'S LDS TILE of the block (the
//             packed 16x16 / 8x8 tile path where a band is a row of tiles, the sample-wise path elsewhere; the sub-blocks of an ATMVP candidate, at
//             most 4x4 samples, four or sixteen side by side in a wavefront through mc_samplewise).  The complete tile then leaves for
//             pred_base in rows, its SSE against the original is taken on the way, and the luma tile's Hadamard (bands of sixteen rows over the
//             wavefronts) or SAD comes from LDS: no prediction is read back from memory.
//   launch 2  one lane per PU: the costs, updateCandList and the ratio cut; it also writes the rows of the PUs outside the contract.
#include "common.h"
#include "dist_dev.h"
#include "mc_dev.h"
#include "owner_dev.h"
#include "pu_entry_host.h"

static_assert(offsetof(vvcgpu_mc_desc, reserved) == 46 && sizeof(vvcgpu_mc_desc) == 48 && sizeof(vvcgpu_dist_desc) == 32, "descriptor layouts");

namespace {

constexpr int MG_WAVE_MAX = 1024;                                         // samples of the largest luma block a wavefront owns
constexpr int MG_MC_BYTES = (WR * WP + WR * ST) * 2 + MC_LDS_DW * 4;      // a wavefront's LDS of mc_generic_pu: window, intermediate, packed tile path
// blocks of at most 4x4 samples run four side by side in a wavefront (sixteen lanes each), blocks of at most 2x2 sixteen side by side (four lanes each):
// a group's window and intermediate of mc_samplewise<G, T>, all groups inside the wavefront's MC scratch
constexpr int mg_small_shorts(int T) { return (T + 7) * (T + 8) + (T + 7) * T; }
static_assert(4 * mg_small_shorts(4) * 2 <= MG_MC_BYTES && 16 * mg_small_shorts(2) * 2 <= MG_MC_BYTES, "the groups share the wavefront's MC scratch");
constexpr int MG_SLOT_BYTES = 32;                                         // owner_sum_waves
constexpr int MG_MAX_CAND = 7, MG_FAST_CAND = 4;                          // MRG_MAX_NUM_CANDS, NUM_MRG_SATD_CAND
static_assert(MG_MC_BYTES % 16 == 0, "the tile behind the wavefronts' MC scratch is 16-byte aligned");

// LDS of an owner of `lanes` lanes for a luma block of w x h: every wavefront's MC scratch, the sum slots, the tile (a chroma block is no larger)
inline int mg_lds_bytes(int w, int h, int lanes) { return (lanes / 64) * MG_MC_BYTES + MG_SLOT_BYTES + w * h * 2; }

typedef const __attribute__((address_space(3))) short* MgLdsPel;

struct MgArgs
{
  const Pel* ref0; const Pel* ref1; const Pel* org; Pel* pred;
  const vvcgpu_mc_desc* mc; const int* candMcFirst; const vvcgpu_dist_desc* candDist;
  unsigned long long* distOut; unsigned long long* sseOut;
  int nMc, nCand, nComp, useHad, bd, cmin, cmax, waveBytes;
};

// where the destination rectangle of descriptor d lies in the `cur` block of its component: false if it leaves the block
__device__ __forceinline__ bool mg_place(const vvcgpu_mc_desc& d, const vvcgpu_dist_desc& dC, int& x, int& y)
{
  const long long rel = d.dst_off - dC.cur_off;
  if (d.dst_stride != dC.cur_stride || rel < 0 || rel >= (long long)dC.cur_stride * dC.h) return false;
  // (a 64-bit division is a long routine here: the offset of a block inside a picture-sized buffer fits 32 bits)
  y = rel < (1ll << 31) ? (int)((unsigned)rel / (unsigned)dC.cur_stride) : (int)(rel / dC.cur_stride);
  x = (int)(rel - (long long)y * dC.cur_stride);
  return x + d.w <= dC.w && y + d.h <= dC.h;
}

// true in every lane of the owner if `v` holds in any
template <int NT> __device__ __forceinline__ bool mg_any(bool v, unsigned long long* slots, int tid)
{
  return owner_sum_waves<NT>(__builtin_amdgcn_ballot_w64(v) != 0ull ? 1ull : 0ull, slots, tid) != 0ull;
}

// The descriptors `todo` (bits: index from base) of component dC, blocks of at most T x T samples: 64 / G side by side, G lanes each.  Wavefront wv of
// the owner's NW takes every NW-th step (turn: steps so far, the same count in every wavefront).  A wavefront per block spends its time waiting for one
// block's descriptor and window after the other.
template <int G, int T, int NW>
__device__ __forceinline__ void mg_small_blocks(const MgArgs& a, unsigned long long todo, int base, const vvcgpu_dist_desc& dC, short* tile, short* scratch,
                                                int lane, int wv, int& turn)
{
  constexpr int GROUPS = 64 / G;
  while (todo)
  {
    const int firstSel = (int)__builtin_ctzll(todo);
    int sel = -1;
#pragma unroll
    for (int k = 0; k < GROUPS; k++)
      if (todo) { const int b = (int)__builtin_ctzll(todo); todo &= todo - 1ull; if (k == lane / G) sel = b; }
    if ((turn++ % NW) != wv) continue;
    vvcgpu_mc_desc d = a.mc[base + (sel >= 0 ? sel : firstSel)];
    int x, y;
    mg_place(d, dC, x, y);
    d.dst_off = (int64_t)y * dC.w + x; d.dst_stride = dC.w;             // into the tile, pitch = the block's width
    if (sel < 0) d.w = d.h = 0;                                           // an idle group walks the same code over no sample
    short* gw = scratch + (lane / G) * mg_small_shorts(T);
    mc_samplewise<G, T, false, false>(d, a.ref0, a.ref1, tile, a.bd, a.cmin, a.cmax, lane % G, gw, gw + (T + 7) * (T + 8), nullptr, nullptr);
  }
}

template <int NT>
__device__ __forceinline__ void mg_candidate(const MgArgs& a, int c, bool sidesOk, unsigned char* smem, int tid)
{
  constexpr int NW = NT / 64;
  const int lane = tid & 63, wv = NT == 256 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  short* win = reinterpret_cast<short*>(smem + wv * MG_MC_BYTES);
  short* tmp = win + WR * WP;
  unsigned* tileL = reinterpret_cast<unsigned*>(tmp + WR * ST);
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(smem + NW * MG_MC_BYTES);
  short* tile = reinterpret_cast<short*>(smem + NW * MG_MC_BYTES + MG_SLOT_BYTES);
  const vvcgpu_dist_desc dY = a.candDist[(size_t)a.nComp * c];
  const int m0 = a.candMcFirst[c], m1 = a.candMcFirst[c + 1];

  // ---- the contract, before anything is written
  bool bad = !sidesOk || m0 < 0 || m1 > a.nMc || m1 <= m0 || dY.cur_stride < dY.w;
  for (int comp = 1; comp < a.nComp; comp++)                               // (a chroma block shares the owner's tile: no larger than the luma block)
  {
    const vvcgpu_dist_desc dC = a.candDist[(size_t)a.nComp * c + comp];
    bad = bad || dC.w < 1 || dC.h < 1 || dC.w > dY.w || dC.h > dY.h || dC.cur_stride < dC.w;
  }
  if (!bad)
  {
    bool mine = false;
    for (int i = m0 + tid; i < m1; i += NT)
    {
      const vvcgpu_mc_desc d = a.mc[i];
      const int comp = d.reserved, fmax = d.is_luma ? 16 : 32;
      bool ok = comp >= 0 && comp < a.nComp && d.w >= 1 && d.w <= 128 && d.h >= 1 && d.h <= 128 && d.bi >= 0 && d.bi <= 1;
      ok = ok && d.frac_x0 >= 0 && d.frac_x0 < fmax && d.frac_y0 >= 0 && d.frac_y0 < fmax;
      ok = ok && (d.bi == 0 || (d.frac_x1 >= 0 && d.frac_x1 < fmax && d.frac_y1 >= 0 && d.frac_y1 < fmax));
      if (ok) { int x, y; ok = mg_place(d, a.candDist[(size_t)a.nComp * c + comp], x, y); }
      mine = mine || !ok;
    }
    bad = mg_any<NT>(mine, slots, tid);
  }
  if (bad)
  {
    if (tid == 0) a.distOut[c] = ~0ull;
    if (a.sseOut && tid < a.nComp) a.sseOut[(size_t)a.nComp * c + tid] = ~0ull;
    return;
  }

  // ---- the components, one after the other through the tile
  for (int comp = 0; comp < a.nComp; comp++)
  {
    if (comp > 0 && !a.pred && !a.sseOut) break;                          // a cost-only call without SSE: chroma has no output
    const vvcgpu_dist_desc dC = a.candDist[(size_t)a.nComp * c + comp];
    const int w = dC.w, h = dC.h;
    owner_sync<NT>();                                                     // the previous component has left the tile
    int turn = 0, turnS = 0, turnT = 0;                                   // bands / steps of small blocks so far (the same counts in every wavefront of the owner)
    for (int base = m0; base < m1; base += 64)
    {
      const int i = base + lane;
      bool mine = false, small = false, tiny = false;
      if (i < m1)
      {
        const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(a.mc + i) + 32);     // dst_stride | w, h | phases | is_luma, bi, reserved
        const int qw = (int)(short)(q.y & 0xFFFFu), qh = (int)(short)(q.y >> 16);
        mine = (int)(short)(q.w >> 16) == comp;
        tiny = mine && qw <= 2 && qh <= 2;
        small = mine && !tiny && qw <= 4 && qh <= 4;
      }
      unsigned long long todo = __builtin_amdgcn_ballot_w64(mine && !small && !tiny);
      // the sub-blocks of an ATMVP candidate: 4x4 luma and chroma four at a time, 2x2 chroma sixteen at a time
      mg_small_blocks<16, 4, NW>(a, __builtin_amdgcn_ballot_w64(small), base, dC, tile, win, lane, wv, turnS);
      mg_small_blocks<4, 2, NW>(a, __builtin_amdgcn_ballot_w64(tiny), base, dC, tile, win, lane, wv, turnT);
      while (todo)
      {
        const int li = base + (int)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        vvcgpu_mc_desc d = a.mc[li];
        int x, y;
        mg_place(d, dC, x, y);
        // bands of tile rows (16 luma, 8 chroma where the block is a grid of 8x8 tiles): the same samples whichever way a block is cut
        const int bandH = (!d.is_luma && (d.w & 7) == 0 && (d.h & 7) == 0) ? 8 : 16, nBands = (d.h + bandH - 1) / bandH;
        const int first = (wv - turn % NW + NW) % NW;                   // this wavefront's first band of the descriptor
        turn += nBands;
        for (int b = first; b < nBands; b += NW)
        {
          vvcgpu_mc_desc q = d;
          const int y0 = b * bandH;
          q.h = (short)min(bandH, d.h - y0);
          q.ref0_off += (int64_t)y0 * d.ref0_stride; q.ref1_off += (int64_t)y0 * d.ref1_stride;
          q.dst_off = (int64_t)(y + y0) * w + x; q.dst_stride = w;         // into the tile, pitch = the block's width
          mc_generic_pu<false, 3>(q, a.ref0, a.ref1, tile, a.bd, a.cmin, a.cmax, lane, win, tmp, tileL, nullptr);
        }
      }
    }
    owner_sync<NT>();                                                     // the tile is complete

    // the tile leaves in rows; SSE (and the luma SAD) against the original on the way
    const Pel* org = a.org + dC.org_off;
    Pel* out = a.pred ? a.pred + dC.cur_off : nullptr;
    const bool wantSad = comp == 0 && !a.useHad;
    unsigned long long sse = 0, sad = 0;
    if (out || a.sseOut || wantSad)
      for (int i = tid; i < w * h; i += NT)
      {
        const int r = i / w, k = i - r * w;
        const int v = tile[i];
        if (out) out[(size_t)r * dC.cur_stride + k] = (short)v;
        const int df = (int)org[(ptrdiff_t)r * dC.org_stride + k] - v;
        sse += (unsigned)(df * df);
        sad += (unsigned)abs(df);
      }
    if (a.sseOut)
    {
      sse = owner_sum<NT>(sse, slots, tid);
      if (tid == 0) a.sseOut[(size_t)a.nComp * c + comp] = sse;
    }
    if (comp == 0)
    {
      unsigned long long dist;
      if (wantSad) dist = owner_sum<NT>(sad, slots, tid);
      else
      {
        unsigned long long sum = 0;
        if (NT == 64) sum = satd_block<64, MgLdsPel>(org, dC.org_stride, (MgLdsPel)tile, w, w, h, lane);
        else                                                              // (h >= 16 here: w h > 1024 with w <= 128; every Hadamard tile is at most 16 rows)
          for (int b = wv; b * 16 < h; b += NW)
            sum += satd_block<64, MgLdsPel>(org + (ptrdiff_t)b * 16 * dC.org_stride, dC.org_stride, (MgLdsPel)tile + b * 16 * w, w, w, 16, lane, 0, h);
        dist = owner_sum_waves<NT>(sum, slots, tid);
      }
      if (tid == 0) a.distOut[c] = dist;
    }
  }
}

__global__ __launch_bounds__(256, 2) void merge_pred_kernel(const MgArgs a)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const OwnerSlot o = owner_slot(a.nCand, wave);
  if (o.leave) return;
  const vvcgpu_dist_desc dY = a.candDist[(size_t)a.nComp * o.unit];
  const bool sidesOk = pu_side_pow2_ok(dY.w) && pu_side_pow2_ok(dY.h);
  // a luma block outside the served sides has no tile: the wavefront owner writes its sentinels
  if ((!sidesOk || dY.w * dY.h <= MG_WAVE_MAX) != o.waveOwner) return;
  if (o.waveOwner) mg_candidate<64>(a, o.unit, sidesOk, smem + (size_t)wave * a.waveBytes, tid & 63);
  else mg_candidate<256>(a, o.unit, sidesOk, smem, tid);
}

// element i of a list of MG_FAST_CAND, by comparison (no dynamically indexed private array, which would live in scratch memory)
template <class T> __device__ __forceinline__ T mg_pick(const T (&l)[MG_FAST_CAND], int i)
{
  T v = l[0];
#pragma unroll
  for (int j = 1; j < MG_FAST_CAND; j++) v = i == j ? l[j] : v;
  return v;
}

// per PU, one lane: :1594-1612
__global__ __launch_bounds__(256) void merge_list_kernel(const int* __restrict__ puCandFirst, int nPu, int nCand, int maxNumMergeCand, double sqrtLambda,
                                                         const unsigned long long* __restrict__ distOut, double* __restrict__ costOut, int* __restrict__ rdList)
{
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nPu) return;
  const int c0 = puCandFirst[p], c1 = puCandFirst[p + 1], cnt = c1 - c0;
  int row[8] = { -1, -1, -1, -1, -1, -1, -1, -1 };
  const bool rangeOk = c0 >= 0 && c1 <= nCand && cnt >= 1 && cnt <= MG_MAX_CAND;
  bool ok = rangeOk;
  unsigned long long dist[MG_MAX_CAND];
#pragma unroll
  for (int k = 0; k < MG_MAX_CAND; k++)
  {
    dist[k] = (rangeOk && k < cnt) ? distOut[c0 + k] : 0ull;
    ok = ok && dist[k] != ~0ull;
  }
  if (ok)
  {
    double costL[MG_FAST_CAND] = { 0.0, 0.0, 0.0, 0.0 };
    int modeL[MG_FAST_CAND] = { -1, -1, -1, -1 }, size = 0;
#pragma unroll
    for (int k = 0; k < MG_MAX_CAND; k++)
      if (k < cnt)
      {
        const unsigned bits = (unsigned)(k + 1 - (k == maxNumMergeCand - 1 ? 1 : 0));
        const double prod = (double)bits * sqrtLambda;                    // a product, then a sum (the library is built with -ffp-contract=off)
        const double cost = (double)dist[k] + prod;
        costOut[c0 + k] = cost;
        // updateCandList (uiFastCandNum = 4); the lists have the same size throughout, so currSize = size
        int shift = 0;
        while (shift < MG_FAST_CAND && shift < size && cost < mg_pick(costL, size - 1 - shift)) shift++;
        if (size < MG_FAST_CAND || shift != 0)                            // a full list takes the mode only ahead of its last entry
        {
          const int pos = size - shift;
#pragma unroll
          for (int i = MG_FAST_CAND - 1; i >= 0; i--)
          {
            if (i > pos) { if (i > 0) { costL[i] = costL[i - 1]; modeL[i] = modeL[i - 1]; } }
            else if (i == pos) { costL[i] = cost; modeL[i] = k; }
          }
          if (size < MG_FAST_CAND) size++;
        }
      }
    int num = size;                                                       // min(NUM_MRG_SATD_CAND, count): the cut stops at the list's size
#pragma unroll
    for (int i = MG_FAST_CAND - 1; i >= 1; i--)
      if (i < size && costL[i] > 1.25 * costL[0]) num = i;              // the first i that exceeds MRG_FAST_RATIO
    row[0] = num;
#pragma unroll
    for (int i = 0; i < MG_FAST_CAND; i++) row[1 + i] = i < size ? modeL[i] : -1;
  }
  else if (rangeOk)
  {
    for (int k = 0; k < cnt; k++) costOut[c0 + k] = __builtin_inf();
  }
#pragma unroll
  for (int i = 0; i < 8; i++) rdList[8 * (size_t)p + i] = row[i];
}

}  // namespace

extern "C" int vvcgpu_merge_cand_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, const vvc_pel* org_base, vvc_pel* pred_base,
                                       const vvcgpu_mc_desc* mc_descs, int n_mc, const int32_t* cand_mc_first, const vvcgpu_dist_desc* cand_dist, int n_cand,
                                       int n_comp, const int32_t* pu_cand_first, int n_pu, int max_num_merge_cand, int use_hadamard, double sqrt_lambda,
                                       int bit_depth, int clp_min, int clp_max, uint64_t* dist_out, uint64_t* sse_out, double* cost_out,
                                       int32_t* rd_list_out, void* stream)
{
  const char* name = "merge_cand_batch";
  VVC_CHECK_ARG(n_mc >= 0 && n_cand >= 0 && n_pu >= 0, "%s: n_mc %d, n_cand %d, n_pu %d", name, n_mc, n_cand, n_pu);
  if (n_pu == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(ref0_base && org_base && mc_descs && cand_mc_first && cand_dist && pu_cand_first && dist_out && cost_out && rd_list_out, "%s: null pointer", name);
  VVC_CHECK_ARG(n_comp == 1 || n_comp == 3, "%s: n_comp %d (1 or 3)", name, n_comp);
  VVC_CHECK_ARG(max_num_merge_cand >= 1 && max_num_merge_cand <= MG_MAX_CAND, "%s: max_num_merge_cand %d outside 1..%d", name, max_num_merge_cand, MG_MAX_CAND);
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "%s: clip range %d..%d", name, clp_min, clp_max);
  VVC_CHECK_ARG(sqrt_lambda >= 0.0 && sqrt_lambda < 1048576.0, "%s: sqrt_lambda out of range", name);
  VVC_CHECK_ARG(((uintptr_t)mc_descs & 15) == 0 && ((uintptr_t)cand_dist & 15) == 0, "%s: descriptor array must be 16-byte aligned", name);
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("%s: bit depth %d outside 8..10", name, bit_depth); return VVCGPU_E_UNSUPPORTED; }
  VVC_CHECK_ARG(n_cand < (1 << 27) && n_pu < (1 << 27), "%s: n %d", name, n_cand > n_pu ? n_cand : n_pu);
  hipStream_t st = (hipStream_t)stream;
  if (n_cand > 0)
  {
    const PuOwnerLds L = pu_owner_lds(4, 128, 128, MG_WAVE_MAX, mg_lds_bytes);
    MgArgs a;
    a.ref0 = ref0_base; a.ref1 = ref1_base ? ref1_base : ref0_base; a.org = org_base; a.pred = pred_base;
    a.mc = mc_descs; a.candMcFirst = cand_mc_first; a.candDist = cand_dist;
    a.distOut = reinterpret_cast<unsigned long long*>(dist_out); a.sseOut = reinterpret_cast<unsigned long long*>(sse_out);
    a.nMc = n_mc; a.nCand = n_cand; a.nComp = n_comp; a.useHad = use_hadamard ? 1 : 0; a.bd = bit_depth; a.cmin = clp_min; a.cmax = clp_max;
    a.waveBytes = L.waveBytes;
    VVC_HIP(vvc_allow_lds(merge_pred_kernel, L.lds));
    hipLaunchKernelGGL(merge_pred_kernel, dim3(pu_owner_grid(n_cand, true)), dim3(256), L.lds, st, a);
    VVC_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(merge_list_kernel, dim3(cdiv(n_pu, 256)), dim3(256), 0, st, pu_cand_first, n_pu, n_cand, max_num_merge_cand, sqrt_lambda,
                     reinterpret_cast<const unsigned long long*>(dist_out), cost_out, rd_list_out);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
