// sadsearch.hip -- the integer SAD search surface for gfx950: every position of a grid around a block, with an optional fused arg-min of
// SAD + motion-vector cost (vvcgpu_sad_search), and the raster stage of the whole-PU TZ searches (tzsearch.hip).
//
// Reference behaviour reproduced (bit-exact):
//   RdCost::xGetSAD*  CommonLib/RdCost.cpp:450-1000   (SIMD twins x86/RdCostX86.h:215-432; no early exit)
//   RdCost::getCostOfVectorWithPredictor / xGetExpGolombNumberOfBits   CommonLib/RdCost.h:172-199
//   InterSearch::xPatternSearch scan order and tie rule               EncoderLib/InterSearch.cpp:1887-1935
//
// Design
//   * generic kernel: one workgroup per (block, strip of search rows).  The reference window of the strip is
//     staged ONCE in LDS as packed 16-bit pairs in two alignments (even / odd start) so that every position reads
//     aligned dwords; samples are biased by 0x8000 so v_sad_u16 (2 abs-diffs per lane-op) is exact for any int16;
//     one lane = one search position, the org pairs are LDS broadcasts.
//   * the grids the encoder really asks for have kernels of their own: the step-5 raster of xTZSearch (pair, quad and group forms) and the
//     9 x 9 / small dense windows of xPatternSearch.  The host code at the end of the file plans each form and tries them in order.
#include "common.h"
#include "raster_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// Batched window fill: every lane keeps FB independent global loads in flight before the first LDS store (the simple
// load->store loop serialises one L2 round trip per element and dominated the kernel).
template <int FB>
__device__ __forceinline__ void fill_window_pairs(unsigned* __restrict__ lds, const unsigned* __restrict__ g, int rsDw,
                                                  int winRows, int pitchDw, int nPairs, int tid, int nthreads)
{
  const int total = winRows * pitchDw;
  int e = tid, r = tid / pitchDw, k = tid - r * pitchDw;
  const int dr = nthreads / pitchDw, dk = nthreads - dr * pitchDw;
  for (int base = 0; base < total; base += FB * nthreads)
  {
    unsigned v[FB];
    int idx[FB];
#pragma unroll
    for (int u = 0; u < FB; u++)
    {
      idx[u] = e < total ? e : -1;
      v[u] = e < total ? g[(ptrdiff_t)r * rsDw + min(k, nPairs - 1)] : 0u;
      e += nthreads; r += dr; k += dk;
      if (k >= pitchDw) { k -= pitchDw; r++; }
    }
#pragma unroll
    for (int u = 0; u < FB; u++) if (idx[u] >= 0) lds[idx[u]] = v[u] ^ 0x80008000u;
  }
}

constexpr int SS_THREADS = 512;

// `groups` sub-workgroups of gsz = SS_THREADS / groups lanes each take one block (small windows: several blocks per
// workgroup amortise launch / barrier cost); a group stages its own window slice of LDS.
__global__ __launch_bounds__(SS_THREADS) void sad_search_kernel(const Pel* __restrict__ org, int os,
                                                         const Pel* __restrict__ ref, int rs,
                                                         const vvcgpu_search_blk* __restrict__ blocks, int nblocks, int w, int h,
                                                         int subShift, int dx0, int dy0, int nx, int ny, int sx, int sy,
                                                         int rowsPerStrip, int colsPerStrip, int pitchDw, int split,
                                                         int groups, int groupDw, vvcgpu_mvcost mv, int useBest,
                                                         unsigned* __restrict__ out, vvcgpu_search_best* __restrict__ best)
{
  extern __shared__ __align__(16) unsigned lds_all[];
  const int gsz = SS_THREADS / groups;
  const int grp = threadIdx.x / gsz;
  const int tid = threadIdx.x - grp * gsz, lane = tid & 63, wave = tid >> 6, nwaves = gsz >> 6;
  unsigned* lds = lds_all + grp * groupDw;
  const int b = blockIdx.x * groups + grp, j0 = blockIdx.y * rowsPerStrip;
  const bool active = b < nblocks;
  const int nj = min(rowsPerStrip, ny - j0);
  const int i0 = blockIdx.z * colsPerStrip;
  const int ni = min(colsPerStrip, nx - i0);
  const int hs = h >> subShift, wp = w >> 1;
  const int winRows = (nj - 1) * sy + h;
  const int Ww = (ni - 1) * sx + w;
  unsigned* orgL = lds;                              // hs x wp pairs (biased)
  unsigned* refL = lds + ((hs * wp + 3) & ~3);       // winRows x pitchDw ALIGNED pairs of the window (biased)
  int odd = 0;
  if (active)
  {
    const vvcgpu_search_blk blk = blocks[b];
    const Pel* o = org + (size_t)blk.org_y * os + blk.org_x;
    for (int k = lane; k < wp; k += 64)
      for (int r = wave; r < hs; r += nwaves)
      {
        const Pel* q = o + (size_t)(r << subShift) * os + 2 * k;
        orgL[r * wp + k] = ((unsigned)(unsigned short)q[0] | ((unsigned)(unsigned short)q[1] << 16)) ^ 0x80008000u;
      }
    // Window fill: ONE copy, as the aligned dword pairs of the plane (sample 0 of the window is the low or the high half
    // of pair 0, `odd`); a position whose first sample sits in a high half re-pairs on the fly with v_alignbit.
    const ptrdiff_t winOff = (ptrdiff_t)(blk.ref_y + dy0 + j0 * sy) * rs + blk.ref_x + dx0 + i0 * sx;
    const bool fast = ((rs & 1) == 0) && ((reinterpret_cast<uintptr_t>(ref) & 3) == 0);
    odd = fast ? (int)(winOff & 1) : 0;
    const int nPairs = ((Ww - 1 + odd) >> 1) + 1;    // pairs that hold at least one window sample
    if (fast)
    {
      const unsigned* g = reinterpret_cast<const unsigned*>(ref + (winOff - odd));
      fill_window_pairs<8>(refL, g, rs >> 1, winRows, pitchDw, nPairs, tid, gsz);
    }
    else
    {
      const Pel* win = ref + winOff;
      for (int r = wave; r < winRows; r += nwaves)
      {
        const Pel* row = win + (ptrdiff_t)r * rs;
        for (int k = lane; k < pitchDw; k += 64)
        {
          const unsigned p0 = (unsigned short)row[min(2 * k, Ww - 1)], p1 = (unsigned short)row[min(2 * k + 1, Ww - 1)];
          refL[r * pitchDw + k] = (p0 | (p1 << 16)) ^ 0x80008000u;
        }
      }
    }
  }
  __syncthreads();
  if (!active) return;

  // task = (position, row class): `split` adjacent lanes share one position and take rows r = s, s+split, ...
  unsigned long long kmin = ~0ull;
  const int nTasks = nj * ni * split;
  const int sMask = split - 1;
  const int sLog = 31 - __clz(split);
  for (int t = tid; t < ((nTasks + 63) & ~63); t += gsz)
  {
    const bool live = t < nTasks;
    const int p = min(t, nTasks - 1) >> sLog, s = t & sMask;
    const int jj = p / ni, i = p - jj * ni;
    const int cx = i * sx + odd;                        // first sample, counted from the low half of pair 0
    const unsigned sh = (cx & 1) << 4;                   // 0: pairs are aligned; 16: re-pair (hi of g0, lo of g1)
    const unsigned* base = refL + (cx >> 1) + (jj * sy) * pitchDw;
    unsigned acc = 0;
    for (int r = s; r < hs; r += split)
    {
      const unsigned* rp = base + (r << subShift) * pitchDw;
      const unsigned* op = orgL + r * wp;
      unsigned g0 = rp[0];
      int k = 0;
      if ((wp & 3) == 0)                                 // 16-byte aligned org rows -> 128-bit broadcast reads
      {
#pragma unroll 2
        for (; k + 4 <= wp; k += 4)
        {
          const uint4 ov = *reinterpret_cast<const uint4*>(op + k);
          const unsigned g1 = rp[k + 1], g2 = rp[k + 2], g3 = rp[k + 3], g4 = rp[k + 4];
          acc = __builtin_amdgcn_sad_u16(ov.x, __builtin_amdgcn_alignbit(g1, g0, sh), acc);
          acc = __builtin_amdgcn_sad_u16(ov.y, __builtin_amdgcn_alignbit(g2, g1, sh), acc);
          acc = __builtin_amdgcn_sad_u16(ov.z, __builtin_amdgcn_alignbit(g3, g2, sh), acc);
          acc = __builtin_amdgcn_sad_u16(ov.w, __builtin_amdgcn_alignbit(g4, g3, sh), acc);
          g0 = g4;
        }
      }
      for (; k < wp; k++)
      {
        const unsigned g1 = rp[k + 1];
        acc = __builtin_amdgcn_sad_u16(op[k], __builtin_amdgcn_alignbit(g1, g0, sh), acc);
        g0 = g1;
      }
    }
    for (int o2 = 1; o2 < split; o2 <<= 1) acc += __shfl_xor(acc, o2);
    if (live && s == 0)
    {
      const int idx = (j0 + jj) * nx + i0 + i;
      if (out) out[(size_t)b * ny * nx + idx] = acc << subShift;
      if (useBest)                                                      // fused arg-min, see sad_raster5c_kernel
      {
        const int x = dx0 + (i0 + i) * sx, y = dy0 + (j0 + jj) * sy;
        const unsigned bits = expgolomb_bits(((x << mv.cost_scale) - mv.pred_hor) >> mv.imv_shift) +
                              expgolomb_bits(((y << mv.cost_scale) - mv.pred_ver) >> mv.imv_shift);
        const unsigned long long key = (((unsigned long long)(acc << subShift) + (unsigned long long)(mv.lambda * (double)bits)) << 24) | (unsigned)idx;
        kmin = key < kmin ? key : kmin;
      }
    }
  }
  if (useBest)
  {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long ok = __shfl_xor(kmin, o); kmin = ok < kmin ? ok : kmin; }
    if (lane == 0 && kmin != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(&best[b].cost), kmin);
  }
}

// ---------------------------------------------------------------------------------------------------
// Raster kernel ("r5c": step 5 in both directions = iRaster of xTZSearch under the shipped cfgs, InterSearch.cpp:1979-2000),
// fourth generation of this kernel, built around the fact that it is
// bound by instruction ISSUE (scalar + vector), not by LDS or HBM: rocprofv3 showed v_sad_u16 to be ~15 % of the vector
// instructions of the first version, the rest being window fill, addressing, realignment and the argmin.  (VOP3 instructions
// such as v_sad_u16 issue once per 4 cycles and SIMD, tools/micro/valu_rate.hip; every scalar instruction costs the wave a
// 4-cycle issue slot as well, SQ_ACTIVE_INST_SCA.)
//   * raster columns are split into the four classes i = c (mod 4): inside a class consecutive columns start exactly
//     20 samples = 5 aligned 8-byte LDS words apart and the sub-word offset o = (5 i + off) & 3 is the same for every
//     column, so a wave that works on ONE class needs no per-lane realignment: the word index and (for odd o) one
//     v_alignbit with a constant shift are compile-time choices (4 instantiations picked by a wave-uniform switch).
//   * one lane owns TWO positions, columns i and i+2 (classes c and c+2): their windows start 10 samples apart, so the
//     two share their 8-byte words (7 or 8 loaded instead of 5 + 5) and the same wave-uniform org row: the scalar work
//     per position (org loads, bias xor, addressing, loop) is halved and the LDS reads drop by a quarter.
//   * a 32-lane half carries 10 columns x 3 raster rows.  ds_read_b64 banks are (a/4) mod 64, i.e. 32 word slots; the
//     10 columns sit on slots 5k and the row pitch is chosen = 20 or 44 (mod 64) dwords, which puts the next raster row
//     (5 window rows further) 10 or 22 "column steps" away: the three rows interleave into 30 distinct slots and every
//     ds_read_b64 is conflict free at 2 LDS cycles per 8 bytes.  Dead lanes re-read a live lane's address (broadcast).
//   * blocks wider than 16 are walked as 16-sample chunks, so one code path serves w = 16..128.
//   * the org rows are wave-uniform scalar loads from a PACKED copy of the block (r5c_pack_org_kernel, a few microseconds per
//     launch): biased, row sub-sampling and odd origins resolved, in an even and an odd-shifted layout, so that the hot loop
//     has no scalar work on the org row and an odd window offset costs one merge instead of eight realignments
//     (r5c_compute); SMEM and LDS share lgkmcnt and SMEM returns out of order, so the
//     loop is software pipelined by hand: wait for stage s, issue the loads of stage s+1, then do the SADs of stage s.
//   * optional fused argmin: cost = SAD + motion-vector cost (the bit counts of the columns / rows
//     and lambda * bits come from small LDS tables built once per workgroup), packed as (cost << 24 | scan index) and
//     reduced with 64-bit min (DPP row operations -> LDS -> one global atomicMin per workgroup), so that the raster stage need
//     not write the SAD surface at all when the caller only wants the best candidate (xTZSearch does).
// One stage = two 16-sample chunk-rows for the lane's two positions i and i+2 (classes c and c+2, whose windows overlap:
// their 8-byte words are shared, 7 or 8 words for the two instead of 5 + 5).
// full 8-byte words in d[], plus the two half words at the ends of the span that are only half used (x0 = high dword of word 0
// when OA >= 2, x1 = low dword of the last word when OA is 0 or 3): 13-14 VGPRs per chunk-row instead of 16, which is what
// lets the kernel fit 80 VGPRs (6 waves per SIMD) without scratch.
struct R5cStage { unsigned ov[2][8]; unsigned long long d[2][7]; unsigned x0[2], x1[2]; };

// ADD = constant byte offset folded into the ds_read immediates (the second chunk-row of a stage, 32 bytes on in the same row)
template <int OA, int ADD>
__device__ __forceinline__ void r5c_issue_row(unsigned (&ov)[8], unsigned long long (&d)[7], unsigned& x0, unsigned& x1,
                                              const unsigned* __restrict__ op, unsigned a)
{
#pragma unroll
  for (int k = 0; k < 8; k++) ov[k] = op[k];
  // single ds_read_b64 (2 LDS cycles each); left to the compiler they are merged into ds_read2_b64, which runs at half
  // that rate.  The compiler cannot see that the destination registers stay busy until the explicit lgkmcnt(0) of the
  // pipeline: r5c_compute pins every one of them live past it, and nothing that is not needed is loaded.
#define R5C_OFFS "i"(ADD), "i"(ADD + 4), "i"(ADD + 8), "i"(ADD + 16), "i"(ADD + 24), "i"(ADD + 32), "i"(ADD + 40), "i"(ADD + 48), "i"(ADD + 56)
  //                %9        %10          %11          %12           %13           %14           %15           %16           %17   (after 8 outputs + address)
  if (OA == 0)        // words 0..5, low half of word 6
  {
    unsigned dummy;
    asm volatile("ds_read_b64 %0, %8 offset:%9\n\tds_read_b64 %1, %8 offset:%11\n\tds_read_b64 %2, %8 offset:%12\n\tds_read_b64 %3, %8 offset:%13\n\t"
                 "ds_read_b64 %4, %8 offset:%14\n\tds_read_b64 %5, %8 offset:%15\n\tds_read_b32 %6, %8 offset:%16"
                 : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(x1), "=&v"(dummy) : "v"(a), R5C_OFFS : "memory");
  }
  else if (OA == 1)   // words 0..6
  {
    unsigned dummy;
    asm volatile("ds_read_b64 %0, %8 offset:%9\n\tds_read_b64 %1, %8 offset:%11\n\tds_read_b64 %2, %8 offset:%12\n\tds_read_b64 %3, %8 offset:%13\n\t"
                 "ds_read_b64 %4, %8 offset:%14\n\tds_read_b64 %5, %8 offset:%15\n\tds_read_b64 %6, %8 offset:%16"
                 : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(d[6]), "=&v"(dummy) : "v"(a), R5C_OFFS : "memory");
  }
  else if (OA == 2)   // high half of word 0, words 1..6
  {
    unsigned dummy;
    asm volatile("ds_read_b32 %0, %8 offset:%10\n\tds_read_b64 %1, %8 offset:%11\n\tds_read_b64 %2, %8 offset:%12\n\tds_read_b64 %3, %8 offset:%13\n\t"
                 "ds_read_b64 %4, %8 offset:%14\n\tds_read_b64 %5, %8 offset:%15\n\tds_read_b64 %6, %8 offset:%16"
                 : "=&v"(x0), "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(dummy) : "v"(a), R5C_OFFS : "memory");
  }
  else                // high half of word 0, words 1..6, low half of word 7
    asm volatile("ds_read_b32 %0, %8 offset:%10\n\tds_read_b64 %1, %8 offset:%11\n\tds_read_b64 %2, %8 offset:%12\n\tds_read_b64 %3, %8 offset:%13\n\t"
                 "ds_read_b64 %4, %8 offset:%14\n\tds_read_b64 %5, %8 offset:%15\n\tds_read_b64 %6, %8 offset:%16\n\tds_read_b32 %7, %8 offset:%17"
                 : "=&v"(x0), "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(x1) : "v"(a), R5C_OFFS : "memory");
#undef R5C_OFFS
}

// acc0 / acc1 = positions i / i+2.  Class c+2 starts 10 samples after class c: dword (OA + 10) >> 1 of the span, same parity.
// The org row comes PACKED (r5c_pack_org_kernel): already biased, and in two layouts per 16-sample chunk --
//   even: dword k = samples (2k, 2k+1);
//   odd : dword k < 7 = samples (2k+1, 2k+2), dword 7 = (15 | 0 << 16)
// so that a position whose window starts on an ODD sample needs no realignment of its nine window dwords: the seven inner
// ones pair up with the shifted org pairs as they are, and the two half-used end dwords are merged by ONE v_perm/v_bfi
// (low half of the last, high half of the first) against the org pair (15, 0): 8 v_sad_u16 + 1 merge per position and
// chunk-row instead of 8 + 8, and no scalar work on the org row at all (no bias xor, no funnel shift for odd block origins).
template <int OA>
__device__ __forceinline__ void r5c_compute(const R5cStage& st, unsigned& acc0, unsigned& acc1)
{
  constexpr int W0 = OA >= 2 ? 1 : 0;                       // first word held in d[]
  constexpr int NF = OA == 1 ? 7 : 6;                       // full words in d[]
  constexpr int IA = OA >> 1, IB = (OA + 10) >> 1;          // first dword of the two positions
#pragma unroll
  for (int j = 0; j < 2; j++)
  {
    unsigned dd[16];
#pragma unroll
    for (int k = 0; k < NF; k++)
    {
      asm volatile("" :: "v"(st.d[j][k]));                  // whole 64-bit destination stays allocated until here
      dd[2 * (W0 + k)] = (unsigned)st.d[j][k]; dd[2 * (W0 + k) + 1] = (unsigned)(st.d[j][k] >> 32);
    }
    if (OA >= 2) { asm volatile("" :: "v"(st.x0[j])); dd[1] = st.x0[j]; }
    if (OA == 0) { asm volatile("" :: "v"(st.x1[j])); dd[12] = st.x1[j]; }
    if (OA == 3) { asm volatile("" :: "v"(st.x1[j])); dd[14] = st.x1[j]; }
    if (OA & 1)
    {
#pragma unroll
      for (int k = 0; k < 7; k++)
      {
        acc0 = __builtin_amdgcn_sad_u16(st.ov[j][k], dd[IA + 1 + k], acc0);
        acc1 = __builtin_amdgcn_sad_u16(st.ov[j][k], dd[IB + 1 + k], acc1);
      }
      acc0 = __builtin_amdgcn_sad_u16(st.ov[j][7], (dd[IA + 8] & 0xFFFFu) | (dd[IA] & 0xFFFF0000u), acc0);
      acc1 = __builtin_amdgcn_sad_u16(st.ov[j][7], (dd[IB + 8] & 0xFFFFu) | (dd[IB] & 0xFFFF0000u), acc1);
    }
    else
    {
#pragma unroll
      for (int k = 0; k < 8; k++)
      {
        acc0 = __builtin_amdgcn_sad_u16(st.ov[j][k], dd[IA + k], acc0);
        acc1 = __builtin_amdgcn_sad_u16(st.ov[j][k], dd[IB + k], acc1);
      }
    }
  }
}

// walks the hs x CH chunk-rows of the block, one stage = two chunk-rows at a time: oOff = dword offset of the current chunk-row of the packed org
// (8 dwords per chunk-row, rows without a gap), lOff = byte offset of the current chunk-row in the window
struct R5cCursor { unsigned oOff; unsigned lOff; int ch; };

// CH1: 16-wide blocks, the two chunk-rows of a stage are two window rows; otherwise (CH even) they are neighbours in one
// row and the second one is reached through the ds_read immediate offsets (one address add per stage)
template <int OA, bool CH1>
__device__ __forceinline__ void r5c_issue(R5cStage& st, const unsigned* __restrict__ orgDw, unsigned base, R5cCursor& cur, int CH,
                                          unsigned ldsStepB, unsigned lRowB)
{
  const unsigned a = base + cur.lOff;
  const unsigned* op = orgDw + cur.oOff;                                  // wave-uniform: scalar loads
  r5c_issue_row<OA, 0>(st.ov[0], st.d[0], st.x0[0], st.x1[0], op, a);
  if (CH1)
  {
    r5c_issue_row<OA, 0>(st.ov[1], st.d[1], st.x0[1], st.x1[1], op + 8, a + ldsStepB);
    cur.lOff += 2 * ldsStepB;
  }
  else
  {
    r5c_issue_row<OA, 32>(st.ov[1], st.d[1], st.x0[1], st.x1[1], op + 8, a);
    cur.ch += 2; cur.lOff += 64;
    if (cur.ch == CH) { cur.ch = 0; cur.lOff += lRowB; }
  }
  cur.oOff += 16;
}

template <int OA, bool CH1>
__device__ __forceinline__ void r5c_positions(const unsigned* __restrict__ orgDw, unsigned base, int ldsStep, R5cCursor cur,
                                              int nStages, int CH, unsigned& acc0, unsigned& acc1)
{
  R5cStage A, B;
  const unsigned ldsStepB = (unsigned)ldsStep * 4u, lRowB = (unsigned)(ldsStep - 8 * CH) * 4u;
  r5c_issue<OA, CH1>(A, orgDw, base, cur, CH, ldsStepB, lRowB);
  for (int s = 0; s < nStages; s += 2)
  {
    R5C_WAIT_LGKM0();
    if (s + 1 < nStages) r5c_issue<OA, CH1>(B, orgDw, base, cur, CH, ldsStepB, lRowB);
    __builtin_amdgcn_sched_barrier(0);
    r5c_compute<OA>(A, acc0, acc1);
    if (s + 1 >= nStages) break;
    R5C_WAIT_LGKM0();
    if (s + 2 < nStages) r5c_issue<OA, CH1>(A, orgDw, base, cur, CH, ldsStepB, lRowB);
    __builtin_amdgcn_sched_barrier(0);
    r5c_compute<OA>(B, acc0, acc1);
  }
}

// org rows of the raster kernel, packed per block: [block][layout even | odd][hs rows][w / 2 dwords], biased (^ 0x8000 per
// sample), row sub-sampling and odd block origins resolved here.  Layouts per 16-sample chunk: see r5c_compute.
// interleave != 0 (quad form): [block][chunk-row][even 8 | odd 8] -- both layouts of a chunk-row are one 64-byte scalar load.
// One thread per 16-sample chunk-row: 8 dword loads (16 sample loads when the chunk is not 4-byte aligned) issued together, both layouts
// built in registers, four 16-byte stores (one thread per output dword with two sample loads each took 13 - 16 us per 4K launch).
// initBest != nullptr: the arg-min keys of the raster kernels start at all-ones (saves the separate fill launch).
__global__ __launch_bounds__(256) void r5c_pack_org_kernel(const Pel* __restrict__ org, int os, const vvcgpu_search_blk* __restrict__ blocks,
                                                           int nblocks, int w, int hs, int subShift, unsigned* __restrict__ packed, int interleave,
                                                           unsigned long long* __restrict__ initBest, const VvcRasterPer* __restrict__ per = nullptr)
{
  const int CH = w >> 4, perBlockUnits = hs * CH;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (initBest)
    for (size_t i = gid; i < (size_t)nblocks * 3; i += (size_t)gridDim.x * blockDim.x) initBest[i] = ~0ull;
  if (gid >= (size_t)nblocks * perBlockUnits) return;
  const int b = (int)(gid / (unsigned)perBlockUnits), rem = (int)(gid - (size_t)b * perBlockUnits);
  const int row = rem / CH, chunk = rem - row * CH;
  if (per && !per[b].active) return;                                         // per-block form: a block that takes no part may not even be w x h
  const vvcgpu_search_blk blk = blocks[b];
  const Pel* o = org + (size_t)(blk.org_y + (row << subShift)) * os + blk.org_x + 16 * chunk;
  unsigned d[8];
  if ((reinterpret_cast<uintptr_t>(o) & 3) == 0)
  {
    const unsigned* q = reinterpret_cast<const unsigned*>(o);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = q[k];
  }
  else
  {
    unsigned short sm[16];
#pragma unroll
    for (int k = 0; k < 16; k++) sm[k] = (unsigned short)o[k];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = (unsigned)sm[2 * k] | ((unsigned)sm[2 * k + 1] << 16);
  }
  unsigned E[8], O[8];
#pragma unroll
  for (int k = 0; k < 8; k++)
  {
    E[k] = d[k] ^ 0x80008000u;
    O[k] = __builtin_amdgcn_alignbit(d[(k + 1) & 7], d[k], 16) ^ 0x80008000u;          // k < 7: samples (2k+1, 2k+2); k = 7: (15, 0)
  }
  const unsigned perLayout = (unsigned)(hs * (w >> 1));
  unsigned* pe; unsigned* po;
  if (interleave) { pe = packed + (size_t)b * 2u * perLayout + (size_t)(row * CH + chunk) * 16; po = pe + 8; }
  else            { pe = packed + (size_t)b * 2u * perLayout + (size_t)row * (w >> 1) + chunk * 8; po = pe + perLayout; }
  reinterpret_cast<uint4*>(pe)[0] = make_uint4(E[0], E[1], E[2], E[3]); reinterpret_cast<uint4*>(pe)[1] = make_uint4(E[4], E[5], E[6], E[7]);
  reinterpret_cast<uint4*>(po)[0] = make_uint4(O[0], O[1], O[2], O[3]); reinterpret_cast<uint4*>(po)[1] = make_uint4(O[4], O[5], O[6], O[7]);
}

// MINW = waves per SIMD the register allocation must allow: 6 (<= 80 VGPRs) when three workgroups fit the CU's LDS, else 4.
// Serves grids wider than 40 columns; narrower ones take the quad form below.
template <int MAXT, int MINW>
__global__ __launch_bounds__(MAXT, MINW) void sad_raster5c_kernel(const unsigned* __restrict__ orgPacked,
                                                           const Pel* __restrict__ ref, int rs,
                                                           const vvcgpu_search_blk* __restrict__ blocks, int w, int h, int subShift,
                                                           int dx0, int dy0, int nx, int ny, int rowsPerStrip, int pitchDw,
                                                           int nstrips, unsigned invStrips, int total, int winBytes, vvcgpu_mvcost mv, int useBest,
                                                           unsigned* __restrict__ out, vvcgpu_search_best* __restrict__ best)
{
  extern __shared__ __align__(16) unsigned refL[];
  __shared__ unsigned long long wgKey;
  const int tid = threadIdx.x;
  // XCD-aware order (speed only): workgroups are dealt round-robin over the 8 XCDs, so workgroup L lands with L+8, L+16...
  // Give each XCD one CONTIGUOUS run of (block, strip) items: the strips of one block and the windows of neighbouring
  // blocks overlap heavily, and this way the overlap is found in that XCD's own L2 instead of being fetched 8 times.
  const int chunk = (total + 7) >> 3;
  const int item = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
  if (item >= total) return;
  const int b = nstrips == 1 ? item : (int)__umulhi((unsigned)item, invStrips), j0 = (item - b * nstrips) * rowsPerStrip;   // item / nstrips (item < 2^32 / nstrips)
  const int nj = min(rowsPerStrip, ny - j0);
  const vvcgpu_search_blk blk = blocks[b];
  const int hs = h >> subShift;
  const int winRows = (nj - 1) * 5 + h;
  const int Ww = (nx - 1) * 5 + w;
  const ptrdiff_t winOff = (ptrdiff_t)(blk.ref_y + dy0 + j0 * 5) * rs + blk.ref_x + dx0;
  const int off = (int)(winOff & 7);
  fill_window_cols<8>(refL, reinterpret_cast<const uint4*>(ref + (winOff - off)), rs >> 3, winRows, pitchDw,
                      ((Ww - 1 + off) >> 3) + 1, tid, (int)blockDim.x);
  unsigned char* bitsX = reinterpret_cast<unsigned char*>(refL) + winBytes;   // [nx] then [rowsPerStrip]
  unsigned char* bitsY = bitsX + nx;
  // lambda * bits as a table over the bit count (<= 2 * 65): the double-precision product, its truncation and the 64-bit
  // conversion are done once per workgroup and entry instead of twice per lane and wave item
  unsigned long long* costTab = reinterpret_cast<unsigned long long*>(bitsX + ((nx + rowsPerStrip + 15) & ~15));
  if (useBest)
  {
    if (tid == 0) wgKey = ~0ull;
    for (int n = tid; n < R5C_COST_N; n += (int)blockDim.x) costTab[n] = (unsigned long long)(mv.lambda * (double)n);
    for (int n = tid; n < nx + nj; n += (int)blockDim.x)
    {
      const int v = n < nx ? (((dx0 + n * 5) << mv.cost_scale) - mv.pred_hor) : (((dy0 + (j0 + n - nx) * 5) << mv.cost_scale) - mv.pred_ver);
      bitsX[n] = (unsigned char)expgolomb_bits(v >> mv.imv_shift);
    }
  }
  __syncthreads();

  const int CH = w >> 4;
  const int nStages = (hs * CH) >> 1;
  const int ngrp = (nj + 5) / 6, ncg = (nx + 39) / 40;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = (int)(blockDim.x >> 6);
  const int lane = tid & 63;
  const unsigned layoutDw = (unsigned)(hs * (w >> 1));                     // one packed layout of the block (even, then odd)
  const unsigned* orgDw = orgPacked + (size_t)b * 2u * layoutDw;
  const int ldsStep = pitchDw << subShift;
  const unsigned ldsBase = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)refL;
  unsigned long long kmin = ~0ull;
  // lane -> (column k of 10, raster row m of 3) of its half; lanes 30, 31 of a half (m = 3) are dead and re-read lanes 0, 1.
  // The mapping is re-derived from an opaque copy of the lane id after the SAD loop, so that none of it has to stay in
  // registers across the loop (the kernel sits right at the 80-VGPR limit of 6 waves per SIMD).
  auto lane_map = [](int ln, int& k, int& m, bool& dead) { const int q = ln & 31; m = (q * 26) >> 8; k = q - 10 * m; dead = m >= 3; if (dead) m = 0; };
  // epilogue of one wave item (classes c and c + 2 of row group g, column group cg): SAD surface and / or the packed arg-min key
  auto finish = [&](int c, int g, int cg, unsigned acc0, unsigned acc1)
  {
      int lane2 = lane;
      asm volatile("" : "+v"(lane2));                                       // opaque: forces the re-derivation below
      int k, m; bool dead;
      lane_map(lane2, k, m, dead);
      const int jj = g * 6 + (lane2 >> 5) * 3 + m;
      const int i0 = cg * 40 + 4 * k + c;
      if (!dead && jj < nj)
      {
        const int idx0 = (j0 + jj) * nx + i0;
        unsigned* o = out ? out + (size_t)b * ny * nx + idx0 : nullptr;
        const unsigned v0 = acc0 << subShift, v1 = acc1 << subShift;
        const bool in0 = i0 < nx, in1 = i0 + 2 < nx;
        if (o)
        {
          if (in0) o[0] = v0;
          if (in1) o[2] = v1;
        }
        if (useBest)
        {
          // all three bit counts first, then both table entries: two dependent LDS round trips for the lane's two positions
          const unsigned by = bitsY[jj], bx0 = bitsX[in0 ? i0 : 0], bx1 = bitsX[in1 ? i0 + 2 : 0];
          const unsigned long long c0 = costTab[bx0 + by], c1 = costTab[bx1 + by];
          const unsigned long long key0 = ((v0 + c0) << 24) | (unsigned)idx0, key1 = ((v1 + c1) << 24) | (unsigned)(idx0 + 2);
          if (in0) kmin = key0 < kmin ? key0 : kmin;
          if (in1) kmin = key1 < kmin ? key1 : kmin;
        }
      }
  };
  const R5cCursor cur0 = { 0u, 0u, 0 };
  for (int cg = 0; cg < ncg; cg++)
    for (int it = wave; it < 2 * ngrp; it += nwaves)
    {
      const int c = it & 1, g = it >> 1;                                    // classes c and c + 2
      const int OA = (c + off) & 3;                                         // == cx & 3 for every lane of the wave
      unsigned acc0 = 0, acc1 = 0;
      {
        int k, m; bool dead;
        lane_map(lane, k, m, dead);
        const int jj = g * 6 + (lane >> 5) * 3 + m;
        const int i0 = cg * 40 + 4 * k + c;                                 // positions i0 and i0 + 2
        const int cx = 5 * (i0 < nx ? i0 : c) + off;                        // dead lanes re-read a live lane's address (broadcast)
        const unsigned base = ldsBase + (unsigned)(2 * (cx >> 2) + (min(jj, nj - 1) * 5) * pitchDw) * 4u;
#define R5C_CALL(OV)                                                                                                            \
        do { if (CH == 1) r5c_positions<OV, true>(orgDw + ((OV) & 1) * layoutDw, base, ldsStep, cur0, nStages, CH, acc0, acc1);          \
             else         r5c_positions<OV, false>(orgDw + ((OV) & 1) * layoutDw, base, ldsStep, cur0, nStages, CH, acc0, acc1); } while (0)
        if (OA == 0) R5C_CALL(0); else if (OA == 1) R5C_CALL(1); else if (OA == 2) R5C_CALL(2); else R5C_CALL(3);
#undef R5C_CALL
      }
      finish(c, g, cg, acc0, acc1);
    }
  if (useBest)
  {
    kmin = wave_min_u64(kmin);
    if (lane == 0 && kmin != ~0ull) atomicMin(&wgKey, kmin);
    __syncthreads();
    if (tid == 0 && wgKey != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(&best[b].cost), wgKey);
  }
}

// ---------------------------------------------------------------------------------------------------
// Raster kernel, QUAD form ("r5q").  PMC of the r5c form at 4K (profiles/r02_pmc_sq.csv): the vector pipe and the LDS pipe are both ~60 %
// busy -- a lane reads 13-14 dwords of window per chunk-row for the 16 v_sad_u16 of its two positions (3.4 B per v_sad_u16; four SIMDs at
// full rate would need 197 B/clk of the CU's 128).  Here a lane owns FOUR consecutive raster columns 4k .. 4k+3 (all four alignment
// classes): their windows start 0 / 5 / 10 / 15 samples into the same span of 31 + 16 samples, so 16 (17) dwords serve 32 v_sad_u16 --
// 2 B per v_sad_u16.  Columns on an odd sample use the odd-shifted org layout and one merge, exactly as in r5c; the two layouts of the
// org row are both held as scalar operands (16 SGPRs per chunk-row).  One stage = ONE chunk-row (17 VGPRs, two stages in flight).
// A wave item is a row group of six raster rows (10 column groups x 3 rows per 32-lane half, the r5c lane map and bank analysis
// unchanged: the ds_read_b64 of step n reads slot 5k + n); items are twice as heavy as in r5c and half as many, so the rows of a block
// are split over up to four waves (SPLIT), the partial sums meeting in LDS after the loop.
// Measured (profiles/r02_raster_parts.txt): equal to the pair form for 32-wide blocks, 4 % faster for 64-wide ones -- with the window staging
// taken out the SAD loop alone is 90 % of the kernel time and its executed vector instructions (v_sad_u16 incl. lane / row / column padding
// + 28 % moves and merges) x 4.4 cycles account for that time: the loop is bound by the VOP3 issue rate, not by LDS.
template <int MAXT, int MINW, int SPLIT>
__global__ __launch_bounds__(MAXT, MINW) void sad_raster5q_kernel(const unsigned* __restrict__ orgPacked,
                                                           const Pel* __restrict__ ref, int rs,
                                                           const vvcgpu_search_blk* __restrict__ blocks, int w, int h, int subShift,
                                                           int dx0, int dy0, int nxU, int nyU, int rowsPerStrip, int pitchDw,
                                                           int nstrips, unsigned invStrips, int total, int winBytes, int maxRows, vvcgpu_mvcost mv, int useBest,
                                                           unsigned* __restrict__ out, vvcgpu_search_best* __restrict__ best, const VvcRasterPer* __restrict__ per)
{
  extern __shared__ __align__(16) unsigned refL[];
  __shared__ unsigned long long wgKey;
  const int tid = threadIdx.x;
  const int chunk = (total + 7) >> 3;                                       // XCD-aware order, as r5c
  const int item = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
  if (item >= total) return;
  const int b = nstrips == 1 ? item : (int)__umulhi((unsigned)item, invStrips), strip = item - b * nstrips, j0 = strip * rowsPerStrip;
  // per != nullptr (raster stage of whole-PU TZ searches): grid size, grid origin and predictor per block; inactive blocks and strips below
  // the block's grid leave at once (before any barrier)
  int nx = nxU, ny = nyU;
  if (per)
  {
    const VvcRasterPer pb = per[b];
    if (!pb.active) return;
    nx = pb.nx; ny = pb.ny; dx0 = pb.x0; dy0 = pb.y0; mv.pred_hor = pb.pred_hor; mv.pred_ver = pb.pred_ver;
  }
  const int nj = strip == nstrips - 1 ? ny - j0 : min(rowsPerStrip, ny - j0);  // the last strip takes the remainder (<= maxRows, may exceed rowsPerStrip)
  if (nj <= 0) return;
  const vvcgpu_search_blk blk = blocks[b];
  const int hs = h >> subShift;
  // The SAD loop takes the packed org rows as scalar operands, one 64-byte line per stage with one stage of look-ahead: a line that is
  // not in the scalar cache costs a trip to L2 / HBM per stage.  Every wave touches the lines of its part here, in flight during the
  // window fill, so that the loop's scalar loads hit.
  unsigned touched = 0;
  if (SPLIT <= 2 && (useBest & 2))                                            // measured: 261 -> 254 us for 32x32 at 4K; no gain with four parts per block
  {
    const int nStW = (hs * (w >> 4)) / SPLIT;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned* p = orgPacked + (size_t)b * 2u * (unsigned)(hs * (w >> 1)) + (size_t)(wv % SPLIT) * nStW * 16;
    int s0 = 0;
    for (; s0 + 8 <= nStW; s0 += 8)
#pragma unroll
      for (int u = 0; u < 8; u++) touched += p[(s0 + u) * 16];
    for (; s0 < nStW; s0++) touched += p[s0 * 16];
  }
  useBest &= 1;
  const int winRows = (nj - 1) * 5 + h;
  const int Ww = (nx - 1) * 5 + w;
  const ptrdiff_t winOff = (ptrdiff_t)(blk.ref_y + dy0 + j0 * 5) * rs + blk.ref_x + dx0;
  const int off = (int)(winOff & 7);
  fill_window_cols<8>(refL, reinterpret_cast<const uint4*>(ref + (winOff - off)), rs >> 3, winRows, pitchDw,
                      ((Ww - 1 + off) >> 3) + 1, tid, (int)blockDim.x);
  unsigned char* bitsX = reinterpret_cast<unsigned char*>(refL) + winBytes;   // [nx] then [rowsPerStrip]
  unsigned char* bitsY = bitsX + nx;
  unsigned long long* costTab = reinterpret_cast<unsigned long long*>(bitsX + ((nx + maxRows + 15) & ~15));
  if (useBest)
  {
    if (tid == 0) wgKey = ~0ull;
    for (int n = tid; n < R5C_COST_N; n += (int)blockDim.x) costTab[n] = (unsigned long long)(mv.lambda * (double)n);
    for (int n = tid; n < nx + nj; n += (int)blockDim.x)
    {
      const int v = n < nx ? (((dx0 + n * 5) << mv.cost_scale) - mv.pred_hor) : (((dy0 + (j0 + n - nx) * 5) << mv.cost_scale) - mv.pred_ver);
      bitsX[n] = (unsigned char)expgolomb_bits(v >> mv.imv_shift);
    }
  }
  __syncthreads();

  const int CH = w >> 4;
  const int nStages = hs * CH;                                                // chunk-rows of the block
  const int ngrp = (nj + 5) / 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = (int)(blockDim.x >> 6);
  const int lane = tid & 63;
  const unsigned layoutDw = (unsigned)(hs * (w >> 1));
  const unsigned* orgQ = orgPacked + (size_t)b * 2u * layoutDw;             // interleaved layout: 16 dwords per chunk-row
  const int ldsStep = pitchDw << subShift;
  const unsigned ldsBase = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)refL;
  const int OA = off & 3;                                                     // sub-word offset of column 4 k: the same for every lane
  unsigned long long kmin = ~0ull;
  auto lane_map = [](int ln, int& k, int& m, bool& dead) { const int q = ln & 31; m = (q * 26) >> 8; k = q - 10 * m; dead = m >= 3; if (dead) m = 0; };
  auto finish = [&](int g, const unsigned (&acc)[4])
  {
    int lane2 = lane;
    asm volatile("" : "+v"(lane2));                                           // opaque: the lane map is re-derived here instead of being kept live
    int k, m; bool dead;
    lane_map(lane2, k, m, dead);
    const int jj = g * 6 + (lane2 >> 5) * 3 + m;
    const int i0 = 4 * k;
    if (!dead && jj < nj && i0 < nx)
    {
      const int idx0 = (j0 + jj) * nx + i0;
      unsigned* o = out ? out + (size_t)b * ny * nx + idx0 : nullptr;
      const unsigned by = useBest ? bitsY[jj] : 0u;
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        if (i0 + q >= nx) break;
        const unsigned v = acc[q] << subShift;
        if (o) o[q] = v;
        if (useBest)
        {
          const unsigned long long key = ((v + costTab[bitsX[i0 + q] + by]) << 24) | (unsigned)(idx0 + q);
          kmin = key < kmin ? key : kmin;
        }
      }
    }
  };
  unsigned keep[4] = { 0u, 0u, 0u, 0u }; int keepIt = -1;
  for (int it = wave; it < ngrp * SPLIT; it += nwaves)
  {
    const int part = SPLIT == 1 ? 0 : it % SPLIT, g = SPLIT == 1 ? it : it / SPLIT;
    const int nSt = nStages / SPLIT;
    unsigned acc[4] = { 0u, 0u, 0u, 0u };
    {
      int k, m; bool dead;
      lane_map(lane, k, m, dead);
      const int jj = g * 6 + (lane >> 5) * 3 + m;
      const int i0 = 4 * k;
      const int cx = 5 * (i0 < nx ? i0 : 0) + off;                           // dead lanes re-read a live lane's address (broadcast)
      const unsigned base = ldsBase + (unsigned)(2 * (cx >> 2) + (min(jj, nj - 1) * 5) * pitchDw) * 4u;
      if (OA == 0)      r5q_positions<0>(orgQ, base, ldsStep, CH, part * nSt, nSt, acc);
      else if (OA == 1) r5q_positions<1>(orgQ, base, ldsStep, CH, part * nSt, nSt, acc);
      else if (OA == 2) r5q_positions<2>(orgQ, base, ldsStep, CH, part * nSt, nSt, acc);
      else              r5q_positions<3>(orgQ, base, ldsStep, CH, part * nSt, nSt, acc);
    }
    if (SPLIT > 1) { keep[0] = acc[0]; keep[1] = acc[1]; keep[2] = acc[2]; keep[3] = acc[3]; keepIt = it; }   // one item per wave (host)
    else finish(g, acc);
  }
  if (SPLIT > 1)
  {
    __syncthreads();                                                          // every wave is done with the window: its first bytes are re-used
    uint4* xch = reinterpret_cast<uint4*>(refL);
    if (keepIt >= 0 && (keepIt % SPLIT) != 0) xch[((keepIt / SPLIT) * (SPLIT - 1) + (keepIt % SPLIT) - 1) * 64 + lane] = make_uint4(keep[0], keep[1], keep[2], keep[3]);
    __syncthreads();
    if (keepIt >= 0 && (keepIt % SPLIT) == 0)
    {
#pragma unroll
      for (int p = 1; p < SPLIT; p++)
      {
        const uint4 o = xch[((keepIt / SPLIT) * (SPLIT - 1) + p - 1) * 64 + lane];
        keep[0] += o.x; keep[1] += o.y; keep[2] += o.z; keep[3] += o.w;
      }
      finish(keepIt / SPLIT, keep);
    }
  }
  if (useBest)
  {
    kmin = wave_min_u64(kmin);
    if (lane == 0 && kmin != ~0ull) atomicMin(&wgKey, kmin);
    __syncthreads();
    if (tid == 0 && wgKey != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(&best[b].cost), wgKey);
  }
  asm volatile("" :: "s"(touched));                                           // keeps the touch loads (no scalar load follows: an asm statement counts as a clobber)
}

// ---------------------------------------------------------------------------------------------------
// Raster kernel, GROUP form for 16-wide blocks with QUAD columns ("r5gq").  PMC of sad_raster5c_kernel on a 3840x2160 picture of 16x16 blocks
// (profiles/r02a_pmc_sq.csv): 331 vector + 278 scalar instructions per wave item for the 128 v_sad_u16 that are the work -- a wave item
// of a 16x16 block is only four software-pipeline stages long, so the window fill (every block stages its own 206-column window), the
// item set-up (lane map, LDS address, cost table look-ups) and the arg-min epilogue outweigh the SAD loop.  Here a workgroup serves a
// GROUP of up to 8 blocks that are horizontal neighbours in the reference picture (the caller's list order; runs are detected on the
// device, a group that is not one run is served run by run):
//   * ONE window for the run: (nx - 1) 5 + 16 n columns instead of n ((nx - 1) 5 + 16) -- 4.2x less fill for n = 8, nx = 39;
//   * a unit = (row group of six raster rows, SUB-RUN of up to two blocks), four columns per lane with the SAD loop of r5q: block t of the
//     run sees the same lane -> position map shifted by 16 t samples = 32 t bytes of LDS, so the set-up and the cost look-ups are paid once
//     per sub-run; the loop spends 70 vector instructions per 64 v_sad_u16, and the per-block epilogue folds the lane's four candidates into
//     one 32-bit word (cost << 2 | candidate: cost < 2^30, the host checks lambda), a 32-bit minimum and one 64-bit compare;
//   * the lower LDS demand per block allows strips of 12 raster rows (two full row groups: 36 + 3 rows of a 39-row raster in 42 row
//     slots instead of 48) at three workgroups per CU.
// Everything else (row pitch 20 / 44 mod 64 dwords, packed org rows as scalar operands) is the r5q form.  ~600 vector instructions per 512
// v_sad_u16; the first group form (pair columns, sub-runs of four blocks, cost << 1 | candidate) needed 813 and is gone: its numbers are in
// docs/OPTIMISATION_LOG.md.  A lambda too large for the 32-bit key goes to the per-block quad form.
constexpr int R5G_MAXNB = 8;                            // blocks per group
// above every valid cost: SAD + cost < 0x30000000 = 2^28 + 2^29 (SAD of a 16-wide block of any two int16 planes <= 16 * 128 * 65535 < 2^28; cost = lambda * bits
// < 2^29: the host checks lambda < 4e6, bits <= 131), and below 2^30, so (cost << 2 | candidate) fits 32 bits, an invalid lane's (R5GQ_INVALID + SAD) << 2
// included.  tests/test_search_bounds_cpu.py puts inputs on these bounds
constexpr unsigned R5GQ_INVALID = 0x30000000u;

__global__ __launch_bounds__(1024, 6) void sad_raster5gq_kernel(const unsigned* __restrict__ orgPacked, const Pel* __restrict__ ref, int rs,
                                                                const vvcgpu_search_blk* __restrict__ blocks, int nblocks, int nbg, int h, int subShift,
                                                                int dx0, int dy0, int nx, int ny, int rowsPerStrip, int pitchDw,
                                                                int nstrips, unsigned invStrips, int total, int winBytes, vvcgpu_mvcost mv,
                                                                vvcgpu_search_best* __restrict__ best)
{
  extern __shared__ __align__(16) unsigned refL[];
  __shared__ unsigned long long wgKey[R5G_MAXNB];
  const int tid = threadIdx.x;
  const int chunk = (total + 7) >> 3;                                          // XCD-aware order, as r5c
  const int item = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
  if (item >= total) return;
  const int q = nstrips == 1 ? item : (int)__umulhi((unsigned)item, invStrips), j0 = (item - q * nstrips) * rowsPerStrip;
  const int nj = min(rowsPerStrip, ny - j0);
  const int b0 = q * nbg, nbk = min(nbg, nblocks - b0);
  const int hs = h >> subShift;
  const int winRows = (nj - 1) * 5 + h;
  unsigned char* bitsX = reinterpret_cast<unsigned char*>(refL) + winBytes;   // [nx] then [rowsPerStrip]
  unsigned char* bitsY = bitsX + nx;
  unsigned* costTab = reinterpret_cast<unsigned*>(bitsX + ((nx + rowsPerStrip + 15) & ~15));   // lambda * bits, truncated (host: below 2^29)
  for (int n = tid; n < R5C_COST_N; n += (int)blockDim.x) costTab[n] = (unsigned)(unsigned long long)(mv.lambda * (double)n);
  for (int n = tid; n < nx + nj; n += (int)blockDim.x)
  {
    const int v = n < nx ? (((dx0 + n * 5) << mv.cost_scale) - mv.pred_hor) : (((dy0 + (j0 + n - nx) * 5) << mv.cost_scale) - mv.pred_ver);
    bitsX[n] = (unsigned char)expgolomb_bits(v >> mv.imv_shift);
  }
  const int ngrp = (nj + 5) / 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned layoutDw = (unsigned)(hs * 8);                                // one layout of a 16-wide block; a block = 2 layouts, interleaved per chunk-row
  const int ldsStep = pitchDw << subShift;
  const unsigned ldsBase = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)refL;

  for (int k0 = 0; k0 < nbk; )
  {
    const int rx = blocks[b0 + k0].ref_x, ry = blocks[b0 + k0].ref_y;
    int n = 1;
    while (k0 + n < nbk && blocks[b0 + k0 + n].ref_y == ry && blocks[b0 + k0 + n].ref_x == rx + 16 * n) n++;
    const ptrdiff_t winOff = (ptrdiff_t)(ry + dy0 + j0 * 5) * rs + rx + dx0;
    const int off = (int)(winOff & 7);
    if (k0 > 0) __syncthreads();                                               // every wave is done with the previous run's window and keys
    fill_window_cols<8>(refL, reinterpret_cast<const uint4*>(ref + (winOff - off)), rs >> 3, winRows, pitchDw,
                        (((nx - 1) * 5 + 16 * n - 1 + off) >> 3) + 1, tid, (int)blockDim.x);
    if (tid < R5G_MAXNB) wgKey[tid] = ~0ull;
    __syncthreads();

    const int nsub = (n + 1) >> 1;                                            // sub-runs of up to two blocks
    const int g = wave / nsub, t0 = (wave - g * nsub) * 2, nt = min(2, n - t0);
    if (g < ngrp)
    {
      const int OA = off & 3;
      const int lane = tid & 63, ql = lane & 31, m0 = (ql * 26) >> 8, kk = ql - 10 * m0;
      const bool dead = m0 >= 3;
      const int jj = g * 6 + (lane >> 5) * 3 + (dead ? 0 : m0);
      const int i0 = 4 * kk;                                                  // positions i0 .. i0 + 3
      const int cx = 5 * (i0 < nx ? i0 : 0) + off;                            // dead lanes re-read a live lane's address (broadcast)
      const int jc = min(jj, nj - 1);
      const unsigned base = ldsBase + (unsigned)(2 * (cx >> 2) + (jc * 5) * pitchDw) * 4u + 32u * (unsigned)t0;
      const bool live = !dead && jj < nj;
      const unsigned by = bitsY[jc];
      unsigned cst[4];
#pragma unroll
      for (int m = 0; m < 4; m++)
      {
        const bool in = live && i0 + m < nx;
        cst[m] = ((in ? costTab[bitsX[in ? i0 + m : 0] + by] : R5GQ_INVALID) << 2) | (unsigned)m;
      }
      const unsigned* orgBlk = orgPacked + (size_t)(b0 + k0 + t0) * 2u * layoutDw;
      unsigned kmin[2];
#pragma unroll
      for (int t = 0; t < 2; t++)
      {
        if (t >= nt) break;                                                    // wave-uniform
        unsigned acc[4] = { 0u, 0u, 0u, 0u };
        const unsigned* oq = orgBlk + (size_t)t * 2u * layoutDw;
        const unsigned bt = base + 32u * t;
        if (OA == 0)      r5q_positions<0>(oq, bt, ldsStep, 1, 0, hs, acc);
        else if (OA == 1) r5q_positions<1>(oq, bt, ldsStep, 1, 0, hs, acc);
        else if (OA == 2) r5q_positions<2>(oq, bt, ldsStep, 1, 0, hs, acc);
        else              r5q_positions<3>(oq, bt, ldsStep, 1, 0, hs, acc);
        const int sh = subShift + 2;
        kmin[t] = min(min((acc[0] << sh) + cst[0], (acc[1] << sh) + cst[1]), min((acc[2] << sh) + cst[2], (acc[3] << sh) + cst[3]));
      }
      int lane2 = tid & 63;
      asm volatile("" : "+v"(lane2));                                         // re-derive the lane's scan index after the loops instead of keeping it live
      const int ql2 = lane2 & 31, m2 = (ql2 * 26) >> 8;
      const unsigned idx0 = (unsigned)((j0 + min(g * 6 + (lane2 >> 5) * 3 + m2, nj - 1)) * nx + 4 * (ql2 - 10 * m2));
#pragma unroll
      for (int t = 0; t < 2; t++)
      {
        if (t >= nt) break;
        // cost first, then the lane (lane order = scan order), then the lane's own candidate bits: they must not take part in the minimum across lanes
        const unsigned c = kmin[t] >> 2;
        const unsigned km = wave_min_u32(c);
        const unsigned long long hit = __ballot(c == km);
        const int src = __builtin_ctzll(hit);
        const unsigned sel = (unsigned)__builtin_amdgcn_readlane((int)kmin[t], src) & 3u;
        const unsigned idx = (unsigned)__builtin_amdgcn_readlane((int)idx0, src) + sel;
        if ((tid & 63) == 0) atomicMin(&wgKey[t0 + t], ((unsigned long long)km << 24) | idx);
      }
    }
    __syncthreads();
    if (tid < n) atomicMin(reinterpret_cast<unsigned long long*>(&best[b0 + k0 + tid].cost), wgKey[tid]);
    k0 += n;
  }
}

// ---------------------------------------------------------------------------------------------------
// Dense small grids (step 1 in both directions, nx * ny <= 256: the +-4 window of xPatternSearch): the (block, position)
// pairs of G = 256 / (nx ny) blocks are laid flat over the 256 lanes of a workgroup (81 positions: 3 blocks, 95 % of the
// lanes busy, where one block per 128 lanes would leave a third idle); each block's org and window sit in LDS as biased
// 16-bit pairs, the org row is a broadcast 16-byte LDS read per lane group.  A block is finished by exactly one workgroup,
// so the arg-min needs no global atomic, no memset and no decode pass: per-block 64-bit LDS min, then one lane writes the
// finished vvcgpu_search_best.
__global__ __launch_bounds__(256) void sad_dense_kernel(const Pel* __restrict__ org, int os, const Pel* __restrict__ ref, int rs,
                                                        const vvcgpu_search_blk* __restrict__ blocks, int nblocks, int w, int h,
                                                        int subShift, int dx0, int dy0, int nx, int ny, int pitchDw, int blkDw, int G,
                                                        int npos, unsigned recipNpos, unsigned recipNx, vvcgpu_mvcost mv, int useBest,
                                                        unsigned* __restrict__ out, vvcgpu_search_best* __restrict__ best)
{
  extern __shared__ __align__(16) unsigned ldsD[];
  __shared__ unsigned long long keyL[32];
  __shared__ int oddL[32];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * G;
  const int hs = h >> subShift, wp = w >> 1, lwp = 31 - __clz(wp);
  const int winRows = ny - 1 + h, Ww = nx - 1 + w;
  const int orgDw = (hs * wp + 3) & ~3;
  if (tid < 32) keyL[tid] = ~0ull;
  for (int g = 0; g < G && b0 + g < nblocks; g++)
  {
    const vvcgpu_search_blk blk = blocks[b0 + g];
    unsigned* orgL = ldsD + g * blkDw;
    unsigned* refL = orgL + orgDw;
    const Pel* o = org + (size_t)blk.org_y * os + blk.org_x;
    for (int e = tid; e < hs * wp; e += 256)
    {
      const int r = e >> lwp, k = e & (wp - 1);
      const Pel* q = o + (size_t)(r << subShift) * os + 2 * k;
      orgL[e] = ((unsigned)(unsigned short)q[0] | ((unsigned)(unsigned short)q[1] << 16)) ^ 0x80008000u;
    }
    const ptrdiff_t winOff = (ptrdiff_t)(blk.ref_y + dy0) * rs + blk.ref_x + dx0;
    const int odd = (int)(winOff & 1);
    if (tid == 0) oddL[g] = odd;
    const int nPairs = ((Ww - 1 + odd) >> 1) + 1;
    const unsigned* gp = reinterpret_cast<const unsigned*>(ref + (winOff - odd));
    const int rsDw = rs >> 1;
    for (int r = tid >> 4; r < winRows; r += 16)
      for (int k = tid & 15; k < nPairs; k += 16)
        refL[r * pitchDw + k] = gp[(ptrdiff_t)r * rsDw + k] ^ 0x80008000u;
  }
  __syncthreads();

  const int g = (int)(((unsigned)tid * recipNpos) >> 16), p = tid - g * npos;
  const bool live = g < G && b0 + g < nblocks;
  if (live)
  {
    const int j = (int)(((unsigned)p * recipNx) >> 16), i = p - j * nx;
    const unsigned* orgL = ldsD + g * blkDw;
    const int cx = i + oddL[g];
    const unsigned sh = (cx & 1) << 4;
    const unsigned* base = orgL + orgDw + (cx >> 1) + j * pitchDw;
    unsigned acc = 0;
    for (int r = 0; r < hs; r++)
    {
      const unsigned* rp = base + (r << subShift) * pitchDw;
      const unsigned* op = orgL + r * wp;
      unsigned g0 = rp[0];
#pragma unroll 2
      for (int k = 0; k < wp; k += 4)
      {
        const uint4 ov = *reinterpret_cast<const uint4*>(op + k);
        const unsigned g1 = rp[k + 1], g2 = rp[k + 2], g3 = rp[k + 3], g4 = rp[k + 4];
        acc = __builtin_amdgcn_sad_u16(ov.x, __builtin_amdgcn_alignbit(g1, g0, sh), acc);
        acc = __builtin_amdgcn_sad_u16(ov.y, __builtin_amdgcn_alignbit(g2, g1, sh), acc);
        acc = __builtin_amdgcn_sad_u16(ov.z, __builtin_amdgcn_alignbit(g3, g2, sh), acc);
        acc = __builtin_amdgcn_sad_u16(ov.w, __builtin_amdgcn_alignbit(g4, g3, sh), acc);
        g0 = g4;
      }
    }
    acc <<= subShift;
    if (out) out[((size_t)(b0 + g) * ny + j) * nx + i] = acc;
    if (useBest)
    {
      const int x = dx0 + i, y = dy0 + j;
      const unsigned bits = expgolomb_bits(((x << mv.cost_scale) - mv.pred_hor) >> mv.imv_shift) +
                            expgolomb_bits(((y << mv.cost_scale) - mv.pred_ver) >> mv.imv_shift);
      atomicMin(&keyL[g], (((unsigned long long)acc + (unsigned long long)(mv.lambda * (double)bits)) << 24) | (unsigned)p);
    }
  }
  if (!useBest) return;
  __syncthreads();
  if (tid < G && b0 + tid < nblocks)
  {
    const unsigned long long key = keyL[tid];
    const int idx = (int)(key & 0xFFFFFFu);
    const unsigned long long cost = key >> 24;
    const int j = idx / nx, i = idx - j * nx;
    const int x = dx0 + i, y = dy0 + j;
    const unsigned bits = expgolomb_bits(((x << mv.cost_scale) - mv.pred_hor) >> mv.imv_shift) +
                          expgolomb_bits(((y << mv.cost_scale) - mv.pred_ver) >> mv.imv_shift);
    vvcgpu_search_best r;
    r.x = x; r.y = y; r.cost = cost; r.sad = cost - (unsigned long long)(mv.lambda * (double)bits);
    best[b0 + tid] = r;
  }
}

// ---------------------------------------------------------------------------------------------------
// Dense 9 x 9 grid, ROW form ("d9"): the +-4 window of xPatternSearch around a predictor for blocks made of 16 x 16 tiles with 2:1 row
// sub-sampling.  sad_dense_kernel gives every position its own lane, so each v_sad_u16 costs one LDS dword for the window and a share of
// the org read, plus a funnel shift for odd positions: it is LDS-bound at a tenth of the vector issue rate.  Here a lane owns a whole ROW
// of the position grid for one 16 x 16 UNIT of a block (nine lanes per unit, seven units per wave): a window row is read once
// (13 dwords) and serves all positions of the lane -- the even ones straight from the dwords G[k], the odd ones from the shifted stream
// H[k] = (G[k+1], G[k]) >> 16, built once per row (12 funnel shifts instead of 32).  A unit whose window starts on an odd sample needs
// positions t = 1..9 of the aligned row instead of 0..8: every lane accumulates the ten sums t = 0..9 and picks its nine at the end, so
// lanes of different parity run the same code (80 v_sad_u16 + 12 shifts per row and lane; LDS traffic per v_sad_u16 drops 7x).  The
// window is staged with aligned 8-byte loads and written one dword down when it starts in the upper half of its 8-byte word; the eight
// org rows sit in the four spare dwords of the 20-dword row pitch (rows of a unit's nine lanes fall on distinct banks).  Blocks wider or
// taller than 16 are split into units; their partial sums meet in LDS before the arg-min.
constexpr int D9_PITCH = 20, D9_ROWS = 24, D9_UNIT_DW = D9_ROWS * D9_PITCH;
struct D9Meta { long long refOff, orgOff; int ds, par, valid, pad; };

__global__ __launch_bounds__(384) void sad_dense9_kernel(const Pel* __restrict__ org, int os, const Pel* __restrict__ ref, int rs,
                                                        const vvcgpu_search_blk* __restrict__ blocks, int nblocks, int tilesX, int upb, int G,
                                                        int dx0, int dy0, vvcgpu_mvcost mv, int useBest,
                                                        unsigned* __restrict__ out, vvcgpu_search_best* __restrict__ best)
{
  extern __shared__ __align__(16) unsigned ldsN[];
  const int T = (int)blockDim.x, tid = threadIdx.x;
  const int U = G * upb;
  D9Meta* meta = reinterpret_cast<D9Meta*>(ldsN + U * D9_UNIT_DW);                            // [U]
  unsigned long long* costTab = reinterpret_cast<unsigned long long*>(meta + U);              // [R5C_COST_N]
  unsigned long long* keyL = costTab + R5C_COST_N;                                            // [G]
  unsigned* sums = reinterpret_cast<unsigned*>(keyL + G);                                     // [G * 81] (upb > 1)
  unsigned char* bitsXY = reinterpret_cast<unsigned char*>(sums + (upb > 1 ? G * 81 : 0));    // [9] x, [9] y
  const int b0 = blockIdx.x * G;
  if (tid < U)
  {
    const int g = tid / upb, t = tid - g * upb, ty = t / tilesX, tx = t - ty * tilesX;
    D9Meta m = {};
    m.valid = b0 + g < nblocks;
    if (m.valid)
    {
      const vvcgpu_search_blk blk = blocks[b0 + g];
      const long long winOff = (long long)(blk.ref_y + dy0 + 16 * ty) * rs + blk.ref_x + dx0 + 16 * tx;
      const int o = (int)(((long long)(reinterpret_cast<uintptr_t>(ref) >> 1) + winOff) & 3);   // samples above the 8-byte boundary below the window start
      m.refOff = winOff - o; m.ds = o >> 1; m.par = o & 1;
      m.orgOff = (long long)(blk.org_y + 16 * ty) * os + blk.org_x + 16 * tx;
    }
    meta[tid] = m;
  }
  if (useBest)
  {
    for (int n = tid; n < R5C_COST_N; n += T) costTab[n] = (unsigned long long)(mv.lambda * (double)n);
    if (tid < 18)
    {
      const int v = tid < 9 ? (((dx0 + tid) << mv.cost_scale) - mv.pred_hor) : (((dy0 + tid - 9) << mv.cost_scale) - mv.pred_ver);
      bitsXY[tid] = (unsigned char)expgolomb_bits(v >> mv.imv_shift);
    }
    if (tid < G) keyL[tid] = ~0ull;
  }
  if (upb > 1)
    for (int n = tid; n < G * 81; n += T) sums[n] = 0u;
  __syncthreads();

  // window: 24 rows x 7 aligned 8-byte loads per unit, stored so that LDS dword 0 of a row = samples (winOff - par, winOff - par + 1);
  // org: eight sub-sampled rows of 8 biased pairs in the spare dwords 16..19 of window rows 2 r (pairs 0..3) and 2 r + 1 (pairs 4..7).
  // EVERY load of a thread (<= 20 window words, <= 8 org pairs) is issued before the first store: one memory round trip for the staging, one
  // for the block list in front of it.  (Measured at 4K: staging alone 24 - 36 us per launch, the SAD loop alone 16.)
  constexpr int FBW = 20, FBO = 8;
  const int nW = U * (D9_ROWS * 7), nO = U * 64;
  for (int e0 = tid, f0 = tid; e0 < nW || f0 < nO; e0 += FBW * T, f0 += FBO * T)
  {
    uint2 v[FBW]; int dstHi[FBW]; unsigned skipLo = 0u;                    // dstHi = LDS index of the HIGH dword (>= 0), -1 = nothing to store
    unsigned short lo[FBO], hi[FBO]; int dst[FBO];
#pragma unroll
    for (int i = 0; i < FBW; i++)
    {
      const int e = e0 + i * T;
      dstHi[i] = -1;
      if (e < nW)
      {
        const int u = (int)__umulhi((unsigned)e, 25565282u), rem = e - u * (D9_ROWS * 7);             // e / 168, exact for e < 2^24
        const int r = (int)(((unsigned)rem * 9363u) >> 16), q = rem - r * 7;                        // rem / 7 (rem < 168)
        const D9Meta m = meta[u];
        if (m.valid)
        {
          v[i] = *reinterpret_cast<const uint2*>(ref + (m.refOff + (long long)r * rs + 4 * q));
          dstHi[i] = u * D9_UNIT_DW + r * D9_PITCH + 2 * q - m.ds + 1;
          if (2 * q - m.ds < 0) skipLo |= 1u << i;                                                  // the low dword falls off the row
        }
      }
    }
#pragma unroll
    for (int i = 0; i < FBO; i++)
    {
      const int e = f0 + i * T;
      dst[i] = -1;
      if (e < nO)
      {
        const int u = e >> 6, rem = e & 63, r = rem >> 3, k = rem & 7;
        const D9Meta m = meta[u];
        if (m.valid)
        {
          const Pel* q = org + (m.orgOff + (long long)(2 * r) * os + 2 * k);
          lo[i] = (unsigned short)q[0]; hi[i] = (unsigned short)q[1];
          dst[i] = u * D9_UNIT_DW + (2 * r + (k >> 2)) * D9_PITCH + 16 + (k & 3);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < FBW; i++)
      if (dstHi[i] >= 0)
      {
        if (!(skipLo & (1u << i))) ldsN[dstHi[i] - 1] = v[i].x ^ 0x80008000u;
        ldsN[dstHi[i]] = v[i].y ^ 0x80008000u;
      }
#pragma unroll
    for (int i = 0; i < FBO; i++)
      if (dst[i] >= 0) ldsN[dst[i]] = ((unsigned)lo[i] | ((unsigned)hi[i] << 16)) ^ 0x80008000u;
  }
  __syncthreads();

  const int u = (int)(((unsigned)tid * 7282u) >> 16), j = tid - 9 * u;                          // tid / 9 (tid < 384)
  if (u < U && meta[u].valid)
  {
    const unsigned* base = ldsN + u * D9_UNIT_DW;
    unsigned Tt[10];
#pragma unroll
    for (int t = 0; t < 10; t++) Tt[t] = 0u;
#pragma unroll 2
    for (int r = 0; r < 8; r++)
    {
      const unsigned* row = base + (j + 2 * r) * D9_PITCH;
      const uint4 a = *reinterpret_cast<const uint4*>(row), b = *reinterpret_cast<const uint4*>(row + 4), c = *reinterpret_cast<const uint4*>(row + 8);
      const unsigned Gd[13] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, row[12] };
      const uint4 o0 = *reinterpret_cast<const uint4*>(base + (2 * r) * D9_PITCH + 16), o1 = *reinterpret_cast<const uint4*>(base + (2 * r + 1) * D9_PITCH + 16);
      const unsigned O[8] = { o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w };
      unsigned Hd[12];
#pragma unroll
      for (int k = 0; k < 12; k++) Hd[k] = __builtin_amdgcn_alignbit(Gd[k + 1], Gd[k], 16);
#pragma unroll
      for (int t = 0; t < 10; t++)
#pragma unroll
        for (int k = 0; k < 8; k++) Tt[t] = __builtin_amdgcn_sad_u16(O[k], (t & 1) ? Hd[(t >> 1) + k] : Gd[(t >> 1) + k], Tt[t]);
    }
    const bool par = meta[u].par != 0;
    const int g = u / upb;
    unsigned long long kmin = ~0ull;
#pragma unroll
    for (int x = 0; x < 9; x++)
    {
      const unsigned sad = (par ? Tt[x + 1] : Tt[x]) << 1;                                     // the row sub-sampling shift of the reference
      if (upb > 1) atomicAdd(&sums[g * 81 + j * 9 + x], sad);
      else
      {
        if (out) out[(size_t)(b0 + g) * 81 + j * 9 + x] = sad;
        if (useBest)
        {
          const unsigned long long key = (((unsigned long long)sad + costTab[bitsXY[x] + bitsXY[9 + j]]) << 24) | (unsigned)(j * 9 + x);
          kmin = key < kmin ? key : kmin;
        }
      }
    }
    if (upb == 1 && useBest) atomicMin(&keyL[g], kmin);
  }
  if (upb > 1)
  {
    __syncthreads();
    for (int e = tid; e < G * 81; e += T)
    {
      const int g = e / 81, pidx = e - g * 81;
      if (b0 + g >= nblocks) continue;
      const unsigned sad = sums[e];
      if (out) out[(size_t)(b0 + g) * 81 + pidx] = sad;
      if (useBest)
      {
        const int jj = pidx / 9, x = pidx - jj * 9;
        atomicMin(&keyL[g], (((unsigned long long)sad + costTab[bitsXY[x] + bitsXY[9 + jj]]) << 24) | (unsigned)pidx);
      }
    }
  }
  if (!useBest) return;
  __syncthreads();
  if (tid < G && b0 + tid < nblocks)
  {
    const unsigned long long key = keyL[tid];
    const int idx = (int)(key & 0xFFFFFFu);
    const unsigned long long cost = key >> 24;
    const int jj = idx / 9, i = idx - jj * 9;
    vvcgpu_search_best r;
    r.x = dx0 + i; r.y = dy0 + jj; r.cost = cost; r.sad = cost - costTab[bitsXY[i] + bitsXY[9 + jj]];
    best[b0 + tid] = r;
  }
}

// decodes the packed (cost << 24 | scan index) keys left in best[].cost by sad_raster5c_kernel
__global__ __launch_bounds__(256) void sad_best_decode_kernel(int nblocks, int dx0, int dy0, int nx, int sx, int sy, vvcgpu_mvcost mv,
                                                              vvcgpu_search_best* __restrict__ best)
{
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nblocks) return;
  const unsigned long long key = best[b].cost;
  const int idx = (int)(key & 0xFFFFFFu);
  const unsigned long long cost = key >> 24;
  const int j = idx / nx, i = idx - j * nx;
  const int x = dx0 + i * sx, y = dy0 + j * sy;
  const unsigned bits = expgolomb_bits(((x << mv.cost_scale) - mv.pred_hor) >> mv.imv_shift) +
                        expgolomb_bits(((y << mv.cost_scale) - mv.pred_ver) >> mv.imv_shift);
  vvcgpu_search_best r;
  r.x = x; r.y = y; r.cost = cost; r.sad = cost - (unsigned long long)(mv.lambda * (double)bits);
  best[b] = r;
}

// ---------------------------------------------------------------------------------------------------
// Host side.  Every kernel form has one function that decides whether it takes the call (`taken`) and launches it if so; vvcgpu_sad_search tries
// them in a fixed order.  The geometry of the step-5 raster forms is planned by plain functions of the call's integers (no HIP calls).

struct SadCall                                               // the checked arguments of one search call
{
  const Pel* org; int os; const Pel* ref; int rs;
  const vvcgpu_search_blk* blocks; int nblocks, w, h, subShift, dx0, dy0, nx, ny, sx, sy;
  unsigned* out; const vvcgpu_mvcost* mvHost; vvcgpu_search_best* best; hipStream_t st;
  vvcgpu_mvcost mv() const { return best ? *mvHost : vvcgpu_mvcost{}; }
  int hs() const { return h >> subShift; }
  bool raster5() const                                       // what every step-5 raster form needs of the planes and the grid
  { return sx == 5 && sy == 5 && (os & 1) == 0 && (rs & 7) == 0 && ((uintptr_t)org & 3) == 0 && ((uintptr_t)ref & 15) == 0 && (long long)nx * ny < (1 << 24) && nx >= 1; }
};
constexpr size_t SAD_LDS_HARD = 150 * 1024;                  // no form asks for more dynamic LDS

// behind the launch of a search kernel: its check, then the packed keys of `best` (if asked for) become records
int decode_best(const SadCall& c, const vvcgpu_mvcost& mv)
{
  VVC_LAUNCH_CHECK();
  if (!c.best) return VVCGPU_OK;
  hipLaunchKernelGGL(sad_best_decode_kernel, dim3(cdiv(c.nblocks, 256)), dim3(256), 0, c.st, c.nblocks, c.dx0, c.dy0, c.nx, c.sx, c.sy, mv, c.best);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int try_dense9(const SadCall& c, bool& taken)
{
  taken = c.sx == 1 && c.sy == 1 && c.nx == 9 && c.ny == 9 && c.subShift == 1 && (c.w & 15) == 0 && (c.h & 15) == 0 && c.w <= 64 && c.h <= 64 &&
          (c.rs & 3) == 0 && (!c.best || (c.mvHost->lambda >= 0.0 && c.mvHost->lambda < 1.0e9));
  if (!taken) return VVCGPU_OK;
  const int tilesX = c.w >> 4, upb = tilesX * (c.h >> 4);
  // Workgroup size.  Measured (profiles/r02_dense9.txt): the staging is bound by memory-level parallelism (87 % of the L2 requests miss, ~1.2 TB/s of
  // scattered 128-byte lines whatever the kernel does), so several small workgroups in different phases beat one large one: 128 threads = 14 units
  // (nine lanes per unit, whole blocks per workgroup).  64 x 64 blocks (16 units each) would need 320 threads for two blocks and lose; they stay with
  // sad_dense_kernel.
  const int T = 128, G = upb <= 4 ? (128 / 9) / upb : 0, U = G * upb;
  taken = G > 0;
  if (!taken) return VVCGPU_OK;
  const size_t smem = (size_t)U * D9_UNIT_DW * 4 + (size_t)U * sizeof(D9Meta) + R5C_COST_N * 8 + (size_t)G * 8 + (upb > 1 ? (size_t)G * 81 * 4 : 0) + 32;
  VVC_HIP(vvc_allow_lds(sad_dense9_kernel, smem));
  hipLaunchKernelGGL(sad_dense9_kernel, dim3(cdiv(c.nblocks, G)), dim3(T), smem, c.st, c.org, c.os, c.ref, c.rs, c.blocks, c.nblocks, tilesX, upb, G,
                     c.dx0, c.dy0, c.mv(), c.best ? 1 : 0, c.out, c.best);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int try_dense(const SadCall& c, bool& taken)
{
  taken = c.sx == 1 && c.sy == 1 && c.nx * c.ny <= 256 && c.w >= 8 && c.w <= 128 && (c.w & (c.w - 1)) == 0 && (c.rs & 1) == 0 && ((uintptr_t)c.ref & 3) == 0;
  if (!taken) return VVCGPU_OK;
  const int npos = c.nx * c.ny, wp = c.w >> 1;
  int pitch = (c.nx - 1 + c.w + 1) / 2 + 1;                               // pairs of the widest row + one look-ahead pair
  while ((pitch & 31) != 5 && (pitch & 31) != 27) pitch++;                // consecutive rows 5 banks apart: distinct banks for a wave's ~8 rows
  const int orgDw = (c.hs() * wp + 3) & ~3;
  const int blkDw = (orgDw + (c.ny - 1 + c.h) * pitch + 4 + 3) & ~3;
  int G = 256 / npos;
  if (G > 32) G = 32;
  while (G > 1 && (size_t)G * blkDw * 4 > 60 * 1024) G--;
  const size_t smem = (size_t)G * blkDw * 4;
  taken = smem <= SAD_LDS_HARD;
  if (!taken) return VVCGPU_OK;
  VVC_HIP(vvc_allow_lds(sad_dense_kernel, smem));
  hipLaunchKernelGGL(sad_dense_kernel, dim3(cdiv(c.nblocks, G)), dim3(256), smem, c.st, c.org, c.os, c.ref, c.rs, c.blocks, c.nblocks,
                     c.w, c.h, c.subShift, c.dx0, c.dy0, c.nx, c.ny, pitch, blkDw, G, npos, 65536u / (unsigned)npos + 1u, 65536u / (unsigned)c.nx + 1u,
                     c.mv(), c.best ? 1 : 0, c.out, c.best);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

// ---- step-5 raster forms.  A workgroup stages the window of one strip of raster rows; a wave item covers six raster rows x 40 columns.
struct R5Plan
{
  int pitch, rps, nstrips;   // row pitch of the staged window in dwords; raster rows per strip, strips per block (or group of blocks)
  int maxRows;               // rows of the tallest strip: the last one where it takes a remainder above rps (quad form), else rps
  int split, threads, total; // waves that share a wave item (quad form); workgroup size; (block or group, strip) items = workgroups before XCD padding
  size_t winB, smem;         // bytes of the staged window; all dynamic LDS: window, bit counts of the columns and rows, cost table
  unsigned inv_strips() const { return 0xFFFFFFFFu / (unsigned)nstrips + 1u; }   // item / nstrips by multiply-high
  int grid() const { return cdiv(total, 8) * 8; }                               // whole rounds over the 8 XCDs
};
constexpr size_t R5_BUDGET = 78 * 1024, R5G_BUDGET = 50 * 1024;   // window budgets (the group form's was swept in round 3: docs/OPTIMISATION_LOG.md)

// whole 16-byte quads of the widest row (`cols` samples at any phase of 8), then the next pitch = 20 or 44 (mod 64) dwords: see sad_raster5c_kernel
int r5_pitch(int cols)
{
  int pitch = (((cols - 1 + 7) >> 3) + 1) * 4;
  while ((pitch & 63) != 20 && (pitch & 63) != 44) pitch += 4;
  return pitch;
}
size_t r5_win_bytes(int rows, int h, int pitch) { return (size_t)((rows - 1) * 5 + h) * pitch * 4 + 64; }   // + slack: a dead position's words end <= 64 B on
void r5_set_lds(R5Plan& p, int h, int nx, size_t costBytes)               // window, [nx] + [maxRows] bit counts, cost table of costBytes per entry
{
  p.winB = r5_win_bytes(p.maxRows, h, p.pitch);
  p.smem = p.winB + (((size_t)nx + p.maxRows + 15) & ~(size_t)15) + R5C_COST_N * costBytes;
}

// group form (r5gq): strips of whole row groups (6 raster rows), as many as the budget allows up to 24 rows; one wave per (row group, two blocks)
bool r5gq_plan(int nblocks, int h, int subShift, int nx, int ny, R5Plan& p)
{
  const int hsR = h >> subShift, ngroups = cdiv(nblocks, R5G_MAXNB);
  p.pitch = r5_pitch((nx - 1) * 5 + 16 * R5G_MAXNB);
  int rps = 6;
  while (rps + 6 <= ny + 5 && rps + 6 <= 24 && r5_win_bytes(rps + 6, h, p.pitch) <= R5G_BUDGET) rps += 6;
  if (rps >= ny) rps = cdiv(ny, 3) * 3;
  p.rps = p.maxRows = rps; p.nstrips = cdiv(ny, rps);
  r5_set_lds(p, h, nx, sizeof(unsigned));
  p.split = 1; p.threads = 64 * cdiv(rps, 6) * cdiv(R5G_MAXNB, 2); p.total = ngroups * p.nstrips;      // <= 16 waves: rps <= 24, 8 blocks
  return p.smem <= SAD_LDS_HARD && (hsR & 1) == 0 && hsR >= 2 && nx + rps <= 4096 && (unsigned long long)ngroups * p.nstrips * p.nstrips < (1ull << 32);
}

// per-block forms: the fewest strips whose (3-row rounded) window fits the budget.  False: neither the quad nor the pair form can take the grid.
// (measured and not kept: strips of at most 18 raster rows for 32-wide blocks, 0.315 vs 0.292 ms at 4K; strip heights chosen for the fewest
// six-row groups, 201 vs 185 us -- docs/OPTIMISATION_LOG.md)
bool r5_strip_plan(int nblocks, int w, int h, int subShift, int nx, int ny, R5Plan& p)
{
  p.pitch = r5_pitch((nx - 1) * 5 + w);
  for (p.nstrips = 1;; p.nstrips++)
  {
    p.rps = cdiv(cdiv(ny, p.nstrips), 3) * 3;
    if (r5_win_bytes(p.rps, h, p.pitch) <= R5_BUDGET || p.rps <= 3) break;
  }
  p.nstrips = cdiv(ny, p.rps); p.maxRows = p.rps;
  r5_set_lds(p, h, nx, sizeof(unsigned long long));
  return p.smem <= SAD_LDS_HARD && (((h >> subShift) * (w >> 4)) & 1) == 0 && nx + p.rps <= 4096 &&
         (unsigned long long)nblocks * p.nstrips * p.nstrips < (1ull << 32);   // item decode by multiply-high (and total fits an int)
}

// quad form (r5q, grids of at most 40 columns): items are row groups only, the last strip takes the remainder of the rows, and the block's chunk-rows
// are split over 1 / 2 / 4 / 8 waves so that a workgroup has 8 - 12 waves of at least 8 stages.
// wholeGroups (the block lists of vvcgpu_sad_search; the per-block launch keeps the 3-row rounded strips): a wave item is a group of SIX raster rows,
// so 15 + 15 + 9 rows are 3 + 3 + 2 groups for 6.5 groups of work.  When whole groups per strip with the remainder in the LAST strip give fewer groups
// in no more strips and the same window (39 rows of 64-wide blocks: 12 + 12 + 15 = 2 + 2 + 3 groups), take that split.
bool r5q_plan(int nblocks, int w, int h, int subShift, int nx, int ny, bool wholeGroups, R5Plan& p)
{
  if (nx > 40 || !r5_strip_plan(nblocks, w, h, subShift, nx, ny, p)) return false;
  int last = ny - (p.nstrips - 1) * p.rps;
  const int groupsNow = (p.nstrips - 1) * cdiv(p.rps, 6) + cdiv(last, 6);
  for (int r = (p.rps / 6) * 6; wholeGroups && r >= 6; r -= 6)
  {
    const int ns = ny / r, l = ny - (ns - 1) * r, groups = (ns - 1) * (r / 6) + cdiv(l, 6);
    if (ns >= 1 && ns <= p.nstrips && r5_win_bytes(l, h, p.pitch) <= R5_BUDGET && l <= 24 && groups < groupsNow) { p.rps = r; p.nstrips = ns; last = l; break; }
  }
  p.maxRows = p.rps > last ? p.rps : last;
  r5_set_lds(p, h, nx, sizeof(unsigned long long));
  const int items = cdiv(p.maxRows, 6), nSt = (h >> subShift) * (w >> 4);
  p.split = 1;
  while (p.split < 8 && items * p.split * 2 <= 12 && (nSt % (p.split * 2)) == 0 && nSt / (p.split * 2) >= 8) p.split *= 2;
  p.threads = items * p.split * 64; p.total = nblocks * p.nstrips;
  return true;
}

// packed org rows of the raster kernels (the keys initialised on the way); packed == nullptr: claimed from the call's scratch
int launch_pack_org(const SadCall& c, VvcScratch* sc, unsigned*& packed, int interleave, const VvcRasterPer* per)
{
  if (!packed) packed = sc->take<unsigned>((size_t)c.nblocks * 2 * c.hs() * (c.w >> 1));
  if (!packed) return VVCGPU_E_DEVICE;
  hipLaunchKernelGGL(r5c_pack_org_kernel, dim3((unsigned)(((size_t)c.nblocks * c.hs() * (c.w >> 4) + 255) / 256)), dim3(256), 0, c.st, c.org, c.os, c.blocks, c.nblocks,
                     c.w, c.hs(), c.subShift, packed, interleave, reinterpret_cast<unsigned long long*>(c.best), per);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

// The one launch of the quad form: packed org, the kernel, the decode of the keys.  per: per-block grids (c.nx x c.ny is then the largest one).
// touchOrg: the waves touch their packed org lines during the window fill (see the kernel).
int launch_r5q(const SadCall& c, const R5Plan& p, VvcScratch* sc, unsigned* packed, const VvcRasterPer* per, bool touchOrg, bool decode)
{
  if (int rc = launch_pack_org(c, sc, packed, 1, per)) return rc;
  const vvcgpu_mvcost mv = c.mv();
  auto kfn = p.split == 8 ? sad_raster5q_kernel<1024, 4, 8> : p.split == 4 ? sad_raster5q_kernel<1024, 4, 4> :
             p.split == 2 ? sad_raster5q_kernel<1024, 4, 2> : sad_raster5q_kernel<1024, 4, 1>;
  VVC_HIP(vvc_allow_lds(kfn, p.smem));
  hipLaunchKernelGGL(kfn, dim3(p.grid()), dim3(p.threads), p.smem, c.st, packed, c.ref, c.rs, c.blocks, c.w, c.h, c.subShift, c.dx0, c.dy0, c.nx, c.ny, p.rps,
                     p.pitch, p.nstrips, p.inv_strips(), p.total, (int)p.winB, p.maxRows, mv, (c.best ? 1 : 0) | (touchOrg ? 2 : 0), c.out, c.best, per);
  if (decode) return decode_best(c, mv);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int try_raster_group(const SadCall& c, VvcScratch& sc, bool& taken)
{
  R5Plan p;
  // 16-wide blocks, best candidate only; the 32-bit key cost << 2 | candidate needs SAD + lambda * bits < 0x30000000 (R5GQ_INVALID: SAD < 2^28, lambda * bits < 2^29)
  taken = c.raster5() && c.w == 16 && c.best && !c.out && c.nx <= 40 && c.mvHost->lambda >= 0.0 && c.mvHost->lambda < 4.0e6 &&
          r5gq_plan(c.nblocks, c.h, c.subShift, c.nx, c.ny, p);
  if (!taken) return VVCGPU_OK;
  unsigned* packed = nullptr;
  if (int rc = launch_pack_org(c, &sc, packed, 1, nullptr)) return rc;
  VVC_HIP(vvc_allow_lds(sad_raster5gq_kernel, p.smem));
  hipLaunchKernelGGL(sad_raster5gq_kernel, dim3(p.grid()), dim3(p.threads), p.smem, c.st, packed, c.ref, c.rs, c.blocks, c.nblocks, R5G_MAXNB, c.h, c.subShift,
                     c.dx0, c.dy0, c.nx, c.ny, p.rps, p.pitch, p.nstrips, p.inv_strips(), p.total, (int)p.winB, *c.mvHost, c.best);
  return decode_best(c, *c.mvHost);
}

bool raster_block_widths(int w) { return w == 16 || w == 32 || w == 64 || w == 128; }

int try_raster_quad(const SadCall& c, VvcScratch& sc, bool& taken)
{
  R5Plan p;
  taken = c.raster5() && raster_block_widths(c.w) && r5q_plan(c.nblocks, c.w, c.h, c.subShift, c.nx, c.ny, true, p);
  return taken ? launch_r5q(c, p, &sc, nullptr, nullptr, true, true) : VVCGPU_OK;
}

// pair form (r5c): what the quad form leaves, grids wider than 40 columns; a wave item is (column classes c / c + 2, row group)
int try_raster_pair(const SadCall& c, VvcScratch& sc, bool& taken)
{
  R5Plan p;
  taken = c.raster5() && raster_block_widths(c.w) && r5_strip_plan(c.nblocks, c.w, c.h, c.subShift, c.nx, c.ny, p);
  if (!taken) return VVCGPU_OK;
  const int items = 2 * cdiv(p.rps, 6), threads = items >= 8 ? 512 : items * 64;
  p.total = c.nblocks * p.nstrips;
  unsigned* packed = nullptr;
  if (int rc = launch_pack_org(c, &sc, packed, 0, nullptr)) return rc;
  const vvcgpu_mvcost mv = c.mv();
  auto kfn = (p.smem + 1024) * 3 <= 160 * 1024 ? sad_raster5c_kernel<512, 6> : sad_raster5c_kernel<512, 4>;   // three workgroups per CU fit the LDS: six waves per SIMD
  VVC_HIP(vvc_allow_lds(kfn, p.smem));
  hipLaunchKernelGGL(kfn, dim3(p.grid()), dim3(threads), p.smem, c.st, packed, c.ref, c.rs, c.blocks, c.w, c.h, c.subShift, c.dx0, c.dy0, c.nx, c.ny, p.rps,
                     p.pitch, p.nstrips, p.inv_strips(), p.total, (int)p.winB, mv, c.best ? 1 : 0, c.out, c.best);
  return decode_best(c, mv);
}

int launch_generic(const SadCall& c)
{
  VVC_CHECK_ARG(!c.best || (long long)c.nx * c.ny < (1 << 24), "sad_search: the arg-min packs the scan index into 24 bits (nx * ny = %lld)", (long long)c.nx * c.ny);
  const int hs = c.hs();
  const size_t orgDw = ((size_t)hs * (c.w / 2) + 3) & ~(size_t)3;
  // Strip selection: the staged window (one copy, + 2 pairs of slack per row) must fit an LDS budget that keeps three
  // workgroups per CU when possible; among the feasible strip heights pick the one that fills the 512 lanes best
  // (positions x row-split), preferring taller strips (less window re-staging).
  auto pitch_of = [&](int cps) { return ((cps - 1) * c.sx + c.w + 1) / 2 + 3; };
  auto lds_bytes = [&](int rps, int cps) {
    const size_t winRows = (size_t)(rps - 1) * c.sy + c.h;
    return (orgDw + winRows * (size_t)pitch_of(cps)) * 4;
  };
  const size_t budget = 52 * 1024;
  int colsPerStrip = c.nx;
  while (lds_bytes(1, colsPerStrip) > budget && colsPerStrip > 1) colsPerStrip = (colsPerStrip + 1) / 2;
  colsPerStrip = cdiv(c.nx, cdiv(c.nx, colsPerStrip));
  int rowsPerStrip = 1, split = 1;
  double bestUtil = -1.0;
  for (int rps = 1; rps <= c.ny; rps++)
  {
    if (lds_bytes(rps, colsPerStrip) > budget && rps > 1) break;
    const int pos = rps * colsPerStrip;
    int sp = 1;
    if (pos > 128) while (sp < 8 && sp * 2 <= hs && pos * sp * 2 <= SS_THREADS) sp *= 2;   // small strips keep sp = 1 and share the workgroup
    const int tasks = pos * sp;
    const double util = (double)tasks / (double)(cdiv(tasks, SS_THREADS) * SS_THREADS);
    if (util >= bestUtil - 0.02) { bestUtil = util > bestUtil ? util : bestUtil; rowsPerStrip = rps; split = sp; }
  }
  const int pitchDw = pitch_of(colsPerStrip);
  const size_t groupBytes = (lds_bytes(rowsPerStrip, colsPerStrip) + 15) & ~(size_t)15;
  // small windows: several blocks per workgroup (power-of-two groups of >= 64 lanes, each covering all its tasks at once)
  int groups = 1;
  {
    const int tasks = rowsPerStrip * colsPerStrip * split;
    while (groups < 8 && tasks <= SS_THREADS / (groups * 2) && groupBytes * groups * 2 <= 40 * 1024) groups *= 2;
  }
  if (groups > 1 && split == 1)
  {
    // a dense small grid rarely fills the group's lanes in whole passes (81 positions on 128 lanes): let `split` adjacent
    // lanes share a position, each taking every split-th row, when that lowers the lane-row iterations
    const int gszH = SS_THREADS / groups, pos = rowsPerStrip * colsPerStrip;
    long bestCost = (long)cdiv(pos, gszH) * gszH * hs;
    for (int sp = 2; sp <= 8 && sp <= hs && (hs % sp) == 0; sp *= 2)
    {
      const long cost = (long)cdiv(pos * sp, gszH) * gszH * (hs / sp) + (long)pos * sp;      // + the shuffle reduction
      if (cost < bestCost) { bestCost = cost; split = sp; }
    }
  }
  const size_t smem = groupBytes * groups;
  VVC_CHECK_ARG(smem <= SAD_LDS_HARD, "sad_search: a single position's window (%d x %d) does not fit LDS", c.w, c.h);
  VVC_HIP(vvc_allow_lds(sad_search_kernel, smem));
  const vvcgpu_mvcost mv = c.mv();
  if (c.best) VVC_HIP(hipMemsetAsync(c.best, 0xFF, (size_t)c.nblocks * sizeof(vvcgpu_search_best), c.st));
  hipLaunchKernelGGL(sad_search_kernel, dim3(cdiv(c.nblocks, groups), cdiv(c.ny, rowsPerStrip), cdiv(c.nx, colsPerStrip)), dim3(SS_THREADS), smem, c.st,
                     c.org, c.os, c.ref, c.rs, c.blocks, c.nblocks, c.w, c.h, c.subShift, c.dx0, c.dy0, c.nx, c.ny, c.sx, c.sy, rowsPerStrip, colsPerStrip,
                     pitchDw, split, groups, (int)(groupBytes / 4), mv, c.best ? 1 : 0, c.out, c.best);
  return decode_best(c, mv);
}

}  // namespace

extern "C" int vvcgpu_sad_search(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride,
                                 const vvcgpu_search_blk* blocks, int nblocks, int w, int h, int sub_shift,
                                 int dx0, int dy0, int nx, int ny, int sx, int sy, uint32_t* sad_out,
                                 const vvcgpu_mvcost* mvcost_host, vvcgpu_search_best* best, void* stream)
{
  VVC_CHECK_ARG(nblocks >= 0, "sad_search: nblocks %d", nblocks);
  if (nblocks == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org && ref && blocks && (sad_out || best), "sad_search: null pointer");
  VVC_CHECK_ARG(w >= 4 && w <= 128 && (w & 1) == 0 && h >= 4 && h <= 128, "sad_search: block %dx%d unsupported", w, h);
  VVC_CHECK_ARG(sub_shift >= 0 && sub_shift <= 4 && (h >> sub_shift) >= 1 && (h & ((1 << sub_shift) - 1)) == 0,
                "sad_search: sub_shift %d incompatible with height %d", sub_shift, h);
  VVC_CHECK_ARG(nx > 0 && ny > 0 && sx > 0 && sy > 0, "sad_search: bad position grid");
  VVC_CHECK_ARG((best == nullptr) == (mvcost_host == nullptr), "sad_search: best and mvcost must be given together");
  const SadCall c = { org, org_stride, ref, ref_stride, blocks, nblocks, w, h, sub_shift, dx0, dy0, nx, ny, sx, sy, sad_out, mvcost_host, best, (hipStream_t)stream };
  VvcScratch sc(c.st);
  bool taken = false;
  int rc = try_dense9(c, taken);
  if (!taken) rc = try_dense(c, taken);
  if (!taken) rc = try_raster_group(c, sc, taken);
  if (!taken) rc = try_raster_quad(c, sc, taken);
  if (!taken) rc = try_raster_pair(c, sc, taken);
  return taken ? rc : launch_generic(c);
}

// Raster stage of whole-PU TZ searches (tzsearch.hip): the quad raster kernel with per-block grids.  No decode pass: the caller reads the keys.
// packed: the caller's workspace of nblocks * 2 * (h >> sub_shift) * (w / 2) dwords (the per-stream scratch belongs to the caller here)
int vvcgpu_raster_per_block_launch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_search_blk* blocks,
                                   const VvcRasterPer* per, int nblocks, int w, int h, int sub_shift, int nx_max, int ny_max,
                                   const vvcgpu_mvcost* mvcost_host, vvcgpu_search_best* best, unsigned* packed, hipStream_t st0)
{
  VVC_CHECK_ARG((w == 16 || w == 32 || w == 64) && (h & 15) == 0 && h >= 16 && h <= 64 && nx_max >= 1 && nx_max <= 40 && ny_max >= 1 && ny_max <= 40,
                "raster_per_block: %dx%d blocks, %dx%d grid", w, h, nx_max, ny_max);
  VVC_CHECK_ARG((org_stride & 1) == 0 && (ref_stride & 7) == 0 && ((uintptr_t)org & 3) == 0 && ((uintptr_t)ref & 15) == 0, "raster_per_block: alignment");
  VVC_CHECK_ARG((h >> sub_shift) >= 2 && (((h >> sub_shift) * (w >> 4)) & 1) == 0, "raster_per_block: sub_shift %d", sub_shift);
  VVC_CHECK_ARG(packed && best && mvcost_host, "raster_per_block: null pointer");
  const SadCall c = { org, org_stride, ref, ref_stride, blocks, nblocks, w, h, sub_shift, 0, 0, nx_max, ny_max, 5, 5, nullptr, mvcost_host, best, st0 };
  R5Plan p;
  VVC_CHECK_ARG(r5q_plan(nblocks, w, h, sub_shift, nx_max, ny_max, false, p), "raster_per_block: %d blocks do not fit one launch", nblocks);
  return launch_r5q(c, p, nullptr, packed, per, false, false);
}
