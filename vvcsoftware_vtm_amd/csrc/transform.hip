// transform.hip -- 2-D separable integer transforms (T1 forward, T2 inverse, T3 transform skip) for gfx950; the de-quantiser fused in front of the inverse
// transform (vvcgpu_dequant_tr_inv_batch: it reuses the lane-group tables, the int16 matrix loader and the inverse bodies below); and the ONE definition and
// upload of the device tables (transform matrices, coefficient scans, the trellis' position records), whose addresses vvcgpu_tr_tables hands to the kernels
// of the other sources.  The quantisers live in quant.hip, depquant.hip and rdoq.hip, their shared arithmetic in quant_dev.h.
//
// Reference behaviour reproduced (bit-exact): xTrMxN_EMT / xITrMxN_EMT (CommonLib/TrQuant.cpp:138-310) with the 1-D
// stages of TrQuant_EMT.cpp expressed as integer matrix products with the reference's own tables (tr_tables.inc, dumped
// from initROM(); tests/golden/gen_tr_tables.py proves fast transform == table for every slot), intermediate rounding
// `(sum + rnd) >> shift` between the stages (:214-215), inverse stages clipped to [-2^15, 2^15-1] (:253-256), zero-out of
// columns/rows >= 32 (:157-162, :755-759); xTransformSkip / xITransformSkip (:795-847, :1112-1163).
//
// Design: both 1-D stages of a TU run inside one wave with the intermediate in LDS (the reference's alloca'd `tmp`,
// never in HBM); accumulation is exact int32.  A batch is served by two launches:
//   * LARGE TUs (a side of 32 or 64): one wave per TU, lane = row / column, the matrix row of the current output index
//     is wave-uniform (scalar loads); persistent grid-stride waves that skip the other descriptors.
//   * SMALL TUs (both sides <= 16) and transform skip: a 4x4 TU would leave 60 of 64 lanes idle and, worse, a launch
//     of one workgroup per TU is bound by the dispatcher (~1 workgroup/ns chip-wide: 0.5 ms for a 4K picture of 4x4
//     TUs).  Here a 256-thread workgroup takes 64 consecutive descriptors, bins them by max(w, h) in LDS and gives
//     every TU a group of 4 / 8 / 16 lanes (16 / 8 / 4 TUs per wave); the matrices of sizes <= 16 sit in LDS as int32,
//     each lane group reading the rows of its own TU's transform types (same-address reads broadcast).
#include "common.h"
#include "mfma_tr.h"
#include "quant_dev.h"
#include "tr_tables.inc"

// resichain.hip: the chain's bodies as plain transforms (mode 1 forward, 2 inverse): ONE launch with packed matrix-core tiles for long calls
int vvcgpu_tr_chain_launch(int mode, const vvc_pel* resi_in, vvc_pel* resi_out, vvc_coef* coeff, const vvcgpu_tr_desc* descs, int n, int bit_depth, void* stream);

namespace {

// int32 copies of the golden matrices: d_tr32[type][size] row-major (T[k][n]) and d_tr32t (transposed, T[n][k]) so that the
// row a wave needs is always contiguous -> scalar (SGPR) loads.  Layout as VVC_TR_TABLES: size N at (N*N-4)/3.
__device__ int d_tr32[3 * 5460];
__device__ int d_tr32t[3 * 5460];

__device__ __forceinline__ const int* tr32(int type, int n)  { return d_tr32  + type * 5460 + (n * n - 4) / 3; }
__device__ __forceinline__ const int* tr32t(int type, int n) { return d_tr32t + type * 5460 + (n * n - 4) / 3; }

constexpr int MAXN = 64;
// address-space-qualified views: behind a real call a plain pointer is a FLAT pointer -- every LDS access becomes a flat_load / flat_store that the
// compiler can neither batch nor reorder against the global loads beside it (measured: the staging loop alone ran one memory round trip per element)
typedef __attribute__((address_space(3))) int LdsInt;
typedef const __attribute__((address_space(1))) int GlbCInt;
typedef __attribute__((address_space(1))) int GlbInt;
typedef __attribute__((address_space(1))) short GlbPel;

typedef short short2v __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------
// Small TUs (w, h <= 16) and transform skip: 64 descriptors per 256-thread workgroup, binned in LDS.
constexpr int SM_DESCS = 64, SM_TAB = 376;          // per type: size 4 at 0, 8 at 16, 16 at 80, 2 at 336; padded for over-reads
__device__ __forceinline__ int small_off(int n) { return n == 4 ? 0 : n == 8 ? 16 : n == 16 ? 80 : 336; }
struct SmallShared
{
  vvcgpu_tr_desc d[SM_DESCS];
  int tab[3][SM_TAB];                               // T[k][n]   (forward: row = output index)
  int tabT[3][SM_TAB];                              // T^T       (inverse: row = output index)
  int tmp[4][4 * 16 * 17];                          // per wave: P TUs x S x (S+1)
  int cnt[4];                                       // bins: 0 transform skip, 1 S <= 4, 2 S = 8, 3 S = 16
  unsigned char list[4][SM_DESCS];
};

__device__ __forceinline__ void small_tables(SmallShared& sh, int tid)
{
  for (int i = tid; i < 3 * SM_TAB; i += 256)
  {
    const int t = i / SM_TAB, e = i - t * SM_TAB;
    int nsz = 0, o = 0;
    if (e < 16) { nsz = 4; o = e; } else if (e < 80) { nsz = 8; o = e - 16; } else if (e < 336) { nsz = 16; o = e - 80; } else if (e < 340) { nsz = 2; o = e - 336; }
    sh.tab[t][e] = nsz ? tr32(t, nsz)[o] : 0;
    sh.tabT[t][e] = nsz ? tr32t(t, nsz)[o] : 0;
  }
}
// smCnt / smLists (may be null): the small TUs of the call binned on the device (tr_collect_large_kernel): the batch is then a run of the
// concatenated bin lists (lane groups of 16 first), so that a workgroup's TUs share a bin and its lane groups are full -- in the caller's order a real
// encoder's call mix leaves most groups part-filled (profiles/r04_entry_shapes.txt: the mixed batch took 1.5 x the time of its parts)
__device__ __forceinline__ int small_total(const int* __restrict__ smCnt, int n) { return smCnt ? smCnt[0] + smCnt[1] + smCnt[2] + smCnt[3] : n; }
__device__ __forceinline__ void small_setup(SmallShared& sh, const vvcgpu_tr_desc* __restrict__ descs, int n, int batch, int tid, int useMfma,
                                            const int* __restrict__ smCnt = nullptr, const int* __restrict__ smLists = nullptr)
{
  __syncthreads();                                  // tables ready / previous batch done with d, list, cnt
  if (tid < 4) sh.cnt[tid] = 0;
  __syncthreads();
  const int base = batch * SM_DESCS, total = small_total(smCnt, n);
  if (tid < SM_DESCS && base + tid < total)
  {
    int di = base + tid;
    if (smCnt)
    {
      int v = di, b = 3;
#pragma unroll
      for (int k = 3; k > 0; k--) { const int c = smCnt[k]; if (b == k && v >= c) { v -= c; b = k - 1; } }
      di = smLists[(size_t)b * n + v];
    }
    const vvcgpu_tr_desc d = descs[di];
    sh.d[tid] = d;
    const int S = max((int)d.w, (int)d.h);
    int bin = d.tr_hor == 3 ? 0 : S <= 4 ? 1 : S == 8 ? 2 : S == 16 ? 3 : -1;           // -1: large, the other launches
    if (useMfma && bin == 3 && d.w == 16 && d.h == 16) bin = -1;                           // 16 x 16 runs on the matrix cores
    if (bin >= 0) sh.list[bin][atomicAdd(&sh.cnt[bin], 1)] = (unsigned char)tid;
  }
  __syncthreads();
}

#define TR_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

template <int S>
__device__ __forceinline__ void fwd_small_group(SmallShared& sh, int bin, int grp, int lane, int wave, int bd,
                                                const Pel* __restrict__ resiBase, TCoeff* __restrict__ coeffBase)
{
  constexpr int P = 64 / S;
  const int g = lane / S, r = lane % S, li = grp * P + g;
  const bool act = li < sh.cnt[bin];
  const vvcgpu_tr_desc& d = sh.d[sh.list[bin][act ? li : 0]];
  const int w = d.w, h = d.h, lw = ilog2(w), lh = ilog2(h);
  const int s1 = lw + bd + 6 - 15 + 2, s2 = lh + 6 + 2;
  int* tmp = sh.tmp[wave] + g * (S * (S + 1));
  if (act && r < h)                                 // stage 1 (horizontal): lane = row r
  {
    const Pel* row = resiBase + d.resi_off + (size_t)r * d.resi_stride;
    int x[S];
#pragma unroll
    for (int k = 0; k < S; k++) x[k] = k < w ? (int)row[k] : 0;
    const int* T = sh.tab[d.tr_hor] + small_off(w);
    const int rnd = 1 << (s1 - 1);
    for (int j = 0; j < w; j++)
    {
      int sum = 0;
#pragma unroll
      for (int k = 0; k < S; k++) sum += __mul24(x[k], T[j * w + k]);   // k >= w: x[k] = 0, T reads stay inside the padded table
      tmp[j * (S + 1) + r] = (sum + rnd) >> s1;
    }
  }
  TR_WAVE_SYNC();
  if (act && r < w)                                 // stage 2 (vertical): lane = horizontal frequency r
  {
    int t[S];
#pragma unroll
    for (int k = 0; k < S; k++) t[k] = k < h ? tmp[r * (S + 1) + k] : 0;
    const int* T = sh.tab[d.tr_ver] + small_off(h);
    const int rnd = 1 << (s2 - 1);
    TCoeff* coeff = coeffBase + d.coeff_off;
    for (int j = 0; j < h; j++)
    {
      int sum = 0;
#pragma unroll
      for (int k = 0; k < S; k++) sum += __mul24(t[k], T[j * h + k]);
      coeff[j * w + r] = (sum + rnd) >> s2;
    }
  }
  TR_WAVE_SYNC();
}

__global__ __launch_bounds__(256) void tr_fwd_small_kernel(const Pel* __restrict__ resiBase, TCoeff* __restrict__ coeffBase,
                                                           const vvcgpu_tr_desc* __restrict__ descs, int n, int bd, int useMfma,
                                                           const int* __restrict__ smCnt, const int* __restrict__ smLists)
{
  __shared__ SmallShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  small_tables(sh, tid);
  const int total = small_total(smCnt, n);
  for (int batch = blockIdx.x; batch * SM_DESCS < total; batch += gridDim.x)
  {
  small_setup(sh, descs, n, batch, tid, useMfma, smCnt, smLists);
  for (int q = 0; q < sh.cnt[0]; q++)                // transform skip: element-wise, whole workgroup
  {
    const vvcgpu_tr_desc& d = sh.d[sh.list[0][q]];
    const int w = d.w, h = d.h, lw = ilog2(w), lh = ilog2(h);
    int shift = vq_transform_shift(bd, lw, lh), scale = 1;
    if (vq_sqrt2(lw, lh)) { shift -= 8; scale = 181; }
    const Pel* resi = resiBase + d.resi_off;
    TCoeff* coeff = coeffBase + d.coeff_off;
    for (int i = tid; i < w * h; i += 256)
    {
      const int y = i >> lw, x = i & (w - 1);
      const int v = resi[(size_t)y * d.resi_stride + x] * scale;
      coeff[i] = shift >= 0 ? v << shift : (v + (1 << (-shift - 1))) >> -shift;
    }
  }
  for (int g = wave; g * 16 < sh.cnt[1]; g += 4) fwd_small_group<4>(sh, 1, g, lane, wave, bd, resiBase, coeffBase);
  for (int g = wave; g * 8 < sh.cnt[2]; g += 4)  fwd_small_group<8>(sh, 2, g, lane, wave, bd, resiBase, coeffBase);
  for (int g = wave; g * 4 < sh.cnt[3]; g += 4)  fwd_small_group<16>(sh, 3, g, lane, wave, bd, resiBase, coeffBase);
  }
}

template <int S, bool M24>
__device__ __forceinline__ int inv_dot(const int (&c)[S], const int* T)
{
  int sum = 0;
#pragma unroll
  for (int k = 0; k < S; k++) sum += M24 ? __mul24(c[k], T[k]) : c[k] * T[k];
  return sum;
}

template <int S>
__device__ __forceinline__ void inv_small_group(SmallShared& sh, int bin, int grp, int lane, int wave, int bd,
                                                const TCoeff* __restrict__ coeffBase, Pel* __restrict__ resiBase, const int* ldsCoef = nullptr)
{
  constexpr int P = 64 / S;
  const int g = lane / S, r = lane % S, li = grp * P + g;
  const bool act = li < sh.cnt[bin];
  const vvcgpu_tr_desc& d = sh.d[sh.list[bin][act ? li : 0]];
  const int w = d.w, h = d.h;
  const int s2 = (6 + 15 - 1) - bd + 2;
  int* tmp = sh.tmp[wave] + g * (S * (S + 1));
  {                                                 // stage 1 (vertical): lane = column r
    const bool on = act && r < w;
    int c[S];
    const TCoeff* coeff = ldsCoef ? ldsCoef + g * (S * S) : coeffBase + d.coeff_off;     // fused de-quantiser: the group's TUs sit in LDS, S x S ints each
    bool fits = true;
#pragma unroll
    for (int k = 0; k < S; k++) { c[k] = (on && k < h) ? coeff[k * w + r] : 0; fits = fits && (c[k] >= -(1 << 23)) && (c[k] < (1 << 23)); }
    const int* T = sh.tabT[d.tr_ver] + small_off(h);
    // 24-bit multiplies when every coefficient of the wave allows it (always, for quantiser output); exact 32-bit otherwise
    if (__builtin_amdgcn_ballot_w64(!fits) == 0ull)
    {
      if (on) for (int j = 0; j < h; j++) tmp[r * (S + 1) + j] = clip3(-(1 << 15), (1 << 15) - 1, (inv_dot<S, true>(c, T + j * h) + 256) >> 9);
    }
    else
    {
      if (on) for (int j = 0; j < h; j++) tmp[r * (S + 1) + j] = clip3(-(1 << 15), (1 << 15) - 1, (inv_dot<S, false>(c, T + j * h) + 256) >> 9);
    }
  }
  TR_WAVE_SYNC();
  if (act && r < h)                                 // stage 2 (horizontal): lane = row r; tmp is clipped to 16 bits -> 24-bit multiplies
  {
    int t[S];
#pragma unroll
    for (int k = 0; k < S; k++) t[k] = k < w ? tmp[k * (S + 1) + r] : 0;
    const int* T = sh.tabT[d.tr_hor] + small_off(w);
    const int rnd = 1 << (s2 - 1);
    Pel* row = resiBase + d.resi_off + (size_t)r * d.resi_stride;
    for (int j = 0; j < w; j++) row[j] = (short)clip3(-(1 << 15), (1 << 15) - 1, (inv_dot<S, true>(t, T + j * w) + rnd) >> s2);
  }
  TR_WAVE_SYNC();
}

__global__ __launch_bounds__(256) void tr_inv_small_kernel(const TCoeff* __restrict__ coeffBase, Pel* __restrict__ resiBase,
                                                           const vvcgpu_tr_desc* __restrict__ descs, int n, int bd, int useMfma,
                                                           const int* __restrict__ smCnt, const int* __restrict__ smLists)
{
  __shared__ SmallShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  small_tables(sh, tid);
  const int total = small_total(smCnt, n);
  for (int batch = blockIdx.x; batch * SM_DESCS < total; batch += gridDim.x)
  {
  small_setup(sh, descs, n, batch, tid, useMfma, smCnt, smLists);
  for (int q = 0; q < sh.cnt[0]; q++)
  {
    const vvcgpu_tr_desc& d = sh.d[sh.list[0][q]];
    const int w = d.w, h = d.h, lw = ilog2(w), lh = ilog2(h);
    int shift = vq_transform_shift(bd, lw, lh), scale = 1;
    if (vq_sqrt2(lw, lh)) { shift += 7; scale = 181; }
    const TCoeff* coeff = coeffBase + d.coeff_off;
    Pel* resi = resiBase + d.resi_off;
    for (int i = tid; i < w * h; i += 256)
    {
      const int y = i >> lw, x = i & (w - 1);
      const int c = coeff[i] * scale;
      resi[(size_t)y * d.resi_stride + x] = (short)(shift >= 0 ? (c + (shift ? 1 << (shift - 1) : 0)) >> shift : c << -shift);
    }
  }
  for (int g = wave; g * 16 < sh.cnt[1]; g += 4) inv_small_group<4>(sh, 1, g, lane, wave, bd, coeffBase, resiBase);
  for (int g = wave; g * 8 < sh.cnt[2]; g += 4)  inv_small_group<8>(sh, 2, g, lane, wave, bd, coeffBase, resiBase);
  for (int g = wave; g * 4 < sh.cnt[3]; g += 4)  inv_small_group<16>(sh, 3, g, lane, wave, bd, coeffBase, resiBase);
  }
}

// ---------------------------------------------------------------------------------------------------
// Large TUs, fast path: 256-thread persistent workgroups, one wave per TU; every matrix (int16, 16-byte aligned rows)
// resident in LDS, 16-bit operands packed in pairs and multiplied with v_dot2_i32_i16 (two exact MACs per instruction),
// the matrix row of the current output index read with broadcast 16-byte LDS loads.  When a dimension has fewer than
// 64 rows / columns the idle lanes take a share of the output indices.  Operands that do not fit 16 bits (never the
// case for residuals / quantiser output) and odd row addresses fall back to the scalar-load stages above.
constexpr int LG_TYPE = 1368;                       // shorts per type: size 2 at 0, 4 at 8, 8 at 24, 16 at 88, 32 at 344
constexpr int LG_TAB = 3 * LG_TYPE + 4096;          // + DCT-II 64 at 3 * LG_TYPE
__device__ __forceinline__ int lg_off(int type, int n)
{
  return n == 64 ? 3 * LG_TYPE : type * LG_TYPE + (n == 2 ? 0 : n == 4 ? 8 : n == 8 ? 24 : n == 16 ? 88 : 344);
}
__device__ __forceinline__ void lg_load(short* tab, const int* __restrict__ src32, int tid)
{
  for (int t = 0; t < 3; t++)
    for (int n = 2; n <= 32; n <<= 1)
      for (int e = tid; e < n * n; e += 256) tab[lg_off(t, n) + e] = (short)src32[t * 5460 + (n * n - 4) / 3 + e];
  for (int e = tid; e < 4096; e += 256) tab[3 * LG_TYPE + e] = (short)src32[1364 + e];
}

// sum_k a[k] * T[k], k < N, a packed in pairs, T = LDS row of int16 (wave-uniform or per lane group)
template <int N>
__device__ __forceinline__ int dot_row(const unsigned (&ap)[(N + 1) / 2], const short* T)
{
  int sum = 0;
  if (N >= 8)
  {
    const uint4* tr = reinterpret_cast<const uint4*>(T);
#pragma unroll
    for (int q = 0; q < N / 8; q++)
    {
      const uint4 t = tr[q];
      sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, ap[4 * q]), __builtin_bit_cast(short2v, t.x), sum, false);
      sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, ap[4 * q + 1]), __builtin_bit_cast(short2v, t.y), sum, false);
      sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, ap[4 * q + 2]), __builtin_bit_cast(short2v, t.z), sum, false);
      sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, ap[4 * q + 3]), __builtin_bit_cast(short2v, t.w), sum, false);
    }
  }
  else
  {
    const unsigned* tr = reinterpret_cast<const unsigned*>(T);
#pragma unroll
    for (int q = 0; q < N / 2; q++) sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, ap[q]), __builtin_bit_cast(short2v, tr[q]), sum, false);
  }
  return sum;
}
__device__ __forceinline__ unsigned pack16(int lo, int hi) { return ((unsigned)lo & 0xFFFFu) | ((unsigned)hi << 16); }
__device__ __forceinline__ bool fits16(int v) { return v == (int)(short)v; }

// forward stage 1: lane = row; returns (wave-uniform) whether every intermediate fits 16 bits
template <int W>
__device__ __forceinline__ bool fwd_stage1_fast(const Pel* __restrict__ resi, int stride, int h, int lane, int s1, const short* T,
                                                int* __restrict__ tmpL, int ph)
{
  constexpr int WJ = W > 32 ? 32 : W;
  bool ok = true;
  if (lane < h)
  {
    const unsigned* row = reinterpret_cast<const unsigned*>(resi + (size_t)lane * stride);
    unsigned xp[W / 2];
#pragma unroll
    for (int m = 0; m < W / 2; m++) xp[m] = row[m];
    const int rnd = 1 << (s1 - 1);
#pragma unroll 2
    for (int j = 0; j < WJ; j++)
    {
      const int v = (dot_row<W>(xp, T + j * W) + rnd) >> s1;
      tmpL[j * ph + lane] = v;
      ok = ok && fits16(v);
    }
  }
  return __builtin_amdgcn_ballot_w64(!ok) == 0ull;
}
// forward stage 2: lane = (horizontal frequency i < wj, share g of the output rows)
template <int H>
__device__ __forceinline__ void fwd_stage2_fast(const int* __restrict__ tmpL, int ph, int w, int wj, int lane, int s2, const short* T,
                                                TCoeff* __restrict__ coeff)
{
  constexpr int HJ = H > 32 ? 32 : H;
  const int i = lane & (wj - 1), g = lane / wj, G = 64 / wj, jPer = HJ / G;     // wj < 32 only with h >= 32: HJ = 32 >= G
  unsigned tp[H / 2];
#pragma unroll
  for (int m = 0; m < H / 2; m++) tp[m] = pack16(tmpL[i * ph + 2 * m], tmpL[i * ph + 2 * m + 1]);
  const int rnd = 1 << (s2 - 1);
#pragma unroll 2
  for (int jj = 0; jj < jPer; jj++)
  {
    const int j = g * jPer + jj;
    coeff[j * w + i] = (dot_row<H>(tp, T + j * H) + rnd) >> s2;
  }
}
// Slow generic stages for the cases the packed 16-bit path cannot take (rows at odd addresses, operands beyond 16 bits:
// neither occurs for encoder residuals / quantiser output).  Plain loops, exact 32-bit arithmetic, no register arrays.
__device__ __noinline__ void fwd_stage1_slow(const Pel* __restrict__ resi, int stride, int w, int h, int lane, int wj, int s1,
                                             const short* T, int* __restrict__ tmpL, int ph)
{
  if (lane >= h) return;
  const Pel* row = resi + (size_t)lane * stride;
  const int rnd = 1 << (s1 - 1);
#pragma unroll 1
  for (int j = 0; j < wj; j++)
  {
    int sum = 0;
#pragma unroll 1
    for (int k = 0; k < w; k++) sum += (int)row[k] * (int)T[j * w + k];
    tmpL[j * ph + lane] = (sum + rnd) >> s1;
  }
}
__device__ __noinline__ void fwd_stage2_slow(const int* __restrict__ tmpL, int ph, int w, int h, int wj, int hj, int lane, int s2,
                                             const short* T, TCoeff* __restrict__ coeff)
{
  if (lane >= w) return;
  const int rnd = 1 << (s2 - 1);
#pragma unroll 1
  for (int j = 0; j < h; j++)
  {
    int v = 0;
    if (lane < wj && j < hj)
    {
      int sum = 0;
#pragma unroll 1
      for (int k = 0; k < h; k++) sum += tmpL[lane * ph + k] * (int)T[j * h + k];
      v = (sum + rnd) >> s2;
    }
    coeff[j * w + lane] = v;
  }
}
__device__ __noinline__ void inv_stage1_slow(const TCoeff* __restrict__ coeff, int w, int h, int wj, int hj, int lane, const short* TT,
                                             int* __restrict__ tmpL, int ph)
{
  if (lane >= wj) return;
#pragma unroll 1
  for (int j = 0; j < h; j++)
  {
    int sum = 0;
#pragma unroll 1
    for (int k = 0; k < hj; k++) sum += coeff[k * w + lane] * (int)TT[j * h + k];
    tmpL[lane * ph + j] = clip3(-(1 << 15), (1 << 15) - 1, (sum + 256) >> 9);
  }
}

template <int W>
__device__ __forceinline__ void fwd_tu_large(const vvcgpu_tr_desc& d, const Pel* resi, TCoeff* coeff, int bd, int lane, int* tmpL,
                                             const short* tab)
{
  const int h = d.h, lw = ilog2(W), lh = ilog2(h);
  const int s1 = lw + bd + 6 - 15 + 2, s2 = lh + 6 + 2;
  const int wj = W > 32 ? 32 : W, hj = h > 32 ? 32 : h;
  const int ph = h + 1;
  const bool aligned = (((uintptr_t)resi | (uintptr_t)(d.resi_stride * 2)) & 3) == 0;
  bool fast = false;
  if (aligned) fast = fwd_stage1_fast<W>(resi, d.resi_stride, h, lane, s1, tab + lg_off(d.tr_hor, W), tmpL, ph);
  else fwd_stage1_slow(resi, d.resi_stride, W, h, lane, wj, s1, tab + lg_off(d.tr_hor, W), tmpL, ph);
  TR_WAVE_SYNC();
  if (fast)
  {
    const short* Tv = tab + lg_off(d.tr_ver, h);
    switch (h)
    {
    case 2:  fwd_stage2_fast<2>(tmpL, ph, W, wj, lane, s2, Tv, coeff); break;
    case 4:  fwd_stage2_fast<4>(tmpL, ph, W, wj, lane, s2, Tv, coeff); break;
    case 8:  fwd_stage2_fast<8>(tmpL, ph, W, wj, lane, s2, Tv, coeff); break;
    case 16: fwd_stage2_fast<16>(tmpL, ph, W, wj, lane, s2, Tv, coeff); break;
    case 32: fwd_stage2_fast<32>(tmpL, ph, W, wj, lane, s2, Tv, coeff); break;
    default: fwd_stage2_fast<64>(tmpL, ph, W, wj, lane, s2, Tv, coeff); break;
    }
    // zero-out: rows >= hj (contiguous) and columns >= wj of the kept rows
    for (int e = hj * W + lane; e < h * W; e += 64) coeff[e] = 0;
    if (W > 32) for (int e = lane; e < hj * 32; e += 64) coeff[(e >> 5) * W + 32 + (e & 31)] = 0;
  }
  else fwd_stage2_slow(tmpL, ph, W, h, wj, hj, lane, s2, tab + lg_off(d.tr_ver, h), coeff);
  TR_WAVE_SYNC();
}

__global__ __launch_bounds__(256, 3) void tr_fwd_large_kernel(const Pel* __restrict__ resiBase, TCoeff* __restrict__ coeffBase,
                                                           const vvcgpu_tr_desc* __restrict__ descs, const int* __restrict__ list, int bd)
{
  __shared__ __align__(16) short tab[LG_TAB];
  __shared__ int tmpAll[4][32 * (MAXN + 1)];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cnt = list[0];
  if ((int)blockIdx.x * 4 >= cnt) return;
  lg_load(tab, d_tr32, tid);
  __syncthreads();
  int* tmpL = tmpAll[wave];
  for (int k = blockIdx.x * 4 + wave; k < cnt; k += gridDim.x * 4)
  {
    const vvcgpu_tr_desc d = descs[__builtin_amdgcn_readfirstlane(list[1 + k])];
    const Pel* resi = resiBase + d.resi_off;
    TCoeff* coeff = coeffBase + d.coeff_off;
    switch (d.w)
    {
    case 2:  fwd_tu_large<2>(d, resi, coeff, bd, lane, tmpL, tab); break;
    case 4:  fwd_tu_large<4>(d, resi, coeff, bd, lane, tmpL, tab); break;
    case 8:  fwd_tu_large<8>(d, resi, coeff, bd, lane, tmpL, tab); break;
    case 16: fwd_tu_large<16>(d, resi, coeff, bd, lane, tmpL, tab); break;
    case 32: fwd_tu_large<32>(d, resi, coeff, bd, lane, tmpL, tab); break;
    default: fwd_tu_large<64>(d, resi, coeff, bd, lane, tmpL, tab); break;
    }
  }
}

// inverse stage 1 (vertical): lane = (kept column i < wj, share g of the output rows); false when a coefficient needs > 16 bits
template <int H>
__device__ __forceinline__ bool inv_stage1_fast(const TCoeff* __restrict__ coeff, int w, int wj, int lane, const short* TT,
                                                int* __restrict__ tmpL, int ph)
{
  constexpr int HJ = H > 32 ? 32 : H;
  const int i = lane & (wj - 1), g = lane / wj, G = 64 / wj, jPer = H / G;
  int c[HJ];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < HJ; k++) { c[k] = coeff[k * w + i]; ok = ok && fits16(c[k]); }
  if (__builtin_amdgcn_ballot_w64(!ok) != 0ull) return false;
  unsigned cp[(HJ + 1) / 2];
#pragma unroll
  for (int m = 0; m < HJ / 2; m++) cp[m] = pack16(c[2 * m], c[2 * m + 1]);
#pragma unroll 2
  for (int jj = 0; jj < jPer; jj++)
  {
    const int j = g * jPer + jj;
    tmpL[i * ph + j] = clip3(-(1 << 15), (1 << 15) - 1, (dot_row<HJ>(cp, TT + j * H) + 256) >> 9);
  }
  return true;
}
// inverse stage 2 (horizontal): lane = (row r < h, share g of the output columns); tmp is clipped to 16 bits by stage 1
template <int W>
__device__ __forceinline__ void inv_stage2_fast(const int* __restrict__ tmpL, int ph, int h, int lane, int s2, const short* TT,
                                                Pel* __restrict__ resi, int stride)
{
  constexpr int WJ = W > 32 ? 32 : W;
  const int r = lane & (h - 1), g = lane / h, G = 64 / h, jPer = W / G;
  unsigned tp[(WJ + 1) / 2];
#pragma unroll
  for (int m = 0; m < WJ / 2; m++) tp[m] = pack16(tmpL[(2 * m) * ph + r], tmpL[(2 * m + 1) * ph + r]);
  const int rnd = 1 << (s2 - 1);
  Pel* row = resi + (size_t)r * stride;
#pragma unroll 2
  for (int jj = 0; jj < jPer; jj++)
  {
    const int j = g * jPer + jj;
    row[j] = (short)clip3(-(1 << 15), (1 << 15) - 1, (dot_row<WJ>(tp, TT + j * W) + rnd) >> s2);
  }
}
template <int W>
__device__ __forceinline__ void inv_tu_large(const vvcgpu_tr_desc& d, const TCoeff* coeff, Pel* resi, int bd, int lane, int* tmpL,
                                             const short* tabT, int pitch = W)            // pitch: row pitch of `coeff` (the fused de-quantiser keeps wj)
{
  const int h = d.h;
  const int s2 = (6 + 15 - 1) - bd + 2;
  const int wj = W > 32 ? 32 : W;
  const int ph = h + 1;
  const short* TvT = tabT + lg_off(d.tr_ver, h);
  bool fast;
  switch (h)
  {
  case 2:  fast = inv_stage1_fast<2>(coeff, pitch, wj, lane, TvT, tmpL, ph); break;
  case 4:  fast = inv_stage1_fast<4>(coeff, pitch, wj, lane, TvT, tmpL, ph); break;
  case 8:  fast = inv_stage1_fast<8>(coeff, pitch, wj, lane, TvT, tmpL, ph); break;
  case 16: fast = inv_stage1_fast<16>(coeff, pitch, wj, lane, TvT, tmpL, ph); break;
  case 32: fast = inv_stage1_fast<32>(coeff, pitch, wj, lane, TvT, tmpL, ph); break;
  default: fast = inv_stage1_fast<64>(coeff, pitch, wj, lane, TvT, tmpL, ph); break;
  }
  if (!fast) inv_stage1_slow(coeff, pitch, h, wj, h > 32 ? 32 : h, lane, TvT, tmpL, ph);
  TR_WAVE_SYNC();
  inv_stage2_fast<W>(tmpL, ph, h, lane, s2, tabT + lg_off(d.tr_hor, W), resi, d.resi_stride);
  TR_WAVE_SYNC();
}

__global__ __launch_bounds__(256, 3) void tr_inv_large_kernel(const TCoeff* __restrict__ coeffBase, Pel* __restrict__ resiBase,
                                                           const vvcgpu_tr_desc* __restrict__ descs, const int* __restrict__ list, int bd)
{
  __shared__ __align__(16) short tabT[LG_TAB];
  __shared__ int tmpAll[4][32 * (MAXN + 1)];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cnt = list[0];
  if ((int)blockIdx.x * 4 >= cnt) return;
  lg_load(tabT, d_tr32t, tid);
  __syncthreads();
  int* tmpL = tmpAll[wave];
  for (int k = blockIdx.x * 4 + wave; k < cnt; k += gridDim.x * 4)
  {
    const vvcgpu_tr_desc d = descs[__builtin_amdgcn_readfirstlane(list[1 + k])];
    const TCoeff* coeff = coeffBase + d.coeff_off;
    Pel* resi = resiBase + d.resi_off;
    switch (d.w)
    {
    case 2:  inv_tu_large<2>(d, coeff, resi, bd, lane, tmpL, tabT); break;
    case 4:  inv_tu_large<4>(d, coeff, resi, bd, lane, tmpL, tabT); break;
    case 8:  inv_tu_large<8>(d, coeff, resi, bd, lane, tmpL, tabT); break;
    case 16: inv_tu_large<16>(d, coeff, resi, bd, lane, tmpL, tabT); break;
    case 32: inv_tu_large<32>(d, coeff, resi, bd, lane, tmpL, tabT); break;
    default: inv_tu_large<64>(d, coeff, resi, bd, lane, tmpL, tabT); break;
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Large TUs whose sides are both 16, 32 or 64: the stages of mfma_tr.h on the matrix cores, one wave per TU.  A TU the matrix-core form
// cannot take (residual outside +-1023 / a coefficient beyond 16 bits / rows not 16-byte aligned) is appended to the list of the dot2 kernels,
// which run behind this one.
template <int W, int H>
__device__ __forceinline__ bool fwd_tu_mfma(const Pel* __restrict__ resi, int stride, int trHor, int trVer, TCoeff* __restrict__ coeff, int bd, int lane,
                                            const _Float16* tab)
{
  typedef MtShape<W, H> S;
  constexpr int LW = W == 16 ? 4 : W == 32 ? 5 : 6, LH = H == 16 ? 4 : H == 32 ? 5 : 6;
  const int c = lane & 15, g = lane >> 4;
  if ((((uintptr_t)resi | (uintptr_t)((size_t)stride * 2)) & (W == 16 ? 7u : 15u)) != 0) return false;
  h8 x[S::RT][S::XS];
  bool inRange = true;
  if (W == 16)
  {
#pragma unroll
    for (int rt = 0; rt < S::RT; rt++)
    {
      const pel4 v = *reinterpret_cast<const pel4*>(resi + (size_t)(16 * rt + c) * stride + 4 * g);
      _Float16 a[4];
#pragma unroll
      for (int j = 0; j < 4; j++) { inRange = inRange && v[j] >= -1023 && v[j] <= 1023; a[j] = (_Float16)v[j]; }
      x[rt][0] = h8{ a[0], a[1], a[2], a[3], a[0], a[1], a[2], a[3] };
    }
  }
  else
  {
#pragma unroll
    for (int rt = 0; rt < S::RT; rt++)
#pragma unroll
      for (int s = 0; s < S::XS; s++)
      {
        const pel8 v = *reinterpret_cast<const pel8*>(resi + (size_t)(16 * rt + c) * stride + 32 * s + 8 * g);
#pragma unroll
        for (int j = 0; j < 8; j++) { inRange = inRange && v[j] >= -1023 && v[j] <= 1023; x[rt][s][j] = (_Float16)v[j]; }
      }
  }
  if (__builtin_amdgcn_ballot_w64(!inRange) != 0ull) return false;
  const _Float16* Th = tab + rc_tab_off(trHor, W, 0);
  const _Float16* Tv = tab + rc_tab_off(trVer, H, 0);
  const int s1 = LW + bd + 6 - 15 + 2, s2 = LH + 6 + 2;
  int t1[S::JT][S::RT][4];
  mt_fwd1<W, H>(t1, x, Th, s1, c, g);
  int cf[S::IT][S::JT][4];
  mt_fwd2<W, H>(cf, t1, Tv, s2, c, g);
#pragma unroll
  for (int it = 0; it < S::IT; it++)
#pragma unroll
    for (int jt = 0; jt < S::JT; jt++)
#pragma unroll
      for (int r = 0; r < 4; r++) coeff[(16 * it + 4 * g + r) * W + 16 * jt + c] = cf[it][jt][r];
  // zero-out: columns >= 32 of the kept rows, then the rows >= 32 (TrQuant.cpp:157-162)
  const int4v z = { 0, 0, 0, 0 };
  if (W == 64) for (int e = lane; e < S::HJ * 8; e += 64) *reinterpret_cast<int4v*>(coeff + (e >> 3) * 64 + 32 + 4 * (e & 7)) = z;
  if (H == 64) for (int e = lane; e < 32 * W / 4; e += 64) *reinterpret_cast<int4v*>(coeff + 32 * W + 4 * e) = z;
  return true;
}

// coeff: global or LDS, row pitch `pitch`; only the kept region (columns < WJ, rows < HJ) is read
template <int W, int H, class CP>
__device__ __forceinline__ bool inv_tu_mfma(CP coeff, int pitch, Pel* __restrict__ resi, int stride, int trHor, int trVer, int bd, int lane,
                                            const _Float16* tab)
{
  typedef MtShape<W, H> S;
  const int c = lane & 15, g = lane >> 4;
  int cq[S::JT][S::IT][4];
  bool ok = true;
#pragma unroll
  for (int jt = 0; jt < S::JT; jt++)
#pragma unroll
    for (int it = 0; it < S::IT; it++)
#pragma unroll
      for (int r = 0; r < 4; r++) { const int v = coeff[(16 * it + 4 * g + r) * pitch + 16 * jt + c]; ok = ok && fits16(v); cq[jt][it][r] = v; }
  if (__builtin_amdgcn_ballot_w64(!ok) != 0ull) return false;
  const _Float16* ThT = tab + rc_tab_off(trHor, W, 1);
  const _Float16* TvT = tab + rc_tab_off(trVer, H, 1);
  int y1[S::RT][S::JT][4];
  mt_inv1<W, H>(y1, cq, TvT, c, g);
  const int s2 = (6 + 15 - 1) - bd + 2;
  const bool aligned = (((uintptr_t)resi | (uintptr_t)((size_t)stride * 2)) & 7u) == 0;
  mt_inv2<W, H>(y1, ThT, s2, c, g, [&](int rt, int xt, const int (&v)[4])
  {
    Pel* dst = resi + (size_t)(16 * rt + c) * stride + 16 * xt + 4 * g;
    if (aligned) *reinterpret_cast<pel4*>(dst) = pel4{ (short)v[0], (short)v[1], (short)v[2], (short)v[3] };
    else
    {
#pragma unroll
      for (int r = 0; r < 4; r++) dst[r] = (short)v[r];
    }
  });
  return true;
}

// shapes of the matrix-core forms: both sides in {16, 32, 64}
__device__ __forceinline__ bool is_mfma_shape(int w, int h) { return (w == 16 || w == 32 || w == 64) && (h == 16 || h == 32 || h == 64); }

#define TR_MFMA_SHAPES(X) X(64, 64) X(64, 32) X(32, 64) X(32, 32) X(64, 16) X(16, 64) X(32, 16) X(16, 32) X(16, 16)

// lists: mfmaCount[0] TUs at mfmaList[0 ..]; failures are appended to large[1 + large[0]++]
__global__ __launch_bounds__(256, 2) void tr_fwd_mfma_kernel(const Pel* __restrict__ resiBase, TCoeff* __restrict__ coeffBase,
                                                             const vvcgpu_tr_desc* __restrict__ descs, const int* __restrict__ mfmaCount,
                                                             const int* __restrict__ mfmaList, int* __restrict__ large, int bd,
                                                             const _Float16* __restrict__ image)
{
  __shared__ __align__(16) _Float16 tab[RC_TAB_HALVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int cnt = mfmaCount[0];
  if ((int)blockIdx.x * 4 >= cnt) return;
  rc_load_all_tables(tab, image, tid);
  __syncthreads();
  for (int k = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(tid >> 6); k < cnt; k += gridDim.x * 4)   // wave-uniform for the compiler: list entry and descriptor through the scalar cache
  {
    const int ti = __builtin_amdgcn_readfirstlane(mfmaList[k]);
    const vvcgpu_tr_desc d = descs[ti];
    const Pel* resi = resiBase + d.resi_off;
    TCoeff* coeff = coeffBase + d.coeff_off;
    bool done = false;
#define X(W_, H_) if (d.w == W_ && d.h == H_) done = fwd_tu_mfma<W_, H_>(resi, d.resi_stride, d.tr_hor, d.tr_ver, coeff, bd, lane, tab);
    TR_MFMA_SHAPES(X)
#undef X
    if (!done && lane == 0) large[1 + atomicAdd(&large[0], 1)] = ti;
  }
}
__global__ __launch_bounds__(256, 2) void tr_inv_mfma_kernel(const TCoeff* __restrict__ coeffBase, Pel* __restrict__ resiBase,
                                                             const vvcgpu_tr_desc* __restrict__ descs, const int* __restrict__ mfmaCount,
                                                             const int* __restrict__ mfmaList, int* __restrict__ large, int bd,
                                                             const _Float16* __restrict__ image)
{
  __shared__ __align__(16) _Float16 tab[RC_TAB_HALVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int cnt = mfmaCount[0];
  if ((int)blockIdx.x * 4 >= cnt) return;
  rc_load_all_tables(tab, image, tid);
  __syncthreads();
  for (int k = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(tid >> 6); k < cnt; k += gridDim.x * 4)   // wave-uniform for the compiler: list entry and descriptor through the scalar cache
  {
    const int ti = __builtin_amdgcn_readfirstlane(mfmaList[k]);
    const vvcgpu_tr_desc d = descs[ti];
    const TCoeff* coeff = coeffBase + d.coeff_off;
    Pel* resi = resiBase + d.resi_off;
    bool done = false;
#define X(W_, H_) if (d.w == W_ && d.h == H_) done = inv_tu_mfma<W_, H_>((GlbCInt*)coeff, W_, resi, d.resi_stride, d.tr_hor, d.tr_ver, bd, lane, tab);
    TR_MFMA_SHAPES(X)
#undef X
    if (!done && lane == 0) large[1 + atomicAdd(&large[0], 1)] = ti;
  }
}

// indices of the large TUs of a batch, in two lists (order irrelevant: TUs are independent): ws[0] = count of the matrix-core list (entries at
// ws[2 + n ..]), ws[1] = count of the dot2 list (entries at ws[2 ..]: `large` = ws + 1 is a count followed by its entries)
// (same-address device atomics retire at ~12 ns each: one per wave made this kernel 35 us for 137 k descriptors; here a 1024-thread workgroup
// aggregates its 16 waves in LDS and reserves its range of each list with ONE atomic)
// smCnt / smLists (long calls only, else null): the small TUs as well, one list per bin of the small kernels (0 transform skip, 1 S <= 4, 2 S = 8,
// 3 S = 16); smCnt is a counter set of vvcgpu_counters (nextCnt: the other set, cleared here for the next call on the stream)
__global__ __launch_bounds__(1024) void tr_collect_large_kernel(const vvcgpu_tr_desc* __restrict__ descs, int n, int* __restrict__ ws, int useMfma,
                                                                int* __restrict__ smCnt, int* __restrict__ smLists, int* __restrict__ nextCnt)
{
  if (nextCnt && blockIdx.x == 0 && threadIdx.x < VVC_CTR_INTS) nextCnt[threadIdx.x] = 0;
  __shared__ int wcnt[6][16], gbase[6];
  const int ti = blockIdx.x * 1024 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cat = -1;                                                             // 0 dot2 list, 1 matrix-core list, 2 + bin: small
  if (ti < n)
  {
    const int* f = reinterpret_cast<const int*>(descs + ti) + 5;            // bytes 20..27: w, h, tr_hor, tr_ver
    const int wh = f[0], tt = f[1];
    const int w = (short)(wh & 0xFFFF), h = wh >> 16, S = max(w, h);
    const bool tr = (signed char)(tt & 0xFF) != 3;
    if (tr && useMfma && is_mfma_shape(w, h)) cat = 1;
    else if (tr && (w > 16 || h > 16)) cat = 0;
    else if (smCnt) cat = 2 + (!tr ? 0 : S <= 4 ? 1 : S == 8 ? 2 : 3);
  }
  unsigned long long m[6];
#pragma unroll
  for (int k = 0; k < 6; k++) { m[k] = __builtin_amdgcn_ballot_w64(cat == k); if (lane == 0) wcnt[k][wave] = (int)__popcll(m[k]); }
  __syncthreads();
  if (threadIdx.x < 6)
  {
    const int k = threadIdx.x;
    int tot = 0;
    for (int q = 0; q < 16; q++) { const int c = wcnt[k][q]; wcnt[k][q] = tot; tot += c; }
    gbase[k] = !tot ? 0 : k < 2 ? atomicAdd(&ws[1 - k], tot) : atomicAdd(&smCnt[k - 2], tot);   // ws[1]: dot2 list, ws[0]: matrix-core list
  }
  __syncthreads();
  if (cat < 0) return;
  const int pos = gbase[cat] + wcnt[cat][wave] + (int)__popcll(m[cat] & ((1ull << lane) - 1ull));
  if (cat == 0) ws[2 + pos] = ti;
  else if (cat == 1) ws[2 + n + pos] = ti;
  else smLists[(size_t)(cat - 2) * n + pos] = ti;
}

// ---------------------------------------------------------------------------------------------------
// The scan tables: defined and uploaded here only (upload_tables); the kernels of the other sources get their addresses as arguments (vvcgpu_tr_tables).
__device__ unsigned short d_scan[15876];            // diagonal 4x4-grouped scans of all W x H in 2..64, [log2 w - 1][log2 h - 1]
__device__ int d_scanOff[36];
__device__ unsigned short d_dqInv[15876];           // raster position -> scan id, same layout as d_scan
// What a position record of the trellis (TqRec, depquant.hip) holds that depends on the TU's SHAPE only, per scan id si, for the
// position AFTER si in the walk (scan id max(si - 1, 0)): the byte selectors of its five template neighbours inside the sub-block
// and the word (neighbour positions 5 x 4 bits | sigOff << 20 | gtxOff << 24) for luma (.x) and chroma (.y).
__device__ uint4 d_dqPosSel[15876];
__device__ uint2 d_dqPosMisc[15876];

// ---------------------------------------------------------------------------------------------------
// N1: de-quantisation in front of the inverse transform (vvcgpu_dequant_tr_inv_batch).
//   Quant::dequant (Quant.cpp:277-428, flat scaling): an element-wise map (vq_dequant_one, quant_dev.h).
//   Dependent quantisation (DepQuant.cpp:708-785): the reconstruction level of a coefficient depends on a 4-state
//   machine driven by the parities of the levels before it in (reverse) scan order (dq_group below).

// ---------------------------------------------------------------------------------------------------
// N1 in ONE launch: de-quantiser and inverse transform of a TU in the same wave, the de-quantised coefficients in LDS (a separate form
// wrote them to a workspace in HBM and read them back in a second and third launch).  A workgroup takes `per` consecutive descriptors and serves
// them in phases: transform skip and the lane-group sizes (<= 16), then the matrix-core shapes, then the remaining large shapes; the tables of
// the phases share one LDS region and are reloaded only when a workgroup's phase changes (homogeneous batches: never).
struct DqP
{
  int dep, shift;
  VqInv flat;                                                // the scalar de-quantiser (dep == 0)
  long long invQScale, add;                                  // dependent quantisation: scale and shift of qp + 1 with one more bit (DepQuant.cpp:758-759)
};
__device__ __forceinline__ DqP dq_params(const vvcgpu_dqtr_desc& d, int bd, int lw, int lh)
{
  DqP q;
  const int transformShift = vq_transform_shift(bd, lw, lh);
  const bool sqrt2 = vq_sqrt2(lw, lh);
  q.dep = d.dep_quant;
  q.flat = vq_inv(d.qp, transformShift, sqrt2);
  const VqInv dep = vq_inv(d.qp + 1, transformShift, sqrt2);
  int shift = dep.rightShift + 1;
  long long s = dep.scale;
  if (shift < 0) { s <<= -shift; shift = 0; }
  q.invQScale = s; q.shift = shift; q.add = (1ll << shift) >> 1;
  return q;
}

// position of a scan index without the table (host_scan_order below is the definition): coefficient groups of g x g (g = 4, or 2 when a side is 2)
// in up-right diagonal order over the gw x gh grid, the same order inside a group.  dq_cg: group index -> (gy << 8 | gx).
__device__ __forceinline__ int dq_cg(int c, int gw, int gh)
{
  int D = 0, rem = c;
  for (;;)
  {
    const int len = min(D, gh - 1) - max(0, D - gw + 1) + 1;
    if (rem < len) break;
    rem -= len; D++;
  }
  const int gy = min(D, gh - 1) - rem;
  return (gy << 8) | (D - gy);
}
struct DqScan
{
  int lg, gw, gh, cur, ox, oy;                               // cur: the group (ox, oy) belongs to
  __device__ __forceinline__ void init(int w, int h) { lg = ((w | h) & 3) ? 1 : 2; gw = w >> lg; gh = h >> lg; cur = -1; ox = oy = 0; }
  __device__ __forceinline__ void pos(int s, int& x, int& y)
  {
    const int c = s >> (2 * lg), k = s & ((1 << (2 * lg)) - 1);
    if (c != cur) { const int o = dq_cg(c, gw, gh); cur = c; ox = (o & 255) << lg; oy = (o >> 8) << lg; }
    // in-group offsets of scan position k: 4 x 4: x 0010120123123233, y 0102103210321323; 2 x 2: x 0011, y 0101 (two bits each, k = 0 lowest)
    const unsigned kx = lg == 2 ? 0xFB9E4910u : 0x50u, ky = lg == 2 ? 0xEDB1B184u : 0x44u;
    x = ox + (int)((kx >> (2 * k)) & 3); y = oy + (int)((ky >> (2 * k)) & 3);
  }
};

// De-quantises one TU with a group of L lanes (L = 4, 8, 16: 64 / L TUs side by side in the wave; L = 64: the whole wave).  lig = lane
// index inside the group; act = the group has a TU (all lanes of the wave must call: the scan uses shuffles).  The levels of the kept region
// (x < wj, y < hj) are first staged in `stage` (LDS, row pitch wj); levels outside it (64-wide / 64-high TUs only) are read from memory.
// `sink(pos, x, y, v)` receives every de-quantised coefficient (pos = raster index y w + x), each exactly once.
template <int L, class Sink>
__device__ __forceinline__ void dq_group(const vvcgpu_dqtr_desc& d, const TCoeff* __restrict__ levelFlat, int bd, int lig, bool act, int* stageFlat, Sink sink)
{
  GlbCInt* level = (GlbCInt*)levelFlat;
  LdsInt* stage = (LdsInt*)stageFlat;
  const int w = act ? d.w : 2, h = act ? d.h : 2, lw = ilog2(w), lh = ilog2(h);
  const int wj = w > 32 ? 32 : w, hj = h > 32 ? 32 : h, lwj = ilog2(wj);
  const int cnt = act ? w * h : 0, kept = act ? wj * hj : 0;
  for (int e0 = lig; e0 < kept; e0 += 16 * L)                // all loads of a pass in flight before the first LDS store
  {
    int v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) { const int e = e0 + u * L; v[u] = e < kept ? level[((e >> lwj) << lw) + (e & (wj - 1))] : 0; }
#pragma unroll
    for (int u = 0; u < 16; u++) { const int e = e0 + u * L; if (e < kept) stage[e] = v[u]; }
  }
  TR_WAVE_SYNC();
  const DqP q = dq_params(d, bd, lw, lh);
  if (!act || !q.dep)
  {
    for (int pos = lig; pos < cnt; pos += L)
    {
      const int y = pos >> lw, x = pos & (w - 1);
      const bool in = x < wj && y < hj;
      const int lv = in ? stage[y * wj + x] : level[pos];
      sink(pos, x, y, vq_dequant_one(q.flat, lv));
    }
  }
  const bool dep = act && q.dep;
  // ---- dependent quantisation.  The 4-state machine (transitions 32040, DepQuant.cpp:782) is LINEAR over GF(2): with the state written as
  // (hi, lo), step t maps it to (parity_t ^ lo, hi).  Entering step t, hi = xor of the parities of the earlier steps of the OTHER step parity
  // (t - 1, t - 3, ...) and lo = xor of those of the same parity (t - 2, t - 4, ...), and only hi enters the reconstruction (state >> 1).  So a
  // lane needs two prefix xors: every lane folds the parities of its own steps by step parity, a ballot + popcount gives the prefix over the
  // lanes of the group, and the second pass reconstructs.  Steps run from the END of the scan (step t = scan index cnt - 1 - t; zero levels above
  // the last significant one leave state 0 untouched, so no search for the last level is needed).
  const bool cg4 = ((w | h) & 3) == 0;
  const int laneId = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const unsigned long long below = ((1ull << lig) - 1ull) << (laneId - lig);      // the lanes of my group in front of me
  const bool fast32 = q.invQScale < (1ll << 14) && q.shift < 30;                     // |2 lv +- 1| < 2^17: the product stays inside 31 bits
  const int scale32 = (int)q.invQScale, add32 = (int)q.add;
  auto recon = [&](int lv, int hi) -> int
  {
    if (lv == 0) return 0;
    const int qIdx = 2 * lv + (lv > 0 ? -hi : hi);
    if (fast32) return min(max((qIdx * scale32 + add32) >> q.shift, -(1 << 15)), (1 << 15) - 1);
    return (int)min(max(((long long)qIdx * q.invQScale + q.add) >> q.shift, -(1ll << 15)), (1ll << 15) - 1);
  };
  if (__builtin_amdgcn_ballot_w64(dep && !cg4) == 0ull)
  {
    // coefficient groups of 4 x 4 (every shape without a side of 2): a lane takes whole groups -- 16 levels in registers, the in-group scan unrolled
    constexpr int rasterOf[16] = { 0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15 };      // scan position k -> y * 4 + x inside the group
    const int nCg = dep ? cnt >> 4 : 0, m = nCg > L ? nCg / L : 1;                              // groups per lane (power of two)
    const int gw = w >> 2, gh = h >> 2;
    auto load16 = [&](int T, int (&r)[16], int& ox, int& oy)
    {
      const int o = dq_cg(nCg - 1 - T, gw, gh);
      ox = (o & 255) << 2; oy = (o >> 8) << 2;
      if (ox < wj && oy < hj)
      {
#pragma unroll
        for (int y = 0; y < 4; y++)
        {
          const int4v v = *reinterpret_cast<const __attribute__((address_space(3))) int4v*>(stage + (oy + y) * wj + ox);
          r[4 * y] = v.x; r[4 * y + 1] = v.y; r[4 * y + 2] = v.z; r[4 * y + 3] = v.w;
        }
      }
      else
      {
#pragma unroll
        for (int i = 0; i < 16; i++) r[i] = level[((oy + (i >> 2)) << lw) + ox + (i & 3)];
      }
    };
    int r[16], ox = 0, oy = 0;
    int a0 = 0, a1 = 0;                                      // xor of the levels at even / odd steps (bit 0 is the parity)
    for (int j = 0; j < m; j++)
    {
      const int T = lig * m + j;
      if (T < nCg)
      {
        load16(T, r, ox, oy);
#pragma unroll
        for (int k = 0; k < 16; k++) { if (k & 1) a0 ^= r[rasterOf[k]]; else a1 ^= r[rasterOf[k]]; }      // step t = 16 T + 15 - k: even for odd k
      }
    }
    const unsigned long long B0 = __builtin_amdgcn_ballot_w64((a0 & 1) != 0), B1 = __builtin_amdgcn_ballot_w64((a1 & 1) != 0);
    int x0 = (int)__popcll(B0 & below) & 1, x1 = (int)__popcll(B1 & below) & 1;
    for (int j = 0; j < m; j++)
    {
      const int T = lig * m + j;
      if (T < nCg)
      {
        if (m > 1) load16(T, r, ox, oy);
#pragma unroll
        for (int k = 15; k >= 0; k--)
        {
          const int i = rasterOf[k], lv = r[i], x = ox + (i & 3), y = oy + (i >> 2);
          const int hi = (k & 1) ? x1 : x0;                 // even step (odd k): xor over the odd steps before it
          sink((y << lw) + x, x, y, recon(lv, hi));
          if (k & 1) x0 ^= lv & 1; else x1 ^= lv & 1;
        }
      }
    }
  }
  else
  {
    // some TU of the wave has a side of 2 (groups of 2 x 2): every TU of the wave goes step by step through the analytic scan
    const bool on = dep;
    const int C = on ? (cnt + L - 1) / L : 0;
    const int t0 = lig * C, t1 = min(t0 + C, on ? cnt : 0);
    DqScan sc;
    sc.init(w, h);
    int a0 = 0, a1 = 0;
    for (int t = t0; t < t1; t++)
    {
      int x, y;
      sc.pos(cnt - 1 - t, x, y);
      const int lv = (x < wj && y < hj) ? stage[y * wj + x] : level[(y << lw) + x];
      if (t & 1) a1 ^= lv; else a0 ^= lv;
    }
    const unsigned long long B0 = __builtin_amdgcn_ballot_w64((a0 & 1) != 0), B1 = __builtin_amdgcn_ballot_w64((a1 & 1) != 0);
    int x0 = (int)__popcll(B0 & below) & 1, x1 = (int)__popcll(B1 & below) & 1;
    for (int t = t0; t < t1; t++)
    {
      int x, y;
      sc.pos(cnt - 1 - t, x, y);
      const int lv = (x < wj && y < hj) ? stage[y * wj + x] : level[(y << lw) + x];
      sink((y << lw) + x, x, y, recon(lv, (t & 1) ? x0 : x1));
      if (t & 1) x1 ^= lv & 1; else x0 ^= lv & 1;
    }
  }
  TR_WAVE_SYNC();
}

constexpr int DQ_UNI = ((LG_TAB * 2 + 15) & ~15) + 4 * 32 * (MAXN + 1) * 4;       // the largest phase: int16 matrices + four wave buffers of the dot2 form
static_assert(DQ_UNI >= (int)sizeof(SmallShared) && DQ_UNI >= RC_TAB_HALVES * 2, "phase region");

template <int S>
__device__ __noinline__ void dq_small_group(SmallShared& sh, int bin, int grp, int lane, int wave, int bd, const TCoeff* __restrict__ levelBase,
                                               Pel* __restrict__ resiBase, TCoeff* __restrict__ coeffOut, int* coefW)
{
  constexpr int P = 64 / S, L = S;
  const int g = lane / S, lig = lane % S, li = grp * P + g;
  const bool act = li < sh.cnt[bin];
  const vvcgpu_dqtr_desc& d = reinterpret_cast<const vvcgpu_dqtr_desc&>(sh.d[sh.list[bin][act ? li : 0]]);
  int* stageF = coefW + g * (S * S);
  LdsInt* stage = (LdsInt*)stageF;
  const int w = d.w;
  GlbInt* out = coeffOut ? (GlbInt*)(coeffOut + d.level_off) : nullptr;
  dq_group<L>(d, levelBase + d.level_off, bd, lig, act, stageF, [&](int pos, int x, int y, int v)
  {
    stage[y * w + x] = v;                                    // w <= 16: the kept region is the TU, pitch w
    if (out) out[pos] = v;
  });
  inv_small_group<S>(sh, bin, grp, lane, wave, bd, nullptr, resiBase, coefW);
}

// shape dispatch of the fused kernel as real calls (inlined into one kernel the eight matrix-core bodies and the six dot2 bodies crash hipcc's simplifycfg)
__device__ __noinline__ bool dq_inv_mfma(int w, int h, const TCoeff* coef, Pel* resi, int stride, int trHor, int trVer, int bd, int lane, const _Float16* ftab)
{
  bool done = false;
#define X(W_, H_) if (w == W_ && h == H_) done = inv_tu_mfma<W_, H_>((const LdsInt*)coef, W_ > 32 ? 32 : W_, resi, stride, trHor, trVer, bd, lane, ftab);
  TR_MFMA_SHAPES(X)
#undef X
  return done;
}
__device__ __noinline__ void dq_inv_large(const vvcgpu_tr_desc& d, const TCoeff* coef, Pel* resi, int bd, int lane, int* tmpL, const short* tabT, int wj)
{
  switch (d.w)
  {
  case 2:  inv_tu_large<2>(d, coef, resi, bd, lane, tmpL, tabT, wj); break;
  case 4:  inv_tu_large<4>(d, coef, resi, bd, lane, tmpL, tabT, wj); break;
  case 8:  inv_tu_large<8>(d, coef, resi, bd, lane, tmpL, tabT, wj); break;
  case 16: inv_tu_large<16>(d, coef, resi, bd, lane, tmpL, tabT, wj); break;
  case 32: inv_tu_large<32>(d, coef, resi, bd, lane, tmpL, tabT, wj); break;
  default: inv_tu_large<64>(d, coef, resi, bd, lane, tmpL, tabT, wj); break;
  }
}

// one TU of each phase as a real call (see above)
__device__ __noinline__ void dq_ts_tu(const vvcgpu_dqtr_desc& d, const TCoeff* __restrict__ levelBase, Pel* __restrict__ resiBase, TCoeff* __restrict__ coeffOut,
                                      int bd, int lane, int* coefW)
{
  const int lw = ilog2(d.w), lh = ilog2(d.h);
  int shift = vq_transform_shift(bd, lw, lh), scale = 1;
  if (vq_sqrt2(lw, lh)) { shift += 7; scale = 181; }
  GlbPel* resi = (GlbPel*)(resiBase + d.resi_off);
  GlbInt* out = coeffOut ? (GlbInt*)(coeffOut + d.level_off) : nullptr;
  const int stride = d.resi_stride;
  dq_group<64>(d, levelBase + d.level_off, bd, lane, true, coefW, [&](int pos, int x, int y, int v)
  {
    if (out) out[pos] = v;
    const int c = v * scale;
    resi[(size_t)y * stride + x] = (short)(shift >= 0 ? (c + (shift ? 1 << (shift - 1) : 0)) >> shift : c << -shift);
  });
}
// de-quantises into coefW (kept region, pitch wj) and, if asked, into coeffOut
__device__ __noinline__ void dq_large_stage(const vvcgpu_dqtr_desc& d, const TCoeff* __restrict__ levelBase, TCoeff* __restrict__ coeffOut, int bd, int lane,
                                            int* coefW)
{
  const int wj = d.w > 32 ? 32 : d.w;
  GlbInt* out = coeffOut ? (GlbInt*)(coeffOut + d.level_off) : nullptr;
  LdsInt* cw = (LdsInt*)coefW;
  dq_group<64>(d, levelBase + d.level_off, bd, lane, true, coefW, [&](int pos, int x, int y, int v)
  {
    if (x < wj && y < 32) cw[y * wj + x] = v;
    if (out) out[pos] = v;
  });
}

// ---- device-side order of a batch for the fused kernel.  A workgroup of dqtr_fused_kernel serves `per` descriptors in up to three phases, each
// with its own tables in the phase region (lane-group tables, f16 matrices, int16 matrices).  In the caller's order -- a real encoder's call mix:
// 85 % of the TUs at most 8 wide, a few 32 / 64 wide ones in every run of 64 -- every workgroup walks ALL phases for a handful of TUs each and
// reloads ~26 KB of matrices per 64 descriptors (more bytes than the TUs themselves): the mixed batch took 2.4 x the time of its parts
// (profiles/r04_chain_shapes.txt).  Here the descriptor INDICES are binned by phase class first (the two-pass scheme of rc_classify_kernel,
// resichain.hip: per-workgroup counts in LDS, one global atomic per class and workgroup); the fused kernel then walks the concatenated class lists,
// heaviest class first, so that a workgroup's descriptors share a phase, lane groups are full and the tables stay.
constexpr int DQC_NCLS = 6, DQC_WGS = 128;                 // classes in list order: 0 dot2 form (large), 1 matrix cores, 2 lane groups of 16, 3 of 8, 4 of 4, 5 transform skip
__device__ __forceinline__ int dqc_class(int w, int h, int trHor, int useMfma)
{
  const int S = max(w, h);
  if (trHor == 3) return 5;
  if (S <= 4) return 4;
  if (S == 8) return 3;
  if (S == 16) return 2;
  return useMfma && is_mfma_shape(w, h) ? 1 : 0;
}
__global__ __launch_bounds__(1024) void dqtr_classify_kernel(const vvcgpu_dqtr_desc* __restrict__ descs, int n, int* __restrict__ hdr, int* __restrict__ lists,
                                                             int* __restrict__ nextHdr, int useMfma)
{
  if (blockIdx.x == 0 && threadIdx.x < VVC_CTR_INTS) nextHdr[threadIdx.x] = 0;         // the header of the NEXT call on this stream (vvcgpu_counters)
  __shared__ int cnt[DQC_NCLS], base[DQC_NCLS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int per = (n + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = min(n, lo + per);
  if (tid < DQC_NCLS) cnt[tid] = 0;
  __syncthreads();
  for (int pass = 0; pass < 2; pass++)
  {
    for (int t0 = lo; t0 < hi; t0 += 1024)
    {
      const int ti = t0 + tid;
      int cls = -1;
      if (ti < hi)
      {
        const vvcgpu_tr_desc& d = reinterpret_cast<const vvcgpu_tr_desc*>(descs)[ti];
        cls = dqc_class(d.w, d.h, d.tr_hor, useMfma);
      }
#pragma unroll
      for (int k = 0; k < DQC_NCLS; k++)
      {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(cls == k);
        if (m == 0ull) continue;
        int b = 0;
        if (lane == 0) b = atomicAdd(&cnt[k], (int)__popcll(m));
        b = __builtin_amdgcn_readfirstlane(b);
        if (pass == 1 && cls == k) lists[(size_t)k * n + base[k] + b + (int)__popcll(m & ((1ull << lane) - 1ull))] = ti;
      }
    }
    __syncthreads();
    if (pass == 0 && tid < DQC_NCLS) { base[tid] = cnt[tid] ? atomicAdd(&hdr[tid], cnt[tid]) : 0; cnt[tid] = 0; }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256, 2) void dqtr_fused_kernel(const TCoeff* __restrict__ levelBase, Pel* __restrict__ resiBase,
                                                            const vvcgpu_dqtr_desc* __restrict__ descs, int n, int per, int bd,
                                                            TCoeff* __restrict__ coeffOut, const _Float16* __restrict__ image, int useMfma,
                                                            const int* __restrict__ hdr, const int* __restrict__ lists)
{
  __shared__ int idxOf[SM_DESCS];                            // descriptor index of the batch's t-th entry (the caller's order when lists == nullptr)
  __shared__ __align__(16) unsigned char uni[DQ_UNI];
  __shared__ __align__(16) int coef[4][1024];                // per wave: the kept region of a large TU / the TUs of a lane-group item
  __shared__ int cntM, cntL, cntS[4];
  __shared__ unsigned char listM[SM_DESCS], listL[SM_DESCS];
  __shared__ unsigned short binOf[SM_DESCS];                 // bin * 64 + position in the bin's list (up to 255: a batch of 64 TUs of bin 3), 0xFFFF: not a lane-group TU
  SmallShared& sh = *reinterpret_cast<SmallShared*>(uni);
  _Float16* ftab = reinterpret_cast<_Float16*>(uni);
  short* tabT = reinterpret_cast<short*>(uni);
  int* tmpAll = reinterpret_cast<int*>(uni + ((LG_TAB * 2 + 15) & ~15));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* coefW = coef[wave];
  int curTab = 0;                                            // 0 nothing, 1 lane-group tables, 2 f16 matrices, 3 int16 matrices (workgroup-uniform)
  // ordered form: a batch is a run of ONE class list, short for the classes whose TUs are long serial jobs of a wave (a workgroup that drew 64
  // large TUs would be the tail of the launch), long for the lane-group classes (16 / 8 / 4 TUs side by side in a wave)
  // (and every class shorter when the whole call would otherwise be fewer than ~1024 batches: idle compute units cost more than part-filled waves)
  int bEnd[DQC_NCLS], cCnt[DQC_NCLS], totalBatches = 0, shr = 0;
#pragma unroll
  for (int c = 0; c < DQC_NCLS; c++) cCnt[c] = lists ? hdr[c] : 0;
  auto pkOf = [&](int c) { return max(4, (c <= 1 ? 8 : c == 5 ? 16 : SM_DESCS) >> shr); };
  for (;; shr++)
  {
    totalBatches = 0;
#pragma unroll
    for (int c = 0; c < DQC_NCLS; c++) { const int pk = pkOf(c); totalBatches += (cCnt[c] + pk - 1) / pk; bEnd[c] = totalBatches; }
    if (totalBatches >= 1024 || shr == 4) break;
  }
  if (!lists) totalBatches = (n + per - 1) / per;
  for (int batch = blockIdx.x; batch < totalBatches; batch += gridDim.x)
  {
    int base = batch * per, count = min(per, n - base), cls = 0;
    if (lists)
    {
      int b0 = 0;
#pragma unroll
      for (int c = 0; c < DQC_NCLS - 1; c++) if (batch >= bEnd[c]) { cls = c + 1; b0 = bEnd[c]; }
      const int pk = pkOf(cls);
      base = (batch - b0) * pk;
      count = min(pk, cCnt[cls] - base);
    }
    __syncthreads();                                         // the previous batch is done with the lists and the phase region
    if (tid < 4) cntS[tid] = 0;
    if (tid == 0) { cntM = 0; cntL = 0; }
    __syncthreads();
    // the descriptor copies and lists of the lane-group phase live in the phase region: only a batch that has such TUs touches it, so a run of
    // large-TU batches keeps its matrices
    if (tid < count)
    {
      const int di = lists ? lists[(size_t)cls * n + base + tid] : base + tid;
      idxOf[tid] = di;
      const vvcgpu_tr_desc d = reinterpret_cast<const vvcgpu_tr_desc*>(descs)[di];
      const int S = max((int)d.w, (int)d.h);
      // 16 x 16 stays with the lane groups here: one tile per wave behind a serial de-quantiser was slower (0.122 vs 0.083 ms at 4K)
      const int bin = d.tr_hor == 3 ? 0 : S <= 4 ? 1 : S == 8 ? 2 : S == 16 ? 3 : -1;
      if (bin >= 0) { const int k = atomicAdd(&cntS[bin], 1); binOf[tid] = (unsigned short)(bin * 64 + k); }
      else
      {
        binOf[tid] = 0xFFFFu;
        if (useMfma && is_mfma_shape(d.w, d.h)) listM[atomicAdd(&cntM, 1)] = (unsigned char)tid;
        else listL[atomicAdd(&cntL, 1)] = (unsigned char)tid;
      }
    }
    __syncthreads();
    const int anySmall = cntS[0] + cntS[1] + cntS[2] + cntS[3];
    if (anySmall)
    {
      if (curTab > 1) { curTab = 0; }                        // the matrices are about to be overwritten
      if (tid < 4) sh.cnt[tid] = cntS[tid];
      if (tid < count && binOf[tid] != 0xFFFFu)
      {
        sh.d[tid] = reinterpret_cast<const vvcgpu_tr_desc*>(descs)[idxOf[tid]];
        sh.list[binOf[tid] >> 6][binOf[tid] & 63] = (unsigned char)tid;
      }
      __syncthreads();
    }
    if (anySmall)
    {
      if (curTab != 1) { small_tables(sh, tid); curTab = 1; __syncthreads(); }
      for (int q = wave; q < sh.cnt[0]; q += 4)              // transform skip: the de-quantised value goes straight through the element-wise inverse
        dq_ts_tu(reinterpret_cast<const vvcgpu_dqtr_desc&>(sh.d[sh.list[0][q]]), levelBase, resiBase, coeffOut, bd, lane, coefW);
      for (int g = wave; g * 16 < sh.cnt[1]; g += 4) dq_small_group<4>(sh, 1, g, lane, wave, bd, levelBase, resiBase, coeffOut, coefW);
      for (int g = wave; g * 8 < sh.cnt[2]; g += 4)  dq_small_group<8>(sh, 2, g, lane, wave, bd, levelBase, resiBase, coeffOut, coefW);
      for (int g = wave; g * 4 < sh.cnt[3]; g += 4)  dq_small_group<16>(sh, 3, g, lane, wave, bd, levelBase, resiBase, coeffOut, coefW);
    }
    if (cntM)
    {
      if (curTab != 2)
      {
        __syncthreads();                                     // the lane-group phase is done with the region
        rc_load_all_tables(ftab, image, tid); curTab = 2;
        __syncthreads();
      }
      for (int q = wave; q < cntM; q += 4)
      {
        const vvcgpu_dqtr_desc d = descs[idxOf[listM[q]]];
        dq_large_stage(d, levelBase, coeffOut, bd, lane, coefW);
        const bool done = dq_inv_mfma(d.w, d.h, coefW, resiBase + d.resi_off, d.resi_stride, d.tr_hor, d.tr_ver, bd, lane, ftab);
        if (!done && lane == 0) listL[atomicAdd(&cntL, 1)] = listM[q];          // a coefficient beyond 16 bits: the dot2 form's exact 32-bit stage takes the TU
        TR_WAVE_SYNC();
      }
    }
    __syncthreads();
    if (cntL)
    {
      if (curTab != 3) { lg_load(tabT, d_tr32t, tid); curTab = 3; __syncthreads(); }
      int* tmpL = tmpAll + wave * (32 * (MAXN + 1));
      for (int q = wave; q < cntL; q += 4)
      {
        const vvcgpu_dqtr_desc dq = descs[idxOf[listL[q]]];
        const vvcgpu_tr_desc& d = reinterpret_cast<const vvcgpu_tr_desc&>(dq);
        dq_large_stage(dq, levelBase, coeffOut, bd, lane, coefW);
        dq_inv_large(d, coefW, resiBase + d.resi_off, bd, lane, tmpL, tabT, d.w > 32 ? 32 : d.w);
      }
    }
  }
}

constexpr int g_smallGrid = 1280;                  // workgroups of the small-TU kernels (swept in round 2)

// diagonal 4x4-grouped coefficient scan (Rom.cpp:357-405): groups of 4x4 (2x2 when a side is 2) visited along the diagonals
// x + y = d from the bottom-left end upwards, the positions inside a group likewise
static void host_scan_order(int w, int h, uint16_t* out)
{
  const int lg = ((w & 3) + (h & 3)) > 0 ? 1 : 2, g = 1 << lg, gwN = w >> lg, ghN = h >> lg;
  int n = 0;
  for (int D = 0; D < gwN + ghN - 1; D++)
    for (int gy = (D < ghN - 1 ? D : ghN - 1); gy >= 0; gy--)
    {
      const int gx = D - gy;
      if (gx >= gwN) continue;
      for (int dd = 0; dd < 2 * g - 1; dd++)
        for (int y = (dd < g - 1 ? dd : g - 1); y >= 0; y--)
        {
          const int x = dd - y;
          if (x < g) out[n++] = (uint16_t)((gy * g + y) * w + gx * g + x);
        }
    }
}

// the golden tables of the current device: uploaded by the first call that needs them (vvcgpu_device_image, without memory of its own)
static int upload_tables(void*, const void*)
{
  static int t32[3 * 5460], t32t[3 * 5460];
  for (int t = 0; t < 3; t++)
    for (int n = 2; n <= 64; n <<= 1)
    {
      const int o = t * 5460 + (n * n - 4) / 3;
      for (int k = 0; k < n; k++)
        for (int j = 0; j < n; j++) { t32[o + k * n + j] = VVC_TR_TABLES[o + k * n + j]; t32t[o + j * n + k] = VVC_TR_TABLES[o + k * n + j]; }
    }
  VVC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_tr32), t32, sizeof(t32)));
  VVC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_tr32t), t32t, sizeof(t32t)));
  static uint16_t scan[15876];
  int off[36], o = 0;
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++) { off[a * 6 + b] = o; host_scan_order(2 << a, 2 << b, scan + o); o += (2 << a) * (2 << b); }
  VVC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_scan), scan, sizeof(scan)));
  VVC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_scanOff), off, sizeof(off)));
  // dependent quantisation: raster -> scan id
  static uint16_t invs[15876];
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++)
    {
      const int N = (2 << a) * (2 << b), o0 = off[a * 6 + b];
      for (int i = 0; i < N; i++) invs[o0 + scan[o0 + i]] = (uint16_t)i;
    }
  // depquant_kernel keeps the ancestry of a trellis path as 32 two-bit entries: the sub-block a template read goes to (right of / below / below-right of the
  // sub-block about to be walked) must lie at most 32 sub-blocks back in the scan from the one that just ended.  True for every shape up to 64x64 (30 for 64x64);
  // checked here so that a larger transform size cannot pass silently.
  for (int a = 1; a < 6; a++)
    for (int b = 1; b < 6; b++)
    {
      const int W = 2 << a, H = 2 << b, o0 = off[a * 6 + b], wS = W >> 2, hS = H >> 2;
      for (int n = 0; n + 1 < wS * hS; n++)                     // n: the sub-block about to be walked, n + 1 the one that just ended
      {
        const int p = scan[o0 + 16 * n], sx = (p % W) >> 2, sy = (p / W) >> 2;
        const int cand[3][2] = { { sx + 1, sy }, { sx, sy + 1 }, { sx + 1, sy + 1 } };
        for (auto& c : cand)
          if (c[0] < wS && c[1] < hS)
          {
            const int j = invs[o0 + (4 * c[1]) * W + 4 * c[0]] >> 4;
            if (j - (n + 1) - 1 > 31) { vvcgpu_set_error("depquant tables: a template reaches %d sub-blocks back in a %dx%d TU", j - n - 2, W, H); return VVCGPU_E_UNSUPPORTED; }
          }
      }
    }
  // the shape-only part of the trellis' position records (depquant_kernel, fillRec)
  static uint4 psel[15876];
  static uint2 pmisc[15876];
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++)
    {
      const int W = 2 << a, H = 2 << b, N = W * H, o0 = off[a * 6 + b];
      for (int si = 0; si < N; si++)
      {
        const int sn = si > 0 ? si - 1 : 0, p2 = scan[o0 + sn], x2 = p2 % W, y2 = p2 / W, beg = sn & ~15;
        const int cx[5] = { x2 + 1, x2 + 2, x2 + 1, x2, x2 }, cy[5] = { y2, y2, y2 + 1, y2 + 1, y2 + 2 };
        unsigned nb = 0, selLo[2] = { 0x0C0C0C0Cu, 0x0C0C0C0Cu }, selHi[2] = { 0x0C0C0C0Cu, 0x0C0C0C0Cu };
        for (int t = 0; t < 5; t++)
        {
          const int r = (cx[t] < W && cy[t] < H) ? (int)invs[o0 + cy[t] * W + cx[t]] - beg : 0;
          const unsigned rel = (r > 0 && r < 16) ? (unsigned)r : 0u, sh = (unsigned)(t & 3) * 8u, m = 0xFFu << sh;
          nb |= rel << (4 * t);
          if (rel != 0u && rel < 8u) selLo[t >> 2] = (selLo[t >> 2] & ~m) | (rel << sh);
          if (rel >= 8u) selHi[t >> 2] = (selHi[t >> 2] & ~m) | ((rel - 8u) << sh);
        }
        const int diag = x2 + y2;
        const unsigned sigL = diag < 2 ? 12 : diag < 5 ? 6 : 0, sigC = diag < 2 ? 6 : 0;
        const unsigned gtxL = diag < 1 ? 16 : diag < 3 ? 11 : diag < 10 ? 6 : 1, gtxC = diag < 1 ? 6 : 1;
        psel[o0 + si] = make_uint4(selLo[0], selHi[0], selLo[1], selHi[1]);
        pmisc[o0 + si] = make_uint2(nb | sigL << 20 | gtxL << 24, nb | sigC << 20 | gtxC << 24);
      }
    }
  VVC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_dqPosSel), psel, sizeof(psel)));
  VVC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_dqPosMisc), pmisc, sizeof(pmisc)));
  VVC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_dqInv), invs, sizeof(invs)));
  return VVCGPU_OK;
}
// VVCGPU_NO_MFMA=1 (common.h) keeps every large TU on the dot2 kernels
static int tr_use_mfma() { return vvcgpu_no_mfma() ? 0 : 1; }

// argument checks of the three entries below.  *empty: the call has no descriptors and is done (VVCGPU_OK)
static int check_descs_args(const void* a, const void* b, const void* d, int n, int bd, const char* who, bool* empty)
{
  *empty = n == 0;
  VVC_CHECK_ARG(n >= 0, "%s: n %d", who, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(a && b && d, "%s: null pointer", who);
  if (bd < 8 || bd > 10) { vvcgpu_set_error("%s: bit depth %d outside 8..10", who, bd); return VVCGPU_E_UNSUPPORTED; }
  return VVCGPU_OK;
}

// A plain transform call as lists on the device and three kernels that walk them: in -> out is residual -> coefficients (forward) or the reverse
template <class In, class Out, class SmallK, class MfmaK, class LargeK>
static int tr_launch_lists(SmallK smallK, MfmaK mfmaK, LargeK largeK, const In* in, Out* out, const vvcgpu_tr_desc* descs, int n, int bit_depth,
                           const _Float16* image, hipStream_t st)
{
  // long calls: the small TUs are binned on the device as well and the small kernel walks the bin lists (see small_setup)
  const bool ordered = n >= 16384;
  VvcScratch sc(st);
  int* ws = sc.take<int>(2 + 2 * (size_t)n);                                // two counters, then the lists of dot2 and matrix-core TUs
  int* smLists = ordered ? sc.take<int>(4 * (size_t)n) : nullptr;           // the bins of the small TUs
  if (!ws || (ordered && !smLists)) return VVCGPU_E_DEVICE;
  VVC_HIP(hipMemsetAsync(ws, 0, 2 * sizeof(int), st));
  int* smCnt = nullptr; int* nextCnt = nullptr;
  if (ordered)
  {
    int cur = 0;
    int* counters = vvcgpu_counters(st, &cur);
    if (!counters) return VVCGPU_E_DEVICE;
    smCnt = counters + VVC_CTR_INTS * cur; nextCnt = counters + VVC_CTR_INTS * (cur ^ 1);
  }
  const int nb = cdiv(n, SM_DESCS), nl = cdiv(n, 4);
  hipLaunchKernelGGL(tr_collect_large_kernel, dim3(cdiv(n, 1024)), dim3(1024), 0, st, descs, n, ws, tr_use_mfma(), smCnt, smLists, nextCnt);
  hipLaunchKernelGGL(smallK, dim3(nb < g_smallGrid ? nb : g_smallGrid), dim3(256), 0, st, in, out, descs, n, bit_depth, tr_use_mfma(), smCnt, smLists);
  hipLaunchKernelGGL(mfmaK, dim3(nl < 768 ? nl : 768), dim3(256), 0, st, in, out, descs, ws, ws + 2 + n, ws + 1, bit_depth, image);
  hipLaunchKernelGGL(largeK, dim3(nl < 768 ? nl : 768), dim3(256), 0, st, in, out, descs, ws + 1, bit_depth);
  if (ordered) VVC_LAUNCH_CHECK_COUNTERS(st);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // namespace

// device addresses of the tables on the current device, for the kernels of the other sources (resichain.hip, quant.hip, depquant.hip, rdoq.hip)
int vvcgpu_tr_tables(VvcTrTables* out)
{
  const int rt = vvcgpu_device_image(VVC_IMAGE_TR_TABLES, 0, upload_tables, nullptr, nullptr);     // uploaded by the first call that needs them
  if (rt) return rt;
  void* p = nullptr;
  VVC_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(d_tr32)));      out->tr32 = static_cast<const int*>(p);
  VVC_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(d_tr32t)));     out->tr32t = static_cast<const int*>(p);
  VVC_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(d_scan)));      out->scan = static_cast<const unsigned short*>(p);
  VVC_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(d_dqInv)));     out->dqInv = static_cast<const unsigned short*>(p);
  VVC_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(d_scanOff)));   out->scanOff = static_cast<const int*>(p);
  VVC_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(d_dqPosSel)));  out->dqPosSel = static_cast<const uint4*>(p);
  VVC_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(d_dqPosMisc))); out->dqPosMisc = static_cast<const uint2*>(p);
  return VVCGPU_OK;
}

extern "C" {

int vvcgpu_tr_fwd_batch(const vvc_pel* resi_base, vvc_coef* coeff_base, const vvcgpu_tr_desc* descs, int n,
                        int bit_depth, void* stream)
{
  bool empty;
  const int rc = check_descs_args(resi_base, coeff_base, descs, n, bit_depth, "tr_fwd_batch", &empty);
  if (rc || empty) return rc;
  VvcTrTables tb; const _Float16* image = nullptr;
  const int ri = vvcgpu_tr_images(&tb, &image);                               // the tables (uploaded by the first call) and the f16 image of the matrix-core kernels
  if (ri) return ri;
  // long calls: ONE launch of the residual chain's bodies in forward-only mode (packed matrix-core tiles for TUs with a 4- / 8-point side, lane groups
  // for 8x8 and smaller) instead of the small / matrix-core / dot2 kernels in a row -- on a real encoder's call mix those three were each bound by
  // their own per-wave latency (profiles/r04_shape_mix.txt)
  if (n >= 16384 && tr_use_mfma()) return vvcgpu_tr_chain_launch(1, resi_base, nullptr, coeff_base, descs, n, bit_depth, stream);
  return tr_launch_lists(tr_fwd_small_kernel, tr_fwd_mfma_kernel, tr_fwd_large_kernel, resi_base, coeff_base, descs, n, bit_depth, image, (hipStream_t)stream);
}

int vvcgpu_tr_inv_batch(const vvc_coef* coeff_base, vvc_pel* resi_base, const vvcgpu_tr_desc* descs, int n,
                        int bit_depth, void* stream)
{
  bool empty;
  const int rc = check_descs_args(coeff_base, resi_base, descs, n, bit_depth, "tr_inv_batch", &empty);
  if (rc || empty) return rc;
  VvcTrTables tb; const _Float16* image = nullptr;
  const int ri = vvcgpu_tr_images(&tb, &image);                               // the tables (uploaded by the first call) and the f16 image of the matrix-core kernels
  if (ri) return ri;
  // long calls: the residual chain's bodies in inverse-only mode (see vvcgpu_tr_fwd_batch)
  // (measured on the real call mix: 0.048 vs 0.054 ms at 35 k TUs, 0.126 vs 0.089 at 141 k -- there the three kernels' own latencies are amortised and their
  // lane-group forms run at five waves per SIMD against the chain kernel's three)
  if (n >= 16384 && n < 65536 && tr_use_mfma()) return vvcgpu_tr_chain_launch(2, nullptr, resi_base, const_cast<vvc_coef*>(coeff_base), descs, n, bit_depth, stream);
  return tr_launch_lists(tr_inv_small_kernel, tr_inv_mfma_kernel, tr_inv_large_kernel, coeff_base, resi_base, descs, n, bit_depth, image, (hipStream_t)stream);
}

int vvcgpu_dequant_tr_inv_batch(const vvc_coef* level_base, vvc_pel* resi_base, const vvcgpu_dqtr_desc* descs, int n,
                                int bit_depth, vvc_coef* coeff_out, void* stream)
{
  static_assert(sizeof(vvcgpu_dqtr_desc) == sizeof(vvcgpu_tr_desc), "descriptor layouts must stay interchangeable");
  bool empty;
  const int rc = check_descs_args(level_base, resi_base, descs, n, bit_depth, "dequant_tr_inv_batch", &empty);
  if (rc || empty) return rc;
  VVC_CHECK_ARG(coeff_out != level_base, "dequant_tr_inv_batch: coeff_out must not alias the levels");
  hipStream_t st = (hipStream_t)stream;
  VvcTrTables tb; const _Float16* image = nullptr;
  const int ri = vvcgpu_tr_images(&tb, &image);                               // the tables (uploaded by the first call) and the f16 image of the matrix-core kernels
  if (ri) return ri;
  // descriptors per workgroup: 64 when the batch is long (lane-group TUs need many per wave), fewer when that would leave compute units idle
  int per = SM_DESCS;
  while (per > 4 && cdiv(n, per) < 1024) per >>= 1;
  const int nb = cdiv(n, per);
  // calls long enough to fill workgroups with one phase each are put into class order on the device first (dqtr_classify_kernel)
  const bool ordered = n >= 16384;                                           // shorter calls: the extra launch (~15 us) costs more than the order gains
  if (ordered)
  {
    VvcScratch sc(st);
    int* lists = sc.take<int>((size_t)DQC_NCLS * n);
    if (!lists) return VVCGPU_E_DEVICE;
    int cur = 0;
    int* counters = vvcgpu_counters(st, &cur);
    if (!counters) return VVCGPU_E_DEVICE;
    int* hdr = counters + VVC_CTR_INTS * cur;
    hipLaunchKernelGGL(dqtr_classify_kernel, dim3(n < 1024 * DQC_WGS ? cdiv(n, 1024) : DQC_WGS), dim3(1024), 0, st, descs, n, hdr, lists,
                       counters + VVC_CTR_INTS * (cur ^ 1), tr_use_mfma());
    VVC_LAUNCH_CHECK_COUNTERS(st);
    hipLaunchKernelGGL(dqtr_fused_kernel, dim3(nb < 512 ? nb : 512), dim3(256), 0, st, level_base, resi_base, descs, n, per, bit_depth, coeff_out, image,
                       tr_use_mfma(), hdr, lists);
    VVC_LAUNCH_CHECK_COUNTERS(st);
    return VVCGPU_OK;
  }
  hipLaunchKernelGGL(dqtr_fused_kernel, dim3(nb < 512 ? nb : 512), dim3(256), 0, st, level_base, resi_base, descs, n, per, bit_depth, coeff_out, image,
                     tr_use_mfma(), nullptr, nullptr);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int vvcgpu_scan_order_host(int w, int h, uint16_t* out)
{
  if (!out || w < 2 || w > 64 || h < 2 || h > 64 || (w & (w - 1)) || (h & (h - 1))) return VVCGPU_E_ARG;
  host_scan_order(w, h, out);
  return VVCGPU_OK;
}

const int16_t* vvcgpu_tr_matrix_host(int type, int n)
{
  if (type < 0 || type > 2 || n < 2 || n > 64 || (n & (n - 1))) return nullptr;
  return VVC_TR_TABLES + type * 5460 + (n * n - 4) / 3;
}

}  // extern "C"
