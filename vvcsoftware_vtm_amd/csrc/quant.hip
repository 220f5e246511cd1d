// quant.hip -- forward scalar quantisation without RDOQ (vvcgpu_quant_batch): Quant::quant (Quant.cpp:721-834) + xSignBitHidingHDQ (:142-273).
// Without sign hiding the map is element-wise.  With it, the coefficient groups (16 coefficients in scan order) are independent
// once the TU's abs-sum and its last group with a level are known: pass 1 finds both, pass 2 decides every group's adjustment.
// The scan tables are those of transform.hip (vvcgpu_tr_tables); their addresses arrive as a kernel argument.
#include "common.h"
#include "quant_dev.h"

namespace {

__device__ __forceinline__ int quant_one(const VqFwd& q, int c, int& deltaU)
{
  const long long tmp = (long long)abs(c) * q.scale * q.whScale;
  const int mag = (int)((tmp + q.add) >> q.qBits);
  deltaU = (int)((tmp - ((long long)mag << q.qBits)) >> q.qBits8);
  return mag;
}

// TUs of up to 256 coefficients are handled by 16 lanes each, four side by side in a wavefront (a step = one coefficient group of
// each; most of a picture's TUs are small, so this fills the lanes and shares the set-up); larger TUs take the whole wavefront
// (four coefficient groups per step).
template <bool LARGE>
__device__ __forceinline__ void quant_tu(const TCoeff* __restrict__ coeffBase, TCoeff* __restrict__ levelBase, const vvcgpu_quant_desc& d, bool live,
                                         int ti, int bd, unsigned* __restrict__ absSumOut, int lane, const VvcTrTables& tb)
{
  constexpr int LPT = LARGE ? 64 : 16;
  const int k = lane & 15, slot = lane >> 4, tl = lane & (LPT - 1);
  const int w = d.w, h = d.h, cnt = live ? w * h : 0, lw = ilog2(w), lh = ilog2(h);
  const TCoeff* coef = coeffBase + d.coeff_off;
  TCoeff* level = levelBase + d.level_off;
  const VqFwd q = vq_fwd(d.qp, vq_transform_shift(bd, lw, lh), vq_sqrt2(lw, lh), vq_round9(d.intra_slice));
  const bool sbh = d.sign_hiding && w >= 4 && h >= 4;
  const unsigned short* scan = tb.scan + tb.scanOff[(lw - 1) * 6 + (lh - 1)];
  int maxCnt = cnt;                                         // the wavefront runs as many steps as its largest TU needs
#pragma unroll
  for (int m = LPT; m < 64; m <<= 1) maxCnt = max(maxCnt, __shfl_xor(maxCnt, m));
  if (maxCnt == 0) return;
  int sum = 0;
  if (!sbh || !live)
  {
    // element-wise (sign hiding off): levels are final
    for (int s0 = 0; s0 < maxCnt; s0 += LPT)
    {
      const int si = s0 + tl;
      if (si < cnt && !sbh)
      {
        int du; const int c = coef[si];
        const int mag = quant_one(q, c, du);
        sum += mag;
        level[si] = min(max(c < 0 ? -mag : mag, -32768), 32767);
      }
    }
  }
  // Sign hiding, ONE pass from the end of the scan: the first coefficient group met with a level is the reference's "last" group
  // (:183-186), every other group searches all 16 positions.  The reference hides only if uiAbsSum >= 2; a group that qualifies
  // (last - first >= 4) has two levels, so the test can only fail when the 32-bit sum wrapped -- handled after the loop.
  // 16 lanes per coefficient group; the sequential search for the cheapest parity fix (:196-262, the highest scan position wins
  // ties) is a 16-lane min over (cost, -position).
  bool foundLast = false, fixedAny = false;
  const int steps = (maxCnt + LPT - 1) / LPT;
  for (int st = steps - 1; st >= 0; st--)
  {
    const int si = st * LPT + tl;
    const bool in = sbh && live && si < cnt;
    const int pos = in ? scan[si] : 0;
    const int c = in ? coef[pos] : 0;
    int du;
    const int mag = quant_one(q, c, du);
    sum += in ? mag : 0;
    int lv = min(max(c < 0 ? -mag : mag, -32768), 32767);
    const unsigned long long nzAll = __ballot(lv != 0);
    const unsigned nz = (unsigned)((nzAll >> (16 * slot)) & 0xFFFFull);
    // is this lane's group the last one with a level?  no earlier-met (= later in scan order) group of this TU had one
    bool isLast;
    if (LARGE)
    {
      const unsigned long long higher = slot == 3 ? 0ull : (nzAll >> (16 * (slot + 1)));
      isLast = !foundLast && nz != 0 && higher == 0ull;
      foundLast = foundLast || nzAll != 0ull;
    }
    else { isLast = !foundLast && nz != 0; foundLast = foundLast || nz != 0; }
    const int first = nz ? __ffs((int)nz) - 1 : 16, last = nz ? 31 - __clz((int)nz) : -1;
    int ssum = lv;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) ssum += __shfl_xor(ssum, m);
    const int firstLv = __shfl(lv, (lane & 48) + (first & 15));
    const unsigned signbit = firstLv > 0 ? 0u : 1u;
    const bool fix = last - first >= 4 && signbit != (unsigned)(ssum & 1);
    const int start = isLast ? last : 15;
    const int TMAX = 0x7fffffff;
    int cost = TMAX, change = 0;
    if (k <= start)
    {
      if (lv != 0)
      {
        if (du > 0) { cost = -du; change = 1; }
        else if (!(k == first && abs(lv) == 1)) { cost = du; change = -1; }
      }
      else if (k < first) { if ((c >= 0 ? 0u : 1u) == signbit) { cost = -du; change = 1; } }
      else { cost = -du; change = 1; }
    }
    long long key = ((long long)cost << 5) + (15 - k);
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { const long long o = __shfl_xor(key, m); key = min(key, o); }
    if (fix && k == 15 - (int)(key & 31))
    {
      if (lv == 32767 || lv == -32768) change = -1;
      lv += c >= 0 ? change : -change;
    }
    fixedAny = fixedAny || (fix && in);
    if (in) level[pos] = lv;
  }
#pragma unroll
  for (int m = 1; m < LPT; m <<= 1) sum += __shfl_xor(sum, m);
  if (live && tl == 0) absSumOut[ti] = (unsigned)sum;
  // uiAbsSum is a 32-bit int in the reference: if it wrapped below 2 no hiding happened there -- rewrite the plain levels
  if (sbh && live && sum < 2 && __ballot(fixedAny) != 0ull)
    for (int s0 = 0; s0 < cnt; s0 += LPT)
    {
      const int si = s0 + tl;
      if (si < cnt) { int du; const int c = coef[si]; const int mag = quant_one(q, c, du); level[si] = min(max(c < 0 ? -mag : mag, -32768), 32767); }
    }
}

// two launches: the first takes the small TUs (four per wavefront) and lists the large ones; the second walks that list, one large
// TU per wavefront at a time (a persistent grid: no empty workgroups for the many small TUs of a picture)
__global__ __launch_bounds__(256) void quant_small_kernel(const TCoeff* __restrict__ coeffBase, TCoeff* __restrict__ levelBase,
                                                          const vvcgpu_quant_desc* __restrict__ descs, int n, int bd, unsigned* __restrict__ absSumOut,
                                                          int* __restrict__ largeList, VvcTrTables tb)
{
  const int lane = threadIdx.x & 63;
  const int ti = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const vvcgpu_quant_desc d = descs[ti < n ? ti : n - 1];
  const bool large = (int)d.w * d.h > 256;
  if (ti < n && large && (lane & 15) == 0) largeList[1 + atomicAdd(&largeList[0], 1)] = ti;
  const bool live = ti < n && !large;
  if (__ballot(live) == 0ull) return;
  quant_tu<false>(coeffBase, levelBase, d, live, ti, bd, absSumOut, lane, tb);
}

__global__ __launch_bounds__(256) void quant_large_kernel(const TCoeff* __restrict__ coeffBase, TCoeff* __restrict__ levelBase,
                                                          const vvcgpu_quant_desc* __restrict__ descs, int bd, unsigned* __restrict__ absSumOut,
                                                          const int* __restrict__ largeList, VvcTrTables tb)
{
  const int lane = threadIdx.x & 63;
  const int count = largeList[0], waves = gridDim.x * 4;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < count; i += waves)
  {
    const int ti = largeList[1 + i];
    const vvcgpu_quant_desc d = descs[ti];
    quant_tu<true>(coeffBase, levelBase, d, true, ti, bd, absSumOut, lane, tb);
  }
}

}  // namespace

extern "C" {

int vvcgpu_quant_batch(const vvc_coef* coeff_base, vvc_coef* level_base, const vvcgpu_quant_desc* descs, int n, int bit_depth, uint32_t* abs_sum,
                       void* stream)
{
  VVC_CHECK_ARG(n >= 0, "quant_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(coeff_base && level_base && descs && abs_sum, "quant_batch: null pointer");
  VVC_CHECK_ARG(bit_depth >= 8 && bit_depth <= 10, "quant_batch: bit depth %d outside 8..10", bit_depth);
  VvcTrTables tb;
  const int rt = vvcgpu_tr_tables(&tb);
  if (rt) return rt;
  hipStream_t st = (hipStream_t)stream;
  VvcScratch sc(st);
  int* list = sc.take<int>((size_t)n + 1);
  if (!list) return VVCGPU_E_DEVICE;
  VVC_HIP(hipMemsetAsync(list, 0, sizeof(int), st));
  hipLaunchKernelGGL(quant_small_kernel, dim3(cdiv(n, 16)), dim3(256), 0, st, coeff_base, level_base, descs, n, bit_depth, abs_sum, list, tb);
  const int nl = cdiv(n, 4);
  hipLaunchKernelGGL(quant_large_kernel, dim3(nl < 512 ? nl : 512), dim3(256), 0, st, coeff_base, level_base, descs, bit_depth, abs_sum, list, tb);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
