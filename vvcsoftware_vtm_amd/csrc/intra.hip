// intra.hip -- intra sample predictors (next row N4) for gfx950: planar, DC, 65 angular modes with wide-angle mapping, the
// simplified PDPC, and the [1 2 1] reference sample filter.
//
// Reference behaviour reproduced (bit-exact):
//   IntraPrediction::predIntraAng (mode switch + PDPC, JVET_K0063)   CommonLib/IntraPrediction.cpp:251-347
//   xGetPredValDc :173-211, getWideAngle / setReferenceArrayLengths :213-249, xPredIntraPlanar :424-477,
//   xPredIntraAng :540-773 (linear interpolation iff deltaFract != 0, angular PDPC), xFilterReferenceSamples :1071-1104
//
// Design: the reference walks rows with running sums and early `break`s; every prediction sample is in fact a closed form of
// (x, y) and a handful of reference samples, so one wavefront takes one PU, stages the <= 257 reference samples (optionally
// filtered) and the projected main reference in LDS, and every lane computes samples independently, iterating in destination
// order so that stores coalesce for horizontal modes too.  Four PUs per workgroup, no workgroup barrier.
#include "common.h"
#include "dist_dev.h"
#include "intra_dev.h"

namespace {

__global__ __launch_bounds__(256) void intra_pred_kernel(const Pel* __restrict__ refsBase, Pel* __restrict__ dstBase,
                                                         const vvcgpu_intra_desc* __restrict__ descs, int n, int clpMin, int clpMax)
{
  __shared__ short topS[4][REF_MAX], leftS[4][REF_MAX], tmpS[4][2 * REF_MAX], mainS[4][NEG_MAX + REF_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  if (b >= n) return;                                       // no workgroup barrier below
  const vvcgpu_intra_desc d = descs[b];
  intra_pred_block(d, refsBase, dstBase + d.dst_off, d.dst_stride, clpMin, clpMax, lane, topS[wave], leftS[wave], tmpS[wave], mainS[wave]);
}

// ---- intra mode pre-selection (IntraSearch::estIntraPredLumaQT, EncoderLib/IntraSearch.cpp:397-480): predIntraAng of one candidate mode into
// the wave's LDS tile, then the Hadamard distortion against the original (distParam.distFunc = xGetHADs) -- the prediction never reaches HBM.
// Measured at 4K (31 k blocks of 16 x 16 x 67 modes, tools/intra_search_time.py): 2.55 ms against 1.17 + 1.13 ms for prediction and distortion as two
// launches -- the fused form saves 2 GB of prediction traffic but its waves (prediction AND Hadamard code: 100+ VGPRs, a 32 KB tile per
// workgroup) are latency-bound at a quarter of the separate kernels' occupancy.  Variants tried: a 1024-sample band tile with the Hadamard code
// inlined (187 VGPRs, 5.1 ms), the same with the distortion as a real call and a 128-VGPR cap (3.0 ms), 80-VGPR cap (spills, 9.8 ms).
__global__ __launch_bounds__(256) void intra_satd_kernel(const Pel* __restrict__ refsBase, const Pel* __restrict__ orgBase,
                                                         const vvcgpu_intra_satd_desc* __restrict__ descs, int n, int clpMin, int clpMax,
                                                         unsigned long long* __restrict__ out)
{
  __shared__ short topS[4][REF_MAX], leftS[4][REF_MAX], tmpS[4][2 * REF_MAX], mainS[4][NEG_MAX + REF_MAX];
  __shared__ __align__(16) short predS[4][64 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  if (b >= n) return;                                       // no workgroup barrier below
  const vvcgpu_intra_satd_desc s = descs[b];
  if (s.w < 1 || s.h < 1 || s.w > 64 || s.h > 64) { if (lane == 0) out[b] = ~0ull; return; }   // outside the 64 x 64 LDS tile (wave-uniform): sentinel, no overrun
  vvcgpu_intra_desc d;
  d.ref_off = s.ref_off; d.dst_off = 0; d.dst_stride = s.w; d.w = s.w; d.h = s.h; d.mode = s.mode; d.filter_refs = s.filter_refs;
  intra_pred_block(d, refsBase, predS[wave], s.w, clpMin, clpMax, lane, topS[wave], leftS[wave], tmpS[wave], mainS[wave]);
  wave_sync();
  typedef const __attribute__((address_space(3))) short* LdsPel;
  const unsigned long long res = satd_block<64, LdsPel>(orgBase + s.org_off, s.org_stride, (LdsPel)predS[wave], s.w, s.w, s.h, lane);
  if (lane == 0) out[b] = res;
}


// ---- reference sample gathering: xFillReferenceSamples :807-1004 ---------------------------------------------------------------
// One wavefront per block.  The reference pads through a line buffer (an unavailable unit repeats the last sample of the unit
// before it, a leading unavailable run repeats the first sample of the first available unit); in closed form every sample of an
// unavailable unit is one fixed sample of the nearest available unit, so each lane resolves its output samples independently.
__global__ __launch_bounds__(256) void intra_fill_refs_kernel(const Pel* __restrict__ recBase, const unsigned char* __restrict__ flagsBase,
                                                              Pel* __restrict__ refsBase, const vvcgpu_intra_fill_desc* __restrict__ descs, int n,
                                                              int bitDepth)
{
  __shared__ short srcUnit[4][FILL_UNITS_MAX];          // per unit: the unit that provides its samples (itself when available), or -1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  if (b >= n) return;
  const vvcgpu_intra_fill_desc d = descs[b];
  intra_fill_refs_block(recBase, flagsBase, d, bitDepth, lane, srcUnit[wave], refsBase + d.ref_off);
}

// ---- CCLM (JVET_K0190): xGetLumaRecPixels :1283-1581 + xGetLMParameters :1597-1857 (both through intra_dev.h) + predIntraChromaLM :390-403
// One wavefront per chroma block.  The down-sampled luma is never stored: neighbours are produced for the parameter sums and the
// inner samples on the fly for the final linear map (6 luma reads per chroma sample, all L1/L2 hits of one small region).
__global__ __launch_bounds__(256) void cclm_pred_kernel(const Pel* __restrict__ lumaBase, const Pel* __restrict__ nbBase, Pel* __restrict__ dstBase,
                                                        const vvcgpu_cclm_desc* __restrict__ descs, int n, int bdLuma, int bdChroma, int clpMin,
                                                        int clpMax)
{
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= n) return;
  const vvcgpu_cclm_desc d = descs[b];
  const int w = d.w, h = d.h, rs = d.luma_stride, rs2 = rs * 2;
  const bool aboveAvail = d.above_avail != 0, leftAvail = d.left_avail != 0;
  const Pel* luma = lumaBase + d.luma_off;
  const Pel* nbAbove = nbBase + d.nb_off;
  const Pel* nbLeft = nbAbove + w;
  int a, bb, shift;
  cclm_params(w, h, aboveAvail, leftAvail,
              [&](int idx) { return cclm_down(luma - rs2 + 2 * idx, rs, idx == 0 && !leftAvail); },
              [&](int idx) { return cclm_down(luma + (ptrdiff_t)idx * rs2 - 2, rs, false); },
              nbAbove, nbLeft, bdLuma, bdChroma, lane, a, bb, shift);
  Pel* dst = dstBase + d.dst_off;
  const int lgW = floor_log2((unsigned)w);
  for (int i = lane; i < w * h; i += 64)
  {
    const int yy = i >> lgW, xq = i & (w - 1);
    const int s = (short)cclm_down(luma + (ptrdiff_t)yy * rs2 + 2 * xq, rs, xq == 0 && !leftAvail);
    dst[(ptrdiff_t)yy * d.dst_stride + xq] = (Pel)min(max(((a * s) >> shift) + bb, clpMin), clpMax);
  }
}

}  // namespace

extern "C" int vvcgpu_intra_ref_lengths(int w, int h, int* top_len, int* left_len)
{
  VVC_CHECK_ARG(top_len && left_len && w >= 4 && h >= 4 && w <= 64 && h <= 64 && !(w & (w - 1)) && !(h & (h - 1)), "intra_ref_lengths: %dx%d", w, h);
  int lw = 0, lh = 0; while ((1 << (lw + 1)) <= w) lw++; while ((1 << (lh + 1)) <= h) lh++;
  const int ratio = abs(lw - lh) < 2 ? abs(lw - lh) : 2;
  *left_len = h << 1; *top_len = w << 1;
  if (w > h) *left_len += (w >> ratio) - h + ((w + 31) >> 5);
  else if (h > w) *top_len += (h >> ratio) - w + ((h + 31) >> 5);
  return VVCGPU_OK;
}

extern "C" int vvcgpu_intra_pred_batch(const vvc_pel* refs_base, vvc_pel* dst_base, const vvcgpu_intra_desc* descs, int n, int clp_min,
                                       int clp_max, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "intra_pred_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(refs_base && dst_base && descs, "intra_pred_batch: null pointer");
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "intra_pred_batch: clip range %d..%d", clp_min, clp_max);
  hipLaunchKernelGGL(intra_pred_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, refs_base, dst_base, descs, n, clp_min, clp_max);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

extern "C" int vvcgpu_intra_satd_batch(const vvc_pel* refs_base, const vvc_pel* org_base, const vvcgpu_intra_satd_desc* descs, int n, int clp_min,
                                       int clp_max, uint64_t* out, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "intra_satd_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(refs_base && org_base && descs && out, "intra_satd_batch: null pointer");
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "intra_satd_batch: clip range %d..%d", clp_min, clp_max);
  hipLaunchKernelGGL(intra_satd_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, refs_base, org_base, descs, n, clp_min, clp_max,
                     reinterpret_cast<unsigned long long*>(out));
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

extern "C" int vvcgpu_cclm_pred_batch(const vvc_pel* luma_base, const vvc_pel* nb_base, vvc_pel* dst_base, const vvcgpu_cclm_desc* descs, int n,
                                      int bit_depth_luma, int bit_depth_chroma, int clp_min, int clp_max, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "cclm_pred_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(luma_base && nb_base && dst_base && descs, "cclm_pred_batch: null pointer");
  VVC_CHECK_ARG(bit_depth_luma >= 8 && bit_depth_luma <= 12 && bit_depth_chroma >= 8 && bit_depth_chroma <= 12, "cclm_pred_batch: bit depths %d %d",
                bit_depth_luma, bit_depth_chroma);
  VVC_CHECK_ARG(clp_min <= clp_max, "cclm_pred_batch: clip range");
  hipLaunchKernelGGL(cclm_pred_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, luma_base, nb_base, dst_base, descs, n, bit_depth_luma,
                     bit_depth_chroma, clp_min, clp_max);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

extern "C" int vvcgpu_intra_fill_refs_batch(const vvc_pel* rec_base, const uint8_t* flags_base, vvc_pel* refs_base, const vvcgpu_intra_fill_desc* descs,
                                            int n, int bit_depth, void* stream)
{
  VVC_CHECK_ARG(n >= 0, "intra_fill_refs_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(rec_base && flags_base && refs_base && descs, "intra_fill_refs_batch: null pointer");
  VVC_CHECK_ARG(bit_depth >= 8 && bit_depth <= 12, "intra_fill_refs_batch: bit depth %d", bit_depth);
  hipLaunchKernelGGL(intra_fill_refs_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, rec_base, flags_base, refs_base, descs, n, bit_depth);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
