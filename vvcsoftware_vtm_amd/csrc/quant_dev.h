// quant_dev.h -- the reference's flat-scaling quantiser arithmetic, stated ONCE for every kernel that quantises or de-quantises: quant.hip,
// depquant.hip, rdoq.hip, the fused de-quantiser of transform.hip, resichain.hip and rdpcm.hip.  A kernel may keep a packed struct of its own for
// its hot loop; it fills that struct from these helpers.  (oracle/restate keeps its own statement of the formulas: it is what the kernels are
// tested against, and does not include this header.)
#pragma once
#include "common.h"

// g_quantScales / g_invQuantScales (Rom.cpp:465-473) by qp % 6
__device__ __forceinline__ int vq_quant_scale(int rem) { return rem == 0 ? 26214 : rem == 1 ? 23302 : rem == 2 ? 20560 : rem == 3 ? 18396 : rem == 4 ? 16384 : 14564; }
__device__ __forceinline__ int vq_inv_scale(int rem) { return rem == 0 ? 40 : rem == 1 ? 45 : rem == 2 ? 51 : rem == 3 ? 57 : rem == 4 ? 64 : 72; }
// getTransformShift with maxLog2TrDynamicRange 15 (ChromaFormat.h:117-120)
__device__ __forceinline__ int vq_transform_shift(int bd, int lw, int lh) { return 15 - bd - ((lw + lh) >> 1); }
// TU::needsSqrt2Scale (UnitTools.cpp:3192-3197): 2:1 shapes carry a factor 181 and 7 (forward) / 8 (inverse) more bits of shift
__device__ __forceinline__ bool vq_sqrt2(int lw, int lh) { return ((lw + lh) & 1) != 0; }
// the quantiser scale with the sqrt-2 factor folded in, as the trellis and RDOQ use it (DepQuant.cpp:671, QuantRDOQ.cpp:783)
__device__ __forceinline__ int vq_quant_scale_folded(int rem, bool sqrt2) { const int qs = vq_quant_scale(rem); return sqrt2 ? (qs * 181) >> 7 : qs; }
// QUANT_SHIFT + per + transformShift (Quant.cpp:793, :942), without the sqrt-2 bits
__device__ __forceinline__ int vq_qbits(int per, int transformShift) { return 14 + per + transformShift; }
// the rounding offset of Quant::quant (Quant.cpp:796-797, :945) is round9 << (qBits - 9): 171 in intra slices, 85 otherwise, 256 for the half-round form
__device__ __forceinline__ int vq_round9(int intraSlice) { return intraSlice ? 171 : 85; }

// the diagonal scan inside a 4x4 coefficient group, sixteen 4-bit entries: scan index of in-group position y * 4 + x, or its inverse
constexpr unsigned long long vq_pack_scan4(bool inverse)
{
  unsigned long long kof = 0, posof = 0; int k = 0;
  for (int d = 0; d < 7; d++)
    for (int y = (d < 3 ? d : 3); y >= 0; y--)
    {
      const int x = d - y;
      if (x > 3) continue;
      kof |= (unsigned long long)k << (4 * (y * 4 + x)); posof |= (unsigned long long)(y * 4 + x) << (4 * k); k++;
    }
  return inverse ? posof : kof;
}

// Quant::quant (Quant.cpp:721-834): level = (|c| * scale * whScale + add) >> qBits; qBits8 = qBits - 8 is the shift of the sign-hiding deltaU
struct VqFwd { int qBits, qBits8, scale, whScale; long long add; };
__device__ __forceinline__ VqFwd vq_fwd(int qp, int transformShift, bool sqrt2, int round9)
{
  VqFwd q;
  const int per = qp / 6, rem = qp - 6 * per;
  q.whScale = sqrt2 ? 181 : 1;
  q.qBits = vq_qbits(per, transformShift) + (sqrt2 ? 7 : 0); q.qBits8 = q.qBits - 8;
  q.scale = vq_quant_scale(rem);
  q.add = (long long)round9 << (q.qBits - 9);
  return q;
}

// Quant::dequant (Quant.cpp:277-428): IQUANT_SHIFT - (transformShift + per) with 8 more bits for 2:1 shapes (:312-323, :1000), the input clipped
// to targetInputBitDepth bits (:393-396, :1050)
struct VqInv { int scale, rightShift, inMin, inMax; };
__device__ __forceinline__ VqInv vq_inv(int qp, int transformShift, bool sqrt2)
{
  VqInv q;
  const int per = qp / 6, rem = qp - 6 * per;
  q.rightShift = (sqrt2 ? 8 : 0) + (6 - (transformShift + per));
  q.scale = vq_inv_scale(rem) * (sqrt2 ? 181 : 1);
  const int targetBits = min(16, 32 + q.rightShift - 7);
  q.inMin = -(1 << (targetBits - 1)); q.inMax = (1 << (targetBits - 1)) - 1;
  return q;
}
// one level through the scalar de-quantiser (Quant.cpp:391-425), 64-bit intermediate, output clipped to 16 bits
__device__ __forceinline__ int vq_dequant_one(const VqInv& q, int lv)
{
  const long long c = min(max(lv, q.inMin), q.inMax);
  const long long v = q.rightShift > 0 ? (c * q.scale + (1ll << (q.rightShift - 1))) >> q.rightShift : (c * q.scale) << -q.rightShift;
  return (int)min(max(v, -32768ll), 32767ll);
}
