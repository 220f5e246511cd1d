// depquant_dev.h -- the dependent-quantisation trellis, DQIntern::DepQuant::quant (DepQuant.cpp:1323-1391), stated once for its two kernels:
// depquant_kernel (vvcgpu_depquant_batch: work item ti is descriptor ti) and depquant_listed_kernel (vvcgpu_depquant_listed_launch, the trellis launch of
// the RD pass entries under DepQuant 1: work item ti is descriptor list[ti]), both in depquant.hip.  Here are the types, helpers and constants and the
// workspace layout; the kernels' body is depquant_body.inc, which each kernel includes under its own signature.
// The trellis is a sequential walk down the scan with four states; TUs are independent.  FOUR LANES own one TU, lane k carries
// trellis state k (its previous-position state and its skip state live in the lane's registers), sixteen TUs share a wavefront.
// Per scan position: every lane prices the transitions LEAVING its state (two quantisation candidates + zero), the three 64-bit
// costs entering decision k are gathered with quad shuffles in the reference's comparison order (:1222-1249, strict '<'), the
// winner's template context (16 abs levels + 16 context seeds = 12 dwords) is pulled from the source lane, and the new rates are
// looked up in the caller's rate tables.  Decisions (absLevel << 4 | prevId + 2) go to the workspace for the back-trace; the
// per-state sub-block memory of CommonCtx (:828-858) lives in the workspace as well and is touched only at sub-block ends.
// The scan tables and the shape-only part of the position records (the byte selectors of a position's five template neighbours inside the
// sub-block and its context offsets) are those of transform.hip (vvcgpu_tr_tables); their addresses arrive as a kernel argument.  (Names: tq_ / Tq / TQ_ = the trellis quantiser; dq_ is the de-quantiser of transform.hip.)
#pragma once
#include "common.h"
#include "quant_dev.h"

namespace {

// Small per-lane tables are ext-vector VALUES, not arrays: element selects then stay register selects (with arrays LLVM rewrites a
// select of loads into a load through a selected address, which pins the whole state struct in scratch memory).
typedef unsigned tq_u4 __attribute__((ext_vector_type(4)));
typedef unsigned tq_u8 __attribute__((ext_vector_type(8)));
typedef long long tq_l4 __attribute__((ext_vector_type(4)));
typedef int tq_i4 __attribute__((ext_vector_type(4)));

struct TqState
{
  long long rdCost;
  tq_u4 lev;                          // 16 abs levels of the current sub-block (bytes)
  tq_u4 aux;                          // per level min(4 - (v & 1), v) | (v != 0) << 5: what it adds to sumAbs1 and sumNum of a template
  int numSigSbb, refSbbCtxId;         // refSbbCtxId also names the LDS slot with the 16 template-context seeds of the sub-block (-1: all zero)
  int sbb0, sbb1, sig0, sig1;
  int gc;                             // row of the greater-than-x rate table (coefficient bit sums [0..6])
  int goRice;
};

// member-wise copy: a whole-struct assignment also copies the padding through scratch memory
__device__ __forceinline__ void tq_copy(TqState& d, const TqState& s)
{
  d.rdCost = s.rdCost; d.lev = s.lev; d.aux = s.aux; d.numSigSbb = s.numSigSbb; d.refSbbCtxId = s.refSbbCtxId;
  d.sbb0 = s.sbb0; d.sbb1 = s.sbb1; d.sig0 = s.sig0; d.sig1 = s.sig1; d.gc = s.gc; d.goRice = s.goRice;
}
__device__ __forceinline__ void tq_set_byte(tq_u4& a, int j, unsigned val)
{
  const int d = j >> 2, sh = (j & 3) * 8;
#pragma unroll
  for (int i = 0; i < 4; i++) { const unsigned m = i == d ? 0xFFu << sh : 0u; a[i] = (a[i] & ~m) | ((val << sh) & m); }   // no conditional store: keeps the array in registers
}
__device__ __forceinline__ unsigned tq_get_u16(const tq_u8 c, int j)
{
  const int d = j >> 1;
  unsigned v = c[0];
#pragma unroll
  for (int i = 1; i < 8; i++) v = d == i ? c[i] : v;
  return (v >> ((j & 1) * 16)) & 0xFFFFu;
}
typedef const __attribute__((address_space(3))) vvcgpu_dq_rates* TqLdsRates;
__device__ __forceinline__ int tq_level_bits(TqLdsRates rt, int gc, int goRice, unsigned level)       // State::getLevelBits :909-931
{
  const unsigned idx = level < 5 ? level : 5 + ((level - 5) & 1);
  const int bits = rt->gtx[gc][idx];
  if (level < 5) return bits;
  // escape part; the prefix loop of :924-929 ends at length = floor(log2(value - thres + 2^goRice))
  const unsigned value = (level - 5) >> 1;
  const unsigned range = goRice == 0 ? 6u : goRice == 1 ? 5u : goRice == 2 ? 6u : 3u;              // g_auiGoRiceRange
  const unsigned thres = range << goRice;
  const unsigned length = 31u - (unsigned)__clz((int)(value - thres + (1u << goRice)));
  const unsigned esc = value < thres ? (value >> goRice) + 1 + goRice : range + 1 + (length << 1) - goRice;
  return bits + (int)(esc << 15);
}
__device__ __forceinline__ long long tq_shfl64(long long v, int src) { return __shfl(v, src); }
// quad permutation with a compile-time pattern (v_mov_b32 dpp quad_perm): no LDS round trip on the cost chain
template <int CTRL>
__device__ __forceinline__ long long tq_quad64(long long v)
{
  const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)v, CTRL, 0xF, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)((unsigned long long)v >> 32), CTRL, 0xF, 0xF, true);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

template <int CTRL>
__device__ __forceinline__ unsigned tq_quad32(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true); }

constexpr unsigned long long TQ_KOFPOS = vq_pack_scan4(false), TQ_POSOFK = vq_pack_scan4(true);

// What a trellis step needs that does not depend on the trellis state, per scan position: the four quantisation candidates of
// Quantizer::preQuantCoeff (:786-808), the two "start here" costs (checkRdCostStart :1196-1213: candidate 0 / 2 + last-position bits +
// level bits in the start context), and for the position AFTER it the in-sub-block template neighbours (:139-168) and its context offsets.
// The quad fills the sixteen records of a sub-block when the walk enters it (four positions per lane) instead of every lane repeating
// the same arithmetic at every step: ~250 of a step's ~735 instructions were this.
struct TqRec
{
  long long dist[4];                  // pqData.deltaDist by slot (qIdx & 3)
  unsigned short ab[4];               // pqData.absLevel by slot
  long long start[2];                 // decision 0 / decision 2
  unsigned misc;                      // neighbour positions 5 x 4 bits | sigOff << 20 | gtxOff << 24
  // v_perm_b32 selectors that pick the five neighbours out of the sixteen level bytes: group A = neighbours 0..3, group B = neighbour 4;
  // Lo reads bytes 0..7, Hi bytes 8..15, selector 12 (= constant zero) where the neighbour is in the other half or does not exist
  unsigned selLoA, selHiA, selLoB, selHiB, pad;
};
static_assert(sizeof(TqRec) == 80, "TqRec");
constexpr int TQ_REC_N = 8;                                               // positions filled at a time (half a sub-block)
constexpr int TQ_SEED_BYTES = 5 * 32;                                     // per TU: the seeds of context slots 0..3 + an all-zero slot
constexpr int TQ_LDS_BYTES = 64 * (TQ_REC_N * (int)sizeof(TqRec) + TQ_SEED_BYTES);   // 64 quads per workgroup
constexpr int TQ_RT_SLOTS = 16;

// bytes of trellis workspace for a coefficient extent of c (a multiple of 16): the decisions (4 x u32 per position: [scan index][state]) at
// 16 coeff_off, then the level histories (8 bytes per position) at 8 coeff_off
inline size_t tq_dec_bytes(size_t c) { return c * 16; }
inline size_t tq_ctx_bytes(size_t c) { return c * 8; }

}  // namespace
