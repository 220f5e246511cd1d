// resirate_dev.h -- what the kernel of vvcgpu_resi_rate_batch (resirate.hip) takes from the reference's tables, stated once as arithmetic, and the lane
// layout of a context row.
#pragma once
#include "common.h"
#include "dist_dev.h"

namespace {

typedef vvcgpu_resi_rate_item RrItem;
constexpr int RR_WAVES = 4, RR_THREADS = 64 * RR_WAVES;                   // a wavefront per item: 4x4 and 8x8 items do not take a workgroup each
constexpr int RR_MAX_COEF = 64 * 64, RR_MAX_GROUPS = 256;
constexpr unsigned RR_SCALE_BITS = 15;                                    // SCALE_BITS: a bypass bin costs 1 << 15
constexpr unsigned RR_DQ_ID = 0xE4u, RR_DQ_EVEN = 0xD8u, RR_DQ_ODD = 0x72u;   // the transitions of stateTab 32040 by parity as maps state -> state, 2 bits each

__host__ __device__ inline bool rr_side_ok(int v) { return v >= 2 && v <= 64 && (v & (v - 1)) == 0; }
// g_uiGroupIdx[v], v in 0..63
__device__ __forceinline__ int rr_group_idx(int v) { const int k = 31 - __builtin_clz((unsigned)v | 1u); return v < 4 ? v : 2 * k + ((v >> (k - 1)) & 1); }
// g_auiGoRicePars[min(sum, 31)]
__device__ __forceinline__ int rr_rice_par(int sum) { return sum < 12 ? 0 : sum < 25 ? 1 : 2; }
// the bins of BitEstimatorBase::encodeRemAbsEP (BinEncoder.cpp:452-503, useLimitedPrefixLength false) with g_auiGoRiceRange[0..2] = 6, 5, 6; the
// prefix loop of :489-496 ends at length = floor(log2(bins - threshold + 2^goRicePar))
__device__ __forceinline__ int rr_rem_bins(unsigned rem, int rice)
{
  const unsigned range = rice == 1 ? 5u : 6u, thr = range << rice;
  if (rem < thr) return (int)(rem >> rice) + 1 + rice;
  const int length = 31 - __builtin_clz(rem - thr + (1u << rice));
  return (int)range + 1 + (length << 1) - rice;
}
// a after b of two maps state -> state
__device__ __forceinline__ unsigned rr_dq_compose(unsigned a, unsigned b)
{
  unsigned r = 0;
#pragma unroll
  for (int s = 0; s < 4; s++) r |= ((a >> (2 * ((b >> (2 * s)) & 3u))) & 3u) << (2 * s);
  return r;
}

// Lanes are contexts in the walk: every lane carries three states, and the three sets cover the 192 bytes of a row.
//   set 0: lanes 0..59 the three SigFlag sets, 60..61 SigCoeffGroup, 62..63 the last two bytes of the padding
//   set 1: lanes 0..20 ParFlag, 21..41 GtxFlag[chType + 2] (gt1), 42..62 GtxFlag[chType] (gt2), 63 TransformSkipFlag
//   set 2: lanes 0..24 LastX, 25..49 LastY, 50..53 EMTTuIndex, 54..63 padding
__device__ __forceinline__ int rr_row_byte(int set, int lane)
{
  if (set == 0) return lane < 60 ? VVCGPU_RESI_RATE_SIG + lane : lane < 62 ? VVCGPU_RESI_RATE_SIG_GROUP + lane - 60 : VVCGPU_RESI_RATE_CTX_BYTES - 64 + lane;
  if (set == 1) return lane < 21 ? VVCGPU_RESI_RATE_PAR + lane : lane < 42 ? VVCGPU_RESI_RATE_GT1 + lane - 21
                       : lane < 63 ? VVCGPU_RESI_RATE_GT2 + lane - 42 : VVCGPU_RESI_RATE_TS;
  return lane < 50 ? lane : lane < 54 ? VVCGPU_RESI_RATE_EMT + lane - 50 : VVCGPU_RESI_RATE_CTX_USED + lane - 54;
}

}  // namespace
