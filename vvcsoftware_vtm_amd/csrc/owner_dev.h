// owner_dev.h -- what the whole-PU search entries (affine_me.hip, bipredme.hip, affine_bipredme.hip, unipredme.hip, affine_unipredme.hip) share that is
// neither translational nor affine: the owner split of the grid, the owner's barrier and 64-bit sum, the reference-index bits, the served
// PU sides, and what an item outside the contract gets.  docs/KERNELS.md, "Owners of the whole-PU entries", describes the model.
#pragma once
#include "common.h"
#include "dist_dev.h"

namespace {

// NT = 64: the wavefront owns the unit; NT = 256: the workgroup does (every wavefront follows the same, uniform, control flow)
template <int NT> __device__ __forceinline__ void owner_sync()
{
  if (NT == 256) __syncthreads();
  else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
}

// Sum over the owner of a value that is already the same in every lane of a wavefront.  NT = 256: through slots[4] of the owner's LDS and two
// barriers, the second because slots is written again by the next sum.  NT = 64: the value itself -- no LDS, no barrier.
template <int NT> __device__ __forceinline__ unsigned long long owner_sum_waves(unsigned long long v, unsigned long long* slots, int tid)
{
  if (NT == 64) return v;
  if ((tid & 63) == 0) slots[tid >> 6] = v;
  __syncthreads();
  v = slots[0] + slots[1] + slots[2] + slots[3];
  __syncthreads();
  return v;
}

// Sum of every lane's v over the owner, in every lane
template <int NT> __device__ __forceinline__ unsigned long long owner_sum(unsigned long long v, unsigned long long* slots, int tid)
{
  return owner_sum_waves<NT>(wave_sum(v), slots, tid);
}

// The owner split.  A launch over `units` (items, or searches) has cdiv(units, 4) workgroups of four wavefront owners, then up to `units` workgroup
// owners (workgroup i of them owns unit i).  leave: nothing to own.  The caller then drops the unit whose size belongs to the other kind.
struct OwnerSlot { int unit; bool waveOwner, leave; };
__device__ __forceinline__ OwnerSlot owner_slot(int units, int wave)
{
  const int nWaveGroups = (units + 3) >> 2;
  OwnerSlot s;
  s.waveOwner = (int)blockIdx.x < nWaveGroups;
  s.unit = s.waveOwner ? (int)blockIdx.x * 4 + wave : (int)blockIdx.x - nWaveGroups;
  s.leave = s.unit >= units;
  return s;
}

// the bits of reference index r of a list of nRef (truncated unary)
__device__ __forceinline__ unsigned pu_ref_bits(int nRef, int r) { return nRef > 1 ? (unsigned)(r + 1 - (r == nRef - 1 ? 1 : 0)) : 0u; }

// the served sides of a PU (and of cfg.max_pu): translational 4, 8, .. 128; affine 16, 32, 64, 128
inline __host__ __device__ bool pu_side_pow2_ok(int v) { return v >= 4 && v <= 128 && (v & (v - 1)) == 0; }
inline __host__ __device__ bool pu_side_affine_ok(int v) { return v == 16 || v == 32 || v == 64 || v == 128; }

template <class T> __device__ __forceinline__ void zero_record(T* p) { memset(p, 0, sizeof(T)); }

// An item outside the contract, by its workgroup owner: a zeroed result with cost = all ones, zeroed trace steps (steps may be null); nothing else is
// read or written for it
template <class Result, class Step>
__device__ __forceinline__ void owner_write_sentinel(Result* result, Step* steps, int maxSteps, int tid)
{
  if (tid == 0)
  {
    zero_record(result);
    result->cost = ~0ull;
  }
  if (steps && tid < maxSteps) zero_record(steps + tid);
}

}  // namespace
