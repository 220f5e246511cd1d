// depquant.hip -- vvcgpu_depquant_batch: the dependent-quantisation trellis, DQIntern::DepQuant::quant (DepQuant.cpp:1323-1391), over an array of
// descriptors, and vvcgpu_depquant_listed_launch: the same trellis over a work list, for the RD pass entries under DepQuant 1 (dqpass_dev.h).  The
// trellis itself is stated in depquant_dev.h and depquant_body.inc; here are the two kernels' signatures, the launcher and the entry points.
#include "common.h"
#include "depquant_dev.h"

namespace {

__global__ __launch_bounds__(256) void depquant_kernel(const TCoeff* __restrict__ coeffBase, TCoeff* __restrict__ levelBase,
                                                       const vvcgpu_depquant_desc* __restrict__ descs, int n,
                                                       const vvcgpu_dq_rates* __restrict__ ratesBase, int bd, unsigned* __restrict__ absSumOut,
                                                       unsigned* __restrict__ wsDec, unsigned char* __restrict__ wsCtx, VvcTrTables tb)
{
  constexpr bool LISTED = false;                                          // work item ti is descriptor ti
  const int* const list = nullptr;
#include "depquant_body.inc"
}

// the trellis over a work list: work item ti is descriptor list[ti].  (The body behind the kernel's early exit is a function of its own, and LISTED
// its template parameter, because the kernel's instruction stream is then what it was when the body was tq_trellis<true> of depquant_dev.h; included
// in the kernel itself it comes out five instructions shorter and unmeasured.)
template <bool LISTED>
__device__ __forceinline__ void tq_trellis_listed(const TCoeff* __restrict__ coeffBase, TCoeff* __restrict__ levelBase,
                                                  const vvcgpu_depquant_desc* __restrict__ descs, const int* __restrict__ list, int n,
                                                  const vvcgpu_dq_rates* __restrict__ ratesBase, int bd, unsigned* __restrict__ absSumOut,
                                                  unsigned* __restrict__ wsDec, unsigned char* __restrict__ wsCtx, VvcTrTables tb)
{
#include "depquant_body.inc"
}
__global__ __launch_bounds__(256) void depquant_listed_kernel(const TCoeff* __restrict__ coeffBase, TCoeff* __restrict__ levelBase,
                                                              const vvcgpu_depquant_desc* __restrict__ descs, const int* __restrict__ list,
                                                              const int* __restrict__ count,
                                                              const vvcgpu_dq_rates* __restrict__ ratesBase, int bd, unsigned* __restrict__ absSumOut,
                                                              unsigned* __restrict__ wsDec, unsigned char* __restrict__ wsCtx, VvcTrTables tb)
{
  const int n = *count;                                                   // the served records of the call, counted by the caller's front kernel
  if ((int)blockIdx.x * 64 >= n) return;
  tq_trellis_listed<true>(coeffBase, levelBase, descs, list, n, ratesBase, bd, absSumOut, wsDec, wsCtx, tb);
}

}  // namespace

int vvcgpu_depquant_listed_launch(const vvc_coef* coef, vvc_coef* level, const vvcgpu_depquant_desc* recs, const int* list, const int* count, int max_records,
                                  const vvcgpu_dq_rates* rates, int bit_depth, uint32_t* abs_sum, unsigned* dec, unsigned char* ctx, const VvcTrTables& tb,
                                  hipStream_t stream)
{
  VVC_HIP(vvc_allow_lds(depquant_listed_kernel, TQ_LDS_BYTES));           // (nothing to do below 48 KB, so nothing that could fail with a counter set taken)
  hipLaunchKernelGGL(depquant_listed_kernel, dim3(cdiv(max_records, 64)), dim3(256), TQ_LDS_BYTES, stream, coef, level, recs, list, count, rates, bit_depth,
                     abs_sum, dec, ctx, tb);
  VVC_LAUNCH_CHECK_COUNTERS(stream);
  return VVCGPU_OK;
}

extern "C" {

size_t vvcgpu_depquant_workspace_bytes(size_t total_coeffs, int n)
{
  (void)n;
  const size_t c = (total_coeffs + 15) & ~(size_t)15;
  return tq_dec_bytes(c) + tq_ctx_bytes(c) + 256;
}

int vvcgpu_depquant_batch(const vvc_coef* coeff_base, vvc_coef* level_base, const vvcgpu_depquant_desc* descs, int n,
                          const vvcgpu_dq_rates* rates, int bit_depth, uint32_t* abs_sum, size_t total_coeffs, void* ws, size_t ws_bytes,
                          void* stream)
{
  VVC_CHECK_ARG(n >= 0, "depquant_batch: n %d", n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(coeff_base && level_base && descs && rates && abs_sum && ws, "depquant_batch: null pointer");
  VVC_CHECK_ARG(bit_depth >= 8 && bit_depth <= 10, "depquant_batch: bit depth %d outside 8..10", bit_depth);
  VVC_CHECK_ARG(total_coeffs >= 16 && ws_bytes >= vvcgpu_depquant_workspace_bytes(total_coeffs, n) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
                "depquant_batch: workspace of %zu bytes for %zu coefficients is too small (need %zu) or unaligned", ws_bytes, total_coeffs,
                vvcgpu_depquant_workspace_bytes(total_coeffs, n));
  VvcTrTables tb;
  const int rt = vvcgpu_tr_tables(&tb);
  if (rt) return rt;
  // the workspace is split as vvcgpu_depquant_workspace_bytes lays it out: the decisions, then the level histories
  const size_t c = (total_coeffs + 15) & ~(size_t)15;
  unsigned* dec = static_cast<unsigned*>(ws);
  unsigned char* ctx = static_cast<unsigned char*>(ws) + tq_dec_bytes(c);
  VVC_HIP(vvc_allow_lds(depquant_kernel, TQ_LDS_BYTES));
  hipLaunchKernelGGL(depquant_kernel, dim3(cdiv(n, 64)), dim3(256), TQ_LDS_BYTES, (hipStream_t)stream, coeff_base, level_base, descs, n, rates, bit_depth,
                     abs_sum, dec, ctx, tb);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
