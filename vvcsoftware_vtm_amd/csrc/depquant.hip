// depquant.hip -- vvcgpu_depquant_batch: the dependent-quantisation trellis, DQIntern::DepQuant::quant (DepQuant.cpp:1323-1391), over an array of
// descriptors.  The trellis itself is stated in depquant_dev.h and depquant_body.inc; here are the kernel's signature and the entry points.
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

}  // namespace

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
