// alfdecide.hip -- what EncAdaptiveLoopFilter::alfEncoder reads of the per-CTU covariance records, served where the records are:
//   vvcgpu_alf_frame_stats  getFrameStat (EncAdaptiveLoopFilter.cpp:1303-1315): the sum of the records of the enabled CTUs;
//   vvcgpu_alf_ctu_dist     getUnfilteredDistortion(cov, numClasses) (:618-626) and getFilteredDistortion (:628-639, calcErrorForCoeffs :1157-1174)
//                           of every CTU, as deriveCtbAlfEnableFlags (:272-331) asks for them.
// The records are those vvcgpu_alf_stats / _stats_picture / _classify_stats_picture write: per CTU x class int64 E[N][N], y[N], pixAcc.
// The frame sums are int64 (exact and order-free below 2^53, see vvcgpu.h); the distortions are IEEE double arithmetic in the reference's
// order with contraction off: only the row chains of one class run side by side, everything the reference adds up in sequence is added up in
// that sequence by one lane.
#include "common.h"

namespace {

#pragma clang fp contract(off)

// ---- frame sums --------------------------------------------------------------------------------------------------------------------------------
// A memory-bound reduction over n_ctu records of R = n_classes * n_vals int64.  Thread = one value of the record (consecutive lanes, consecutive
// values), workgroup = 256 values x one slice of FS_SLICE consecutive CTUs.  The enable flags of the slice are read into a bit mask by scalar
// code, so a disabled CTU's record is never touched; the loads of the enabled ones are all issued before the first is added.  One 64-bit atomic
// per thread and slice: ceil(n_ctu / 8) adds per address (64 for a 4K picture of 128x128 CTUs), integer, hence independent of their order.
constexpr int FS_SLICE = 8;
constexpr int FS_THREADS = 256;

__global__ __launch_bounds__(FS_THREADS) void alf_frame_stats_kernel(const int64_t* __restrict__ stats, int nCtu, int R, int nbx,
                                                                     const uint8_t* __restrict__ enable, unsigned long long* __restrict__ out)
{
  const int slice = blockIdx.x / nbx, v = (blockIdx.x - slice * nbx) * FS_THREADS + threadIdx.x;
  const int c0 = slice * FS_SLICE;
  unsigned mask = 0;
  if (enable)
  {
    uint8_t en[FS_SLICE];                                                                    // all eight flag loads in flight together (index clamped, masked below)
#pragma unroll
    for (int k = 0; k < FS_SLICE; k++) en[k] = enable[min(c0 + k, nCtu - 1)];
#pragma unroll
    for (int k = 0; k < FS_SLICE; k++) mask |= (en[k] ? 1u : 0u) << k;
  }
  else mask = (1u << FS_SLICE) - 1;
  mask = __builtin_amdgcn_readfirstlane(mask & ((1u << min(FS_SLICE, nCtu - c0)) - 1));   // the same in every lane: the branches below are scalar
  if (!mask || v >= R) return;
  const int64_t* p = stats + (size_t)c0 * R + v;
  int64_t val[FS_SLICE];
#pragma unroll
  for (int k = 0; k < FS_SLICE; k++) val[k] = (mask >> k) & 1 ? p[(size_t)k * R] : 0;
  int64_t acc = 0;
#pragma unroll
  for (int k = 0; k < FS_SLICE; k++) acc += val[k];
  atomicAdd(out + v, (unsigned long long)acc);
}

// ---- per-CTU distortions -----------------------------------------------------------------------------------------------------------------------
struct AlfDecideTables { int32_t coeff[25 * 13]; int16_t idx[25]; int16_t nCoeffVals; };   // passed by value in the kernel argument block

__device__ __forceinline__ double alf_dbl(int64_t v) { return (double)v; }                  // exact: |v| < 2^53 is the entry's precondition

// Workgroup = one CTU, 16-lane group = one class (seven waves hold the 25 classes; one wave for the single chroma class), lane = row i of
// calcErrorForCoeffs.  The CTU's record (25 x 1464 contiguous bytes for 7x7) is copied to LDS with 16-byte loads -- a record starts on an 8-byte
// boundary only, so the LDS image is shifted by one value where needed and the first / last value go alone -- because a lane reading its own
// 104-byte row from memory would touch every line several times.  `inv` = 1 / factor, factor = 2^(coeff_bits - 1): multiplying by it is the
// reference's division bit for bit (a power of two, no result near the subnormal range: the operands are integers).
template <int N>
__global__ __launch_bounds__(448) void alf_ctu_dist_kernel(const int64_t* __restrict__ stats, int nCls, AlfDecideTables t, double inv, double* __restrict__ out)
{
  constexpr int NV = N * N + N + 1;
  __shared__ __attribute__((aligned(16))) int64_t rec[25 * NV + 2];
  __shared__ double coef[25 * N];
  __shared__ double clsErr[25], clsPix[25];
  const int tid = threadIdx.x, nthr = blockDim.x, T = nCls * NV;
  const int64_t* g = stats + (size_t)blockIdx.x * T;
  const int o = (int)(((uintptr_t)g >> 3) & 1);                                            // rec[o + k] = g[k]: g + k is 16-byte aligned where o + k is even
  typedef int64_t ll2 __attribute__((ext_vector_type(2)));
  constexpr int PASSES = (25 * NV / 2 + 448) / 448;                                        // pairs of the largest record over the 448 threads that come with it
  ll2 v[PASSES];                                                                            // (one class: 64 threads, fewer passes still); all loads first
#pragma unroll
  for (int k = 0; k < PASSES; k++)
  {
    const int j = o + tid + k * nthr;
    if (2 * j + 1 - o < T) v[k] = *reinterpret_cast<const ll2*>(g + 2 * j - o);
  }
#pragma unroll
  for (int k = 0; k < PASSES; k++)
  {
    const int j = o + tid + k * nthr;
    if (2 * j + 1 - o < T) *reinterpret_cast<ll2*>(rec + 2 * j) = v[k];
  }
  if (tid == 0 && o) rec[1] = g[0];
  if (tid == 1 && ((o + T) & 1)) rec[o + T - 1] = g[T - 1];
  for (int k = tid; k < t.nCoeffVals; k += nthr) coef[k] = (double)t.coeff[k];
  __syncthreads();

  const int cls = tid >> 4, i = tid & 15;
  if (cls < nCls)                                                                           // whole 16-lane groups: the shuffles below stay inside one
  {
    const int64_t* r = rec + o + cls * NV;                                                  // E[N][N], y[N], pixAcc
    const double* c = coef + (int)t.idx[cls] * N;
    double term = 0.0;
    if (i < N)
    {
      double sum = 0.0;
      for (int j = i + 1; j < N; j++) sum += alf_dbl(r[i * N + j]) * c[j];
      term = ((alf_dbl(r[i * N + i]) * c[i] + sum * 2.0) * inv - 2.0 * alf_dbl(r[N * N + i])) * c[i];
    }
    double error = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) error += __shfl(term, k, 16);
    if (i == 0) { clsErr[cls] = error * inv; clsPix[cls] = alf_dbl(r[N * N + N]); }
  }
  __syncthreads();
  if (tid < 2)                                                                              // the class folds, in class order: lane 0 pixAcc, lane 1 the errors
  {
    const double* s = tid ? clsErr : clsPix;
    double d = 0.0;
    for (int k = 0; k < nCls; k++) d += s[k];
    out[(size_t)blockIdx.x * 2 + tid] = d;
  }
}

}  // namespace

extern "C" {

int vvcgpu_alf_frame_stats(const int64_t* ctu_stats, int n_ctu, int n_classes, int n_vals, const uint8_t* enable, int accumulate,
                           int64_t* frame_out, void* stream)
{
  VVC_CHECK_ARG(n_ctu >= 0, "alf_frame_stats: n_ctu %d", n_ctu);
  VVC_CHECK_ARG(n_classes == 1 || n_classes == 25, "alf_frame_stats: n_classes %d (1 or 25)", n_classes);
  VVC_CHECK_ARG(n_vals == 57 || n_vals == 183, "alf_frame_stats: n_vals %d (57 or 183)", n_vals);
  if (n_ctu == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(ctu_stats && frame_out, "alf_frame_stats: null pointer");
  const int R = n_classes * n_vals;
  if (!accumulate) VVC_HIP(hipMemsetAsync(frame_out, 0, sizeof(int64_t) * R, (hipStream_t)stream));
  const int nbx = cdiv(R, FS_THREADS), slices = cdiv(n_ctu, FS_SLICE);
  VVC_CHECK_ARG((long long)nbx * slices <= 0x7fffffffLL, "alf_frame_stats: n_ctu %d is too many", n_ctu);
  hipLaunchKernelGGL(alf_frame_stats_kernel, dim3(nbx * slices), dim3(FS_THREADS), 0, (hipStream_t)stream, ctu_stats, n_ctu, R, nbx, enable,
                     reinterpret_cast<unsigned long long*>(frame_out));
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

int vvcgpu_alf_ctu_dist(const int64_t* ctu_stats, int n_ctu, int n_classes, int filter_type, const int32_t* coeff_set_host, int n_filters,
                        const int16_t* filter_idx_host, int coeff_bits, double* dist_out, void* stream)
{
  VVC_CHECK_ARG(n_ctu >= 0, "alf_ctu_dist: n_ctu %d", n_ctu);
  VVC_CHECK_ARG(n_classes == 1 || n_classes == 25, "alf_ctu_dist: n_classes %d (1 or 25)", n_classes);
  VVC_CHECK_ARG(filter_type == 0 || filter_type == 1, "alf_ctu_dist: filter_type %d", filter_type);
  VVC_CHECK_ARG(n_filters >= 1 && n_filters <= 25, "alf_ctu_dist: n_filters %d (1..25)", n_filters);
  VVC_CHECK_ARG(coeff_bits >= 2 && coeff_bits <= 16, "alf_ctu_dist: coeff_bits %d (2..16)", coeff_bits);
  VVC_CHECK_ARG(coeff_set_host && (filter_idx_host || n_classes == 1), "alf_ctu_dist: null table");
  const int N = filter_type ? 13 : 7;
  AlfDecideTables t;
  memset(&t, 0, sizeof t);
  for (int c = 0; c < n_classes && filter_idx_host; c++)
  {
    VVC_CHECK_ARG(filter_idx_host[c] >= 0 && filter_idx_host[c] < n_filters, "alf_ctu_dist: filter index %d of class %d is outside the set of %d",
                  (int)filter_idx_host[c], c, n_filters);
    t.idx[c] = filter_idx_host[c];
  }
  memcpy(t.coeff, coeff_set_host, sizeof(int32_t) * n_filters * N);
  t.nCoeffVals = (int16_t)(n_filters * N);
  if (n_ctu == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(ctu_stats && dist_out, "alf_ctu_dist: null pointer");
  const double inv = 1.0 / (double)(1 << (coeff_bits - 1));
  const dim3 block(n_classes == 25 ? 448 : 64);
  if (filter_type) hipLaunchKernelGGL(alf_ctu_dist_kernel<13>, dim3(n_ctu), block, 0, (hipStream_t)stream, ctu_stats, n_classes, t, inv, dist_out);
  else             hipLaunchKernelGGL(alf_ctu_dist_kernel<7>, dim3(n_ctu), block, 0, (hipStream_t)stream, ctu_stats, n_classes, t, inv, dist_out);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"
