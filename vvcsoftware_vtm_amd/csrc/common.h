// common.h -- shared plumbing of the HIP hot-path library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>
#include "vvcgpu.h"

typedef int16_t Pel;
typedef int32_t TCoeff;

void vvcgpu_set_error(const char* fmt, ...);
// The device workspace of ONE call of an entry point, opened at its top (lib.hip): take<T>(count) returns `count` T, aligned to `align` bytes, that no
// other claim of the scope overlaps (nullptr, error text set, on failure).  Helpers claim from their caller's scope.  The memory is the stream's cached
// buffer: work on one stream is ordered, so the previous call's claims are free again when this call's kernels start.
class VvcScratch
{
public:
  explicit VvcScratch(hipStream_t stream) : stream_(stream) {}
  ~VvcScratch();                                                              // retires the buffers this call outgrew (lib.hip)
  VvcScratch(const VvcScratch&) = delete; VvcScratch& operator=(const VvcScratch&) = delete;
  template <class T> T* take(size_t count, size_t align = 64) { return static_cast<T*>(take_bytes(count * sizeof(T), align)); }
private:
  void* take_bytes(size_t bytes, size_t align);
  hipStream_t stream_;
  int device_ = -1;                                                           // looked up by the first claim
  size_t used_ = 0;                                                           // end of the last claim in the stream's buffer
  std::vector<void*> outgrown_;
};
int* vvcgpu_iota(hipStream_t stream, int n);                                 // device array 0, 1, .. of at least n ints, persistent per stream (lib.hip)
// Per-device constant images (lib.hip): image `key` of the current device, built by its first user -- build(dst, arg) into `bytes` of new device memory
// (bytes 0: none, a symbol upload) on the null stream, then a device synchronisation -- and released by vvcgpu_shutdown.  Returns VVCGPU_OK (*image: the
// memory, if image is not null) or an error code with the text set.
enum { VVC_IMAGE_TR_TABLES, VVC_IMAGE_TR_F16, VVC_IMAGE_MC, VVC_IMAGE_FRAC = VVC_IMAGE_MC + 3, VVC_IMAGE_KEYS = VVC_IMAGE_FRAC + 3 };   // MC, FRAC: + bit depth - 8
int vvcgpu_device_image(int key, size_t bytes, int (*build)(void* dst, const void* arg), const void* arg, void** image);
// The ONE behaviour switch of the library (read per call): VVCGPU_NO_MFMA=1 keeps the interpolation filters, the Hadamard refinement and the
// transforms off the matrix cores (the vector-pipe bodies that otherwise serve flagged PUs / TUs take everything) -- tests/test_gpu_no_mfma.py runs the
// parity cases of those bodies under it.  Every other environment variable the library reads is a measurement aid (VVCGPU_*_DIAG: cycle stamps to
// stderr) or a test hook (VVCGPU_MH_WGS: number of persistent workgroups of the hierarchical search).
int vvcgpu_no_mfma(void);
// eager construction of the per-device table images (vvcgpu_warmup, lib.hip): each returns VVCGPU_OK or an error code with the text set
int vvcgpu_mc_image_build(int bit_depth);          // interp.hip
int vvcgpu_frac_image_build(int bit_depth);        // fracsearch.hip
int vvcgpu_tr_image_build(void);                   // resichain.hip (the tables of transform.hip + f16 image)
int vvcgpu_cu_count(void);                         // compute units of the current device (queried once per device; 256 if the query fails)
constexpr int VVC_CTR_INTS = 32;                       // ints per counter set of vvcgpu_counters
int* vvcgpu_counters(hipStream_t stream, int* cur);     // two persistent zeroed work counters per (device, stream), see lib.hip
void vvcgpu_counters_failed(hipStream_t stream);       // a launch that took a counter set failed: both sets are cleared before their next use
int vvcgpu_frac_refine_launch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_frac_blk* blocks, int nblocks,
                              int w, int h, int bit_depth, int clp_min, int clp_max, int use_hadamard, const vvcgpu_mvcost* mvcost_host,
                              const int* preds, vvcgpu_frac_result* results, void* stream);
// the motion compensation behind vvcgpu_mc_batch / vvcgpu_mc_picture_batch and the affine entry points (interp.hip); it claims its work list from
// the caller's scope.  skip_fast: the caller knows that no descriptor is one of the fast kernel's shapes (affine sub-blocks): its launch is left out
// -- 65 k workgroups that only look at their descriptors and leave cost 80 us for the 518 k sub-blocks of a 4K picture
int vvcgpu_mc_batch_impl(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base, const vvcgpu_mc_desc* descs, int n, int bit_depth,
                         int clp_min, int clp_max, void* stream, VvcScratch& sc, bool skip_fast, bool sub44, bool serve_in_kernel = false);

// Raster stage of whole-PU TZ searches as its own launch (tzsearch.hip -> sadsearch.hip): one record per PU, written on the device.  An active
// PU's raster is the nx x ny grid of step 5 whose position (0, 0) is the motion vector (x0, y0); blocks[] holds the block's origin in the
// original and the reference position of the ZERO vector (as in vvcgpu_sad_search); the best candidate comes back as the packed
// key (cost << 24 | j * nx + i) in best[].cost (all-ones: no candidate).  Every PU of the launch is w x h with row sub-sampling sub_shift.
struct VvcRasterPer { int active, nx, ny, x0, y0, pred_hor, pred_ver, reserved; };
int vvcgpu_raster_per_block_launch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_search_blk* blocks,
                                   const VvcRasterPer* per, int nblocks, int w, int h, int sub_shift, int nx_max, int ny_max,
                                   const vvcgpu_mvcost* mvcost_host, vvcgpu_search_best* best, unsigned* packed_workspace, hipStream_t stream);

// device addresses (current device) of the transform matrices as int32 (tr32[type][size] row-major T[k][n] at type * 5460 + (n n - 4) / 3, tr32t its
// transpose), of the coefficient scans and their inverse, raster position -> scan index (scan / dqInv + scanOff[(log2 w - 1) * 6 + log2 h - 1]) and of the
// shape-only part of the trellis' position records (dqPosSel, dqPosMisc: same offsets).  Defined and uploaded, on first use, in transform.hip alone; device
// code is compiled per source, so the kernels of every other source (resichain.hip, quant.hip, depquant.hip, rdoq.hip) take this struct as an argument.
struct VvcTrTables { const int* tr32; const int* tr32t; const unsigned short* scan; const unsigned short* dqInv; const int* scanOff; const uint4* dqPosSel; const uint2* dqPosMisc; };
int vvcgpu_tr_tables(VvcTrTables* out);
// The dependent-quantisation trellis over a work list (depquant.hip, for the RD pass entries under DepQuant 1): work item ti is record list[ti], and
// *count, on the device, is the list's length -- a front kernel of the caller has counted it on a counter set of vvcgpu_counters.  The grid is sized for
// max_records; workgroups behind the list's end leave at once.  dec, ctx: the trellis' decisions and level histories, indexed as coef is.  Returns
// VVCGPU_OK or an error code with the text set; a failed launch has reported the caller's counter set itself (vvcgpu_counters_failed).
int vvcgpu_depquant_listed_launch(const vvc_coef* coef, vvc_coef* level, const vvcgpu_depquant_desc* recs, const int* list, const int* count, int max_records,
                                  const vvcgpu_dq_rates* rates, int bit_depth, uint32_t* abs_sum, unsigned* dec, unsigned char* ctx, const VvcTrTables& tb,
                                  hipStream_t stream);

#define VVC_CHECK_ARG(cond, ...)                                   \
  do { if (!(cond)) { vvcgpu_set_error(__VA_ARGS__); return VVCGPU_E_ARG; } } while (0)

#define VVC_HIP(call)                                                                        \
  do { hipError_t e_ = (call); if (e_ != hipSuccess) {                                       \
         vvcgpu_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
         return VVCGPU_E_DEVICE; } } while (0)

// A kernel may use more than 48 KB of dynamic LDS only after this has been allowed for it: VVC_HIP(vvc_allow_lds(kernel, bytes)) in front of the launch
// (host-only and idempotent, so it is simply repeated per call; nothing to do up to 48 KB)
template <class K> static inline hipError_t vvc_allow_lds(K kernel, size_t bytes)
{
  if (bytes <= 48 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

#define VVC_LAUNCH_CHECK()                                                                    \
  do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) {                            \
         vvcgpu_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
         return VVCGPU_E_DEVICE; } } while (0)

// the same for launches that own a counter set of vvcgpu_counters: a failure leaves the sets in an unknown state
#define VVC_LAUNCH_CHECK_COUNTERS(st)                                                         \
  do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) {                            \
         vvcgpu_counters_failed(st);                                                         \
         vvcgpu_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
         return VVCGPU_E_DEVICE; } } while (0)

// XCD-aware order of a one-dimensional grid (speed only, never correctness): workgroups are dealt round-robin over the 8 XCDs, each with its own L2.
// A picture pass whose neighbouring tiles share halo lines gives every XCD one CONTIGUOUS run of the logical tile indices, so that a 128-byte
// line is fetched from the fabric by one L2 instead of by up to three (profiles/r03_fabric_requests.csv: the picture passes read 1.6 - 3.1 x
// their planes, every request a whole 128-byte line).  Launch vvc_xcd_grid(total) workgroups; padding workgroups get -1 and leave.
static inline int vvc_xcd_on() { return 1; }
static inline int vvc_xcd_grid(int total, int on) { return on ? ((total + 7) >> 3) << 3 : total; }
// two index ranges [0, nA) and [nA, total) (luma tiles, then chroma tiles), each spread over the XCDs on its own: the heavy and the light part of a
// launch both reach every XCD
static inline int vvc_xcd_grid2(int nA, int total, int on) { return on ? vvc_xcd_grid(nA, 1) + vvc_xcd_grid(total - nA, 1) : total; }
#ifdef __HIPCC__
__device__ __forceinline__ int vvc_xcd_index(int bid, int total, int on)
{
  if (!on) return bid;
  const int chunk = (total + 7) >> 3, i = (bid & 7) * chunk + (bid >> 3);
  return i < total ? i : -1;
}
__device__ __forceinline__ int vvc_xcd_index2(int bid, int nA, int total, int on)
{
  if (!on) return bid;
  const int gridA = ((nA + 7) >> 3) << 3;
  if (bid < gridA) return vvc_xcd_index(bid, nA, 1);
  const int i = vvc_xcd_index(bid - gridA, total - nA, 1);
  return i < 0 ? -1 : nA + i;
}
#endif

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// the grid of a launch that gives every item a wavefront, `waves` to a workgroup (1: a workgroup), and walks the items with at most per_cu workgroups per
// compute unit
static inline int vvc_grid_cap(long long items, int waves, int per_cu)
{
  const long long cap = (long long)per_cu * vvcgpu_cu_count(), wgs = (items + waves - 1) / waves;
  return (int)(wgs < cap ? wgs : cap);
}

__device__ __forceinline__ int clip3(int lo, int hi, int v) { return min(max(v, lo), hi); }
__device__ __forceinline__ int sgn(int v) { return (v > 0) - (v < 0); }
__device__ __forceinline__ int ilog2(int v) { return 31 - __clz(v); }
// a block side that the RD pass entries serve: a power of two from lo (2 or 4) to 64
inline __host__ __device__ bool side_ok(int v, int lo) { return v >= lo && v <= 64 && (v & (v - 1)) == 0; }

// A wavefront that owns its work orders its own lanes without a workgroup barrier: wave_sync for what they exchange through LDS, wave_global_sync for
// stores of the wavefront to global memory that other lanes of it read back.
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ void wave_global_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// 8 Pels = 16 bytes, the coalescing sweet spot for int16 planes (guide G13)
typedef short pel8 __attribute__((ext_vector_type(8)));
typedef short pel4 __attribute__((ext_vector_type(4)));
typedef short pel2 __attribute__((ext_vector_type(2)));
typedef int   int4v __attribute__((ext_vector_type(4)));
