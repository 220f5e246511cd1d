// lib.hip -- library-level entry points of the C ABI (include/vvcgpu.h).
#include "common.h"
#include <algorithm>
#include <atomic>
#include <mutex>
#include <stdarg.h>
#include <string.h>

static thread_local char g_err[512] = "";

void vvcgpu_set_error(const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

// ---- per-(device, stream) resources: scratch buffer (VvcScratch), identity array (vvcgpu_iota), two persistent zeroed counter sets.  One table behind
// one mutex; slots are created on first use, released by vvcgpu_stream_release (before the host destroys the stream) or all at once by vvcgpu_shutdown.
// An outgrown buffer is NOT freed on the spot -- queued work may still read it, and hipFree synchronises the device -- but parked behind an event, freed
// once that has completed (at a later growth) or with the slot.  Capacity at least doubles, so the parked buffers sum to less than the live one.  No
// entry point allocates, frees, queues work or synchronises anything while it holds the mutex (hipEventQuery in retire() does not wait); the one
// exception is vvcgpu_shutdown, which holds both mutexes for its whole length on purpose.  One host thread drives a stream at a time
// (include/vvcgpu.h): between two lookups of one call nobody else creates, changes or releases THAT stream's slot -- which is why retire(),
// vvcgpu_iota and vvcgpu_counters may drop the lock, allocate, and look the slot up again (with create = true: the second lookup finds the slot
// of the first, possibly at another address, since other threads' slots come and go and the vector re-allocates; a pointer into g_slots is never kept
// across an unlock).  tests/test_gpu_threads.py runs this with 4 and 8 threads.
namespace {
struct Retired { void* ptr; hipEvent_t done; };
struct StreamSlot
{
  int device; hipStream_t stream;
  void* scratch = nullptr; size_t scratchCap = 0;
  int* iota = nullptr; int iotaN = 0;                       // the identity array 0 .. iotaN - 1
  std::vector<Retired> retired;                             // outgrown buffers
  int* counters = nullptr; int cur = 0; bool dirty = false; // int[2][VVC_CTR_INTS]; dirty: a launch that owned a set failed -- both are cleared before the next use
};
std::vector<StreamSlot> g_slots;
std::mutex g_slotMutex;

StreamSlot* find_slot(int dev, hipStream_t stream, bool create)
{
  for (auto& s : g_slots)
    if (s.device == dev && s.stream == stream) return &s;
  if (!create) return nullptr;
  g_slots.push_back(StreamSlot{ dev, stream });
  return &g_slots.back();
}
void free_slot(StreamSlot& s)             // the slot is out of the table (or the caller holds the mutex at shutdown), its device is current, its stream is idle
{
  if (s.scratch) (void)hipFree(s.scratch);
  if (s.iota) (void)hipFree(s.iota);
  for (auto& q : s.retired) { (void)hipFree(q.ptr); if (q.done) (void)hipEventDestroy(q.done); }
  s.retired.clear();
  if (s.counters) (void)hipFree(s.counters);
}

// a buffer of at least `bytes` that replaces one of `have` bytes: whole MiB, at least doubling -- the request alone when the doubled size does not fit
void* grow_alloc(size_t bytes, size_t have, size_t* cap, const char* who)
{
  const size_t need = (bytes + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
  for (size_t c : { std::max(need, 2 * have), need })
  {
    void* p = nullptr;
    if (hipMalloc(&p, c) == hipSuccess) { *cap = c; return p; }
    (void)hipGetLastError();                                                // a failed attempt must not surface at the caller's next launch check
  }
  vvcgpu_set_error("%s: hipMalloc(%zu) failed", who, need);
  return nullptr;
}

// parks an outgrown buffer of the stream behind an event recorded after the work queued so far; parked buffers whose event has completed are freed
// here (growth is rare), outside the lock
void retire(int dev, hipStream_t stream, void* p)
{
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, stream) != hipSuccess)
  { (void)hipGetLastError(); if (ev) (void)hipEventDestroy(ev); ev = nullptr; }   // no event: the buffer stays parked until the slot goes
  std::vector<Retired> done;
  {
    std::lock_guard<std::mutex> lock(g_slotMutex);
    StreamSlot* slot = find_slot(dev, stream, true);
    auto& r = slot->retired;
    const auto finished = std::partition(r.begin(), r.end(), [](const Retired& q) { return !q.done || hipEventQuery(q.done) != hipSuccess; });
    done.assign(finished, r.end()); r.erase(finished, r.end());
    (void)hipGetLastError();                                                // hipErrorNotReady of a query is not an error of the caller
    slot->retired.push_back(Retired{ p, ev });
  }
  for (auto& q : done) { (void)hipFree(q.ptr); (void)hipEventDestroy(q.done); }
}
}

// A claim that does not fit moves the stream to a new buffer that holds the whole scope so far (the next call of the same shape fits); the claims
// already made stay where they are, and the outgrown buffer is retired when the scope closes, behind every launch of the call.
void* VvcScratch::take_bytes(size_t bytes, size_t align)
{
  if (device_ < 0 && hipGetDevice(&device_) != hipSuccess) { device_ = -1; vvcgpu_set_error("hipGetDevice failed"); return nullptr; }
  const size_t at = (used_ + align - 1) & ~(align - 1), end = at + (bytes ? bytes : 1);
  size_t have = 0;
  {
    std::lock_guard<std::mutex> lock(g_slotMutex);
    StreamSlot* slot = find_slot(device_, stream_, true);
    if (slot->scratchCap >= end) { used_ = end; return static_cast<char*>(slot->scratch) + at; }   // the hot path: no allocation, no event, no free
    have = slot->scratchCap;
  }
  size_t cap = 0;
  void* p = grow_alloc(end, have, &cap, "scratch");
  if (!p) return nullptr;
  void* old = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_slotMutex);                         // looked up again: the table may have been re-allocated
    StreamSlot* slot = find_slot(device_, stream_, true);
    old = slot->scratch; slot->scratch = p; slot->scratchCap = cap;
  }
  if (old) outgrown_.push_back(old);
  used_ = end;
  return static_cast<char*>(p) + at;
}
VvcScratch::~VvcScratch()
{
  for (void* p : outgrown_) retire(device_, stream_, p);
}

// identity array 0, 1, 2, ... of at least n ints, persistent per (device, stream): written by a launch on that stream when it is first needed or has to
// grow (geometrically, like the scratch), read by every later call (vvcgpu_resi_chain_runs_batch: class lists as ranges of it)
namespace { __global__ void iota_kernel(int* p, int first, int n) { const int i = first + blockIdx.x * 256 + threadIdx.x; if (i < n) p[i] = i; } }
int* vvcgpu_iota(hipStream_t stream, int n)
{
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { vvcgpu_set_error("hipGetDevice failed"); return nullptr; }
  int* old = nullptr; int have = 0;
  {
    std::lock_guard<std::mutex> lock(g_slotMutex);
    StreamSlot* slot = find_slot(dev, stream, true);
    if (slot->iotaN >= n) return slot->iota;                                // the hot path
    old = slot->iota; have = slot->iotaN;
  }
  size_t cap = 0;
  int* p = static_cast<int*>(grow_alloc((size_t)n * sizeof(int), (size_t)have * sizeof(int), &cap, "iota"));
  if (!p) return nullptr;
  const int valid = (int)std::min<size_t>(cap / sizeof(int), (size_t)0x7FFFFFFF);   // the whole buffer is filled
  hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((valid + 255) / 256)), dim3(256), 0, stream, p, 0, valid);
  if (hipGetLastError() != hipSuccess) { (void)hipFree(p); vvcgpu_set_error("iota: kernel launch failed"); return nullptr; }
  {
    std::lock_guard<std::mutex> lock(g_slotMutex);                         // committed only once the fill is queued
    StreamSlot* slot = find_slot(dev, stream, true);
    slot->iota = p; slot->iotaN = valid;
  }
  if (old) retire(dev, stream, old);                                        // queued work of earlier calls may still read it
  return p;
}

// ---- per-device constant images (common.h): one registry behind one mutex, held while an image is built
namespace {
constexpr int VVC_MAX_DEVICES = 64;
struct DeviceImage { void* ptr; bool built; };
DeviceImage g_images[VVC_MAX_DEVICES][VVC_IMAGE_KEYS];
std::mutex g_imageMutex;
}

int vvcgpu_device_image(int key, size_t bytes, int (*build)(void* dst, const void* arg), const void* arg, void** image)
{
  int dev = 0;
  VVC_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= VVC_MAX_DEVICES) { vvcgpu_set_error("table image %d: device index %d out of range", key, dev); return VVCGPU_E_DEVICE; }
  std::lock_guard<std::mutex> lock(g_imageMutex);
  DeviceImage& img = g_images[dev][key];
  if (!img.built)
  {
    // built on the null stream, then a device synchronisation (not on the caller's stream: that would serialise every other thread's first call
    // behind a stream of unknown length); the memory is freed again if any step fails
    void* p = nullptr;
    if (bytes && hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); vvcgpu_set_error("table image %d: hipMalloc(%zu) failed", key, bytes); return VVCGPU_E_DEVICE; }
    int rc = build(p, arg);
    if (rc == VVCGPU_OK && hipDeviceSynchronize() != hipSuccess) { vvcgpu_set_error("building table image %d failed: %s", key, hipGetErrorString(hipGetLastError())); rc = VVCGPU_E_DEVICE; }
    if (rc != VVCGPU_OK) { (void)hipFree(p); return rc; }
    img = DeviceImage{ p, true };
  }
  if (image) *image = img.ptr;
  return VVCGPU_OK;
}

// Two persistent work counters per (device, stream), zero when handed out: a launch that needs a zeroed counter takes counter `cur` and clears
// counter `cur ^ 1` for the next call inside its own kernel (the previous user of that one has finished: same stream), so no fill launch is
// needed in front of it.  EVERY user clears all VVC_CTR_INTS ints of the other set, whatever it uses of its own.  Returns a device pointer to
// int[2][VVC_CTR_INTS] and the index to use; nullptr on failure.  A caller whose launches fail after this call reports it with
// vvcgpu_counters_failed: the sets are then cleared by a memset on the stream in front of the next user.
int* vvcgpu_counters(hipStream_t stream, int* cur)
{
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { vvcgpu_set_error("hipGetDevice failed"); return nullptr; }
  constexpr size_t bytes = 2 * VVC_CTR_INTS * sizeof(int);
  int* have = nullptr; bool clear = false;
  {
    std::lock_guard<std::mutex> lock(g_slotMutex);
    StreamSlot* slot = find_slot(dev, stream, true);
    if ((have = slot->counters) != nullptr)                                 // the hot path
    {
      clear = slot->dirty;
      if (clear) { slot->dirty = false; slot->cur = 0; }
      *cur = slot->cur;
      slot->cur ^= 1;
    }
  }
  if (have)
  {
    // the clearing is queued outside the lock, on the caller's stream: in front of the caller's kernels, behind the failed call's
    if (clear && hipMemsetAsync(have, 0, bytes, stream) != hipSuccess) { (void)hipGetLastError(); vvcgpu_counters_failed(stream); vvcgpu_set_error("counters: hipMemsetAsync failed"); return nullptr; }
    return have;
  }
  // first use on this stream: allocated and zeroed outside the lock.  The zeroing goes onto the CALLER's stream, so it is ordered in front of the first
  // kernel that reads the sets whatever kind of stream that is (a non-blocking stream does not wait for the null stream).
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); vvcgpu_set_error("counters: hipMalloc failed"); return nullptr; }
  if (hipMemsetAsync(p, 0, bytes, stream) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); vvcgpu_set_error("counters: hipMemsetAsync failed"); return nullptr; }
  {
    std::lock_guard<std::mutex> lock(g_slotMutex);                         // looked up again: the table may have been re-allocated
    StreamSlot* slot = find_slot(dev, stream, true);
    if (!slot->counters) { slot->counters = static_cast<int*>(p); slot->cur = 0; slot->dirty = false; p = nullptr; }
    have = slot->counters;
    *cur = slot->cur;
    slot->cur ^= 1;
  }
  if (p) (void)hipFree(p);                                                  // only if a second thread drove the stream meanwhile (outside the contract): its sets stay
  return have;
}
void vvcgpu_counters_failed(hipStream_t stream)
{
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> lock(g_slotMutex);
  if (StreamSlot* slot = find_slot(dev, stream, false)) slot->dirty = true;
}

int vvcgpu_no_mfma(void)
{
  const char* e = getenv("VVCGPU_NO_MFMA");                                 // read per call (a few hundred ns): tools toggle it inside one process
  return e && e[0] == '1';
}

// compute units of the current device, cached per device (persistent kernels size their grids with it on every call)
int vvcgpu_cu_count(void)
{
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int v = cached[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 8) cus = 256;
  cached[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

extern "C" {
int vvcgpu_version(void) { return 1; }
const char* vvcgpu_last_error(void) { return g_err; }
int vvcgpu_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int vvcgpu_malloc(void** dev_ptr, size_t bytes)
{
  VVC_CHECK_ARG(dev_ptr, "malloc: null out pointer");
  VVC_HIP(hipMalloc(dev_ptr, bytes ? bytes : 1));
  return VVCGPU_OK;
}
int vvcgpu_free(void* p) { if (p) VVC_HIP(hipFree(p)); return VVCGPU_OK; }
int vvcgpu_memcpy_h2d(void* d, const void* s, size_t n, void* st) { VVC_HIP(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, (hipStream_t)st)); return VVCGPU_OK; }
int vvcgpu_memcpy_d2h(void* d, const void* s, size_t n, void* st) { VVC_HIP(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, (hipStream_t)st)); return VVCGPU_OK; }
int vvcgpu_memcpy2d_h2d(void* d, size_t dp, const void* s, size_t sp, size_t wb, size_t h, void* st)
{ VVC_HIP(hipMemcpy2DAsync(d, dp, s, sp, wb, h, hipMemcpyHostToDevice, (hipStream_t)st)); return VVCGPU_OK; }
int vvcgpu_memcpy2d_d2h(void* d, size_t dp, const void* s, size_t sp, size_t wb, size_t h, void* st)
{ VVC_HIP(hipMemcpy2DAsync(d, dp, s, sp, wb, h, hipMemcpyDeviceToHost, (hipStream_t)st)); return VVCGPU_OK; }
int vvcgpu_memcpy2d_d2d(void* d, size_t dp, const void* s, size_t sp, size_t wb, size_t h, void* st)
{ VVC_HIP(hipMemcpy2DAsync(d, dp, s, sp, wb, h, hipMemcpyDeviceToDevice, (hipStream_t)st)); return VVCGPU_OK; }
int vvcgpu_stream_sync(void* st) { VVC_HIP(hipStreamSynchronize((hipStream_t)st)); return VVCGPU_OK; }
int vvcgpu_sizeof(int id)
{
  switch (id)
  {
  case 0: return (int)sizeof(vvcgpu_sao_ctu);
  case 1: return (int)sizeof(vvcgpu_deblock_cfg);
  case 2: return (int)sizeof(vvcgpu_dist_desc);
  case 3: return (int)sizeof(vvcgpu_search_blk);
  case 4: return (int)sizeof(vvcgpu_mvcost);
  case 5: return (int)sizeof(vvcgpu_search_best);
  case 6: return (int)sizeof(vvcgpu_if_desc);
  case 7: return (int)sizeof(vvcgpu_mc_desc);
  case 8: return (int)sizeof(vvcgpu_pelop_desc);
  case 9: return (int)sizeof(vvcgpu_pelop_cfg);
  case 10: return (int)sizeof(vvcgpu_tr_desc);
  case 11: return (int)sizeof(vvcgpu_frac_blk);
  case 12: return (int)sizeof(vvcgpu_frac_result);
  case 13: return (int)sizeof(vvcgpu_dqtr_desc);
  case 14: return (int)sizeof(vvcgpu_afg_desc);
  case 15: return (int)sizeof(vvcgpu_afe_desc);
  case 16: return (int)sizeof(vvcgpu_tz_pu);
  case 17: return (int)sizeof(vvcgpu_tz_cfg);
  case 18: return (int)sizeof(vvcgpu_intra_desc);
  case 19: return (int)sizeof(vvcgpu_cclm_desc);
  case 20: return (int)sizeof(vvcgpu_intra_fill_desc);
  case 21: return (int)sizeof(vvcgpu_imv_pu);
  case 22: return (int)sizeof(vvcgpu_imv_result);
  case 23: return (int)sizeof(vvcgpu_quant_desc);
  case 24: return (int)sizeof(vvcgpu_dq_rates);
  case 25: return (int)sizeof(vvcgpu_depquant_desc);
  case 26: return (int)sizeof(vvcgpu_rdoq_rates);
  case 27: return (int)sizeof(vvcgpu_rdoq_desc);
  case 28: return (int)sizeof(vvcgpu_intra_satd_desc);
  case 29: return (int)sizeof(vvcgpu_affine_iter);
  case 30: return (int)sizeof(vvcgpu_me_hier_cfg);
  case 31: return (int)sizeof(vvcgpu_wp_param);
  case 32: return (int)sizeof(vvcgpu_wp_sad_cand);
  case 33: return (int)sizeof(vvcgpu_tile_stats);
  case 34: return (int)sizeof(vvcgpu_affine_me_item);
  case 35: return (int)sizeof(vvcgpu_affine_me_cfg);
  case 36: return (int)sizeof(vvcgpu_affine_me_result);
  case 37: return (int)sizeof(vvcgpu_affine_me_step);
  case 38: return (int)sizeof(vvcgpu_bipred_me_ref);
  case 39: return (int)sizeof(vvcgpu_bipred_me_item);
  case 40: return (int)sizeof(vvcgpu_bipred_me_cfg);
  case 41: return (int)sizeof(vvcgpu_bipred_me_result);
  case 42: return (int)sizeof(vvcgpu_bipred_me_step);
  case 44: return (int)sizeof(vvcgpu_affine_bipred_ref);
  case 45: return (int)sizeof(vvcgpu_affine_bipred_item);
  case 46: return (int)sizeof(vvcgpu_affine_bipred_cfg);
  case 47: return (int)sizeof(vvcgpu_affine_bipred_result);
  case 48: return (int)sizeof(vvcgpu_affine_bipred_step);
  case 50: return (int)sizeof(vvcgpu_unipred_me_ref);
  case 51: return (int)sizeof(vvcgpu_unipred_me_item);
  case 52: return (int)sizeof(vvcgpu_unipred_me_cfg);
  case 53: return (int)sizeof(vvcgpu_unipred_me_search);
  case 54: return (int)sizeof(vvcgpu_unipred_me_result);
  case 56: return (int)sizeof(vvcgpu_affine_unipred_ref);
  case 57: return (int)sizeof(vvcgpu_affine_unipred_item);
  case 58: return (int)sizeof(vvcgpu_affine_unipred_cfg);
  case 59: return (int)sizeof(vvcgpu_affine_unipred_search);
  case 60: return (int)sizeof(vvcgpu_affine_unipred_result);
  case 62: return (int)sizeof(vvcgpu_intra_chroma_pu);
  case 63: return (int)sizeof(vvcgpu_inter_resi_item);
  case 65: return (int)sizeof(vvcgpu_inter_resi_dq);
  default: return -1;
  }
}
int vvcgpu_warmup(int bit_depth)
{
  if (bit_depth < 8 || bit_depth > 10) { vvcgpu_set_error("warmup: bit depth %d outside 8..10", bit_depth); return VVCGPU_E_UNSUPPORTED; }
  int rc = vvcgpu_tr_image_build();
  if (rc == VVCGPU_OK) rc = vvcgpu_mc_image_build(bit_depth);
  if (rc == VVCGPU_OK) rc = vvcgpu_frac_image_build(bit_depth);
  return rc;
}
int vvcgpu_set_device(int device)
{
  VVC_HIP(hipSetDevice(device));
  return VVCGPU_OK;
}
int vvcgpu_stream_release(void* stream)
{
  int dev = 0;
  VVC_HIP(hipGetDevice(&dev));
  // the slot of this stream handle -- on the current device first, else on whichever device holds one (a stream belongs to one device; the caller
  // may have switched devices since it used the stream).  Looked up under the lock; the drain of the stream runs WITHOUT it (other threads' entry
  // points keep going); the slot is taken out of the table under the lock again and freed outside it.
  int sdev = -1;
  {
    std::lock_guard<std::mutex> lock(g_slotMutex);
    for (auto& s : g_slots)
      if (s.stream == (hipStream_t)stream && (s.device == dev || sdev < 0)) { sdev = s.device; if (s.device == dev) break; }
  }
  if (sdev < 0) return VVCGPU_OK;                                           // nothing held for this stream
  if (sdev != dev) VVC_HIP(hipSetDevice(sdev));
  const hipError_t e = hipStreamSynchronize((hipStream_t)stream);           // queued work may still read the buffers
  if (e == hipSuccess)
  {
    StreamSlot taken{ sdev, nullptr };
    bool found = false;
    {
      std::lock_guard<std::mutex> lock(g_slotMutex);
      for (size_t i = 0; i < g_slots.size(); i++)
        if (g_slots[i].stream == (hipStream_t)stream && g_slots[i].device == sdev) { taken = g_slots[i]; g_slots.erase(g_slots.begin() + (ptrdiff_t)i); found = true; break; }
    }
    if (found) free_slot(taken);
  }
  if (sdev != dev) (void)hipSetDevice(dev);
  if (e != hipSuccess) { vvcgpu_set_error("stream_release: hipStreamSynchronize failed on device %d: %s (resources kept)", sdev, hipGetErrorString(e)); return VVCGPU_E_DEVICE; }
  return VVCGPU_OK;
}
int vvcgpu_shutdown(void)
{
  int dev0 = 0;
  VVC_HIP(hipGetDevice(&dev0));
  std::lock_guard<std::mutex> lock(g_slotMutex);
  std::lock_guard<std::mutex> imageLock(g_imageMutex);
  std::vector<StreamSlot> kept;                                             // what a device that cannot be reached holds is kept, and reported
  int unreachable = 0;
  for (int d = 0; d < VVC_MAX_DEVICES; d++)
  {
    bool holds = false;
    for (auto& s : g_slots) holds |= s.device == d;
    for (auto& img : g_images[d]) holds |= img.built;
    if (!holds) continue;
    const bool reached = hipSetDevice(d) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    unreachable += !reached;
    for (auto& s : g_slots)
      if (s.device == d) { if (reached) free_slot(s); else kept.push_back(s); }
    if (reached) for (auto& img : g_images[d]) { if (img.ptr) (void)hipFree(img.ptr); img = DeviceImage{ nullptr, false }; }
  }
  g_slots.swap(kept);
  VVC_HIP(hipSetDevice(dev0));
  if (unreachable) { vvcgpu_set_error("shutdown: %d unreachable device(s): their stream slots and table images were kept", unreachable); return VVCGPU_E_DEVICE; }
  return VVCGPU_OK;
}
}
