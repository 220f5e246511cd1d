// mh_touch.h -- the run of super-blocks a persistent workgroup of me_hier_kernel walks, and the bytes of the packed original rows (mh_pack_org_kernel:
// [block][sampled row][64 bytes]) that one super-block reads.  No HIP dependency: the kernel and the host test (tests/test_mehier_touch_range.py,
// plain g++ with the sanitizers) include the same text.
#ifndef VVCGPU_MH_TOUCH_H
#define VVCGPU_MH_TOUCH_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MH_HD __host__ __device__ __forceinline__
#else
#define MH_HD inline
#endif

// Workgroup `block` of `wgs` (a multiple of 8: XCD x = block & 7 owns the contiguous chunk [x * chunk, (x + 1) * chunk) of the super-blocks) walks the
// items chunk0 + kk, kk0 <= kk < kkEnd, as far as they exist.
struct MhRun { int chunk0, kk0, kkEnd; };

MH_HD MhRun mh_run_of(int total, int wgs, int block)
{
  const int chunk = (total + 7) >> 3, perX = wgs >> 3, runLen = (chunk + perX - 1) / perX, kk0 = (block >> 3) * runLen;
  MhRun r;
  r.chunk0 = (block & 7) * chunk; r.kk0 = kk0; r.kkEnd = kk0 + runLen < chunk ? kk0 + runLen : chunk;
  return r;
}
// item kk of the run: is it walked at all (inside the run, and a super-block of the grid)?
MH_HD bool mh_run_has(const MhRun& r, int kk, int total) { return kk >= r.kk0 && kk < r.kkEnd && r.chunk0 + kk < total; }

// The packed rows of super-block (sbx, sby) = item sby * nsbx + sbx: `runs` contiguous runs (one per row of existing 16x16 blocks) of `runBytes` bytes
// (existing blocks of the row x hs sampled rows x 64), the first at byte `first`, `pitch` bytes apart.  A block record is a multiple of 512 bytes, so every
// run starts and ends on a 128-byte line.  runs = 0 for an item that is no super-block of the grid.
struct MhTouch { unsigned long long first; unsigned pitch, runBytes; int runs; };

MH_HD MhTouch mh_touch_range(int n16x, int n16y, int hs, int sbx, int sby, int item, int total)
{
  MhTouch t;
  t.first = 0; t.pitch = 0; t.runBytes = 0; t.runs = 0;
  if (item < 0 || item >= total || 4 * sbx >= n16x || 4 * sby >= n16y) return t;
  const int nsubx = n16x - 4 * sbx < 4 ? n16x - 4 * sbx : 4, nsuby = n16y - 4 * sby < 4 ? n16y - 4 * sby : 4;
  const unsigned rec = (unsigned)hs * 64u;
  t.first = ((unsigned long long)(4 * sby) * (unsigned)n16x + (unsigned)(4 * sbx)) * rec;
  t.pitch = (unsigned)n16x * rec;
  t.runBytes = (unsigned)nsubx * rec;
  t.runs = nsuby;
  return t;
}
// byte offset of the 128-byte line in slot i of the range, or ~0 for a slot without one.  128 slots = 4 runs x 32: run i >> 5, line i & 31 of it (a run is at
// most 4 blocks x 16 rows x 64 bytes = 32 lines) -- no division; a wave covers the slots with two loads per lane.
MH_HD unsigned long long mh_touch_line(const MhTouch& t, int i)
{
  const int run = i >> 5, l = i & 31;
  if (i < 0 || run >= t.runs || (unsigned)l >= (t.runBytes >> 7)) return ~0ull;
  return t.first + (unsigned long long)run * t.pitch + ((unsigned long long)l << 7);
}

#endif
