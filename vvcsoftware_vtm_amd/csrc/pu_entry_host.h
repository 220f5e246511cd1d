// pu_entry_host.h -- host side of the whole-PU search entries: the argument checks they share, word for word, and the LDS sizing and grid of the owner
// model (owner_dev.h).  Templates over the entry's cfg struct (the four structs name these fields alike).  Every check returns VVCGPU_OK or the
// error code with the text set; `name` is the entry's name as the text starts with it.  An entry calls pu_check_frame, its own checks, then
// pu_check_tail: the order in which a cfg with several faults reports them.
#pragma once
#include "common.h"

namespace {

template <class Cfg> int pu_check_geometry(const char* name, const Cfg& c)
{
  VVC_CHECK_ARG(c.pic_w > 0 && c.pic_h > 0 && c.max_cu_w > 0 && c.max_cu_h > 0 && c.ref_stride > 0, "%s: geometry (picture %d x %d, CTU %d x %d, ref_stride %d)", name,
                c.pic_w, c.pic_h, c.max_cu_w, c.max_cu_h, c.ref_stride);
  VVC_CHECK_ARG(c.pic_w <= 65536 && c.pic_h <= 65536 && c.max_cu_w <= 256 && c.max_cu_h <= 256, "%s: geometry (picture %d x %d, CTU %d x %d)", name, c.pic_w, c.pic_h,
                c.max_cu_w, c.max_cu_h);
  return VVCGPU_OK;
}

template <class Cfg> int pu_check_frame(const char* name, const Cfg& c, int maxPlanes)
{
  VVC_CHECK_ARG(c.n_planes >= 1 && c.n_planes <= maxPlanes, "%s: n_planes %d outside 1..%d", name, c.n_planes, maxPlanes);
  for (int i = 0; i < c.n_planes; i++) VVC_CHECK_ARG(c.ref_planes[i], "%s: null pointer (ref_planes[%d])", name, i);
  if (const int rc = pu_check_geometry(name, c)) return rc;
  VVC_CHECK_ARG(c.clp_min <= c.clp_max && c.clp_min >= -32768 && c.clp_max <= 32767, "%s: clip range %d..%d", name, c.clp_min, c.clp_max);
  VVC_CHECK_ARG(c.lambda >= 0.0 && c.lambda < 1048576.0, "%s: lambda out of range", name);
  return VVCGPU_OK;
}

// cfg.imv of the translational entries: cu.imv of the pass
template <class Cfg> int pu_check_imv(const char* name, const Cfg& c)
{
  VVC_CHECK_ARG(c.imv >= 0 && c.imv <= 2, "%s: imv %d outside 0..2", name, c.imv);
  return VVCGPU_OK;
}

// the reference lists of the uni-predictive entries; perRef(l, r): what else the entry checks of (list, reference index), in its place in the order
template <class Cfg, class PerRef> int pu_check_lists(const char* name, const Cfg& c, int maxRefs, PerRef perRef)
{
  VVC_CHECK_ARG(c.n_ref[0] >= 1 && c.n_ref[0] <= maxRefs && c.n_ref[1] >= 0 && c.n_ref[1] <= maxRefs, "%s: n_ref %d, %d (list 0: 1..%d, list 1: 0..%d)", name, c.n_ref[0],
                c.n_ref[1], maxRefs, maxRefs);
  for (int l = 0; l < 2; l++)
    for (int r = 0; r < c.n_ref[l]; r++)
    {
      VVC_CHECK_ARG(c.ref_plane[l][r] >= 0 && c.ref_plane[l][r] < c.n_planes, "%s: ref_plane[%d][%d] %d outside [0, %d)", name, l, r, c.ref_plane[l][r], c.n_planes);
      if (const int rc = perRef(l, r)) return rc;
    }
  for (int r = 0; r < c.n_ref[1]; r++)
    VVC_CHECK_ARG(c.list1_to_list0[r] >= -1 && c.list1_to_list0[r] < c.n_ref[0], "%s: list1_to_list0[%d] %d outside [-1, %d)", name, r, c.list1_to_list0[r], c.n_ref[0]);
  return VVCGPU_OK;
}

// max_pu (0: 128) against the served sides, the bit depth, n < nBound; then the plane slots from n_planes on are nulled (the kernels take c by value)
template <class Cfg> int pu_check_tail(const char* name, Cfg& c, int n, int nBound, bool (*sideOk)(int), const char* sidesText)
{
  if (c.max_pu_w == 0) c.max_pu_w = 128;
  if (c.max_pu_h == 0) c.max_pu_h = 128;
  VVC_CHECK_ARG(sideOk(c.max_pu_w) && sideOk(c.max_pu_h), "%s: max_pu %d x %d (sides %s, or 0)", name, c.max_pu_w, c.max_pu_h, sidesText);
  if (c.bit_depth > 10 || c.bit_depth < 8) { vvcgpu_set_error("%s: bit depth %d outside 8..10", name, c.bit_depth); return VVCGPU_E_UNSUPPORTED; }
  VVC_CHECK_ARG(n < nBound, "%s: n %d", name, n);
  for (int i = c.n_planes; i < (int)(sizeof(c.ref_planes) / sizeof(c.ref_planes[0])); i++) c.ref_planes[i] = nullptr;
  return VVCGPU_OK;
}

// LDS of the owners of a launch: each kind needs the most that bytesOf(w, h, lanes of the owner) gives among the served shapes within max_pu that the
// kind takes (up to waveMax samples: a wavefront, 64 lanes; above: the workgroup, 256); a workgroup holds four wavefront owners or one workgroup owner.
// groupBytes == 0: max_pu leaves the workgroup owners nothing to serve.
struct PuOwnerLds { int waveBytes, groupBytes; size_t lds; };
template <class BytesOf> PuOwnerLds pu_owner_lds(int minSide, int maxW, int maxH, int waveMax, BytesOf bytesOf)
{
  PuOwnerLds L = { 0, 0, 0 };
  for (int w = minSide; w <= maxW; w <<= 1)
    for (int h = minSide; h <= maxH; h <<= 1)
    {
      const bool wv = w * h <= waveMax;
      const int bytes = bytesOf(w, h, wv ? 64 : 256);
      int& dst = wv ? L.waveBytes : L.groupBytes;
      if (bytes > dst) dst = bytes;
    }
  L.waveBytes = (L.waveBytes + 15) & ~15;
  L.lds = (size_t)(4 * L.waveBytes > L.groupBytes ? 4 * L.waveBytes : L.groupBytes);
  return L;
}

// The grid over `units`: cdiv(units, 4) workgroups of wavefront owners, then the workgroup owners.  Where the workgroup owners write the sentinel of an
// item outside the contract (the single-launch entries: affine_me, bipred_me, affine_bipred_me) there is always one per unit.  Where a later launch
// writes it (the uni-predictive entries' decide kernels) they are launched only if max_pu leaves them a shape to serve: L.groupBytes != 0.
inline int pu_owner_grid(int units, bool groupOwners) { return cdiv(units, 4) + (groupOwners ? units : 0); }

}  // namespace
