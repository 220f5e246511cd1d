// alf_pel4_clamped.inc -- the clamped four-sample read of the ALF tile loads (alf_dev.h), stated once as text for load_tile_clamped and tile_fetch:
// as a forced-inline function it costs alf_stats_picture_kernel<64, *> three instructions (docs/MEASUREMENTS.md).
//   expects  src, stride, w, h   the plane;  x0, y0  the tile's origin;  r, c  the item's row and first column in the tile
//            bool vec_ok         the plane allows 8-byte loads (stride % 4 == 0, 8-byte aligned)
//            PEL4_DST            (macro) the pel4 lvalue that receives the samples at (x0 + c .. + 3, y0 + r), coordinates clamped to the plane
{
  int y = y0 + r;
  y = y < 0 ? 0 : (y >= h ? h - 1 : y);
  const int x = x0 + c;
  const Pel* row = src + (size_t)y * stride;
  if (vec_ok && x >= 0 && x + 3 < w) PEL4_DST = *reinterpret_cast<const pel4*>(row + x);
  else
  {
#pragma unroll
    for (int k = 0; k < 4; k++) { int xx = x + k; xx = xx < 0 ? 0 : (xx >= w ? w - 1 : xx); PEL4_DST[k] = row[xx]; }
  }
}
