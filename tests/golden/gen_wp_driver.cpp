// gen_wp_driver.cpp -- test infrastructure (tests/golden/gen_wp.py builds and loads it on the build machine only): the reference's own
// WeightPrediction::addWeightUni / addWeightBi (WeightPrediction.cpp:157-300) on one block of 14-bit intermediates.  Compiled against the reference's
// headers, linked with oracle/_ref/libvtmref.so; nothing of the reference is copied.
#include "CommonDef.h"
#include "Buffer.h"
#include "Slice.h"
#include "WeightPrediction.h"

extern "C" int wpref_apply(const Pel* p0, const Pel* p1, Pel* dst, int w, int h, int bi, int w0, int w1, int offset, int shift, int bd, int clpMin,
                           int clpMax)
{
  ClpRngs clp;
  for (int c = 0; c < MAX_NUM_COMPONENT; c++) { clp.comp[c].min = clpMin; clp.comp[c].max = clpMax; clp.comp[c].bd = bd; clp.comp[c].n = 0; }
  clp.used = true; clp.chroma = false;
  // WPScalingParam after getWpScaling: w / offset / shift as given (the bi form keeps both lists' copies of offset and shift equal)
  WPScalingParam wp0[MAX_NUM_COMPONENT], wp1[MAX_NUM_COMPONENT];
  for (int c = 0; c < MAX_NUM_COMPONENT; c++)
  {
    wp0[c] = WPScalingParam(); wp1[c] = WPScalingParam();
    wp0[c].w = w0; wp1[c].w = w1;
    wp0[c].offset = wp1[c].offset = offset;
    wp0[c].shift = wp1[c].shift = shift;
  }
  const CPelUnitBuf s0(CHROMA_400, CPelBuf(p0, w, w, h)), s1(CHROMA_400, CPelBuf(p1, w, w, h));
  PelUnitBuf d(CHROMA_400, PelBuf(dst, w, w, h));
  WeightPrediction wpr;
  if (bi) wpr.addWeightBi(s0, s1, clp, wp0, wp1, d, true, COMPONENT_Y);
  else wpr.addWeightUni(s0, clp, wp0, d, COMPONENT_Y);
  return 0;
}
