// gen_analysis_driver.cpp -- test infrastructure (tests/golden/gen_analysis.py builds and loads it on the build machine only): the reference's own
// picture analysis functions behind extern "C" entries.  Compiled against the reference where it lies (-fno-access-control for the member functions;
// the file-static functions come with their translation units, included from the reference's path at compile time) and linked with
// oracle/_ref/libvtmref.so; nothing of the reference is copied.
#include "EncSlice.cpp"
#include "WeightPredAnalysis.cpp"
#include "EncGOP.h"
#include "EncCu.h"

extern "C" {

// EncGOP::xFindDistortionPlane(pic0 = rec, pic1 = org, rshift, chromaShift): rshift 0 = plain SSE, rshift = bit depth = WPSNR (EncGOP.cpp:2720-2828)
uint64_t anaref_dist_plane(const Pel* rec, int recStride, const Pel* org, int orgStride, int w, int h, int rshift, int chromaShift)
{
  static EncGOP* g = static_cast<EncGOP*>(calloc(1, sizeof(EncGOP)));        // the function reads no member
  return g->xFindDistortionPlane(CPelBuf(rec, recStride, w, h), CPelBuf(org, orgStride, w, h), (uint32_t)rshift, (uint32_t)chromaShift);
}

// filterAndCalculateAverageEnergies (EncSlice.cpp:156-184) on a w x h area
double anaref_energy(const Pel* src, int stride, int h, int w, int bitDepth)
{
  double e = 0.0;
  filterAndCalculateAverageEnergies(src, stride, e, h, w, (uint32_t)bitDepth);
  return e;
}

int64_t anaref_wp_sad(int bitDepth, const Pel* org, const Pel* ref, int w, int h, int orgStride, int refStride, int log2Denom, int weight, int offset,
                      int highPrecision, int optionalClipForm, int clipped)
{
  if (optionalClipForm)
    return xCalcSADvalueWPOptionalClip(bitDepth, org, ref, w, h, orgStride, refStride, log2Denom, weight, offset, highPrecision != 0, clipped != 0);
  return xCalcSADvalueWP(bitDepth, org, ref, w, h, orgStride, refStride, log2Denom, weight, offset, highPrecision != 0);
}

void anaref_histogram(const Pel* p, int w, int h, int stride, int maxPel, int* out)
{
  std::vector<int> hist;
  xCalcHistogram(p, hist, w, h, stride, maxPel);
  for (int i = 0; i < maxPel; i++) out[i] = hist[i];
}

// WeightPredAnalysis::xCalcACDCParamSlice (WeightPredAnalysis.cpp:245-301) through a Slice whose Picture carries an original buffer; out: iDC, iAC x 3
int anaref_acdc(const Pel* y, const Pel* cb, const Pel* cr, int w, int h, int highPrecision, int64_t* out)
{
  Picture pic;
  pic.create(CHROMA_420, Size(w, h), 128, 16, false);
  const Pel* in[3] = { y, cb, cr };
  for (int c = 0; c < 3; c++)
  {
    PelBuf b = pic.getOrigBuf().get(ComponentID(c));
    for (int j = 0; j < (int)b.height; j++) memcpy(b.buf + (ptrdiff_t)j * b.stride, in[c] + (size_t)j * b.width, b.width * sizeof(Pel));
  }
  SPS sps;
  sps.getSpsRangeExtension().setHighPrecisionOffsetsEnabledFlag(highPrecision != 0);
  Slice slice;
  slice.setSPS(&sps);
  slice.setPic(&pic);
  WeightPredAnalysis wpa;
  wpa.xCalcACDCParamSlice(&slice);
  const WPACDCParam* p = nullptr;
  slice.getWpAcDcParam(p);
  for (int c = 0; c < 3; c++) { out[2 * c] = p[c].iDC; out[2 * c + 1] = p[c].iAC; }
  pic.destroy();
  return 0;
}

// EncCu::updateCtuDataISlice (EncCu.cpp:468-485) on the clipped CTU
int anaref_ctu_sum_had(const Pel* buf, int stride, int w, int h)
{
  static EncCu* cu = static_cast<EncCu*>(calloc(1, sizeof(EncCu)));          // the function reads no member
  return cu->updateCtuDataISlice(CPelBuf(buf, stride, w, h));
}

}  // extern "C"
