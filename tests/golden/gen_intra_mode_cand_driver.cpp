// gen_intra_mode_cand_driver.cpp -- test infrastructure (tests/golden/gen_intra_mode_cand.py builds and loads it on the build machine only): the
// reference's own IntraPrediction::useFilteredIntraRefSamples, xFilterReferenceSamples, predIntraAng, RdCost::setDistParam(.., bUseHadamard) + distFunc,
// the cost expression of IntraSearch.cpp:436 and updateCandList from its header, on the luma PredictionUnit scaffold of vtmref_intra_pred
// (oracle/ref_wrap_kernels.h).  Compiled against the reference's headers (-fno-access-control), linked with oracle/_ref/libvtmref.so; nothing of the
// reference is copied.
#include "CommonDef.h"
#include "Buffer.h"
#include "Slice.h"
#include "CodingStructure.h"
#include "RdCost.h"
#include "IntraPrediction.h"
#include "UnitTools.h"

namespace {

struct ImCtx
{
  IntraPrediction* ip; SPS* sps; Slice* slice; CodingStructure* cs; PreCalcValues* pcv; RdCost* rc;
  int bd, w, h;
};
ImCtx* g = nullptr;

// the PU of the block that imref_load set up, with intraDir[0] = mode
struct ImPu
{
  CodingUnit cu; PredictionUnit pu;
  explicit ImPu(int mode)
  {
    cu.UnitArea::operator=(UnitArea(CHROMA_420, Area(0, 0, g->w, g->h))); cu.cs = g->cs; cu.chromaFormat = CHROMA_420;
    pu.UnitArea::operator=(cu); pu.cu = &cu; pu.cs = g->cs; pu.chromaFormat = CHROMA_420;
    pu.intraDir[0] = mode; pu.intraDir[1] = mode;
  }
};

}  // namespace

extern "C" int imref_open(int bd, int intraSmoothingDisabled)
{
  if (!g)
  {
    g = new ImCtx();
    g->ip = new IntraPrediction; g->ip->init(CHROMA_420, bd);
    g->sps = new SPS; g->slice = new Slice; g->rc = new RdCost;
    g->sps->getSpsNext().setUseQTBT(true);
    g->rc->setUseQtbt(true);
    g->cs = (CodingStructure*)calloc(1, sizeof(CodingStructure));
    g->pcv = (PreCalcValues*)calloc(1, sizeof(PreCalcValues));
    const_cast<bool&>(g->pcv->rectCUs) = true; const_cast<bool&>(g->pcv->noChroma2x2) = false;
    g->cs->sps = g->sps; g->cs->slice = g->slice; g->cs->pcv = g->pcv;
  }
  g->bd = bd;
  g->sps->setBitDepth(CHANNEL_TYPE_LUMA, bd);
  g->sps->getSpsRangeExtension().setIntraSmoothingDisabledFlag(intraSmoothingDisabled != 0);
  return 0;
}

// the packed references of a w x h block (refs[0] top-left, refs[1 .. T] above, refs[T + 1 .. T + L] left) into the reference's unfiltered buffer and,
// as initIntraPatternChType(cu, area, bFilterRefs) does, through xFilterReferenceSamples into its filtered buffer when
// useFilteredIntraRefSamples(COMPONENT_Y, pu, modeSpecific = false, pu) says so (IntraSearch.cpp:383).  Returns that decision.
extern "C" int imref_load(const Pel* refs, int w, int h, int clpMin, int clpMax)
{
  g->w = w; g->h = h;
  ClpRng& clp = g->slice->m_clpRngs.comp[COMPONENT_Y];
  clp.min = clpMin; clp.max = clpMax; clp.bd = g->bd; clp.n = 0;
  const CompArea area(COMPONENT_Y, CHROMA_420, Area(0, 0, w, h));
  g->ip->setReferenceArrayLengths(area);
  const int T = g->ip->m_topRefLength, L = g->ip->m_leftRefLength, stride = T + 1;
  Pel* unf = g->ip->m_piYuvExt[COMPONENT_Y][PRED_BUF_UNFILTERED];
  for (int x = 0; x <= T; x++) unf[x] = refs[x];
  for (int y = 1; y <= L; y++) unf[y * stride] = refs[T + y];
  ImPu s(0);
  const bool filter = IntraPrediction::useFilteredIntraRefSamples(COMPONENT_Y, s.pu, false, s.pu);
  if (filter) g->ip->xFilterReferenceSamples(unf, g->ip->m_piYuvExt[COMPONENT_Y][PRED_BUF_FILTERED], area, *g->sps);
  return filter ? 1 : 0;
}

// useFilteredIntraRefSamples(COMPONENT_Y, pu, modeSpecific = true, pu) of the loaded block (IntraSearch.cpp:426, 477)
extern "C" int imref_use_filtered(int mode)
{
  ImPu s(mode);
  return IntraPrediction::useFilteredIntraRefSamples(COMPONENT_Y, s.pu, true, s.pu) ? 1 : 0;
}

// predIntraAng(COMPONENT_Y, piPred, pu, useFiltered) of the loaded block into dst (pitch w)
extern "C" int imref_pred(int mode, int useFiltered, Pel* dst)
{
  ImPu s(mode);
  PelBuf pred(dst, g->w, g->w, g->h);
  try { g->ip->predIntraAng(COMPONENT_Y, pred, s.pu, useFiltered != 0); }
  catch (...) { return 1; }
  return 0;
}

// setDistParam(distParam, piOrg, piPred, bitDepth, COMPONENT_Y, bUseHadamard = true), applyWeight = false, distFunc (IntraSearch.cpp:397-399, 429)
extern "C" uint64_t imref_dist(const Pel* org, int orgStride, const Pel* cur, int curStride, int w, int h)
{
  DistParam dp;
  g->rc->setDistParam(dp, CPelBuf(org, orgStride, w, h), CPelBuf(cur, curStride, w, h), g->bd, COMPONENT_Y, true);
  dp.applyWeight = false;
  return dp.distFunc(dp);
}

// :436
extern "C" double imref_cost(uint64_t sad, uint64_t bits, double sqrtLambdaForFirstPass)
{
  Distortion uiSad = sad;
  uint64_t fracModeBits = bits;
  return (double)uiSad + (double)fracModeBits * sqrtLambdaForFirstPass;
}

// updateCandList(mode, cost, list, costList, fastNum) on lists handed over as arrays (*size entries, room for FAST_UDI_MAX_RDMODE_NUM)
extern "C" int imref_update_cand_list(unsigned mode, double cost, unsigned* modes, double* costs, int* size, int fastNum)
{
  static_vector<uint32_t, FAST_UDI_MAX_RDMODE_NUM> modeList;
  static_vector<double, FAST_UDI_MAX_RDMODE_NUM> costList;
  for (int i = 0; i < *size; i++) { modeList.push_back(modes[i]); costList.push_back(costs[i]); }
  int r;
  try { r = (int)updateCandList(mode, cost, modeList, costList, (size_t)fastNum); }
  catch (...) { return -1; }
  *size = (int)modeList.size();
  for (int i = 0; i < *size; i++) { modes[i] = modeList[i]; costs[i] = costList[i]; }
  return r;
}
