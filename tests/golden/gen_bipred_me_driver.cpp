// gen_bipred_me_driver.cpp -- test infrastructure (tests/golden/gen_bipred_me.py builds and loads it on the build machine only): the reference's own
// InterSearch::xMotionEstimation with bBi = true (InterSearch.cpp:1668-1816: its own removeHighFreq, xSetSearchRange, xPatternSearch,
// xPatternSearchFracDIF and cost), InterSearch::xCheckBestMVP (:1537-1603) and InterPrediction::motionCompensation (luma) -- all private, hence
// -fno-access-control -- on a real Picture / Slice / PredictionUnit scaffold with several reference pictures per list.  Compiled against the
// reference's headers, linked with oracle/_ref/libvtmref.so; nothing of the reference is copied.
#include "CommonDef.h"
#include "Buffer.h"
#include "Slice.h"
#include "Picture.h"
#include "CodingStructure.h"
#include "RdCost.h"
#include "InterSearch.h"
#include "EncCfg.h"
#include <vector>

namespace {

struct BpCtx
{
  SPS* sps; PPS* pps; CodingStructure* cs; PreCalcValues* pcv; Slice* slice; InterSearch* is; RdCost* rc; EncCfg* cfg;
  std::vector<Picture*> pics;
  int picW, picH, bd;
};
BpCtx* g = nullptr;

struct BpUnit
{
  CodingUnit cu; PredictionUnit pu;
  BpUnit(int posX, int posY, int w, int h)
  {
    const UnitArea ua(CHROMA_420, Area(posX, posY, w, h));
    cu.UnitArea::operator=(ua);
    pu.UnitArea::operator=(ua);
    cu.cs = g->cs; cu.slice = g->slice; cu.chromaFormat = CHROMA_420;
    cu.affine = false; cu.imv = 0; cu.transQuantBypass = false; cu.partSize = SIZE_2Nx2N;
    pu.cs = g->cs; pu.cu = &cu; pu.chromaFormat = CHROMA_420;
  }
};

}  // namespace

// nPlanes reference pictures (luma planes picW x picH, unpadded, one after the other; the borders are extended as the encoder does) and the
// encoder settings the two functions read.  fastMode3: FASTINTERSEARCH_MODE3, i.e. subShiftMode 2 in the integer search and nothing else.
extern "C" int bpref_open(const Pel* recY, int nPlanes, int picW, int picH, int bd, double lambda, int searchRange, int clipKey, int useHad, int fastMode3,
                          const unsigned* mvpIdxCost)
{
  if (!g)
  {
    g = new BpCtx();
    g->sps = new SPS; g->pps = new PPS;
    g->cs = static_cast<CodingStructure*>(calloc(1, sizeof(CodingStructure)));
    g->cs->sps = g->sps; g->cs->pps = g->pps;
    g->slice = new Slice;
    g->cs->slice = g->slice;
    g->rc = new RdCost; g->cfg = new EncCfg; g->is = new InterSearch;
    g->rc->setUseQtbt(true);
    g->is->InterPrediction::init(g->rc, CHROMA_420);
    g->is->m_pcEncCfg = g->cfg;
    g->is->m_pcRdCost = g->rc;
    g->is->m_maxCompIDToPred = COMPONENT_Y;
    const UnitArea lcu(CHROMA_420, Area(0, 0, MAX_CU_SIZE, MAX_CU_SIZE));
    for (int i = 0; i < NUM_REF_PIC_LIST_01; i++) g->is->m_tmpPredStorage[i].create(lcu);
    g->is->m_tmpStorageLCU.create(lcu);
    g->pcv = nullptr;
  }
  g->picW = picW; g->picH = picH; g->bd = bd;
  g->cfg->setClipForBiPredMeEnabled(clipKey != 0);
  g->cfg->setUseHADME(useHad != 0);
  g->cfg->setFastInterSearchMode(fastMode3 ? FASTINTERSEARCH_MODE3 : FASTINTERSEARCH_DISABLED);
  g->is->m_bipredSearchRange = searchRange;
  g->is->m_motionEstimationSearchMethod = MESEARCH_DIAMOND;
  for (int l = 0; l < MAX_NUM_REF_LIST_ADAPT_SR; l++)
    for (int r = 0; r < MAX_IDX_ADAPT_SR; r++) g->is->m_aaiAdaptSR[l][r] = 64;
  for (int i = 0; i <= AMVP_MAX_NUM_CANDS; i++) g->is->m_auiMVPIdxCost[i][AMVP_MAX_NUM_CANDS] = mvpIdxCost[i];
  g->sps->setBitDepth(CHANNEL_TYPE_LUMA, bd); g->sps->setBitDepth(CHANNEL_TYPE_CHROMA, bd);
  g->sps->setPicWidthInLumaSamples(picW); g->sps->setPicHeightInLumaSamples(picH);
  g->sps->setMaxCUWidth(128); g->sps->setMaxCUHeight(128);
  delete g->pcv;
  g->pcv = new PreCalcValues(*g->sps, *g->pps, true);
  g->cs->pcv = g->pcv;
  g->slice->setSliceType(B_SLICE);
  g->slice->setPPS(g->pps);
  g->slice->m_bTestWeightPred = false; g->slice->m_bTestWeightBiPred = false;
  ClpRngs& clp = g->slice->getClpRngs();
  for (int c = 0; c < MAX_NUM_COMPONENT; c++) { clp.comp[c].min = 0; clp.comp[c].max = (1 << bd) - 1; clp.comp[c].bd = bd; clp.comp[c].n = 0; }
  g->rc->m_motionLambda = lambda;
  for (Picture* pic : g->pics) { free(pic->cs); pic->cs = nullptr; pic->destroy(); delete pic; }
  g->pics.clear();
  for (int k = 0; k < nPlanes; k++)
  {
    Picture* pic = new Picture;
    pic->create(CHROMA_420, Size(picW, picH), 128, 128 + 16, false);
    pic->cs = (CodingStructure*)calloc(1, sizeof(CodingStructure));
    const_cast<ChromaFormat&>(pic->cs->area.chromaFormat) = CHROMA_420;
    for (int c = 0; c < 3; c++)
    {
      PelBuf b = pic->getRecoBuf().get(ComponentID(c));
      for (int j = 0; j < (int)b.height; j++)
        for (int i = 0; i < (int)b.width; i++) b.buf[(ptrdiff_t)j * b.stride + i] = c ? (Pel)(1 << (bd - 1)) : recY[((size_t)k * picH + j) * picW + i];
    }
    pic->m_bIsBorderExtended = false;
    pic->extendPicBorder();
    g->pics.push_back(pic);
  }
  return 0;
}

// the slice's reference picture lists: plane index per (list, reference index)
extern "C" int bpref_set_lists(int n0, const int* planes0, int n1, const int* planes1)
{
  for (int r = 0; r < n0; r++) g->slice->m_apcRefPicList[REF_PIC_LIST_0][r] = g->pics[planes0[r]];
  for (int r = 0; r < n1; r++) g->slice->m_apcRefPicList[REF_PIC_LIST_1][r] = g->pics[planes1[r]];
  g->slice->m_aiNumRefIdx[REF_PIC_LIST_0] = n0; g->slice->m_aiNumRefIdx[REF_PIC_LIST_1] = n1;
  return 0;
}

// motionCompensation(pu, m_tmpPredStorage[list], list) as :1077-1084 / :1130-1138 make it; dst (optional): the luma prediction, w x h
extern "C" int bpref_mc(int posX, int posY, int w, int h, int list, int refIdx, int mvX, int mvY, Pel* dst)
{
  BpUnit u(posX, posY, w, h);
  u.pu.mv[list] = Mv(mvX, mvY); u.pu.refIdx[list] = (int8_t)refIdx;
  u.pu.refIdx[1 - list] = -1;
  PelUnitBuf predBufTmp = g->is->m_tmpPredStorage[list].getBuf(UnitAreaRelative(u.cu, u.pu));
  g->is->motionCompensation(u.pu, predBufTmp, RefPicList(list));
  if (dst)
    for (int j = 0; j < h; j++)
      for (int i = 0; i < w; i++) dst[(size_t)j * w + i] = predBufTmp.Y().at(i, j);
  return 0;
}

// xMotionEstimation(pu, origBuf, list, mvPred, refIdx, mv, mvpIdx, bits, cost, amvp, true) against the other list's prediction that the last
// bpref_mc(1 - list) of the same PU left in m_tmpPredStorage.  mvPred / mv: quarter units; mv, bits in and out.  Returns 1 when the reference throws.
extern "C" int bpref_me(const Pel* org, int orgStride, int posX, int posY, int w, int h, int list, int refIdx, const int* mvPred, int* mv, int mvpIdx,
                        unsigned* bits, uint64_t* cost)
{
  BpUnit u(posX, posY, w, h);
  std::vector<Pel> y((size_t)w * h), cb((w >> 1) * (h >> 1), 0), cr((w >> 1) * (h >> 1), 0);
  for (int j = 0; j < h; j++)
    for (int i = 0; i < w; i++) y[(size_t)j * w + i] = org[(size_t)j * orgStride + i];
  PelUnitBuf other = g->is->m_tmpPredStorage[1 - list].getBuf(UnitAreaRelative(u.cu, u.pu));
  other.bufs[1].fill(0); other.bufs[2].fill(0);
  PelUnitBuf origBuf;
  origBuf.chromaFormat = CHROMA_420;
  origBuf.bufs.push_back(PelBuf(y.data(), w, w, h));
  origBuf.bufs.push_back(PelBuf(cb.data(), w >> 1, w >> 1, h >> 1));
  origBuf.bufs.push_back(PelBuf(cr.data(), w >> 1, w >> 1, h >> 1));
  Mv cMvPred(mvPred[0], mvPred[1]), cMv(mv[0], mv[1]);
  AMVPInfo amvp;
  amvp.numCand = 0;
  uint32_t ruiBits = *bits;
  Distortion ruiCost = 0;
  int idx = mvpIdx;
  try
  {
    g->is->xMotionEstimation(u.pu, origBuf, RefPicList(list), cMvPred, refIdx, cMv, idx, ruiBits, ruiCost, amvp, true);
  }
  catch (...) { return 1; }
  mv[0] = cMv.getHor(); mv[1] = cMv.getVer();
  *bits = ruiBits; *cost = ruiCost;
  return 0;
}

// xCheckBestMVP(list, mv, mvPred, mvpIdx, amvp = {cands, numCand}, bits, cost, imv 0); mvPred, mvpIdx, bits, cost in and out.
// Returns 1 when the reference throws (its CHECK "Invalid MV prediction candidate").
extern "C" int bpref_check_best_mvp(int list, const int* mv, int* mvPred, int* mvpIdx, const int* cands, int numCand, unsigned* bits, uint64_t* cost)
{
  AMVPInfo amvp;
  amvp.numCand = numCand;
  for (int k = 0; k < 2; k++) amvp.mvCand[k] = Mv(cands[2 * k], cands[2 * k + 1]);
  Mv cMv(mv[0], mv[1]), cMvPred(mvPred[0], mvPred[1]);
  uint32_t ruiBits = *bits;
  Distortion ruiCost = *cost;
  int idx = *mvpIdx;
  try
  {
    g->is->xCheckBestMVP(RefPicList(list), cMv, cMvPred, idx, amvp, ruiBits, ruiCost, 0);
  }
  catch (...) { return 1; }
  mvPred[0] = cMvPred.getHor(); mvPred[1] = cMvPred.getVer();
  *mvpIdx = idx; *bits = ruiBits; *cost = ruiCost;
  return 0;
}
