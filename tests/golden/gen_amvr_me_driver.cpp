// gen_amvr_me_driver.cpp -- test infrastructure (tests/golden/gen_amvr_me.py builds and loads it on the build machine only): the scaffold of
// gen_unipred_me_driver.cpp and gen_bipred_me_driver.cpp with cu.imv set (AMVR: 1 integer-sample, 2 four-sample vectors) -- the reference's own
// InterSearch::xEstimateMvPredAMVP with bFilled = true (InterSearch.cpp:1443-1483), InterSearch::xMotionEstimation with both bBi values (:1668-1816:
// its own xTZSearch / xPatternSearch with imvShift and xPatternSearchIntRefine :2408-2500) handed the real AMVPInfo, InterSearch::xCheckBestMVP with imv
// (:1537-1603), InterPrediction::motionCompensation (luma) and the two RdCost functions the list-1 shortcut uses -- all private, hence
// -fno-access-control -- on a real Picture / Slice / PredictionUnit scaffold with several reference pictures per list.  No mode control is attached, so
// the block cache (the cached-start path) is not reached.  Compiled against the reference's headers, linked with oracle/_ref/libvtmref.so; nothing of
// the reference is copied.
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

struct AmCtx
{
  SPS* sps; PPS* pps; CodingStructure* cs; PreCalcValues* pcv; Slice* slice; InterSearch* is; RdCost* rc; EncCfg* cfg;
  std::vector<Picture*> pics;
  int picW, picH, bd, imv;
};
AmCtx* g = nullptr;

struct AmUnit
{
  CodingUnit cu; PredictionUnit pu;
  AmUnit(int posX, int posY, int w, int h)
  {
    const UnitArea ua(CHROMA_420, Area(posX, posY, w, h));
    cu.UnitArea::operator=(ua);
    pu.UnitArea::operator=(ua);
    cu.cs = g->cs; cu.slice = g->slice; cu.chromaFormat = CHROMA_420;
    cu.affine = false; cu.imv = (uint8_t)g->imv; cu.transQuantBypass = false; cu.partSize = SIZE_2Nx2N; cu.qtDepth = 0;
    pu.cs = g->cs; pu.cu = &cu; pu.chromaFormat = CHROMA_420;
  }
};

struct AmOrg
{
  std::vector<Pel> y, cb, cr;
  PelUnitBuf buf;
  AmOrg(const Pel* org, int orgStride, int w, int h) : y((size_t)w * h), cb((w >> 1) * (h >> 1) + 1, 0), cr((w >> 1) * (h >> 1) + 1, 0)
  {
    for (int j = 0; j < h; j++)
      for (int i = 0; i < w; i++) y[(size_t)j * w + i] = org[(size_t)j * orgStride + i];
    buf.chromaFormat = CHROMA_420;
    buf.bufs.push_back(PelBuf(y.data(), w, w, h));
    buf.bufs.push_back(PelBuf(cb.data(), w >> 1, w >> 1, h >> 1));
    buf.bufs.push_back(PelBuf(cr.data(), w >> 1, w >> 1, h >> 1));
  }
};

AMVPInfo amvp_of(const int* cands, int numCand)
{
  AMVPInfo a;
  a.numCand = numCand;
  for (int k = 0; k < 2; k++) a.mvCand[k] = Mv(cands[2 * k], cands[2 * k + 1]);
  return a;
}

}  // namespace

// nPlanes reference pictures (luma planes picW x picH, unpadded, one after the other; the borders are extended as the encoder does) and the encoder
// settings the functions read.  fastMode3: FASTINTERSEARCH_MODE3, i.e. subShiftMode 2 in the integer searches; enhanced: MESEARCH_DIAMOND_ENHANCED;
// imv: cu.imv of every unit made from here on.
extern "C" int amref_open(const Pel* recY, int nPlanes, int picW, int picH, int bd, double lambda, int useHad, int fastMode3, int enhanced, int firstSearchStop,
                          int bipredSearchRange, int clipKey, int imv, const unsigned* mvpIdxCost)
{
  if (!g)
  {
    g = new AmCtx();
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
    g->is->m_modeCtrl = nullptr;
    const UnitArea lcu(CHROMA_420, Area(0, 0, MAX_CU_SIZE, MAX_CU_SIZE));
    for (int i = 0; i < NUM_REF_PIC_LIST_01; i++) g->is->m_tmpPredStorage[i].create(lcu);
    g->is->m_tmpStorageLCU.create(lcu);
    g->pcv = nullptr;
  }
  g->picW = picW; g->picH = picH; g->bd = bd; g->imv = imv;
  g->cfg->setUseHADME(useHad != 0);
  g->cfg->setClipForBiPredMeEnabled(clipKey != 0);
  g->cfg->setFastInterSearchMode(fastMode3 ? FASTINTERSEARCH_MODE3 : FASTINTERSEARCH_DISABLED);
  g->cfg->setFastMEAssumingSmootherMVEnabled(firstSearchStop != 0);
  g->cfg->setRestrictMESampling(false);
  g->cfg->setMotionEstimationSearchMethod(enhanced ? MESEARCH_DIAMOND_ENHANCED : MESEARCH_DIAMOND);
  g->is->m_motionEstimationSearchMethod = enhanced ? MESEARCH_DIAMOND_ENHANCED : MESEARCH_DIAMOND;
  g->is->m_bipredSearchRange = bipredSearchRange;
  for (int i = 0; i <= AMVP_MAX_NUM_CANDS; i++) g->is->m_auiMVPIdxCost[i][AMVP_MAX_NUM_CANDS] = mvpIdxCost[i];
  g->sps->setBitDepth(CHANNEL_TYPE_LUMA, bd); g->sps->setBitDepth(CHANNEL_TYPE_CHROMA, bd);
  g->sps->setPicWidthInLumaSamples(picW); g->sps->setPicHeightInLumaSamples(picH);
  g->sps->setMaxCUWidth(128); g->sps->setMaxCUHeight(128);
  delete g->pcv;
  g->pcv = new PreCalcValues(*g->sps, *g->pps, true);
  const_cast<bool&>(g->pcv->only2Nx2N) = false;               // the 2Nx2N predictor is a per-call statement here: qtDepth != 0 hands it over
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

// the slice's reference picture lists: plane index and adaptive search range per (list, reference index)
extern "C" int amref_set_lists(int n0, const int* planes0, const int* range0, int n1, const int* planes1, const int* range1)
{
  for (int r = 0; r < n0; r++) { g->slice->m_apcRefPicList[REF_PIC_LIST_0][r] = g->pics[planes0[r]]; g->is->m_aaiAdaptSR[0][r] = range0[r]; }
  for (int r = 0; r < n1; r++) { g->slice->m_apcRefPicList[REF_PIC_LIST_1][r] = g->pics[planes1[r]]; g->is->m_aaiAdaptSR[1][r] = range1[r]; }
  g->slice->m_aiNumRefIdx[REF_PIC_LIST_0] = n0; g->slice->m_aiNumRefIdx[REF_PIC_LIST_1] = n1;
  return 0;
}

// xEstimateMvPredAMVP(pu, origBuf, list, refIdx, mvPred, amvp = {cands, numCand}, bFilled = true, &distBiP) -> mvPred, mvpIdx, distBiP; tmpl[i] =
// xGetTemplateCost of candidate i on its own.  Returns 1 when the reference throws.
extern "C" int amref_amvp(const Pel* org, int orgStride, int posX, int posY, int w, int h, int list, int refIdx, const int* cands, int numCand, int* mvPred,
                          int* mvpIdx, uint64_t* distBiP, uint64_t* tmpl)
{
  AmUnit u(posX, posY, w, h);
  AmOrg o(org, orgStride, w, h);
  AMVPInfo amvp = amvp_of(cands, numCand);
  Mv cMvPred;
  Distortion d = 0;
  try
  {
    g->is->xEstimateMvPredAMVP(u.pu, o.buf, RefPicList(list), refIdx, cMvPred, amvp, true, &d);
    PelUnitBuf predBuf = g->is->m_tmpStorageLCU.getBuf(UnitAreaRelative(u.cu, u.pu));
    for (int k = 0; k < numCand; k++) tmpl[k] = g->is->xGetTemplateCost(u.pu, o.buf, predBuf, amvp.mvCand[k], k, AMVP_MAX_NUM_CANDS, RefPicList(list), refIdx);
  }
  catch (...) { return 1; }
  mvPred[0] = cMvPred.getHor(); mvPred[1] = cMvPred.getVer();
  *mvpIdx = u.pu.mvpIdx[list]; *distBiP = d;
  return 0;
}

// motionCompensation(pu, m_tmpPredStorage[list], list) as :1077-1084 / :1130-1138 make it
extern "C" int amref_mc(int posX, int posY, int w, int h, int list, int refIdx, int mvX, int mvY)
{
  AmUnit u(posX, posY, w, h);
  u.pu.mv[list] = Mv(mvX, mvY); u.pu.refIdx[list] = (int8_t)refIdx;
  u.pu.refIdx[1 - list] = -1;
  PelUnitBuf predBufTmp = g->is->m_tmpPredStorage[list].getBuf(UnitAreaRelative(u.cu, u.pu));
  g->is->motionCompensation(u.pu, predBufTmp, RefPicList(list));
  return 0;
}

// xMotionEstimation(pu, origBuf, list, mvPred, refIdx, mv, mvpIdx, bits, cost, amvp = {cands, numCand}, bBi).  bBi: against the other list's prediction
// that the last amref_mc(1 - list) of the same PU left in m_tmpPredStorage; mv is then the entry vector too.  pred2 (integer units, may be null;
// bBi = false): m_integerMv2Nx2N of this (list, reference), handed to the search the way the reference does for a CU below the first quad-tree level.
// mvPred, mv (quarter units), mvpIdx, bits: in and out; cost: out; intMv (bBi = false): what the search leaves in m_integerMv2Nx2N.  Returns 1 when the
// reference throws.
extern "C" int amref_me(const Pel* org, int orgStride, int posX, int posY, int w, int h, int list, int refIdx, int* mvPred, const int* pred2, int* mv, int* intMv,
                        int* mvpIdx, unsigned* bits, uint64_t* cost, const int* cands, int numCand, int bBi)
{
  AmUnit u(posX, posY, w, h);
  AmOrg o(org, orgStride, w, h);
  if (bBi)
  {
    PelUnitBuf other = g->is->m_tmpPredStorage[1 - list].getBuf(UnitAreaRelative(u.cu, u.pu));
    other.bufs[1].fill(0); other.bufs[2].fill(0);
  }
  else if (pred2) { u.cu.qtDepth = 1; g->is->m_integerMv2Nx2N[list][refIdx] = Mv(pred2[0], pred2[1]); }
  Mv cMvPred(mvPred[0], mvPred[1]), cMv(mv[0], mv[1]);
  AMVPInfo amvp = amvp_of(cands, numCand);
  uint32_t ruiBits = *bits;
  Distortion ruiCost = 0;
  int idx = *mvpIdx;
  try
  {
    g->is->xMotionEstimation(u.pu, o.buf, RefPicList(list), cMvPred, refIdx, cMv, idx, ruiBits, ruiCost, amvp, bBi != 0);
  }
  catch (...) { return 1; }
  mv[0] = cMv.getHor(); mv[1] = cMv.getVer();
  mvPred[0] = cMvPred.getHor(); mvPred[1] = cMvPred.getVer();
  if (!bBi) { intMv[0] = g->is->m_integerMv2Nx2N[list][refIdx].getHor(); intMv[1] = g->is->m_integerMv2Nx2N[list][refIdx].getVer(); }
  *mvpIdx = idx; *bits = ruiBits; *cost = ruiCost;
  return 0;
}

// xCheckBestMVP(list, mv, mvPred, mvpIdx, amvp = {cands, numCand}, bits, cost, cu.imv); mvPred, mvpIdx, bits, cost in and out.
// Returns 1 when the reference throws.
extern "C" int amref_check_best_mvp(int list, const int* mv, int* mvPred, int* mvpIdx, const int* cands, int numCand, unsigned* bits, uint64_t* cost)
{
  AMVPInfo amvp = amvp_of(cands, numCand);
  Mv cMv(mv[0], mv[1]), cMvPred(mvPred[0], mvPred[1]);
  uint32_t ruiBits = *bits;
  Distortion ruiCost = *cost;
  int idx = *mvpIdx;
  try
  {
    g->is->xCheckBestMVP(RefPicList(list), cMv, cMvPred, idx, amvp, ruiBits, ruiCost, (uint8_t)g->imv);
  }
  catch (...) { return 1; }
  mvPred[0] = cMvPred.getHor(); mvPred[1] = cMvPred.getVer();
  *mvpIdx = idx; *bits = ruiBits; *cost = ruiCost;
  return 0;
}

// RdCost::setPredictor(mvPred) + getBitsOfVectorWithPredictor(mv, imvShift = cu.imv << 1) at the cost scale the loop has at :915 (0: every
// xMotionEstimation leaves it there), and RdCost::getCost(bits)
extern "C" unsigned amref_vector_bits(const int* mvPred, const int* mv)
{
  g->rc->setPredictor(Mv(mvPred[0], mvPred[1]));
  g->rc->setCostScale(0);
  return g->rc->getBitsOfVectorWithPredictor(mv[0], mv[1], (unsigned)(g->imv << 1));
}
extern "C" uint64_t amref_get_cost(unsigned bits) { return g->rc->getCost(bits); }
