// gen_affine_bipred_driver.cpp -- test infrastructure (tests/golden/gen_affine_bipred.py builds and loads it on the build machine only): the
// reference's own InterSearch::xAffineMotionEstimation with bBi = true (InterSearch.cpp:3286-3743: its own removeHighFreq against
// m_tmpPredStorage[1 - list]), InterSearch::xCheckBestAffineMVP (:3181-3284) and the luma InterPrediction::motionCompensation of an affine PU after
// PU::setAllAffineMv -- private members, hence -fno-access-control -- on a real Picture / Slice / PredictionUnit scaffold with a motion buffer and
// several reference pictures per list.  Compiled against the reference's headers, linked with oracle/_ref/libvtmref.so; nothing of the reference is
// copied.
#include "CommonDef.h"
#include "Buffer.h"
#include "Slice.h"
#include "Picture.h"
#include "CodingStructure.h"
#include "UnitTools.h"
#include "RdCost.h"
#include "InterSearch.h"
#include "EncCfg.h"
#include <vector>

namespace {

struct AbCtx
{
  SPS* sps; PPS* pps; CodingStructure* cs; PreCalcValues* pcv; Slice* slice; InterSearch* is; RdCost* rc; EncCfg* cfg;
  std::vector<Picture*> pics;
  int picW, picH, bd;
};
AbCtx* g = nullptr;

struct AbUnit
{
  CodingUnit cu; PredictionUnit pu;
  AbUnit(int posX, int posY, int w, int h, int six)
  {
    const UnitArea ua(CHROMA_420, Area(posX, posY, w, h));
    cu.UnitArea::operator=(ua);
    pu.UnitArea::operator=(ua);
    cu.cs = g->cs; cu.slice = g->slice; cu.chromaFormat = CHROMA_420;
    cu.affine = true; cu.affineType = six ? AFFINEMODEL_6PARAM : AFFINEMODEL_4PARAM;
    cu.imv = 0; cu.transQuantBypass = false; cu.partSize = SIZE_2Nx2N;
    pu.cs = g->cs; pu.cu = &cu; pu.chromaFormat = CHROMA_420;
    pu.refIdx[0] = pu.refIdx[1] = -1;
  }
};

void mv3(Mv (&m)[3], const int* v) { for (int k = 0; k < 3; k++) m[k] = Mv(v[2 * k], v[2 * k + 1], true); }

}  // namespace

// nPlanes reference pictures (luma planes picW x picH, unpadded, one after the other; the borders are extended as the encoder does) and the
// settings the three functions read
extern "C" int abref_open(const Pel* recY, int nPlanes, int picW, int picH, int bd, double lambda, int clipKey, int affineType, const unsigned* mvpIdxCost)
{
  if (!g)
  {
    g = new AbCtx();
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
    g->is->m_tmpAffiStorage.create(lcu);
    g->is->m_tmpAffiError = new Pel[MAX_CU_SIZE * MAX_CU_SIZE];
    g->is->m_tmpAffiDeri[0] = new int[MAX_CU_SIZE * MAX_CU_SIZE];
    g->is->m_tmpAffiDeri[1] = new int[MAX_CU_SIZE * MAX_CU_SIZE];
    g->pcv = nullptr;
  }
  g->picW = picW; g->picH = picH; g->bd = bd;
  g->cfg->setClipForBiPredMeEnabled(clipKey != 0);
  for (int i = 0; i <= AMVP_MAX_NUM_CANDS; i++) g->is->m_auiMVPIdxCost[i][AMVP_MAX_NUM_CANDS] = mvpIdxCost[i];
  g->sps->setBitDepth(CHANNEL_TYPE_LUMA, bd); g->sps->setBitDepth(CHANNEL_TYPE_CHROMA, bd);
  g->sps->setPicWidthInLumaSamples(picW); g->sps->setPicHeightInLumaSamples(picH);
  g->sps->setMaxCUWidth(128); g->sps->setMaxCUHeight(128);
  g->sps->getSpsNext().setUseAffineType(affineType != 0);
  delete g->pcv;
  g->pcv = new PreCalcValues(*g->sps, *g->pps, true);
  g->cs->pcv = g->pcv;
  // the motion buffer PU::setAllAffineMv writes and xPredInterUni reads
  const_cast<UnitArea&>(g->cs->area) = UnitArea(CHROMA_420, Area(0, 0, picW, picH));
  delete[] g->cs->m_motionBuf;
  g->cs->m_motionBuf = new MotionInfo[(size_t)(picW >> 2) * (picH >> 2)];
  g->slice->setSliceType(B_SLICE);
  g->slice->setPPS(g->pps);
  g->slice->m_bTestWeightPred = false; g->slice->m_bTestWeightBiPred = false;
  ClpRngs& clp = g->slice->getClpRngs();
  for (int c = 0; c < MAX_NUM_COMPONENT; c++) { clp.comp[c].min = 0; clp.comp[c].max = (1 << bd) - 1; clp.comp[c].bd = bd; clp.comp[c].n = 0; }
  g->rc->m_motionLambda = lambda;
  g->rc->m_dLambdaMotionSAD[0] = g->rc->m_dLambdaMotionSAD[1] = lambda;      // xCheckBestAffineMVP selects it again
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
extern "C" int abref_set_lists(int n0, const int* planes0, int n1, const int* planes1)
{
  for (int r = 0; r < n0; r++) g->slice->m_apcRefPicList[REF_PIC_LIST_0][r] = g->pics[planes0[r]];
  for (int r = 0; r < n1; r++) g->slice->m_apcRefPicList[REF_PIC_LIST_1][r] = g->pics[planes1[r]];
  g->slice->m_aiNumRefIdx[REF_PIC_LIST_0] = n0; g->slice->m_aiNumRefIdx[REF_PIC_LIST_1] = n1;
  return 0;
}

// PU::setAllAffineMv + motionCompensation(pu, m_tmpPredStorage[list], list); mv6 = LT, RT, LB as (hor, ver) in 1/16 sample; dst (optional): the luma
// prediction, w x h
extern "C" int abref_mc(int posX, int posY, int w, int h, int six, int list, int refIdx, const int* mv6, Pel* dst)
{
  AbUnit u(posX, posY, w, h, six);
  Mv mv[3];
  mv3(mv, mv6);
  PU::setAllAffineMv(u.pu, mv[0], mv[1], mv[2], RefPicList(list));
  u.pu.refIdx[list] = (int8_t)refIdx;
  PelUnitBuf predBufTmp = g->is->m_tmpPredStorage[list].getBuf(UnitAreaRelative(u.cu, u.pu));
  g->is->motionCompensation(u.pu, predBufTmp, RefPicList(list));
  if (dst)
    for (int j = 0; j < h; j++)
      for (int i = 0; i < w; i++) dst[(size_t)j * w + i] = predBufTmp.Y().at(i, j);
  return 0;
}

// xAffineMotionEstimation(pu, origBuf, list, mvPred, refIdx, mv, bits, cost, true) against the other list's prediction that the last
// abref_mc(1 - list) of the same PU left in m_tmpPredStorage.  mvPred6 / mv6: 1/16 units; mv6, bits in and out.
extern "C" int abref_me(const Pel* org, int orgStride, int posX, int posY, int w, int h, int six, int list, int refIdx, const int* mvPred6, int* mv6,
                        unsigned* bits, uint64_t* cost)
{
  AbUnit u(posX, posY, w, h, six);
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
  Mv acMv[3], acMvPred[3];
  mv3(acMv, mv6); mv3(acMvPred, mvPred6);
  uint32_t ruiBits = *bits;
  Distortion ruiCost = 0;
  g->is->xAffineMotionEstimation(u.pu, origBuf, RefPicList(list), acMvPred, refIdx, acMv, ruiBits, ruiCost, true);
  for (int k = 0; k < 3; k++) { mv6[2 * k] = acMv[k].getHor(); mv6[2 * k + 1] = acMv[k].getVer(); }
  *bits = ruiBits; *cost = ruiCost;
  return 0;
}

// xCheckBestAffineMVP(pu, info = {cands, numCand}, list, mv, mvPred, mvpIdx, bits, cost); cands: [2][3][2] = candidate, (LT, RT, LB), (hor, ver);
// mvPred6, mvpIdx, bits, cost in and out
extern "C" int abref_check_best_mvp(int six, int list, const int* mv6, int* mvPred6, int* mvpIdx, const int* cands, int numCand, unsigned* bits, uint64_t* cost)
{
  AbUnit u(0, 0, 16, 16, six);
  AffineAMVPInfo info;
  info.numCand = numCand;
  for (int k = 0; k < 2; k++)
  {
    info.mvCandLT[k] = Mv(cands[6 * k + 0], cands[6 * k + 1], true);
    info.mvCandRT[k] = Mv(cands[6 * k + 2], cands[6 * k + 3], true);
    info.mvCandLB[k] = Mv(cands[6 * k + 4], cands[6 * k + 5], true);
  }
  Mv acMv[3], acMvPred[3];
  mv3(acMv, mv6); mv3(acMvPred, mvPred6);
  uint32_t ruiBits = *bits;
  Distortion ruiCost = *cost;
  int idx = *mvpIdx;
  g->is->xCheckBestAffineMVP(u.pu, info, RefPicList(list), acMv, acMvPred, idx, ruiBits, ruiCost);
  for (int k = 0; k < 3; k++) { mvPred6[2 * k] = acMvPred[k].getHor(); mvPred6[2 * k + 1] = acMvPred[k].getVer(); }
  *mvpIdx = idx; *bits = ruiBits; *cost = ruiCost;
  return 0;
}
