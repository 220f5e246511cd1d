// gen_affine_unipred_driver.cpp -- test infrastructure (tests/golden/gen_affine_unipred.py builds and loads it on the build machine only): the
// reference's own InterSearch::xGetAffineTemplateCost (InterSearch.cpp:1645-1665), InterSearch::xAffineMotionEstimation with bBi = false
// (:3286-3743), InterSearch::xCheckBestAffineMVP (:3181-3284) and Mv::roundMV2SignalPrecision -- private members, hence -fno-access-control -- on a
// real Picture / Slice / PredictionUnit scaffold with several reference pictures per list.  Every vector comes with the precision flag its Mv
// object carries where the reference makes the call, and the flags of the vectors a search returns are handed back.  Compiled against the
// reference's headers, linked with oracle/_ref/libvtmref.so; nothing of the reference is copied.
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

struct AuCtx
{
  SPS* sps; PPS* pps; CodingStructure* cs; PreCalcValues* pcv; Slice* slice; InterSearch* is; RdCost* rc; EncCfg* cfg;
  std::vector<Picture*> pics;
  int picW, picH, bd;
};
AuCtx* g = nullptr;

struct AuUnit
{
  CodingUnit cu; PredictionUnit pu;
  AuUnit(int posX, int posY, int w, int h, int six)
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

// hp: the precision flag the Mv objects carry where the reference calls the function (1: 1/16 sample, 0: quarter sample)
void mv3(Mv (&m)[3], const int* v, int hp) { for (int k = 0; k < 3; k++) m[k] = Mv(v[2 * k], v[2 * k + 1], hp != 0); }

struct AuOrg
{
  std::vector<Pel> y, cb, cr;
  PelUnitBuf buf;
  AuOrg(const Pel* org, int orgStride, int w, int h) : y((size_t)w * h), cb((w >> 1) * (h >> 1), 0), cr((w >> 1) * (h >> 1), 0)
  {
    for (int j = 0; j < h; j++)
      for (int i = 0; i < w; i++) y[(size_t)j * w + i] = org[(size_t)j * orgStride + i];
    buf.chromaFormat = CHROMA_420;
    buf.bufs.push_back(PelBuf(y.data(), w, w, h));
    buf.bufs.push_back(PelBuf(cb.data(), w >> 1, w >> 1, h >> 1));
    buf.bufs.push_back(PelBuf(cr.data(), w >> 1, w >> 1, h >> 1));
  }
};

}  // namespace

// nPlanes reference pictures (luma planes picW x picH, unpadded, one after the other; the borders are extended as the encoder does) and the
// settings the functions read
extern "C" int auref_open(const Pel* recY, int nPlanes, int picW, int picH, int bd, double lambda, int affineType, const unsigned* mvpIdxCost)
{
  if (!g)
  {
    g = new AuCtx();
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
  g->cfg->setClipForBiPredMeEnabled(false);
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
extern "C" int auref_set_lists(int n0, const int* planes0, int n1, const int* planes1)
{
  for (int r = 0; r < n0; r++) g->slice->m_apcRefPicList[REF_PIC_LIST_0][r] = g->pics[planes0[r]];
  for (int r = 0; r < n1; r++) g->slice->m_apcRefPicList[REF_PIC_LIST_1][r] = g->pics[planes1[r]];
  g->slice->m_aiNumRefIdx[REF_PIC_LIST_0] = n0; g->slice->m_aiNumRefIdx[REF_PIC_LIST_1] = n1;
  return 0;
}

// xGetAffineTemplateCost(pu, origBuf, m_tmpStorageLCU, mv, mvpIdx, AMVP_MAX_NUM_CANDS, list, refIdx); mv6 = LT, RT, LB as (hor, ver) with precision hp
extern "C" uint64_t auref_template_cost(const Pel* org, int orgStride, int posX, int posY, int w, int h, int six, int list, int refIdx, const int* mv6, int hp,
                                        int mvpIdx)
{
  AuUnit u(posX, posY, w, h, six);
  AuOrg o(org, orgStride, w, h);
  Mv mv[3];
  mv3(mv, mv6, hp);
  PelUnitBuf predBuf = g->is->m_tmpStorageLCU.getBuf(UnitAreaRelative(u.cu, u.pu));
  return g->is->xGetAffineTemplateCost(u.pu, o.buf, predBuf, mv, mvpIdx, AMVP_MAX_NUM_CANDS, RefPicList(list), refIdx);
}

// xAffineMotionEstimation(pu, origBuf, list, mvPred, refIdx, mv, bits, cost) (bBi = false).  mvPred6 with precision predHp, mv6 with mvHp on entry;
// mv6, bits in and out; mvHpOut: 1 when all three returned vectors carry the high-precision flag
extern "C" int auref_me(const Pel* org, int orgStride, int posX, int posY, int w, int h, int six, int list, int refIdx, const int* mvPred6, int predHp, int* mv6,
                        int mvHp, unsigned* bits, uint64_t* cost, int* mvHpOut)
{
  AuUnit u(posX, posY, w, h, six);
  AuOrg o(org, orgStride, w, h);
  Mv acMv[3], acMvPred[3];
  mv3(acMv, mv6, mvHp); mv3(acMvPred, mvPred6, predHp);
  uint32_t ruiBits = *bits;
  Distortion ruiCost = 0;
  g->is->xAffineMotionEstimation(u.pu, o.buf, RefPicList(list), acMvPred, refIdx, acMv, ruiBits, ruiCost);
  for (int k = 0; k < 3; k++) { mv6[2 * k] = acMv[k].getHor(); mv6[2 * k + 1] = acMv[k].getVer(); }
  *mvHpOut = acMv[0].highPrec && acMv[1].highPrec && acMv[2].highPrec;
  *bits = ruiBits; *cost = ruiCost;
  return 0;
}

// xCheckBestAffineMVP(pu, info = {cands, numCand}, list, mv, mvPred, mvpIdx, bits, cost); cands: [2][3][2] = candidate, (LT, RT, LB), (hor, ver) with
// precision candHp (mvPred6 too); mv6 with mvHp; mvPred6, mvpIdx, bits, cost in and out
extern "C" int auref_check_best_mvp(int six, int list, const int* mv6, int mvHp, int* mvPred6, int* mvpIdx, const int* cands, int candHp, int numCand,
                                    unsigned* bits, uint64_t* cost)
{
  AuUnit u(0, 0, 16, 16, six);
  AffineAMVPInfo info;
  info.numCand = numCand;
  for (int k = 0; k < 2; k++)
  {
    info.mvCandLT[k] = Mv(cands[6 * k + 0], cands[6 * k + 1], candHp != 0);
    info.mvCandRT[k] = Mv(cands[6 * k + 2], cands[6 * k + 3], candHp != 0);
    info.mvCandLB[k] = Mv(cands[6 * k + 4], cands[6 * k + 5], candHp != 0);
  }
  Mv acMv[3], acMvPred[3];
  mv3(acMv, mv6, mvHp); mv3(acMvPred, mvPred6, candHp);
  uint32_t ruiBits = *bits;
  Distortion ruiCost = *cost;
  int idx = *mvpIdx;
  g->is->xCheckBestAffineMVP(u.pu, info, RefPicList(list), acMv, acMvPred, idx, ruiBits, ruiCost);
  for (int k = 0; k < 3; k++) { mvPred6[2 * k] = acMvPred[k].getHor(); mvPred6[2 * k + 1] = acMvPred[k].getVer(); }
  *mvpIdx = idx; *bits = ruiBits; *cost = ruiCost;
  return 0;
}

// Mv(hor, ver, hp).roundMV2SignalPrecision() -> hv[0..1]
extern "C" int auref_round_mv(int hor, int ver, int hp, int* hv)
{
  Mv m(hor, ver, hp != 0);
  m.roundMV2SignalPrecision();
  hv[0] = m.getHor(); hv[1] = m.getVer();
  return 0;
}

// RdCost::getCost(bits)
extern "C" uint64_t auref_get_cost(unsigned bits) { return g->rc->getCost(bits); }

// the bits of one control-point vector at cost scale 0 through the reference's RdCost::setPredictor / getBitsOfVectorWithPredictor and Mv operators:
// v = (mv, mvHp) against pred = (pred, predHp), or, when second, against pred + (mv0 - pred0) (mv0 with mvHp, pred0 with predHp)
extern "C" unsigned auref_vector_bits(const int* mv, int mvHp, const int* pred, int predHp, int second, const int* mv0, const int* pred0)
{
  const Mv v(mv[0], mv[1], mvHp != 0), p(pred[0], pred[1], predHp != 0);
  g->rc->setCostScale(0);
  g->rc->setPredictor(p);
  if (second)
  {
    const Mv sp = p + (Mv(mv0[0], mv0[1], mvHp != 0) - Mv(pred0[0], pred0[1], predHp != 0));
    g->rc->setPredictor(sp);
  }
  const int shift = v.highPrec ? VCEG_AZ07_MV_ADD_PRECISION_BIT_FOR_STORE : 0;
  return g->rc->getBitsOfVectorWithPredictor(v.getHor() >> shift, v.getVer() >> shift, 0);
}
