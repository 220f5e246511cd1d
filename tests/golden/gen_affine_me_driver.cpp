// gen_affine_me_driver.cpp -- test infrastructure (tests/golden/gen_affine_me.py builds and loads it on the build machine only): the reference's own
// InterSearch::xAffineMotionEstimation (InterSearch.cpp:3286-3743; private, hence -fno-access-control) and InterPrediction::xPredAffineBlk on a real
// Picture / Slice / PredictionUnit that carry exactly what the two functions read.  Compiled against the reference's headers, linked with
// oracle/_ref/libvtmref.so; nothing of the reference is copied.
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

struct AfmCtx
{
  SPS* sps; CodingStructure* cs; PreCalcValues* pcv; Slice* slice; InterSearch* is; RdCost* rc; EncCfg* cfg; Picture* pic;
  int picW, picH, bd;
};
AfmCtx* g = nullptr;

}  // namespace

// one reference picture: luma plane (picW x picH, unpadded; the border is extended as the encoder does), bit depth, getUseAffineType, motion lambda
extern "C" int afmref_open(const Pel* recY, int picW, int picH, int bd, int affineType, double lambda)
{
  if (!g)
  {
    g = new AfmCtx();
    g->sps = new SPS;
    g->cs = static_cast<CodingStructure*>(calloc(1, sizeof(CodingStructure)));
    g->cs->sps = g->sps;
    g->slice = new Slice;
    g->cs->slice = g->slice;
    g->rc = new RdCost; g->cfg = new EncCfg; g->is = new InterSearch;
    g->rc->setUseQtbt(true);
    g->is->InterPrediction::init(g->rc, CHROMA_420);
    g->is->m_pcEncCfg = g->cfg;
    g->is->m_pcRdCost = g->rc;
    const UnitArea lcu(CHROMA_420, Area(0, 0, MAX_CU_SIZE, MAX_CU_SIZE));
    for (int i = 0; i < NUM_REF_PIC_LIST_01; i++) g->is->m_tmpPredStorage[i].create(lcu);
    g->is->m_tmpStorageLCU.create(lcu);
    g->is->m_tmpAffiStorage.create(lcu);
    g->is->m_tmpAffiError = new Pel[MAX_CU_SIZE * MAX_CU_SIZE];
    g->is->m_tmpAffiDeri[0] = new int[MAX_CU_SIZE * MAX_CU_SIZE];
    g->is->m_tmpAffiDeri[1] = new int[MAX_CU_SIZE * MAX_CU_SIZE];
    g->pcv = nullptr; g->pic = nullptr;
  }
  g->picW = picW; g->picH = picH; g->bd = bd;
  g->cfg->setClipForBiPredMeEnabled(false);
  g->sps->setBitDepth(CHANNEL_TYPE_LUMA, bd); g->sps->setBitDepth(CHANNEL_TYPE_CHROMA, bd);
  g->sps->setPicWidthInLumaSamples(picW); g->sps->setPicHeightInLumaSamples(picH);
  g->sps->setMaxCUWidth(128); g->sps->setMaxCUHeight(128);
  g->sps->getSpsNext().setUseAffineType(affineType != 0);
  delete g->pcv;
  g->pcv = new PreCalcValues(*g->sps, *(new PPS), true);
  g->cs->pcv = g->pcv;
  ClpRngs& clp = g->slice->getClpRngs();
  for (int c = 0; c < MAX_NUM_COMPONENT; c++) { clp.comp[c].min = 0; clp.comp[c].max = (1 << bd) - 1; clp.comp[c].bd = bd; clp.comp[c].n = 0; }
  g->rc->m_motionLambda = lambda;
  if (g->pic) { free(g->pic->cs); g->pic->cs = nullptr; g->pic->destroy(); delete g->pic; }
  g->pic = new Picture;
  g->pic->create(CHROMA_420, Size(picW, picH), 128, 128 + 16, false);
  g->pic->cs = (CodingStructure*)calloc(1, sizeof(CodingStructure));
  const_cast<ChromaFormat&>(g->pic->cs->area.chromaFormat) = CHROMA_420;
  for (int c = 0; c < 3; c++)
  {
    PelBuf b = g->pic->getRecoBuf().get(ComponentID(c));
    for (int j = 0; j < (int)b.height; j++)
      for (int i = 0; i < (int)b.width; i++) b.buf[(ptrdiff_t)j * b.stride + i] = c ? (Pel)(1 << (bd - 1)) : recY[(size_t)j * picW + i];
  }
  g->pic->m_bIsBorderExtended = false;
  g->pic->extendPicBorder();
  g->slice->m_apcRefPicList[REF_PIC_LIST_0][0] = g->pic;
  return 0;
}

namespace {

struct AfmUnit
{
  CodingUnit cu; PredictionUnit pu;
  AfmUnit(int posX, int posY, int w, int h, int six)
  {
    const UnitArea ua(CHROMA_420, Area(posX, posY, w, h));
    cu.UnitArea::operator=(ua);
    pu.UnitArea::operator=(ua);
    cu.cs = g->cs; cu.slice = g->slice; cu.chromaFormat = CHROMA_420;
    cu.affine = true; cu.affineType = six ? AFFINEMODEL_6PARAM : AFFINEMODEL_4PARAM;
    pu.cs = g->cs; pu.cu = &cu; pu.chromaFormat = CHROMA_420;
  }
};

}  // namespace

// the reference's affine luma prediction of one PU (final, rounded and clipped); mv6 = LT, RT, LB as (hor, ver) in 1/16 sample
extern "C" int afmref_pred(int posX, int posY, int w, int h, int six, const int* mv6, Pel* dst)
{
  AfmUnit u(posX, posY, w, h, six);
  Mv mv[3];
  for (int k = 0; k < 3; k++) mv[k] = Mv(mv6[2 * k], mv6[2 * k + 1], true);
  std::vector<Pel> cb((w >> 1) * (h >> 1)), cr((w >> 1) * (h >> 1));
  PelUnitBuf dstPic;
  dstPic.chromaFormat = CHROMA_420;
  dstPic.bufs.push_back(PelBuf(dst, w, w, h));
  dstPic.bufs.push_back(PelBuf(cb.data(), w >> 1, w >> 1, h >> 1));
  dstPic.bufs.push_back(PelBuf(cr.data(), w >> 1, w >> 1, h >> 1));
  g->is->xPredAffineBlk(COMPONENT_Y, u.pu, g->pic, mv, dstPic, false, g->slice->clpRng(COMPONENT_Y));
  return 0;
}

// one search.  org: the w x h block the search is made against (row stride orgStride); with bBi it is the "2 org - other prediction" block, which
// the reference forms itself as 2 * origBuf - m_tmpPredStorage[1 - list]: origBuf = 0 and the other prediction = -org reproduce the block exactly.
// mv6 / mvp6: acMv / acMvPred in 1/16 sample units (high precision); out: acMv (6 ints), ruiBits, then ruiCost in outCost.
extern "C" int afmref_search(const Pel* org, int orgStride, int posX, int posY, int w, int h, int six, int bBi, const int* mv6, const int* mvp6,
                             unsigned bits, int* outMv6, unsigned* outBits, uint64_t* outCost)
{
  AfmUnit u(posX, posY, w, h, six);
  std::vector<Pel> y((size_t)w * h), cb((w >> 1) * (h >> 1), 0), cr((w >> 1) * (h >> 1), 0);
  if (bBi)
  {
    PelUnitBuf other = g->is->m_tmpPredStorage[1].getBuf(UnitAreaRelative(u.cu, u.pu));
    other.bufs[1].fill(0); other.bufs[2].fill(0);
    for (int j = 0; j < h; j++)
      for (int i = 0; i < w; i++) { other.Y().at(i, j) = (Pel)(-org[(size_t)j * orgStride + i]); y[(size_t)j * w + i] = 0; }
  }
  else
    for (int j = 0; j < h; j++)
      for (int i = 0; i < w; i++) y[(size_t)j * w + i] = org[(size_t)j * orgStride + i];
  PelUnitBuf origBuf;
  origBuf.chromaFormat = CHROMA_420;
  origBuf.bufs.push_back(PelBuf(y.data(), w, w, h));
  origBuf.bufs.push_back(PelBuf(cb.data(), w >> 1, w >> 1, h >> 1));
  origBuf.bufs.push_back(PelBuf(cr.data(), w >> 1, w >> 1, h >> 1));
  Mv acMv[3], acMvPred[3];
  for (int k = 0; k < 3; k++) { acMv[k] = Mv(mv6[2 * k], mv6[2 * k + 1], true); acMvPred[k] = Mv(mvp6[2 * k], mvp6[2 * k + 1], true); }
  uint32_t ruiBits = bits;
  Distortion ruiCost = 0;
  g->is->xAffineMotionEstimation(u.pu, origBuf, REF_PIC_LIST_0, acMvPred, 0, acMv, ruiBits, ruiCost, bBi != 0);
  for (int k = 0; k < 3; k++) { outMv6[2 * k] = acMv[k].getHor(); outMv6[2 * k + 1] = acMv[k].getVer(); }
  *outBits = ruiBits; *outCost = ruiCost;
  return 0;
}
