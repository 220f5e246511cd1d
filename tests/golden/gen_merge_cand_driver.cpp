// gen_merge_cand_driver.cpp -- test infrastructure (tests/golden/gen_merge_cand.py builds and loads it on the build machine only): the reference's own
// InterPrediction::motionCompensation(pu, predBuf) for REF_PIC_LIST_X -- xPredInterUni / xPredInterBi for a MRG_TYPE_DEFAULT_N candidate, xSubPuMC on a
// hand-filled motion buffer for an ATMVP candidate --, RdCost::setDistParam(.., bUseHadamard) + distFunc, RdCost::getDistPart(DF_SSE), the cost
// expression of EncCu.cpp:1599 and updateCandList from its header, on a 4:2:0 Picture / Slice / PredictionUnit scaffold with four reference pictures
// in both lists.  Compiled against the reference's headers (-fno-access-control), linked with oracle/_ref/libvtmref.so; nothing of the reference is copied.
#include "CommonDef.h"
#include "Buffer.h"
#include "Slice.h"
#include "Picture.h"
#include "CodingStructure.h"
#include "RdCost.h"
#include "InterPrediction.h"
#include "UnitTools.h"
#include <vector>

namespace {

struct MgCtx
{
  SPS* sps; PPS* pps; CodingStructure* cs; PreCalcValues* pcv; Slice* slice; InterPrediction* ip; RdCost* rc;
  std::vector<Picture*> pics;
  int picW, picH, bd;
};
MgCtx* g = nullptr;

// eight ints of one block's motion: per list (present, picture = reference index, mv_x, mv_y)
MotionInfo motion_of(const int* m, bool highPrec)
{
  MotionInfo mi;
  mi.isInter = true; mi.sliceIdx = 0;
  mi.interDir = (char)((m[0] ? 1 : 0) | (m[4] ? 2 : 0));
  for (int l = 0; l < 2; l++)
  {
    mi.refIdx[l] = m[4 * l] ? (int16_t)m[4 * l + 1] : (int16_t)NOT_VALID;
    mi.mv[l] = m[4 * l] ? Mv(m[4 * l + 2], m[4 * l + 3], highPrec) : Mv(0, 0, highPrec);
  }
  return mi;
}

}  // namespace

// nPics reference pictures: luma planes picW x picH one after the other, chroma planes [picture][Cb, Cr] of half the size; unpadded, the borders
// are extended as the encoder does.  Both lists hold all of them in order (reference index = picture), POC = picture.
extern "C" int mgref_open(const Pel* recY, const Pel* recC, int nPics, int picW, int picH, int bd)
{
  if (!g)
  {
    g = new MgCtx();
    g->sps = new SPS; g->pps = new PPS;
    g->cs = static_cast<CodingStructure*>(calloc(1, sizeof(CodingStructure)));
    g->cs->sps = g->sps; g->cs->pps = g->pps;
    g->slice = new Slice;
    g->cs->slice = g->slice;
    g->rc = new RdCost; g->ip = new InterPrediction;
    g->rc->setUseQtbt(true);
    g->ip->init(g->rc, CHROMA_420);
    g->ip->m_maxCompIDToPred = COMPONENT_Cr;
    g->pcv = nullptr;
  }
  g->picW = picW; g->picH = picH; g->bd = bd;
  g->sps->setBitDepth(CHANNEL_TYPE_LUMA, bd); g->sps->setBitDepth(CHANNEL_TYPE_CHROMA, bd);
  g->sps->setPicWidthInLumaSamples(picW); g->sps->setPicHeightInLumaSamples(picH);
  g->sps->setMaxCUWidth(128); g->sps->setMaxCUHeight(128);
  g->sps->getSpsNext().setUseHighPrecMv(true);
  delete g->pcv;
  g->pcv = new PreCalcValues(*g->sps, *g->pps, true);
  g->cs->pcv = g->pcv;
  // the motion buffer xSubPuMC reads through pu.getMotionInfo(): the whole picture at the 4x4 granularity, by hand
  const_cast<UnitArea&>(g->cs->area) = UnitArea(CHROMA_420, Area(0, 0, picW, picH));
  free(g->cs->m_motionBuf);
  g->cs->m_motionBuf = static_cast<MotionInfo*>(calloc((size_t)(picW >> 2) * (picH >> 2), sizeof(MotionInfo)));
  g->slice->setSliceType(B_SLICE);
  g->slice->setPPS(g->pps);
  g->slice->setSPS(g->sps);
  ClpRngs& clp = g->slice->getClpRngs();
  for (int c = 0; c < MAX_NUM_COMPONENT; c++) { clp.comp[c].min = 0; clp.comp[c].max = (1 << bd) - 1; clp.comp[c].bd = bd; clp.comp[c].n = 0; }
  for (Picture* pic : g->pics) { free(pic->cs); pic->cs = nullptr; pic->destroy(); delete pic; }
  g->pics.clear();
  for (int k = 0; k < nPics; k++)
  {
    Picture* pic = new Picture;
    pic->create(CHROMA_420, Size(picW, picH), 128, 128 + 16, false);
    pic->cs = (CodingStructure*)calloc(1, sizeof(CodingStructure));
    const_cast<ChromaFormat&>(pic->cs->area.chromaFormat) = CHROMA_420;
    pic->poc = k;
    for (int c = 0; c < 3; c++)
    {
      PelBuf b = pic->getRecoBuf().get(ComponentID(c));
      const Pel* src = c ? recC + ((size_t)k * 2 + (c - 1)) * (picW >> 1) * (picH >> 1) : recY + (size_t)k * picW * picH;
      for (int j = 0; j < (int)b.height; j++)
        for (int i = 0; i < (int)b.width; i++) b.buf[(ptrdiff_t)j * b.stride + i] = src[(size_t)j * b.width + i];
    }
    pic->m_bIsBorderExtended = false;
    pic->extendPicBorder();
    g->pics.push_back(pic);
    g->slice->m_apcRefPicList[REF_PIC_LIST_0][k] = pic; g->slice->m_apcRefPicList[REF_PIC_LIST_1][k] = pic;
  }
  g->slice->m_aiNumRefIdx[REF_PIC_LIST_0] = nPics; g->slice->m_aiNumRefIdx[REF_PIC_LIST_1] = nPics;
  return 0;
}

// motionCompensation(pu, predBuf) of one merge candidate of the CU (x, y, w, h) into outY (pitch w), outCb, outCr (pitch w / 2).
// atmvp == 0: MRG_TYPE_DEFAULT_N with motion[8]; else MRG_TYPE_SUBPU_ATMVP with sub-blocks of 1 << subLog2 and motion[(h / 4)(w / 4)][8], the motion of
// every 4x4 unit of the CU.  highPrec: the vectors are in 1/16 units.  Returns 1 when the reference throws.
extern "C" int mgref_mc(int x, int y, int w, int h, int atmvp, int subLog2, const int* motion, int highPrec, Pel* outY, Pel* outCb, Pel* outCr)
{
  const UnitArea ua(CHROMA_420, Area(x, y, w, h));
  CodingUnit cu; PredictionUnit pu;
  cu.UnitArea::operator=(ua);
  pu.UnitArea::operator=(ua);
  cu.cs = g->cs; cu.slice = g->slice; cu.chromaFormat = CHROMA_420;
  cu.affine = false; cu.imv = 0; cu.transQuantBypass = false; cu.partSize = SIZE_2Nx2N; cu.qtDepth = 0;
  pu.cs = g->cs; pu.cu = &cu; pu.chromaFormat = CHROMA_420;
  pu.mergeFlag = true;
  g->slice->setSubPuMvpSubblkLog2Size(subLog2);
  if (!atmvp)
  {
    pu.mergeType = MRG_TYPE_DEFAULT_N;
    pu = motion_of(motion, highPrec != 0);
  }
  else
  {
    pu.mergeType = MRG_TYPE_SUBPU_ATMVP;
    pu.interDir = 3; pu.refIdx[0] = pu.refIdx[1] = 0;
    const int stride = g->picW >> 2;
    for (int j = 0; j < (h >> 2); j++)
      for (int i = 0; i < (w >> 2); i++)
        g->cs->m_motionBuf[(size_t)((y >> 2) + j) * stride + (x >> 2) + i] = motion_of(motion + 8 * ((size_t)j * (w >> 2) + i), highPrec != 0);
  }
  PelUnitBuf predBuf;
  predBuf.chromaFormat = CHROMA_420;
  predBuf.bufs.push_back(PelBuf(outY, w, w, h));
  predBuf.bufs.push_back(PelBuf(outCb, w >> 1, w >> 1, h >> 1));
  predBuf.bufs.push_back(PelBuf(outCr, w >> 1, w >> 1, h >> 1));
  try { g->ip->motionCompensation(pu, predBuf, REF_PIC_LIST_X); }
  catch (...) { return 1; }
  return 0;
}

// setDistParam(distParam, org, cur, bitDepth, compID, bUseHadamard) + distFunc (EncCu.cpp:1565, 1590)
extern "C" uint64_t mgref_dist(const Pel* org, int orgStride, const Pel* cur, int curStride, int w, int h, int comp, int useHad)
{
  DistParam dp;
  g->rc->setDistParam(dp, CPelBuf(org, orgStride, w, h), CPelBuf(cur, curStride, w, h), g->bd, ComponentID(comp), useHad != 0);
  return dp.distFunc(dp);
}

// getDistPart(org, cur, bitDepth, compID, DF_SSE) with the chroma distortion weight 1 (InterSearch.cpp:4762-4790; the weight stays on the host side of the entry)
extern "C" uint64_t mgref_sse(const Pel* org, int orgStride, const Pel* cur, int curStride, int w, int h, int comp)
{
  g->rc->setDistortionWeight(COMPONENT_Cb, 1.0); g->rc->setDistortionWeight(COMPONENT_Cr, 1.0);
  return g->rc->getDistPart(CPelBuf(org, orgStride, w, h), CPelBuf(cur, curStride, w, h), g->bd, ComponentID(comp), DF_SSE);
}

// :1594-1599
extern "C" double mgref_cost(uint64_t sad, unsigned mergeCand, int maxNumMergeCand, double sqrtLambda)
{
  Distortion uiSad = sad;
  uint32_t uiBitsCand = mergeCand + 1;
  if ((int)mergeCand == maxNumMergeCand - 1) uiBitsCand--;
  return (double)uiSad + (double)uiBitsCand * sqrtLambda;
}

// updateCandList(mode, cost, RdModeList, candCostList, fastNum) on lists handed over as arrays (*size entries, room for MRG_MAX_NUM_CANDS)
extern "C" int mgref_update_cand_list(unsigned mode, double cost, unsigned* modes, double* costs, int* size, int fastNum)
{
  static_vector<unsigned, MRG_MAX_NUM_CANDS> modeList;
  static_vector<double, MRG_MAX_NUM_CANDS> costList;
  for (int i = 0; i < *size; i++) { modeList.push_back(modes[i]); costList.push_back(costs[i]); }
  int r;
  try { r = (int)updateCandList(mode, cost, modeList, costList, (size_t)fastNum); }
  catch (...) { return -1; }
  *size = (int)modeList.size();
  for (int i = 0; i < *size; i++) { modes[i] = modeList[i]; costs[i] = costList[i]; }
  return r;
}
