// gen_alf_decide_driver.cpp -- test infrastructure (tests/golden/gen_alf_decide.py builds and loads it on the build machine only): the reference's own
// EncAdaptiveLoopFilter::getFrameStat (EncAdaptiveLoopFilter.cpp:1303-1315), getUnfilteredDistortion(cov, numClasses) (:618-626) and
// getFilteredDistortion (:628-639; private, hence -fno-access-control) on AlfCovariance objects filled from int64 records (E[N][N], y[N], pixAcc per
// CTU x class, as vvcgpu_alf_stats writes them).  Compiled against the reference's headers, linked with oracle/_ref/libvtmref.so; nothing of the
// reference is copied.
#include "CommonDef.h"
#include "EncAdaptiveLoopFilter.h"
#include <stdint.h>
#include <vector>

namespace {

EncAdaptiveLoopFilter* g = nullptr;

EncAdaptiveLoopFilter& enc()
{
  if (!g)
  {
    g = new EncAdaptiveLoopFilter;
    g->m_filterCoeffSet = new int*[MAX_NUM_ALF_CLASSES];
    for (int i = 0; i < MAX_NUM_ALF_CLASSES; i++) g->m_filterCoeffSet[i] = new int[MAX_NUM_ALF_LUMA_COEFF]();
  }
  return *g;
}

// nCtu x nCls objects of N coefficients, filled from the records
struct Covs
{
  std::vector<AlfCovariance*> ctu;
  int nCls;
  Covs(const int64_t* rec, int nCtu, int nCls_, int N) : ctu(nCtu), nCls(nCls_)
  {
    const int nv = N * N + N + 1;
    for (int c = 0; c < nCtu; c++)
    {
      ctu[c] = new AlfCovariance[nCls];
      for (int k = 0; k < nCls; k++)
      {
        AlfCovariance& a = ctu[c][k];
        const int64_t* r = rec + ((size_t)c * nCls + k) * nv;
        a.create(N);
        for (int i = 0; i < N; i++)
        {
          for (int j = 0; j < N; j++) a.E[i][j] = (double)r[i * N + j];
          a.y[i] = (double)r[N * N + i];
        }
        a.pixAcc = (double)r[N * N + N];
      }
    }
  }
  ~Covs()
  {
    for (AlfCovariance* p : ctu) { for (int k = 0; k < nCls; k++) p[k].destroy(); delete[] p; }
  }
};

}  // namespace

// getFrameStat into a reset frame record; out: nCls x (N*N+N+1) doubles in the record layout
extern "C" int alfref_frame_stat(const int64_t* rec, int nCtu, int nCls, int N, uint8_t* enable, double* out)
{
  EncAdaptiveLoopFilter& e = enc();
  Covs covs(rec, nCtu, nCls, N);
  std::vector<AlfCovariance> frame(nCls);
  for (int k = 0; k < nCls; k++) { frame[k].create(N); frame[k].reset(); }
  e.m_numCTUsInPic = nCtu;
  e.getFrameStat(frame.data(), covs.ctu.data(), enable, nCls);
  const int nv = N * N + N + 1;
  for (int k = 0; k < nCls; k++)
  {
    double* o = out + (size_t)k * nv;
    for (int i = 0; i < N; i++)
    {
      for (int j = 0; j < N; j++) o[i * N + j] = frame[k].E[i][j];
      o[N * N + i] = frame[k].y[i];
    }
    o[N * N + N] = frame[k].pixAcc;
    frame[k].destroy();
  }
  return 0;
}

// per CTU: out[2c] = getUnfilteredDistortion(cov, nCls), out[2c + 1] = getFilteredDistortion(cov, nCls, nFilters - 1, N) with m_filterCoeffSet =
// coeffSet (nFilters x N) and the row nFilters - 1 of m_filterIndices = idx.  getFilteredDistortion is compiled for m_NUM_BITS; any other coeffBits
// goes through the reference's calcErrorForCoeffs, class by class as :632-636 does.
extern "C" int alfref_ctu_dist(const int64_t* rec, int nCtu, int nCls, int N, const int* coeffSet, int nFilters, const short* idx, int coeffBits,
                               double* out)
{
  EncAdaptiveLoopFilter& e = enc();
  Covs covs(rec, nCtu, nCls, N);
  for (int f = 0; f < nFilters; f++)
    for (int i = 0; i < N; i++) e.m_filterCoeffSet[f][i] = coeffSet[f * N + i];
  for (int k = 0; k < nCls; k++) e.m_filterIndices[nFilters - 1][k] = nCls == 1 ? 0 : idx[k];
  for (int c = 0; c < nCtu; c++)
  {
    out[2 * c] = e.getUnfilteredDistortion(covs.ctu[c], nCls);
    if (coeffBits == AdaptiveLoopFilter::m_NUM_BITS) out[2 * c + 1] = e.getFilteredDistortion(covs.ctu[c], nCls, nFilters - 1, N);
    else
    {
      double dist = 0;
      for (int k = 0; k < nCls; k++)
      {
        AlfCovariance& a = covs.ctu[c][k];
        dist += e.calcErrorForCoeffs(a.E, a.y, e.m_filterCoeffSet[nCls == 1 ? 0 : e.m_filterIndices[nFilters - 1][k]], N, coeffBits);
      }
      out[2 * c + 1] = dist;
    }
  }
  return 0;
}
