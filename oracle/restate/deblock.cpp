// oracle/restate/deblock.cpp -- TEST INFRASTRUCTURE: CPU restatement of the deblocking sample filters.
// Follows LoopFilter::xEdgeFilterLuma (CommonLib/LoopFilter.cpp:543-681), xEdgeFilterChroma (:684-838),
// xPelFilterLuma (:856-916), xPelFilterChroma (:928-949), xUseStrongFiltering (:960-970), xCalcDP/DQ
// (:972-980), tables sm_tcTable/sm_betaTable (:66-80), g_aucChromaScale[CHROMA_420] (Rom.cpp:528);
// pass order of loopFilterPic (:149-230): every vertical edge of the picture, then every horizontal edge.
// Edge selection / boundary strength arrive as maps (see include/vvcgpu.h, vvcgpu_deblock).
#include "orc_common.h"

static const uint8_t tcTable[66] = {
  0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,1,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,5,5,6,6,7,8,9,10,11,13,14,16,18,20,22,24,
  26,28,30,32,34,36,38,40,42,44,46,48 };
static const uint8_t betaTable[64] = {
  0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,6,7,8,9,10,11,12,13,14,15,16,17,18,20,22,24,26,28,30,32,34,36,38,40,42,44,46,48,50,52,
  54,56,58,60,62,64,66,68,70,72,74,76,78,80,82,84,86,88 };
static const uint8_t chromaScale420[70] = {
  0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,29,30,31,32,33,33,34,34,35,35,36,36,
  37,37,38,39,40,41,42,43,44,45,46,47,48,49,50,51,52,53,54,55,56,57,58,59,60,61,62,63 };
static const int MAXQP = 63, TCOFF = 2, QPMAPSZ = 70;

// ---- census ---------------------------------------------------------------------------------------------------------------------
// orc_deblock_census runs the code below with a counter array; orc_deblock runs it with none.  The events are named ONCE, here: the enum and
// the text orc_deblock_census_names() returns come from this list.  `_eq_` in a name marks an event of a value sitting exactly on (or one below)
// its threshold (`_m1`: one below it, the last value that passes).  Luma events count 4-line segments, those of pelFilterLuma count lines; the chroma
// events exist once per plane (cb_, cr_).  Counters: [direction (0 vertical edges, 1 horizontal edges)][event].
//   the three terms of xUseStrongFiltering (ds: |m0-m3|+|m7-m4| against beta>>3, dd: 2 d_line against beta>>2, dm: |m3-m4| against (5 tc+1)>>1) are
//   counted per decision line (0 and 3) and only where the term DECIDES: every other term of both lines holds, so that `<=` for `<` in this term
//   would turn a weak segment strong (`_eq_thr`), or `< thr - 1` a strong one weak (`_eq_thr_m1`); dpq_* are counted on weak segments (fP / fQ in use)
#define DB_LUMA_EVENTS(X) \
  X(seg) X(d_lt_beta) X(d_eq_beta) X(d_eq_beta_m1) X(strong) X(weak) \
  X(ds_eq_thr) X(ds_eq_thr_m1) X(dd_eq_thr) X(dd_eq_thr_m1) X(dm_eq_thr) X(dm_eq_thr_m1) \
  X(fP) X(fQ) X(dpq_eq_side) X(dpq_eq_side_m1) \
  X(delta_ge_thr) X(delta_eq_thr) X(delta_eq_thr_m1) X(delta_clipped) X(tc2_clipped) \
  X(strong_clip_p0) X(strong_clip_q0) X(strong_clip_p1) X(strong_clip_q1) X(strong_clip_p2) X(strong_clip_q2) \
  X(weak_clp_clipped) X(strong_outside_clp) X(strong_noP) X(strong_noQ) X(weak_noP) X(weak_noQ) \
  X(tc_idx_lo) X(tc_idx_hi) X(beta_idx_lo) X(beta_idx_hi) X(tc0_d_lt_beta)
#define DB_CHROMA_EVENTS(X, c) \
  X(c##_seg) X(c##_qp_ge70) X(c##_qp_lt0) X(c##_tc0) X(c##_delta_clipped) X(c##_clp_clipped) X(c##_noP) X(c##_noQ)
#define DB_EVENTS(X) DB_LUMA_EVENTS(X) DB_CHROMA_EVENTS(X, cb) DB_CHROMA_EVENTS(X, cr)
#define DB_ENUM(n) EV_##n,
enum { DB_EVENTS(DB_ENUM) EV_COUNT };
#define DB_NAME(n) #n ","
static const char dbEventNames[] = DB_EVENTS(DB_NAME);
static const int EV_CHROMA_STEP = EV_cr_seg - EV_cb_seg;

static inline void hit(int64_t* cn, int ev, bool cond = true) { if (cn && cond) cn[ev]++; }

static inline void pelFilterLuma(Pel* s, int o, int tc, bool sw, bool noP, bool noQ, int thrCut, bool fP, bool fQ,
                                 int cmin, int cmax, int64_t* cn)
{
  const int m4 = s[0], m3 = s[-o], m5 = s[o], m2 = s[-2 * o], m6 = s[2 * o], m1 = s[-3 * o], m7 = s[3 * o], m0 = s[-4 * o];
  if (sw)
  {
    const int f3 = (m1 + 2 * m2 + 2 * m3 + 2 * m4 + m5 + 4) >> 3, f4 = (m2 + 2 * m3 + 2 * m4 + 2 * m5 + m6 + 4) >> 3;
    const int f2 = (m1 + m2 + m3 + m4 + 2) >> 2, f5 = (m3 + m4 + m5 + m6 + 2) >> 2;
    const int f1 = (2 * m0 + 3 * m1 + m2 + m3 + m4 + 4) >> 3, f6 = (m3 + m4 + m5 + 3 * m6 + 2 * m7 + 4) >> 3;
    s[-o]     = (Pel)clip3i(m3 - 2 * tc, m3 + 2 * tc, f3);
    s[0]      = (Pel)clip3i(m4 - 2 * tc, m4 + 2 * tc, f4);
    s[-2 * o] = (Pel)clip3i(m2 - 2 * tc, m2 + 2 * tc, f2);
    s[o]      = (Pel)clip3i(m5 - 2 * tc, m5 + 2 * tc, f5);
    s[-3 * o] = (Pel)clip3i(m1 - 2 * tc, m1 + 2 * tc, f1);
    s[2 * o]  = (Pel)clip3i(m6 - 2 * tc, m6 + 2 * tc, f6);
    if (cn)
    {
      hit(cn, EV_strong_clip_p0, abs(f3 - m3) > 2 * tc); hit(cn, EV_strong_clip_q0, abs(f4 - m4) > 2 * tc);
      hit(cn, EV_strong_clip_p1, abs(f2 - m2) > 2 * tc); hit(cn, EV_strong_clip_q1, abs(f5 - m5) > 2 * tc);
      hit(cn, EV_strong_clip_p2, abs(f1 - m1) > 2 * tc); hit(cn, EV_strong_clip_q2, abs(f6 - m6) > 2 * tc);
      bool out = false;
      for (int k = -3; k < 3; k++) out = out || s[k * o] < cmin || s[k * o] > cmax;
      hit(cn, EV_strong_outside_clp, out);
    }
  }
  else
  {
    int delta = (9 * (m4 - m3) - 3 * (m5 - m2) + 8) >> 4;
    hit(cn, EV_delta_ge_thr, abs(delta) >= thrCut); hit(cn, EV_delta_eq_thr, abs(delta) == thrCut); hit(cn, EV_delta_eq_thr_m1, abs(delta) == thrCut - 1);
    if (abs(delta) < thrCut)
    {
      hit(cn, EV_delta_clipped, abs(delta) > tc);
      delta = clip3i(-tc, tc, delta);
      bool clp = m3 + delta != clip3i(cmin, cmax, m3 + delta) || m4 - delta != clip3i(cmin, cmax, m4 - delta), t2 = false;
      s[-o] = (Pel)clip3i(cmin, cmax, m3 + delta);
      s[0]  = (Pel)clip3i(cmin, cmax, m4 - delta);
      const int tc2 = tc >> 1;
      if (fP)
      {
        const int r1 = ((((m1 + m3 + 1) >> 1) - m2 + delta) >> 1), d1 = clip3i(-tc2, tc2, r1);
        s[-2 * o] = (Pel)clip3i(cmin, cmax, m2 + d1);
        t2 = t2 || r1 != d1; clp = clp || s[-2 * o] != m2 + d1;
      }
      if (fQ)
      {
        const int r2 = ((((m6 + m4 + 1) >> 1) - m5 - delta) >> 1), d2 = clip3i(-tc2, tc2, r2);
        s[o] = (Pel)clip3i(cmin, cmax, m5 + d2);
        t2 = t2 || r2 != d2; clp = clp || s[o] != m5 + d2;
      }
      hit(cn, EV_tc2_clipped, t2); hit(cn, EV_weak_clp_clipped, clp);
    }
  }
  if (noP) { s[-o] = (Pel)m3; s[-2 * o] = (Pel)m2; s[-3 * o] = (Pel)m1; }
  if (noQ) { s[0] = (Pel)m4; s[o] = (Pel)m5; s[2 * o] = (Pel)m6; }
}

// the three terms of xUseStrongFiltering of one line: bit 0 ds, bit 1 dd, bit 2 dm hold; v[k] = the term's value, t[k] = its threshold
static inline int strongTerms(const Pel* s, int o, int d, int beta, int tc, int* v, int* t)
{
  const int m4 = s[0], m3 = s[-o], m7 = s[3 * o], m0 = s[-4 * o];
  v[0] = abs(m0 - m3) + abs(m7 - m4); t[0] = beta >> 3;
  v[1] = d;                           t[1] = beta >> 2;
  v[2] = abs(m3 - m4);                t[2] = (tc * 5 + 1) >> 1;
  return (v[0] < t[0] ? 1 : 0) | (v[1] < t[1] ? 2 : 0) | (v[2] < t[2] ? 4 : 0);
}
static inline int calcDP(const Pel* s, int o) { return abs(s[-3 * o] - 2 * s[-2 * o] + s[-o]); }
static inline int calcDQ(const Pel* s, int o) { return abs(s[0] - 2 * s[o] + s[2 * o]); }

// one 4-line luma segment; s points at line 0, Q-side sample 0; o = step across the edge, ls = step along it
static void lumaSegment(Pel* s, int o, int ls, int bs, int qpP, int qpQ, bool noP, bool noQ, const vvcgpu_deblock_cfg& c, int64_t* cn)
{
  const int qp = (qpP + qpQ + 1) >> 1;
  const int scale = 1 << (c.bit_depth_luma - 8);
  const int rawTc = qp + TCOFF * (bs - 1) + (c.tc_offset_div2 << 1), rawB = qp + (c.beta_offset_div2 << 1);
  const int idxTc = clip3i(0, MAXQP + TCOFF, rawTc);
  const int idxB = clip3i(0, MAXQP, rawB);
  const int tc = tcTable[idxTc] * scale, beta = betaTable[idxB] * scale;
  const int side = (beta + (beta >> 1)) >> 3, thrCut = tc * 10;
  const int dp0 = calcDP(s, o), dq0 = calcDQ(s, o), dp3 = calcDP(s + 3 * ls, o), dq3 = calcDQ(s + 3 * ls, o);
  const int d0 = dp0 + dq0, d3 = dp3 + dq3, dp = dp0 + dp3, dq = dq0 + dq3, d = d0 + d3;
  hit(cn, EV_seg);
  hit(cn, EV_tc_idx_lo, rawTc < 0); hit(cn, EV_tc_idx_hi, rawTc > MAXQP + TCOFF); hit(cn, EV_beta_idx_lo, rawB < 0); hit(cn, EV_beta_idx_hi, rawB > MAXQP);
  hit(cn, EV_d_eq_beta, d == beta); hit(cn, EV_d_eq_beta_m1, d == beta - 1);
  if (d < beta)
  {
    const bool fP = dp < side, fQ = dq < side;
    int v0[3], t0[3], v3[3], t3[3];
    const int ok0 = strongTerms(s, o, 2 * d0, beta, tc, v0, t0), ok3 = strongTerms(s + 3 * ls, o, 2 * d3, beta, tc, v3, t3);
    const bool sw = ok0 == 7 && ok3 == 7;
    if (cn)
    {
      hit(cn, EV_d_lt_beta); hit(cn, EV_tc0_d_lt_beta, tc == 0); hit(cn, sw ? EV_strong : EV_weak);
      for (int k = 0; k < 3; k++)
      {
        const int rest = 7 & ~(1 << k);
        hit(cn, EV_ds_eq_thr + 2 * k, v0[k] == t0[k] && (ok0 & rest) == rest && ok3 == 7);
        hit(cn, EV_ds_eq_thr + 2 * k, v3[k] == t3[k] && (ok3 & rest) == rest && ok0 == 7);
        hit(cn, EV_ds_eq_thr_m1 + 2 * k, sw && v0[k] == t0[k] - 1);
        hit(cn, EV_ds_eq_thr_m1 + 2 * k, sw && v3[k] == t3[k] - 1);
      }
      hit(cn, EV_fP, fP); hit(cn, EV_fQ, fQ);
      hit(cn, EV_dpq_eq_side, !sw && (dp == side || dq == side)); hit(cn, EV_dpq_eq_side_m1, !sw && (dp == side - 1 || dq == side - 1));
      hit(cn, sw ? EV_strong_noP : EV_weak_noP, noP); hit(cn, sw ? EV_strong_noQ : EV_weak_noQ, noQ);
    }
    for (int i = 0; i < 4; i++) pelFilterLuma(s + i * ls, o, tc, sw, noP, noQ, thrCut, fP, fQ, c.clp_min[0], c.clp_max[0], cn);
  }
}

static void chromaSegment(Pel* s, int o, int ls, int n, int qpP, int qpQ, int qpOff, bool noP, bool noQ, int comp,
                          const vvcgpu_deblock_cfg& c, int64_t* cn)
{
  int qp = ((qpP + qpQ + 1) >> 1) + qpOff;
  int64_t* cc = cn ? cn + (comp - 1) * EV_CHROMA_STEP : nullptr;
  hit(cc, EV_cb_seg); hit(cc, EV_cb_qp_ge70, qp >= QPMAPSZ); hit(cc, EV_cb_qp_lt0, qp < 0); hit(cc, EV_cb_noP, noP); hit(cc, EV_cb_noQ, noQ);
  if (qp >= QPMAPSZ) qp -= 6;                            // 4:2:0 (:812-817)
  else if (qp >= 0) qp = chromaScale420[qp];             // getScaledChromaQP clips to [0, size-1]
  const int idxTc = clip3i(0, MAXQP + TCOFF, qp + TCOFF * (2 - 1) + (c.tc_offset_div2 << 1));
  const int tc = tcTable[idxTc] * (1 << (c.bit_depth_chroma - 8));
  hit(cc, EV_cb_tc0, tc == 0);
  for (int i = 0; i < n; i++)
  {
    Pel* q = s + i * ls;
    const int m4 = q[0], m3 = q[-o], m5 = q[o], m2 = q[-2 * o];
    const int raw = ((((m4 - m3) << 2) + m2 - m5 + 4) >> 3);
    const int delta = clip3i(-tc, tc, raw);
    if (!noP) q[-o] = (Pel)clip3i(c.clp_min[comp], c.clp_max[comp], m3 + delta);
    if (!noQ) q[0] = (Pel)clip3i(c.clp_min[comp], c.clp_max[comp], m4 - delta);
    hit(cc, EV_cb_delta_clipped, raw != delta);
    hit(cc, EV_cb_clp_clipped, (!noP && q[-o] != m3 + delta) || (!noQ && q[0] != m4 - delta));
  }
}

static int deblockPicture(Pel* Y, int strideY, Pel* Cb, Pel* Cr, int strideC, int w, int h,
                          const uint8_t* edgeV, const uint8_t* edgeH, const int8_t* qpY, const int8_t* qpC,
                          const vvcgpu_deblock_cfg* cfg, int64_t* counters)
{
  const vvcgpu_deblock_cfg& c = *cfg;
  const int w4 = w >> 2, h4 = h >> 2;
  for (int dir = 0; dir < 2; dir++)
  {
    const uint8_t* em = dir == 0 ? edgeV : edgeH;
    int64_t* cn = counters ? counters + dir * EV_COUNT : nullptr;
    for (int uy = 0; uy < h4; uy++)
      for (int ux = 0; ux < w4; ux++)
      {
        const int u = uy * w4 + ux;
        const int e = em[u];
        if (!e) continue;
        if (dir == 0 ? ux == 0 : uy == 0) continue;           // picture border: never an edge (leftEdge/topEdge, :408-415)
        const int uP = dir == 0 ? u - 1 : u - w4;
        const bool noP = (e >> 4) & 1, noQ = (e >> 5) & 1;
        const int bsY = e & 3, bsC = (e >> 2) & 3;
        const int x = ux * 4, y = uy * 4;
        if (bsY && (dir == 0 ? (x & 7) == 0 : (y & 7) == 0))
        {
          Pel* s = Y + y * strideY + x;
          lumaSegment(s, dir == 0 ? 1 : strideY, dir == 0 ? strideY : 1, bsY, qpY[uP], qpY[u], noP, noQ, c, cn);
        }
        if (Cb && bsC > 1 && (dir == 0 ? (x & 15) == 0 : (y & 15) == 0))
        {
          Pel* planes[2] = { Cb, Cr };
          for (int k = 0; k < 2; k++)
          {
            Pel* s = planes[k] + (y >> 1) * strideC + (x >> 1);
            chromaSegment(s, dir == 0 ? 1 : strideC, dir == 0 ? strideC : 1, 2, qpC[uP], qpC[u],
                          k == 0 ? c.cb_qp_offset : c.cr_qp_offset, noP, noQ, 1 + k, c, cn);
          }
        }
      }
  }
  return 0;
}

// Cb == Cr == NULL: luma alone, as vvcgpu_deblock takes it
ORC_API int orc_deblock(Pel* Y, int strideY, Pel* Cb, Pel* Cr, int strideC, int w, int h,
                        const uint8_t* edgeV, const uint8_t* edgeH, const int8_t* qpY, const int8_t* qpC,
                        const vvcgpu_deblock_cfg* cfg)
{
  return deblockPicture(Y, strideY, Cb, Cr, strideC, w, h, edgeV, edgeH, qpY, qpC, cfg, nullptr);
}

// the same pass, counting which branches it takes: counters[dir * n + event] += ..., dir 0 = vertical edges, 1 = horizontal edges, n and the
// events' order as orc_deblock_census_names gives them.  The caller zeroes (or keeps accumulating into) the array.
ORC_API int orc_deblock_census(Pel* Y, int strideY, Pel* Cb, Pel* Cr, int strideC, int w, int h,
                               const uint8_t* edgeV, const uint8_t* edgeH, const int8_t* qpY, const int8_t* qpC,
                               const vvcgpu_deblock_cfg* cfg, int64_t* counters)
{
  return deblockPicture(Y, strideY, Cb, Cr, strideC, w, h, edgeV, edgeH, qpY, qpC, cfg, counters);
}

// comma-terminated names of the events, in the order of the counters; returns their number
ORC_API int orc_deblock_census_names(const char** names)
{
  *names = dbEventNames;
  return EV_COUNT;
}
