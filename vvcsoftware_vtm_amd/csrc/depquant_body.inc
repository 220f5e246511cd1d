// depquant_body.inc -- the body of the two trellis kernels (depquant_dev.h): workgroups of 256 threads with TQ_LDS_BYTES of dynamic LDS, quad
// 64 blockIdx.x + threadIdx.x / 4 takes work item wi of n (n >= 1).  The including kernel has the parameters coeffBase, levelBase, descs, n,
// ratesBase, bd, absSumOut, wsDec, wsCtx and tb under these names and defines LISTED and list.  LISTED: work item wi is the descriptor list[wi], and
// its abs_sum goes to that index; otherwise descriptor wi (list is not read).  A body function that both kernels called would change the code of
// depquant_kernel (docs/MEASUREMENTS.md); this way it is compiled from the same statements as before.
  const int lane = threadIdx.x & 63, k = lane & 3, qbase = lane & ~3;
  const int wi = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (lane >> 2);
  const bool live = wi < n;
  const int ti = LISTED ? list[live ? wi : n - 1] : wi;                    // (used as an index under `live` only)
  const vvcgpu_depquant_desc d = descs[LISTED ? ti : live ? ti : n - 1];
  const int w = d.w, h = d.h, N = w * h, lw = ilog2(w), lh = ilog2(h);
  const int widthInSbb = w >> 2, heightInSbb = h >> 2, numSbb = N >> 4;
  const bool luma = d.luma != 0;
  const TCoeff* coef = coeffBase + d.coeff_off;
  TCoeff* level = levelBase + d.level_off;
  const int tabOff = tb.scanOff[(lw - 1) * 6 + (lh - 1)];
  const unsigned short* scan = tb.scan + tabOff;
  const unsigned short* inv = tb.dqInv + tabOff;
  const uint4* posSel = tb.dqPosSel + tabOff;
  const uint2* posMisc = tb.dqPosMisc + tabOff;
  unsigned* dec = wsDec + (size_t)d.coeff_off * 4;                         // [scanIdx][4]
  // CommonCtx's per-state sub-block memory (:828-858) as a pool of 16-byte blocks [sub-block in scan order][context slot]: the levels of a
  // sub-block as the state that took slot k at its end left them (the first 4 N of the 8 N bytes a TU has in the workspace)
  unsigned char* ctxMem = wsCtx + (size_t)d.coeff_off * 8;

  // Quantizer::initQuantBlock :647-706 (the same IEEE double arithmetic)
  int qShift, maxQIdx, thresLast, distShift;
  long long qAdd, qScale, distAdd, distStepAdd, distOrgFact;
  {
    const int qpDQ = d.qp + 1, qpPer = qpDQ / 6, qpRem = qpDQ - 6 * qpPer;
    const bool sqrt2 = vq_sqrt2(lw, lh);
    const int transformShift = vq_transform_shift(bd, lw, lh);
    const int qs = vq_quant_scale(qpRem);
    qShift = vq_qbits(qpPer, transformShift) - 1;
    qAdd = -((3ll << qShift) >> 1);
    const int invShift = vq_inv(qpDQ, transformShift, sqrt2).rightShift + 1;
    qScale = vq_quant_scale_folded(qpRem, sqrt2);
    const unsigned qIdxBD = min(16u, (unsigned)(32 + invShift - 6 - 1));
    maxQIdx = (1 << (qIdxBD - 1)) - 4;
    thresLast = (int)((3ll << qShift) / (4 * qScale));
    const int nomDShift = 15 - 2 * transformShift + qShift;
    const double qScale2 = (double)((long long)qs * qs);
    const double nomDistFactor = nomDShift < 0 ? 1.0 / ((double)(1ll << (-nomDShift)) * qScale2 * d.lambda) : (double)(1ll << nomDShift) / (qScale2 * d.lambda);
    const long long pow2dfShift = (long long)(nomDistFactor * qScale2) + 1;
    int dfShift = 0;
    while ((1ull << dfShift) < (unsigned long long)pow2dfShift && dfShift < 63) dfShift++;
    distShift = 62 + qShift - 2 * 15 - dfShift;
    distAdd = (1ll << distShift) >> 1;
    distStepAdd = (long long)(nomDistFactor * (double)(1ll << (distShift + qShift)) + .5);
    distOrgFact = (long long)(nomDistFactor * (double)(1ll << (distShift + 1)) + .5);
  }

  // first tested position :1337-1349 (four lanes split the search), levels start as zero
  int first = -1;
  if (live)
  {
    for (int i = k; i < N; i += 4) level[i] = 0;
    // (sixteen positions a round per quad, the loads of a round independent of each other: the search of a 64x64 TU with a zeroed-out
    // high-frequency region walks ~2000 positions whose coefficients come from memory)
    for (int i = N - 1 - k; i >= 0 && first < 0; i -= 16)
    {
      int a[4];
#pragma unroll
      for (int u = 0; u < 4; u++) a[u] = abs(coef[scan[max(i - 4 * u, 0)]]);
#pragma unroll
      for (int u = 3; u >= 0; u--) if (i - 4 * u >= 0 && a[u] > thresLast) first = i - 4 * u;
    }
  }
  first = max(first, __shfl_xor(first, 1));
  first = max(first, __shfl_xor(first, 2));
  if (live && first < 0 && k == 0) absSumOut[ti] = 0;

  // LDS: per quad the position records and the template seeds of its four context slots; per workgroup the rate tables.  The tables
  // are looked up on the critical path of every step, so the walk only ever reads them from LDS: up to TQ_RT_SLOTS distinct tables of
  // the workgroup's 64 TUs are staged per pass, TUs whose table found no slot walk in the next pass (one pass unless a caller
  // mixes more than sixteen tables inside 64 consecutive TUs).
  extern __shared__ __align__(16) unsigned char tqSmem[];
  TqRec* const recTu = reinterpret_cast<TqRec*>(tqSmem) + (threadIdx.x >> 2) * TQ_REC_N;
  unsigned* const seedTu = reinterpret_cast<unsigned*>(tqSmem + 64 * TQ_REC_N * sizeof(TqRec)) + (threadIdx.x >> 2) * (TQ_SEED_BYTES / 4);
  __shared__ vvcgpu_dq_rates rtCache[TQ_RT_SLOTS];
  __shared__ int rtSlot[TQ_RT_SLOTS];
  __shared__ int rtPending;
#pragma unroll
  for (int i = 0; i < TQ_SEED_BYTES / 4 / 4; i++) seedTu[k * (TQ_SEED_BYTES / 4 / 4) + i] = 0u;

  auto walk = [&](const bool run, TqLdsRates rt)
  {
  int maxFirst = run ? first : -1;
#pragma unroll
  for (int m = 4; m < 64; m <<= 1) maxFirst = max(maxFirst, __shfl_xor(maxFirst, m));
  maxFirst = __builtin_amdgcn_readfirstlane(maxFirst);                    // the walk's position is the same in every lane: keep it (and what
  if (maxFirst < 0) return;                                               // derives from it) in scalar registers

  const int sigSet = max(k - 1, 0);                                       // RateEstimator::sigFlagBits(stateId) :282-285
  TqState P, S;                                                           // previous-position state k, skip state k
  {
    P.rdCost = 0x7FFFFFFFFFFFFFFFll >> 1; P.numSigSbb = 0; P.refSbbCtxId = -1; P.goRice = 0; P.sbb0 = P.sbb1 = 0;
    P.sig0 = rt->sig[sigSet][0][0]; P.sig1 = rt->sig[sigSet][0][1];
    P.lev = tq_u4{ 0, 0, 0, 0 }; P.aux = tq_u4{ 0, 0, 0, 0 }; P.gc = 0;
    tq_copy(S, P);
  }
  TqState P0; tq_copy(P0, P);
  // The level history of a state (CommonCtx::update copies `setCpSize` bytes of it from the parent state at every sub-block end, :1104-1130)
  // is never copied here: a block of the pool is written once, and a context slot carries the ANCESTRY of its path -- which slot its
  // ancestor took at the end of each of the last 32 sub-blocks, two bits each, youngest in the low bits, and how many of them exist
  // (a path that starts inside a sub-block has none: the reference zeroes its history).  The farthest block a template reads lies 30
  // sub-blocks back (64x64).  Like the flags below, the pair lives in the lane whose number is the slot's.  The copy was 30 x 64 lines
  // of 16 bytes per wavefront and sub-block end for 64x64 TUs, a twentieth of their walk.
  unsigned long long ancCur = 0; int ancLen = 0;
  tq_u8 Fcur;                                                             // coded-sub-block flags (bit per sub-block) of context slot k, current half
#pragma unroll
  for (int i = 0; i < 8; i++) Fcur[i] = 0;
  long long finalCost = 0;

  auto fillRec = [&](int si, int p, int coefAbs, const uint4 sel, const unsigned misc)
  {
    const int x = p & (w - 1), y = p >> lw;
    // Quantizer::preQuantCoeff :786-808
    tq_l4 pqDist = { 0, 0, 0, 0 }; tq_i4 pqAbs = { 0, 0, 0, 0 };
    {
      const long long scaledOrg = (long long)coefAbs * qScale;
      int qIdx = max(1, min(maxQIdx, (int)((scaledOrg + qAdd) >> qShift)));
      long long scaledAdd = qIdx * distStepAdd - scaledOrg * distOrgFact;
#pragma unroll
      for (int i = 0; i < 4; i++)
      {
        const int slot = qIdx & 3;
        const long long dd = (scaledAdd * qIdx + distAdd) >> distShift;
        const int al = (++qIdx) >> 1;
#pragma unroll
        for (int t = 0; t < 4; t++) { pqDist[t] = t == slot ? dd : pqDist[t]; pqAbs[t] = t == slot ? al : pqAbs[t]; }
        scaledAdd += distStepAdd;
      }
    }
    const int lastOffset = rt->last_x[x] + rt->last_y[y];
    TqRec* r = recTu + (si & (TQ_REC_N - 1));
    r->selLoA = sel.x; r->selHiA = sel.y; r->selLoB = sel.z; r->selHiB = sel.w;       // the shape-only part: straight from the table
#pragma unroll
    for (int t = 0; t < 4; t++) r->dist[t] = pqDist[t];
    *reinterpret_cast<uint2*>(r->ab) = make_uint2((unsigned)pqAbs[0] | (unsigned)pqAbs[1] << 16, (unsigned)pqAbs[2] | (unsigned)pqAbs[3] << 16);
    r->start[0] = pqDist[0] + lastOffset + tq_level_bits(rt, 0, 0, (unsigned)pqAbs[0]);
    r->start[1] = pqDist[2] + lastOffset + tq_level_bits(rt, 0, 0, (unsigned)pqAbs[2]);
    r->misc = misc;
  };
  // transitions leaving state k: state 0: pq0 -> dec0, pq2 -> dec2; state 1: pq2 -> dec0, pq0 -> dec2; state 2: pq3 -> dec1, pq1 -> dec3;
  // state 3: pq1 -> dec1, pq3 -> dec3; the zero transition goes to dec0 / dec2 / dec1 / dec3  (:1229-1240)
  const int lowIdx = k == 0 ? 0 : k == 1 ? 2 : k == 2 ? 3 : 1, highIdx = lowIdx ^ 2;
  struct TqRecRegs { long long dl, dh, start; uint2 ab; unsigned misc; uint4 sel; };
  auto loadRec = [&](int inside)
  {
    const TqRec* r = recTu + inside;
    TqRecRegs v;
    v.dl = r->dist[lowIdx]; v.dh = r->dist[highIdx]; v.start = r->start[k >> 1];
    v.ab = *reinterpret_cast<const uint2*>(r->ab); v.misc = r->misc;
    v.sel = make_uint4(r->selLoA, r->selHiA, r->selLoB, r->selHiB);
    return v;
  };
  auto abOf = [](uint2 ab, int t) { return (int)(((t < 2 ? ab.x : ab.y) >> ((t & 1) * 16)) & 0xFFFFu); };
  TqRecRegs R, Rn;
  int pfPos[2] = { 0, 0 }, pfAbs[2] = { 0, 0 };
  uint4 pfSel[2] = { make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0) }; unsigned pfMisc[2] = { 0, 0 };
  auto prefetch = [&](int beg)
  {
#pragma unroll
    for (int j = 0; j < 2; j++)
    {
      const int si = beg + k + 4 * j;
      pfPos[j] = scan[si]; const int c = coef[pfPos[j]]; pfAbs[j] = abs(c);
      pfSel[j] = posSel[si]; const uint2 m = posMisc[si]; pfMisc[j] = (luma ? m.x : m.y) | (c < 0 ? 0x80000000u : 0u);   // bit 31: the coefficient's sign
    }
  };
  Rn.dl = Rn.dh = Rn.start = 0; Rn.ab = make_uint2(0, 0); Rn.misc = 0; Rn.sel = make_uint4(0, 0, 0, 0);

  for (int scanIdx = maxFirst; scanIdx >= 0; scanIdx--)
  {
    const bool act = run && scanIdx <= first;                             // quad-uniform
    const int sIdx = scanIdx;                                             // inactive quads compute on valid indices and discard
    const int insidePos = sIdx & 15;
    const bool eosbb = insidePos == 0, sosbb = insidePos == 15;
    const bool socsbb = sosbb && sIdx > 16 && sIdx < N - 1;
    const bool eocsbb = eosbb && sIdx > 0 && sIdx < N - 16;
    const int spt = socsbb ? 1 : (eocsbb ? 2 : 0);
    const int nxt = max(sIdx - 1, 0);
    // a quad that is not active yet (scanIdx > first) computes along and its state is whatever that leaves: it starts from the
    // initial state at its first tested position (instead of guarding every state copy of every step)
    if (scanIdx == first)
    {
      tq_copy(P, P0); tq_copy(S, P0); ancCur = 0; ancLen = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) Fcur[i] = 0;
    }
    const int recPos = sIdx & (TQ_REC_N - 1);
    if (recPos == TQ_REC_N - 1 || scanIdx == maxFirst)                    // wave-uniform: the walk enters a group of positions
    {
      const int beg = sIdx & ~(TQ_REC_N - 1);
      static_assert(TQ_REC_N == 8, "two records per lane");
      if (scanIdx == maxFirst) prefetch(beg);
#pragma unroll
      for (int j = 0; j < 2; j++) fillRec(beg + k + 4 * j, pfPos[j], pfAbs[j], pfSel[j], pfMisc[j]);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      R = loadRec(recPos);
      // the coefficients of the NEXT group are the one stream of a TU that comes from HBM: requested here (with the shape part of its
      // records), used eight steps later
      prefetch(max(beg - TQ_REC_N, 0));
    }
    else R = Rn;
    if (recPos != 0) Rn = loadRec(recPos - 1);                            // the next step's record is in flight during this one

    const long long INF = 0x7FFFFFFFFFFFFFFFll;
    long long cLow, cHigh, cZero = INF;
    {
      // checkRdCostNonZero / checkRdCostZero by scan-position type (:1133-1177) as selects (the three-way branch diverges inside a wavefront):
      // the significance bits count unless the sub-block's coded flag is inferred (its end with nothing significant so far: no zero either),
      // the coded-flag bits at its start
      const bool zeroOk = !(spt == 2 && P.numSigSbb == 0);
      const int sb = spt == 1 ? P.sbb1 : 0;
      const int extra1 = (zeroOk ? P.sig1 : 0) + sb, extra0 = (zeroOk ? P.sig0 : 0) + sb;
      cLow = P.rdCost + R.dl + tq_level_bits(rt, P.gc, P.goRice, (unsigned)abOf(R.ab, lowIdx)) + extra1;
      cHigh = P.rdCost + R.dh + tq_level_bits(rt, P.gc, P.goRice, (unsigned)abOf(R.ab, highIdx)) + extra1;
      if (zeroOk) cZero = P.rdCost + extra0;
    }
    // decision k: sources a = 0 / 2, b = a + 1; k < 2 takes their "low" transitions, k >= 2 the "high" ones.  The source lanes are a fixed
    // pattern of the quad: lanes (0, 1, 2, 3) read a = (0, 2, 0, 2) and b = (1, 3, 1, 3)
    const int a = (k & 1) * 2, b = a + 1;
    const long long aLow = tq_quad64<0x88>(cLow), aHigh = tq_quad64<0x88>(cHigh), aZero = tq_quad64<0x88>(cZero);
    const long long bLow = tq_quad64<0xDD>(cLow), bHigh = tq_quad64<0xDD>(cHigh), bZero = tq_quad64<0xDD>(cZero);
    long long dCost = INF >> 2; int dAbs = -1, dPrev = -2;
    {
      // pq index of the transition a -> k and b -> k
      const int ia = k == 0 ? 0 : k == 2 ? 2 : k == 1 ? 3 : 1, ib = ia ^ 2;
      const int absA = abOf(R.ab, ia), absB = abOf(R.ab, ib);
      // comparison order (strict '<'): k < 2: a, a's zero, b; k >= 2: a, b, b's zero -- as selects, the two orders share one code path
      const bool lo = k < 2;
      const long long cA = lo ? aLow : aHigh, cB = lo ? bLow : bHigh;
      const long long c2 = lo ? aZero : cB, c3 = lo ? cB : bZero;
      const int abs2 = lo ? 0 : absB, prev2 = lo ? a : b, abs3 = lo ? absB : 0;
      if (cA < dCost) { dCost = cA; dAbs = absA; dPrev = a; }
      if (c2 < dCost) { dCost = c2; dAbs = abs2; dPrev = prev2; }
      if (c3 < dCost) { dCost = c3; dAbs = abs3; dPrev = b; }
      if (spt == 2) { const long long c = S.rdCost + S.sbb0; if (c < dCost) { dCost = c; dAbs = 0; dPrev = 4 + k; } }          // checkRdCostSkipSbb
      if ((k & 1) == 0 && R.start < dCost) { dCost = R.start; dAbs = abOf(R.ab, k); dPrev = -1; }                     // checkRdCostStart (decisions 0, 2)
    }
    // (with the coefficient's sign in bit 31: the back-trace then reads nothing but the decisions -- the coefficients of a picture do not stay in L2)
    if (act) dec[(size_t)sIdx * 4 + k] = ((unsigned)max(dAbs, 0) << 4) | (unsigned)(dPrev + 2) | (R.misc & 0x80000000u);
    if (scanIdx == 0) finalCost = dCost;

    // ---- state update (:1259-1318); every lane pulls its winner's context from the source lane
    TqState C; tq_copy(C, P);                                              // becomes the new previous state
    if (sIdx > 0)
    {
      const int sigOff = (int)((R.misc >> 20) & 15u), gtxOff = (int)((R.misc >> 24) & 31u);
      const int nextInside = nxt & 15;
      // source of the copied context: lane dPrev (0..3), own skip state (4 + k) or nothing
      const int srcLane = qbase + (dPrev >= 0 && dPrev < 4 ? dPrev : k);
      tq_u4 lv = { 0, 0, 0, 0 }, ax = { 0, 0, 0, 0 }; int sNum, sRef, sSbb0, sSbb1;
#pragma unroll
      for (int i = 0; i < 4; i++) lv[i] = (unsigned)__shfl((int)P.lev[i], srcLane);
      if (!eosbb)
#pragma unroll
        for (int i = 0; i < 4; i++) ax[i] = (unsigned)__shfl((int)P.aux[i], srcLane);
      sNum = __shfl(P.numSigSbb, srcLane); sRef = __shfl(P.refSbbCtxId, srcLane);
      sSbb0 = __shfl(P.sbb0, srcLane); sSbb1 = __shfl(P.sbb1, srcLane);
      if (dPrev >= 4) { sNum = S.numSigSbb; sRef = S.refSbbCtxId;
#pragma unroll
        for (int i = 0; i < 4; i++) lv[i] = S.lev[i]; }
      // sub-block flags of the inherited context slot: a register pull from the lane that owns the slot (slot id = lane in the quad);
      // done by the whole quad (the branch below diverges inside a quad)
      tq_u8 nf = { 0, 0, 0, 0, 0, 0, 0, 0 };
      unsigned long long nAnc = 0; int nLen = 0;
      if (eosbb)
      {
        const int pr = dPrev >= 0 ? sRef : -1;
#pragma unroll
        for (int i = 0; i < 8; i++) { const unsigned v = (unsigned)__shfl((int)Fcur[i], qbase + max(pr, 0)); nf[i] = pr >= 0 ? v : 0u; }
        const unsigned long long pa = (unsigned long long)tq_shfl64((long long)ancCur, qbase + max(pr, 0));
        const int pl = __shfl(ancLen, qbase + max(pr, 0));
        nAnc = pr >= 0 ? (pa << 2) | (unsigned long long)pr : 0ull; nLen = pr >= 0 ? min(pl + 1, 32) : 0;
      }
      C.rdCost = dCost;
      if (dPrev > -2)
      {
        int sumAbs, sumAbs1, sumNum;
        if (!eosbb)                                                        // State::updateState :1004-1068
        {
          if (dPrev >= 0) { C.numSigSbb = sNum + (dAbs != 0); C.refSbbCtxId = sRef; C.sbb0 = sSbb0; C.sbb1 = sSbb1;
#pragma unroll
            for (int i = 0; i < 4; i++) { C.lev[i] = lv[i]; C.aux[i] = ax[i]; } }
          else { C.numSigSbb = 1; C.refSbbCtxId = -1;
#pragma unroll
            for (int i = 0; i < 4; i++) { C.lev[i] = 0; C.aux[i] = 0; } }
          const unsigned lvNew = (unsigned)min(255, dAbs);
          tq_set_byte(C.lev, insidePos, lvNew);
          tq_set_byte(C.aux, insidePos, min(4u - (lvNew & 1u), lvNew) | (lvNew != 0u ? 32u : 0u));
          // the seeds of a sub-block belong to the context slot that was current when the walk entered it; every state that descends
          // from it reads the same sixteen values (slot 4 = zeros: a path that started inside the sub-block)
          const unsigned tinit = reinterpret_cast<const unsigned short*>(seedTu)[(C.refSbbCtxId < 0 ? 4 : C.refSbbCtxId) * 16 + nextInside];
          sumAbs = (int)(tinit >> 8); sumAbs1 = (int)((tinit >> 3) & 31); sumNum = (int)(tinit & 7);
          // the five template neighbours inside the sub-block: four byte permutes pick them out of the sixteen levels (and out of their
          // sumAbs1 / sumNum contributions), v_sad_u8 against zero adds the picked bytes up
          {
            const unsigned nA = __builtin_amdgcn_perm(C.lev[1], C.lev[0], R.sel.x) | __builtin_amdgcn_perm(C.lev[3], C.lev[2], R.sel.y);
            const unsigned nB = __builtin_amdgcn_perm(C.lev[1], C.lev[0], R.sel.z) | __builtin_amdgcn_perm(C.lev[3], C.lev[2], R.sel.w);
            const unsigned xA = __builtin_amdgcn_perm(C.aux[1], C.aux[0], R.sel.x) | __builtin_amdgcn_perm(C.aux[3], C.aux[2], R.sel.y);
            const unsigned xB = __builtin_amdgcn_perm(C.aux[1], C.aux[0], R.sel.z) | __builtin_amdgcn_perm(C.aux[3], C.aux[2], R.sel.w);
            sumAbs = (int)__builtin_amdgcn_sad_u8(nB, 0u, __builtin_amdgcn_sad_u8(nA, 0u, (unsigned)sumAbs));
            const unsigned sx = __builtin_amdgcn_sad_u8(xB, 0u, __builtin_amdgcn_sad_u8(xA, 0u, 0u));
            sumAbs1 += (int)(sx & 31u); sumNum += (int)(sx >> 5);
          }
        }
        else                                                               // State::updateStateEOS :1071-1102 + CommonCtx::update :1104-1164
        {
          if (dPrev >= 0) { C.numSigSbb = sNum + (dAbs != 0);
#pragma unroll
            for (int i = 0; i < 4; i++) C.lev[i] = lv[i]; }
          else { C.numSigSbb = 1;
#pragma unroll
            for (int i = 0; i < 4; i++) C.lev[i] = 0; }
          tq_set_byte(C.lev, insidePos, (unsigned)min(255, dAbs));
          const int sbbId = sIdx >> 4;
          if (act) *reinterpret_cast<uint4*>(ctxMem + (size_t)(sbbId * 4 + k) * 16) = make_uint4(C.lev[0], C.lev[1], C.lev[2], C.lev[3]);
          const int pos = scan[sIdx], px = pos & (w - 1), py = pos >> lw, nxtPos = scan[nxt], nx = nxtPos & (w - 1), ny = nxtPos >> lw;
          {
            const int sbbPos = (py >> 2) * widthInSbb + (px >> 2);
#pragma unroll
            for (int i = 0; i < 8; i++) { const unsigned m = i == (sbbPos >> 5) ? 1u << (sbbPos & 31) : 0u; nf[i] = (nf[i] & ~m) | (C.numSigSbb != 0 ? m : 0u); }
          }
          const int nsx = nx >> 2, nsy = ny >> 2, nsp = nsy * widthInSbb + nsx;
          const int right = nsx < widthInSbb - 1 ? nsp + 1 : 0, below = nsy < heightInSbb - 1 ? nsp + widthInSbb : 0;
          unsigned fr = nf[0], fb = nf[0];
#pragma unroll
          for (int i = 1; i < 8; i++) { fr = (right >> 5) == i ? nf[i] : fr; fb = (below >> 5) == i ? nf[i] : fb; }
          const int sigNSbb = ((right && ((fr >> (right & 31)) & 1u)) || (below && ((fb >> (below & 31)) & 1u))) ? 1 : 0;
#pragma unroll
          for (int i = 0; i < 8; i++) Fcur[i] = nf[i];
          ancCur = nAnc; ancLen = nLen;
          C.numSigSbb = 0; C.refSbbCtxId = k;
          C.sbb0 = rt->sig_sbb[sigNSbb][0]; C.sbb1 = rt->sig_sbb[sigNSbb][1];
          // template seeds of the sixteen positions of the next sub-block from the levels outside it (:1131-1160).  Every template
          // neighbour outside a 4x4 sub-block lies in the sub-block to its right, below it or below-right of it, whose sixteen levels
          // are sixteen consecutive bytes of the history (scan order): three 16-byte loads and compile-time byte picks replace eighty
          // dependent byte loads behind eighty table look-ups (13.6 us per sub-block end, a fifth of the kernel).
          tq_u8 cti = { 0, 0, 0, 0, 0, 0, 0, 0 };
          if (act)
          {
            const int bx = nsx * 4, by = nsy * 4;
            const bool hasR = nsx + 1 < widthInSbb, hasB = nsy + 1 < heightInSbb;
            // read from the blocks of this state's ancestors (the sub-block that just ended: its levels are still in C.lev)
            const uint4 own = make_uint4(C.lev[0], C.lev[1], C.lev[2], C.lev[3]), zero4 = make_uint4(0, 0, 0, 0);
            // (loads from addresses that are always valid, the choice made on the VALUES: a choice between a loaded value and `own` / zero
            // becomes a load through a selected address, i.e. `own` goes to scratch memory and the three loads wait for each other)
            auto sbbLevels = [&](bool exists, int rasterPos)
            {
              const int j = inv[exists ? rasterPos : 0] >> 4, back = j - sbbId - 1;      // back = 0: the parent's sub-block
              const unsigned slot = (unsigned)(nAnc >> (2 * min(max(back, 0), 31))) & 3u;
              const uint4 hv = *reinterpret_cast<const uint4*>(ctxMem + (size_t)(j * 4 + (int)slot) * 16);
              const bool fromHist = exists && back >= 0 && back < nLen, fromOwn = exists && j == sbbId;
              uint4 r;
              r.x = fromHist ? hv.x : fromOwn ? own.x : 0u; r.y = fromHist ? hv.y : fromOwn ? own.y : 0u;
              r.z = fromHist ? hv.z : fromOwn ? own.z : 0u; r.w = fromHist ? hv.w : fromOwn ? own.w : 0u;
              return r;
            };
            const uint4 LR = sbbLevels(hasR, by * w + bx + 4), LB = sbbLevels(hasB, (by + 4) * w + bx), LD = sbbLevels(hasR && hasB, (by + 4) * w + bx + 4);
            auto pick = [](const uint4& v, int j) { const unsigned q = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w; return (q >> ((j & 3) * 8)) & 0xFFu; };
            // contribution of one neighbour level to (sumNum | sumAbs1 << 3 | sumAbs << 8): at most five are added, the fields do not carry
            auto cv = [](unsigned v) { return (v != 0u ? 1u : 0u) + (min(4u - (v & 1u), v) << 3) + (v << 8); };
            unsigned cR[4][2], cB[2][4];
#pragma unroll
            for (int y = 0; y < 4; y++)
#pragma unroll
              for (int x = 0; x < 2; x++) cR[y][x] = cv(pick(LR, (int)((TQ_KOFPOS >> (4 * (y * 4 + x))) & 15)));
#pragma unroll
            for (int y = 0; y < 2; y++)
#pragma unroll
              for (int x = 0; x < 4; x++) cB[y][x] = cv(pick(LB, (int)((TQ_KOFPOS >> (4 * (y * 4 + x))) & 15)));
            const unsigned cD = cv(pick(LD, (int)(TQ_KOFPOS & 15)));
#pragma unroll
            for (int i = 0; i < 16; i++)
            {
              const int pi = (int)((TQ_POSOFK >> (4 * i)) & 15), x = pi & 3, y = pi >> 2;
              const int dx[5] = { 1, 2, 1, 0, 0 }, dy[5] = { 0, 0, 1, 1, 2 };
              unsigned sum = 0;
#pragma unroll
              for (int t = 0; t < 5; t++)
              {
                const int X = x + dx[t], Y = y + dy[t];
                if (X > 3 && Y > 3) sum += cD; else if (X > 3) sum += cR[Y][X - 4]; else if (Y > 3) sum += cB[Y - 4][X];
              }
              const unsigned seed = (sum & 0xFFu) | (min(127u, sum >> 8) << 8);
              cti[i >> 1] |= seed << ((i & 1) * 16);
            }
            *reinterpret_cast<uint4*>(seedTu + k * 8) = make_uint4(cti[0], cti[1], cti[2], cti[3]);
            *reinterpret_cast<uint4*>(seedTu + k * 8 + 4) = make_uint4(cti[4], cti[5], cti[6], cti[7]);
          }
#pragma unroll
          for (int i = 0; i < 4; i++) { C.lev[i] = 0; C.aux[i] = 0; }
          const unsigned tinit = tq_get_u16(cti, nextInside);
          sumNum = (int)(tinit & 7); sumAbs1 = (int)((tinit >> 3) & 31); sumAbs = (int)(tinit >> 8);
        }
        const int sumGt1 = sumAbs1 - sumNum;
        sumAbs -= sumNum;
        const int sc = sigOff + min(sumAbs1, 5), gc = gtxOff + min(sumGt1, 4);
        C.sig0 = rt->sig[sigSet][sc][0]; C.sig1 = rt->sig[sigSet][sc][1];
        C.gc = gc;
        const int ga = min(sumAbs, 31);
        C.goRice = ga < 12 ? 0 : ga < 25 ? 1 : 2;                          // g_auiGoRicePars
      }
      if (eosbb) { __threadfence_block(); }
    }
    if (socsbb) tq_copy(S, P);                                             // swap( m_prevStates, m_skipStates ) :1314-1317
    tq_copy(P, C);
  }

  // ---- best final state and back-trace :1368-1390.  Decisions 4..7 are implicit: at a sub-block end they are a copy of decisions
  // 0..3 (:1269), elsewhere { level 0, same skip id } (startDec :1218).  The chain through the decisions is serial, the loads are not: the
  // quad takes eight scan positions a round, lane j loads the four decisions of positions base + j and base + 4 + j (16 bytes each, the coefficient's sign in bit 31) and
  // their raster positions -- one round ahead --, the chain then runs over quad broadcasts in registers (every lane alike) and lane j writes the
  // level of its position.  (With lane 0 alone every position was a dependent load from memory: ~0.5 ms of a 64x64 TU's 3.1 ms.)
  long long c1 = tq_shfl64(finalCost, qbase + 1), c2 = tq_shfl64(finalCost, qbase + 2), c3 = tq_shfl64(finalCost, qbase + 3);
  const long long c0 = tq_shfl64(finalCost, qbase);
  if (!run) return;
  int prevId = -2; long long minCost = 0;
  if (c0 < minCost) { prevId = 0; minCost = c0; }
  if (c1 < minCost) { prevId = 1; minCost = c1; }
  if (c2 < minCost) { prevId = 2; minCost = c2; }
  if (c3 < minCost) { prevId = 3; minCost = c3; }
  unsigned absSum = 0;
  __threadfence_block();                                                   // the decisions were stored by the four lanes
  const uint4* dec4 = reinterpret_cast<const uint4*>(dec);
  // (eight positions a round, two per lane: the chain over eight positions takes about as long as the loads of the next eight)
  uint4 dv[2]; int pos[2];
#pragma unroll
  for (int u = 0; u < 2; u++) { const int i = min(4 * u + k, N - 1); dv[u] = dec4[i]; pos[u] = scan[i]; }
  for (int base = 0; prevId >= 0; base += 8)
  {
    uint4 dn[2]; int posn[2];
#pragma unroll
    for (int u = 0; u < 2; u++) { const int i = min(base + 8 + 4 * u + k, N - 1); dn[u] = dec4[i]; posn[u] = scan[i]; }
#pragma unroll
    for (int u = 0; u < 2; u++)
    {
      int myAl = 0; bool mine = false, myNeg = false;
      // a link of the chain: every lane picks the decision of the current state out of ITS position's four (two selects on the bits of
      // the state: nested conditionals became branches), lane j's pick is the one that counts
      auto pick = [&]()
      {
        const bool b0 = (prevId & 1) != 0, b1 = (prevId & 2) != 0;
        const unsigned lo = b0 ? dv[u].y : dv[u].x, hi = b0 ? dv[u].w : dv[u].z;
        return b1 ? hi : lo;
      };
      auto link = [&](int j, unsigned v)
      {
        const bool on = prevId >= 0, keep = prevId >= 4 && ((base + 4 * u + j) & 15) != 0;
        const int al = keep ? 0 : (int)((v >> 4) & 0x7FFFFFFu), nextPrev = keep ? prevId : (int)(v & 15) - 2;
        if (on && j == k) { myAl = al; mine = true; myNeg = (v >> 31) != 0u; }
        absSum += on ? (unsigned)al : 0u; prevId = on ? nextPrev : prevId;
      };
      link(0, tq_quad32<0x00>(pick()));                                    // quad_perm [j, j, j, j]: lane j of the quad to all four
      link(1, tq_quad32<0x55>(pick()));
      link(2, tq_quad32<0xAA>(pick()));
      link(3, tq_quad32<0xFF>(pick()));
      if (mine) level[pos[u]] = myNeg ? -myAl : myAl;
    }
#pragma unroll
    for (int u = 0; u < 2; u++) { dv[u] = dn[u]; pos[u] = posn[u]; }
  }
  if (k != 0) return;
  absSumOut[ti] = absSum;
  };

  bool done = !(live && first >= 0);
  for (;;)
  {
    if (threadIdx.x < TQ_RT_SLOTS) rtSlot[threadIdx.x] = -1;
    if (threadIdx.x == 0) rtPending = 0;
    __syncthreads();
    int mySlot = -1;
    if (!done && k == 0)
    {
      for (int t = 0; t < TQ_RT_SLOTS && mySlot < 0; t++)
      {
        const int sl = (d.rates_idx + t) & (TQ_RT_SLOTS - 1);
        const int old = atomicCAS(&rtSlot[sl], -1, d.rates_idx);
        if (old == -1 || old == d.rates_idx) mySlot = sl;
      }
      if (mySlot < 0) rtPending = 1;
    }
    mySlot = __shfl(mySlot, qbase);
    __syncthreads();
    const bool more = rtPending != 0;
    for (int sl = 0; sl < TQ_RT_SLOTS; sl++)
      if (rtSlot[sl] >= 0)
      {
        const int* src = reinterpret_cast<const int*>(ratesBase + rtSlot[sl]);
        int* dst = reinterpret_cast<int*>(&rtCache[sl]);
        for (int i = threadIdx.x; i < (int)(sizeof(vvcgpu_dq_rates) / 4); i += 256) dst[i] = src[i];
      }
    __syncthreads();
    const bool run = !done && mySlot >= 0;
    walk(run, (TqLdsRates)&rtCache[max(mySlot, 0)]);
    done = done || run;
    if (!more) break;
    __syncthreads();
  }
