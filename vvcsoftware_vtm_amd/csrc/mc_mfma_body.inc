// mc_mfma_body.inc -- the body of the matrix-core MC kernels (interp.hip), included by both: mc_mfma_kernel<KIND_T> and mc_mfma_wp_kernel
// (vvcgpu_mc_wp_batch).  The including kernel defines KIND_T, WPF (the weighted epilogue), serve, diag, genCount, wp, nWp and allGen.  A body
// function called from the two kernels would change the code of mc_mfma_kernel<KIND_T> (the inlined call reorders it); this way the kernel is
// compiled from the same statements as before, with every WPF branch discarded.
  if (blockIdx.x == 0 && threadIdx.x < VVC_CTR_INTS) nextCounters[threadIdx.x] = 0;       // the counter set of the NEXT call on this stream (vvcgpu_counters)
  // KIND_T 0: ONE launch, workgroups alternate between the two shapes (both kinds of waves on every CU at the same time)
  const int KIND = KIND_T ? KIND_T : 1 + ((int)blockIdx.x & 1);
  const int T0 = KIND == 1 ? MM_TAL : MM_TAC, T1 = KIND == 1 ? MM_TAC : MM_ENTRIES;          // this kind's table entries
  __shared__ __align__(16) _Float16 tabL[(KIND_T == 2 ? MM_ENTRIES - MM_TAC : MM_TAC - MM_TAL) * 8];
  __shared__ __align__(16) short genS[4][MM_GEN_SHORTS];                     // the generic body's window / intermediate, per wave
  __shared__ __align__(16) unsigned genT[4][MC_LDS_DW];                      // ... and its packed-form tile
  __shared__ typename std::conditional<WPF, MmServeWp, MmServe>::type serveS;
  __shared__ int anyGenS[4];                                 // serve: per wave, what its walk left to the generic body (the count lands here instead of in genCount)
  for (int i = threadIdx.x; i < T1 - T0; i += 256) reinterpret_cast<uint4*>(tabL)[i] = reinterpret_cast<const uint4*>(image)[T0 + i];
  if (threadIdx.x < 4) anyGenS[threadIdx.x] = 0;
  MmK K;                                                     // (the barrier behind the table copy follows the lane constants and the serve record)
  K.genCount = serve ? &anyGenS[threadIdx.x >> 6] : genCount;
  K.tabS = tabL - T0 * 8;                                    // (indexed with the image's entry numbers)
  K.lane = threadIdx.x & 63; K.c16 = K.lane & 15; K.g = K.lane >> 4;
  const int g = K.g;
  const int hr = max(2, IF_INTERNAL_PREC - bd), S = 1 << (IF_FILTER_PREC - hr);
  K.hr = hr;
  if constexpr (WPF) { K.cmin = cmin; K.cmax = cmax; }
  K.rangeMask = (unsigned)((1 << bd) - 1) * 0x10001u;
  K.uLo = (unsigned)(16384 + cmin) * 0x10001u; K.uHi = (unsigned)(16384 + cmax) * 0x10001u;
  // limb masks / exponent patterns of a pass-1 result by row-chunk kind: 0 every row real; 1 luma rows 16..31 (lane group 2: the constants 1.0, 1024.0;
  // 3: nothing); 2 chroma rows 0..15 (lane group 3: the constants)
  K.m7[0] = 0x007F007Fu; K.m8[0] = 0x00FF00FFu; K.orX[0] = 0x64006400u;
  asm("" : "+v"(K.m7[0]), "+v"(K.m8[0]), "+v"(K.orX[0]));   // held in vector registers (v_and_or_b32 takes no literal)
  K.orR[0] = K.orX[0];
  K.m7[1] = g < 2 ? 0x007F007Fu : 0u; K.m8[1] = g < 2 ? 0x00FF00FFu : 0u; K.orX[1] = g < 2 ? 0x64006400u : g == 2 ? 0x64003C00u : 0u; K.orR[1] = g < 2 ? 0x64006400u : 0u;
  K.m7[2] = g < 3 ? 0x007F007Fu : 0u; K.m8[2] = g < 3 ? 0x00FF00FFu : 0u; K.orX[2] = g < 3 ? 0x64006400u : 0x64003C00u; K.orR[2] = g < 3 ? 0x64006400u : 0u;
  K.magicN = 8388608.f * (float)S; K.magicH = 536870912.f;
  K.cinN = 8192.f * (float)S - 65536.f - 0.5f * (float)(S - 1); K.cinH = 983040.5f;     // start values of a luma pass-1 sum (the chroma tables carry theirs)
  K.perm = (4 * K.c16 + K.g) * 4;
  K.pmin = mm_h2{ (_Float16)(short)(1024 + cmin), (_Float16)(short)(1024 + cmin) }; K.pmax = mm_h2{ (_Float16)(short)(1024 + cmax), (_Float16)(short)(1024 + cmax) };
  K.pmin0 = mm_h2{ (_Float16)1024.f, (_Float16)1024.f }; K.pmaxF = mm_h2{ (_Float16)(short)(1023 + (1 << bd)), (_Float16)(short)(1023 + (1 << bd)) };
  // second-stage rounding as fma + floor (exact: f32 integers below 2^24 times powers of two)
  K.scBi1 = 1.f / 64.f; K.scUni1 = 1.f / (float)(64 << hr); K.ofUni1 = (float)((1 << (5 + hr)) + (IF_INTERNAL_OFFS << 6)) * K.scUni1;
  K.scBi2 = 1.f / (float)(2 << hr); K.ofBi2 = (float)((1 << hr) + 2 * IF_INTERNAL_OFFS) * K.scBi2 + 1024.f;

  const int nb = KIND_T ? (int)gridDim.x : (KIND == 1 ? ((int)gridDim.x + 1) >> 1 : (int)gridDim.x >> 1), bi_ = KIND_T ? (int)blockIdx.x : (int)blockIdx.x >> 1;
  // XCD-aware walk (workgroups are dealt round-robin over the 8 XCDs, each with its own L2): at every step the waves of ONE XCD hold one contiguous
  // run of W / 8 descriptors, so the window lines that neighbouring PUs share are fetched from the fabric by one L2 (speed only)
  const int W = nb * 4, perX = W >> 3;
  const int w = (nb & 7) ? bi_ * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6)
                         : (bi_ & 7) * perX + (bi_ >> 3) * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (serve && threadIdx.x == 0) static_cast<MmServe&>(serveS) = MmServe{ ref0Base, ref1Base, dstBase, descs, flags, n, bd, cmin, cmax, w, W, KIND == 1 ? 1 : 0 };     // (w of wave 0; read behind the walks)
  if constexpr (WPF) { if (threadIdx.x == 0) { MmServeWp& sw = reinterpret_cast<MmServeWp&>(serveS); sw.wp = wp; sw.nWp = nWp; sw.allGen = allGen; } }
  __syncthreads();
  // The wave's descriptors w + j W are classified 64 at a time, one per LANE (one gather load and a ballot; a descriptor-by-descriptor walk on the scalar
  // unit -- one per CU, shared by its 20 waves -- bound the kernel: 400 scalar instructions per PU); the walk over the set bits is a few scalar operations.
  // Three steps are in flight (in-kernel stamps, VVCGPU_MC_DIAG: with the descriptor read inside the step that requests the samples, 1400 of a step's
  // 5500 cycles were that read's latency): the descriptor of step k + 2 is being read, the samples of step k + 1 are requested, step k is computed.
  MmRaw raw;
  bool pend = false;
  if (KIND == 1)
  {
    vvcgpu_mc_desc dP = descs[0];
    vvcgpu_wp_param eP;                                      // WPF: dP's table entry (scalars)
    int iP = 0, dstep = 0;
    for (int j0 = 0; w + (long long)j0 * W < n; j0 += 64)
    {
      const long long iL = w + (long long)(j0 + K.lane) * W;
      int k = 0;
      if (iL < n)
      {
        const uint4 q1 = reinterpret_cast<const uint4*>(descs + iL)[1], q2 = reinterpret_cast<const uint4*>(descs + iL)[2];
        k = mm_kind_of(q2);
        const int bi = (int)(signed char)((q2.w >> 8) & 0xFFu);
        if (k == 1 && ((q1.z | (bi == 1 ? q1.w : 0u)) & 7u)) k = -1;           // aligned 16-byte words need rows that keep their alignment (ref strides: bytes 24..31)
        if constexpr (WPF) k = mm_wp_kind(k, q2, wp, nWp, bd, allGen);
        if (k < 0) flags[iL] = 1;                            // a fast SHAPE these kernels do not take: the generic kernel's
      }
      {
        const unsigned long long gm = __ballot(iL < n && k <= 0);             // every other shape, and the fast shapes left above: the generic kernel's work
        if (gm != 0ull && K.lane == 0) atomicAdd(K.genCount, (int)__popcll(gm));
      }
      unsigned long long mine = __ballot(k == 1);
      auto nextIdx = [&]() -> int { if (mine == 0ull) return -1; const int j = (int)__builtin_ctzll(mine); mine &= mine - 1ull; return w + (j0 + j) * W; };
      // A step's descriptor is wave-uniform, but it is read with VECTOR loads (every lane the same address) a step ahead and moved to scalar registers
      // when its step begins: scalar loads return out of order, so with one in flight every LDS wait of the step (operand permutes, table reads) is an
      // lgkmcnt(0) that also waits for the descriptor -- ~2000 of a step's 5000 cycles (VVCGPU_MC_DIAG stamps).
      auto descLoad = [&](int i, uint4 (&v)[3]) { const uint4* q = reinterpret_cast<const uint4*>(descs + i); v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; };
      auto descScalar = [&](const uint4 (&v)[3]) -> vvcgpu_mc_desc
      {
        unsigned u[12] = { v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w, v[2].x, v[2].y, v[2].z, v[2].w };
#pragma unroll
        for (int t = 0; t < 12; t++) u[t] = (unsigned)__builtin_amdgcn_readfirstlane((int)u[t]);
        vvcgpu_mc_desc d;
        d.ref0_off = (long long)(((unsigned long long)u[1] << 32) | u[0]); d.ref1_off = (long long)(((unsigned long long)u[3] << 32) | u[2]);
        d.dst_off = (long long)(((unsigned long long)u[5] << 32) | u[4]);
        d.ref0_stride = (int)u[6]; d.ref1_stride = (int)u[7]; d.dst_stride = (int)u[8];
        d.w = (short)(u[9] & 0xFFFFu); d.h = (short)(u[9] >> 16);
        d.frac_x0 = (signed char)(u[10] & 0xFFu); d.frac_y0 = (signed char)((u[10] >> 8) & 0xFFu); d.frac_x1 = (signed char)((u[10] >> 16) & 0xFFu); d.frac_y1 = (signed char)(u[10] >> 24);
        d.is_luma = (signed char)(u[11] & 0xFFu); d.bi = (signed char)((u[11] >> 8) & 0xFFu); d.reserved = WPF ? (short)(u[11] >> 16) : 0;
        return d;
      };
      int iA = nextIdx();
      if (iA < 0) continue;
      uint4 dv[3];
      descLoad(iA, dv);
      while (iA >= 0)
      {
        const vvcgpu_mc_desc dA = descScalar(dv);
        vvcgpu_wp_param eA;
        if constexpr (WPF) eA = wp_load(wp, dA.reserved);  // (requested with the step's samples, used a step later)
        const int iB = nextIdx();
        descLoad(iB >= 0 ? iB : iA, dv);                     // the next step's descriptor: a whole step ahead
        if (pend)
        {
          // VVCGPU_MC_DIAG (measurement aid): core-clock stamps of one wave's steps: step start, samples arrived + operands, next samples requested, done
          const bool st = diag && bi_ == (nb >> 1) && (threadIdx.x >> 6) == 0 && dstep < 12;
          if (st && K.lane == 0) diag[dstep * 4 + 0] = __builtin_amdgcn_s_memtime();
          MmWin Wn;
          mm_luma_win(K, raw, Wn);                           // the previous PU's samples have arrived: operands; the loaded registers are free
          if (st && K.lane == 0) { asm volatile("" :: "v"(Wn.w[0][0]), "v"(Wn.w[1][1])); diag[dstep * 4 + 1] = __builtin_amdgcn_s_memtime(); }
          mm_fetch_luma(K, dA, ref0Base, ref1Base, raw);     // this PU's samples travel behind the previous PU's products
          if (st && K.lane == 0) diag[dstep * 4 + 2] = __builtin_amdgcn_s_memtime();
          mm_luma<WPF>(K, dP, Wn, ref0Base, ref1Base, dstBase, flags, iP, &eP);
          if (st && K.lane == 0) diag[dstep * 4 + 3] = __builtin_amdgcn_s_memtime();
          dstep++;
        }
        else mm_fetch_luma(K, dA, ref0Base, ref1Base, raw);
        dP = dA; iP = iA; pend = true;
        if constexpr (WPF) eP = eA;
        iA = iB;
      }
    }
    if (pend) { MmWin Wn; mm_luma_win(K, raw, Wn); mm_luma<WPF>(K, dP, Wn, ref0Base, ref1Base, dstBase, flags, iP, &eP); }
    if (serve && anyGenS[(int)threadIdx.x >> 6] != 0) mm_second_pass<WPF>(&serveS, genS[(int)threadIdx.x >> 6], genT[(int)threadIdx.x >> 6]);
  }
  else
  {
    const int units = (n + 1) >> 1;
    int iAP = -1, iBP = -1;
    for (int j0 = 0; w + (long long)j0 * W < units; j0 += 64)
    {
      const long long uL = w + (long long)(j0 + K.lane) * W;
      int iAv = -1, iBv = -1;
      if (uL < units)
      {
        const uint4* q0 = reinterpret_cast<const uint4*>(descs + 2 * uL) + 2;
        const int k0 = WPF ? mm_wp_kind(mm_kind_of(*q0), *q0, wp, nWp, bd, allGen) : mm_kind_of(reinterpret_cast<const uint4*>(descs + 2 * uL)[2]);
        const int k1 = 2 * uL + 1 < n ? (WPF ? mm_wp_kind(mm_kind_of(q0[3]), q0[3], wp, nWp, bd, allGen) : mm_kind_of(reinterpret_cast<const uint4*>(descs + 2 * uL + 1)[2])) : 0;
        iAv = k0 == 2 ? (int)(2 * uL) : k1 == 2 ? (int)(2 * uL + 1) : -1;
        iBv = (k0 == 2 && k1 == 2) ? (int)(2 * uL + 1) : -1;
      }
      unsigned long long mine = __ballot(iAv >= 0);
      auto nextJ = [&]() -> int { if (mine == 0ull) return -1; const int j = (int)__builtin_ctzll(mine); mine &= mine - 1ull; return j; };
      int jA = nextJ();
      if (jA < 0) continue;
      int iA = __builtin_amdgcn_readlane(iAv, jA), iB = __builtin_amdgcn_readlane(iBv, jA);
      MmCDesc cA;
      mm_chroma_desc(K, descs, iA, iB, cA);
      while (jA >= 0)
      {
        const int jN = nextJ();
        const int iAN = __builtin_amdgcn_readlane(iAv, jN >= 0 ? jN : jA), iBN = __builtin_amdgcn_readlane(iBv, jN >= 0 ? jN : jA);
        MmCDesc cN;
        mm_chroma_desc(K, descs, iAN, iBN, cN);              // the descriptor fields of the step after this one (vector loads, consumed next iteration)
        if (pend)
        {
          MmWin Wn;
          mm_chroma_win(K, raw, Wn);
          mm_fetch_chroma(K, cA, ref0Base, ref1Base, raw);
          mm_chroma<WPF>(K, Wn, iAP, iBP, dstBase, flags, wp);
        }
        else mm_fetch_chroma(K, cA, ref0Base, ref1Base, raw);
        iAP = iA; iBP = iB; pend = true;
        jA = jN; iA = iAN; iB = iBN; cA = cN;
      }
    }
    if (pend) { MmWin Wn; mm_chroma_win(K, raw, Wn); mm_chroma<WPF>(K, Wn, iAP, iBP, dstBase, flags, wp); }
    if (serve && anyGenS[(int)threadIdx.x >> 6] != 0) mm_second_pass<WPF>(&serveS, genS[(int)threadIdx.x >> 6], genT[(int)threadIdx.x >> 6]);
  }
