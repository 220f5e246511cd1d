// alf_quad_sums.inc -- first piece of the ALF block classifier (AdaptiveLoopFilter::deriveClassificationBlk, CommonLib/AdaptiveLoopFilter.cpp:292-463),
// stated once as text and included where it runs: alf_classify_kernel (alf.hip) and alf_ctu_luma<C, true> (alfstats.hip).  Text, not a function: a
// forced-inline function is simplified on its own before it is inlined, and alf_stats_picture_kernel<*, true> then loses the parent's instruction
// stream (docs/MEASUREMENTS.md).
//   expects  const unsigned* base   the LDS tile at the quad's row 0, column 0 (8-byte aligned); the quad's pixels are rows 1 .. 4, columns 2 .. 5
//            quadPitch              the tile's row pitch in samples (a constant, a multiple of 4)
//   declares unsigned sv, sh, sd0, sd1   the quad's sums of the vertical, horizontal and the two diagonal Laplacians
// Two samples per instruction: a row of the 6x6 neighbourhood (columns 1 .. 6) is four aligned dwords, its five sample pairs
// P0..P4 = (s0,s1) .. (s4,s5) are two of the dwords and three v_alignbit; |2c - a - b| of a pair of samples is ONE v_sad_u16 of the
// doubled centre pair against the packed sum of the two neighbour pairs (samples are non-negative, <= 15 bits: nothing wraps), which also
// accumulates.  18 instructions per row of four samples instead of 64.
unsigned sv = 0, sh = 0, sd0 = 0, sd1 = 0;
{
  unsigned rowA[5], rowB[5], rowC[5];                        // pairs of the rows above / at / below the centre row
  auto loadRow = [&](int r, unsigned (&P)[5])
  {
    const uint2 lo = *reinterpret_cast<const uint2*>(base + r * (quadPitch / 2)), hi = *reinterpret_cast<const uint2*>(base + r * (quadPitch / 2) + 2);
    P[0] = __builtin_amdgcn_alignbit(lo.y, lo.x, 16); P[1] = lo.y; P[2] = __builtin_amdgcn_alignbit(hi.x, lo.y, 16); P[3] = hi.x;
    P[4] = __builtin_amdgcn_alignbit(hi.y, hi.x, 16);
  };
  typedef unsigned short us2v __attribute__((ext_vector_type(2)));
  auto padd = [](unsigned a, unsigned b) { return __builtin_bit_cast(unsigned, __builtin_bit_cast(us2v, a) + __builtin_bit_cast(us2v, b)); };
  loadRow(0, rowA); loadRow(1, rowB);
#pragma unroll
  for (int y = 0; y < 4; y++)
  {
    loadRow(y + 2, rowC);
    // centre row = rowB: centres (s1,s2) = rowB[1], (s3,s4) = rowB[3]
    const unsigned c01 = padd(rowB[1], rowB[1]), c23 = padd(rowB[3], rowB[3]);
    sv  = __builtin_amdgcn_sad_u16(c01, padd(rowA[1], rowC[1]), sv);   sv  = __builtin_amdgcn_sad_u16(c23, padd(rowA[3], rowC[3]), sv);
    sh  = __builtin_amdgcn_sad_u16(c01, padd(rowB[0], rowB[2]), sh);   sh  = __builtin_amdgcn_sad_u16(c23, padd(rowB[2], rowB[4]), sh);
    sd0 = __builtin_amdgcn_sad_u16(c01, padd(rowA[0], rowC[2]), sd0);  sd0 = __builtin_amdgcn_sad_u16(c23, padd(rowA[2], rowC[4]), sd0);
    sd1 = __builtin_amdgcn_sad_u16(c01, padd(rowC[0], rowA[2]), sd1);  sd1 = __builtin_amdgcn_sad_u16(c23, padd(rowC[2], rowA[4]), sd1);
#pragma unroll
    for (int k = 0; k < 5; k++) { rowA[k] = rowB[k]; rowB[k] = rowC[k]; }
  }
}
