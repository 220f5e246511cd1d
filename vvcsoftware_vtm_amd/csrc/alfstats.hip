// alfstats.hip -- encoder-side ALF covariances (A3) for gfx950.
//
// Reference behaviour reproduced (bit-exact integers):
//   EncAdaptiveLoopFilter::deriveStatsForFiltering/getBlkStats/calcCovariance  EncoderLib/EncAdaptiveLoopFilter.cpp:1317-1515
// The reference accumulates the ALF products into doubles; every partial sum is an integer < 2^53, so the
// int64 sums produced here convert to exactly the same doubles in any summation order.
#include "common.h"
#include "alf_dev.h"

namespace {

// record layout of the C ABI (alfdecide.hip and ops.py keep their own checks): per CTU and class N x N entries of E, N of y and pixAcc
constexpr int ALF_CLASSES = 25;
constexpr int ALF_REC7 = 13 * 13 + 13 + 1;        // 7x7 diamond, N = 13: 183 entries
constexpr int ALF_REC5 = 7 * 7 + 7 + 1;           // 5x5 diamond, N = 7: 57 entries
// below this many CTUs the fused form (vvcgpu_alf_classify_stats_picture) gives the classifier its own launch (measurements at the call)
constexpr int ALF_CLS_OWN_LAUNCH_CTUS = 320;

// =====================================================================================================
// A3: ALF covariance.  One workgroup per 64x64 tile (256 blocks of 4x4, one per thread): the rec tile with a
// 3-sample halo is staged in LDS (border replicated), each thread builds the 13 (7) symmetric tap sums of its
// 16 pixels in the canonical (transposeIdx 0) order and accumulates the upper triangle of E, y and pixAcc in
// registers with 24-bit integer MADs; the per-class buckets live in LDS (64-bit atomics, indices permuted by
// the block's transposeIdx) and are flushed to the per-CTU output with 64-bit global atomics.
// =====================================================================================================
constexpr int AT = 64, AP = AT + 8, AR = AT + 6;
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef short short2v __attribute__((ext_vector_type(2)));

// covariance sums of one 4x4 block in the canonical (transposeIdx 0) tap order: blk = LDS tile at (row by - 3, column bx - 4) of a tile
// with row pitch PITCH samples, orgBlk = the original at (by, bx).  A = upper triangle of E (row-major), Y = cross terms, pix = sum d^2.
template <bool IS7, int PITCH>
__device__ __forceinline__ void alf_block_acc(const short* __restrict__ blk, const Pel* __restrict__ orgBlk, int ostride,
                                              int (&A)[(IS7 ? 13 : 7) * ((IS7 ? 13 : 7) + 1) / 2], int (&Y)[IS7 ? 13 : 7], int& pix)
{
  constexpr int N = IS7 ? 13 : 7, R = IS7 ? 3 : 2;
#pragma unroll 1
  for (int i = 0; i < 4; i++)                  // pixel row by+i (not unrolled: one row of tap sums live at a time)
  {
    // two horizontally adjacent pixels share every instruction: tap sums are built as packed 16-bit pairs
    // (v_pk_add_u16, <= 2 * 1023) and multiplied with v_dot2_i32_i16 (two exact MACs per instruction)
    us2 E[2][N];
#pragma unroll
    for (int jp = 0; jp < 2; jp++)
#pragma unroll
      for (int k = 0; k < N; k++) E[jp][k] = us2{ 0, 0 };
    const short* p = blk + (i + 3 - R) * PITCH;     // row by+i-R, col bx-4
    unsigned cen[2];
#pragma unroll
    for (int r = 0; r <= 2 * R; r++)
    {
      unsigned d[6];                                                // samples bx-4 .. bx+7 as pairs
      const uint2 v0 = *reinterpret_cast<const uint2*>(p + r * PITCH);
      const uint2 v1 = *reinterpret_cast<const uint2*>(p + r * PITCH + 4);
      const uint2 v2 = *reinterpret_cast<const uint2*>(p + r * PITCH + 8);
      d[0] = v0.x; d[1] = v0.y; d[2] = v1.x; d[3] = v1.y; d[4] = v2.x; d[5] = v2.y;
      if (r == R) { cen[0] = d[2]; cen[1] = d[3]; }
      const int dy = r - R;
#pragma unroll
      for (int dx = -R; dx <= R; dx++)
      {
        const int k = tapIndex<IS7>(dy, dx);
        if (k < 0) continue;
#pragma unroll
        for (int jp = 0; jp < 2; jp++)
        {
          const int s0 = 4 + 2 * jp + dx;                           // first sample of the pair (compile-time)
          const unsigned pr = (s0 & 1) ? __builtin_amdgcn_alignbit(d[(s0 + 1) >> 1], d[(s0 - 1) >> 1], 16) : d[s0 >> 1];
          E[jp][k] += __builtin_bit_cast(us2, pr);
        }
      }
    }
    const uint2 ov = *reinterpret_cast<const uint2*>(orgBlk + (size_t)i * ostride);
#pragma unroll
    for (int jp = 0; jp < 2; jp++)
    {
      const short2v yl = __builtin_bit_cast(short2v, jp ? ov.y : ov.x) - __builtin_bit_cast(short2v, cen[jp]);
      int idx = 0;
#pragma unroll
      for (int k = 0; k < N; k++)
      {
        const short2v ek = __builtin_bit_cast(short2v, E[jp][k]);
#pragma unroll
        for (int l = k; l < N; l++) { A[idx] = __builtin_amdgcn_sdot2(ek, __builtin_bit_cast(short2v, E[jp][l]), A[idx], false); idx++; }
        Y[k] = __builtin_amdgcn_sdot2(ek, yl, Y[k], false);
      }
      pix = __builtin_amdgcn_sdot2(yl, yl, pix, false);
    }
  }
}

template <bool IS7>
__device__ __forceinline__ void alf_stats_body(const int bidx, const int bidy, const Pel* __restrict__ org, int ostride,
                                                        const Pel* __restrict__ rec, int rstride, int w, int h,
                                                        int ctu, int wCtu, const uint16_t* __restrict__ cls,
                                                        int nCls, unsigned long long* __restrict__ out)
{
  constexpr int N = IS7 ? 13 : 7, R = IS7 ? 3 : 2;
  constexpr int NT = N * (N + 1) / 2;            // upper triangle
  constexpr int NB = NT + N + 1;                 // bucket entries: tri(E), y, pixAcc
  constexpr int RECSZ = N * N + N + 1;
  __shared__ short tile[AR * AP];
  // REP replicas of the class buckets, picked by the low lane bits: neighbouring blocks mostly share class and transpose, and
  // same-address LDS atomics serialise -- REP copies divide that queue; they are summed when the tile is flushed
  constexpr int REP = IS7 ? 2 : 4;              // 7x7: 2 x 21 KB keeps two workgroups per CU
  __shared__ unsigned long long bucket[REP * ALF_CLASSES * NB];
  const int tid = threadIdx.x;
  const int tx0 = bidx * AT, ty0 = bidy * AT;
  load_tile_clamped<AP>(tile, rec, rstride, w, h, tx0 - 4, ty0 - 3, AR, tid, 256);
  for (int i = tid; i < REP * ALF_CLASSES * NB; i += 256) bucket[i] = 0ull;
  __syncthreads();

  const int bj = tid & 15, bi = tid >> 4;
  const int bx = tx0 + 4 * bj, by = ty0 + 4 * bi;
  if (bx < w && by < h)
  {
    int A[NT], Y[N], pix = 0;
#pragma unroll
    for (int i = 0; i < NT; i++) A[i] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) Y[i] = 0;

    alf_block_acc<IS7, AP>(tile + (4 * bi) * AP + 4 * bj, org + (size_t)by * ostride + bx, ostride, A, Y, pix);
    // flush into the class bucket with the block's transpose permutation
    int classIdx = 0, t = 0;
    if (cls) { const uint16_t c = cls[(size_t)(by >> 2) * (w >> 2) + (bx >> 2)]; classIdx = c & 0xff; t = c >> 8; }
    unsigned long long perm;                    // nibble k = coefficient index that canonical tap k feeds
    if (IS7) perm = t == 0 ? 0xCBA9876543210ull : t == 1 ? 0xC62037B518A49ull : t == 2 ? 0xCBA9456781230ull : 0xC62015B734A89ull;
    else     perm = t == 0 ? 0x6543210ull : t == 1 ? 0x6203514ull : t == 2 ? 0x6541230ull : 0x6201534ull;
    // without a classifier (chroma) every block feeds class 0: spread over all REP * ALF_CLASSES slots instead
    constexpr int SLOTS1 = 1 << (31 - __builtin_clz(REP * ALF_CLASSES));           // largest power of two <= REP * ALF_CLASSES
    unsigned long long* b = bucket + (cls ? (tid & (REP - 1)) * ALF_CLASSES + classIdx : (tid & (SLOTS1 - 1))) * NB;
    int idx = 0;
#pragma unroll
    for (int k = 0; k < N; k++)
    {
      const int ck = (int)((perm >> (4 * k)) & 15);
#pragma unroll
      for (int l = k; l < N; l++)
      {
        const int cl = (int)((perm >> (4 * l)) & 15);
        const int lo = min(ck, cl), hi = max(ck, cl);
        // position of (lo,hi) in the row-major upper triangle
        const int pos = lo * N - (lo * (lo - 1)) / 2 + (hi - lo);
        atomicAdd(&b[pos], (unsigned long long)(long long)A[idx]);
        idx++;
      }
      atomicAdd(&b[NT + ck], (unsigned long long)(long long)Y[k]);
    }
    atomicAdd(&b[NT + N], (unsigned long long)(long long)pix);
  }
  __syncthreads();
  // flush LDS buckets to the CTU's record (a CTU is covered by several tiles -> global 64-bit atomics)
  const int ctuIdx = (ty0 / ctu) * wCtu + tx0 / ctu;
  unsigned long long* o = out + (size_t)ctuIdx * nCls * RECSZ;
  for (int i = tid; i < nCls * NB; i += 256)
  {
    unsigned long long v = 0ull;
    if (cls)
    {
#pragma unroll
      for (int r = 0; r < REP; r++) v += bucket[r * ALF_CLASSES * NB + i];
    }
    else
    {
      constexpr int SLOTS1 = 1 << (31 - __builtin_clz(REP * ALF_CLASSES));
      for (int r = 0; r < SLOTS1; r++) v += bucket[r * NB + i];     // i < NB here (nCls == 1)
    }
    if (v == 0ull) continue;
    const int c = i / NB, e = i - c * NB;
    unsigned long long* oc = o + (size_t)c * RECSZ;
    if (e < NT)
    {
      // invert pos -> (lo,hi)
      int lo = 0, rem = e;
      while (rem >= N - lo) { rem -= N - lo; lo++; }
      const int hi = lo + rem;
      atomicAdd(&oc[lo * N + hi], v);
      if (hi != lo) atomicAdd(&oc[hi * N + lo], v);
    }
    else
      atomicAdd(&oc[N * N + (e - NT)], v);
  }
}

template <bool IS7>
__global__ __launch_bounds__(256) void alf_stats_kernel(const Pel* __restrict__ org, int ostride, const Pel* __restrict__ rec, int rstride, int w, int h,
                                                        int ctu, int wCtu, const uint16_t* __restrict__ cls, int nCls, unsigned long long* __restrict__ out)
{
  alf_stats_body<IS7>((int)blockIdx.x, (int)blockIdx.y, org, ostride, rec, rstride, w, h, ctu, wCtu, cls, nCls, out);
}

// both chroma planes (5x5, no classifier) in one launch: blockIdx.z selects the plane
__global__ __launch_bounds__(256) void alf_stats_chroma2_kernel(const Pel* __restrict__ orgCb, const Pel* __restrict__ orgCr, int ostride,
                                                                const Pel* __restrict__ recCb, const Pel* __restrict__ recCr, int rstride, int w, int h,
                                                                int ctu, int wCtu, unsigned long long* __restrict__ outCb, unsigned long long* __restrict__ outCr)
{
  const bool cr = blockIdx.z != 0;
  alf_stats_body<false>((int)blockIdx.x, (int)blockIdx.y, cr ? orgCr : orgCb, ostride, cr ? recCr : recCb, rstride, w, h, ctu, wCtu, nullptr, 1, cr ? outCr : outCb);
}

// ---------------------------------------------------------------------------------------------------
// Picture form of A3 (vvcgpu_alf_stats_picture, vvcgpu_alf_classify_stats_picture): ONE workgroup of 512 threads per CTU (64 or 128) writes the
// CTU's 7x7 and 5x5 records of every class and both chroma records -- no zero-fill pass, no global atomics, no 5x5-from-7x7 pass.  The
// statistics are Gram matrices on the matrix cores, one 64-bit record per class in LDS: alf_ctu_luma (blocks sorted by class) and
// alf_ctu_chroma (the CTU's chroma pair, run while the luma tile is in flight) say how.
// ---------------------------------------------------------------------------------------------------
constexpr int ACT = 512;                          // threads per CTU workgroup

template <int C> struct AlfCtuLds
{
  static constexpr int P = C + 8, ROWS = C + 6;                          // luma tile
  static constexpr int tileBytes = (ROWS * P * 2 + 15) & ~15;
  static constexpr int zeroBytes = (3 * P * 2 + 16 + 15) & ~15;          // four rows of zeros at the tile's pitch: what an empty slot of a step reads
  static constexpr int bucketBytes = ALF_CLASSES * ALF_REC7 * 8;                   // one 64-bit record per class
  static constexpr int MAXSTEPS = (C / 4) * (C / 4) / 4 + ALF_CLASSES;           // steps of four blocks, every class padded to whole steps
  static constexpr int listBytes = MAXSTEPS * 4 * 4;                     // u32 per slot: centre sample index | transposition << 16 | block << 18
  static constexpr int stepClsBytes = (MAXSTEPS + 15) & ~15;
  static constexpr int stageBytes = (ACT / 64) * 128;                    // per wave: the org rows of the current step (4 blocks x 4 rows x 8 bytes)
  static constexpr int lumaBytes = tileBytes + zeroBytes + bucketBytes + listBytes + stepClsBytes + stageBytes + 64 * 4;
  static constexpr int CP = C / 2 + 8, CROWS = C / 2 + 6;                // chroma tiles (two planes)
  static constexpr int ctileBytes = (CROWS * CP * 2 + 15) & ~15;
  static constexpr int chromaBytes = 2 * ctileBytes + 2 * ALF_REC5 * 8;
  static constexpr int bytes = lumaBytes > chromaBytes ? lumaBytes : chromaBytes;
};

struct AlfStatsPic
{
  const Pel* org[3]; const Pel* rec[3]; int ostride[3], rstride[3];
  int w, h, wCtu, nCtu, xcd;
  const uint16_t* cls;
  uint16_t* clsOut; int clsShift;                  // fused form (vvcgpu_alf_classify_stats_picture): the classes are DERIVED here and written out
  unsigned long long* out7; unsigned long long* out5; unsigned long long* outC[2];
};

typedef int alf_i4 __attribute__((ext_vector_type(4)));

// Luma CTU on the matrix cores.  The statistics of a class are the Gram matrix of x = (s_0 .. s_11, centre, org - rec) over the pixels of the
// class's blocks (s_k = the two samples of tap pair k, in FILTER coefficient order, i.e. behind the block's transposition): E = X X^T restricted
// to 13 x 13, y = its column 13, pixAcc = entry (13, 13).  Values need 11 bits (+ sign for org - rec), so x = 256 H + L with L = the low byte read
// as SIGNED (the matrix cores multiply signed bytes) and H = (x + 128) >> 8 in [-4, 8] = the high byte of x + 128: both limbs are byte picks
// (v_perm_b32), no masks or shifts; four v_mfma_i32_16x16x64_i8 per step of 64 pixels accumulate L L^T, H L^T, L H^T and H H^T exactly in int32
// (a whole CTU of one class stays below 2^29: L L^T reaches 128 x 128 x 16384 pixels = 2^28 exactly when every pixel of a 128 x 128 CTU falls into one
// class with L = -128 -- rec = 64 everywhere for the tap pairs, 128 for the centre sample; tests/test_gpu_stats.py::test_alf_stats_single_class_worst_limbs
// and tests/test_gpu_inloop_picture.py::test_alf_stats_picture_single_class_worst_limbs run it), and E = 65536 HH + 256 (HL + LH) + LL is formed in 64
// bits when a class is finished.
//   * the CTU's 4x4 blocks are counting-sorted by class in LDS; a class is padded to whole steps of four blocks;
//   * lane (c, g) of a step builds variable c for the 16 pixels of block g: two unaligned 4-sample reads per row from the LDS tile (offset of
//     the tap that the block's transposition puts at coefficient c), one v_pk_add_u16, limb split, byte pack -- the SAME registers are the A
//     and the B operand, so the k order inside the instruction does not matter;
//   * the eight waves take contiguous ranges of steps; a wave adds its accumulators to the class's 64-bit LDS record when the class changes
//     (distinct addresses inside a wave, so the LDS atomics do not serialise).
// The old form (per-lane upper-triangle accumulation with v_dot2, ~1100 vector instructions and 105 serialising LDS atomics per block) took
// 83 us for a 3840x2160 picture; see DESIGN.md for the measured time of this one.
// CLS: the block classes are not read but derived from the tile (AdaptiveLoopFilter::deriveClassificationBlk, :248-455; the text of
// alf_classify_kernel in alf.hip, alf_quad_sums.inc and alf_class_key.inc: the tile has the same origin and clamping) and written to a.clsOut --
// the classifier's own launch and its read of the picture are gone.  The Laplacian sums of the (C / 4 + 1)^2 4x4 quads live where the class records are accumulated later.
// `between` runs while the luma tile is on its way into the threads' registers (the kernel puts the CTU's chroma pair there).
template <int C, bool CLS, typename Between>
__device__ __forceinline__ void alf_ctu_luma(const AlfStatsPic& a, int ctuIdx, unsigned char* smem, Between between)
{
  using L = AlfCtuLds<C>;
  constexpr int P = L::P, BPR = C / 4, NBLK = BPR * BPR, S = (NBLK + ACT - 1) / ACT, NW = ACT / 64;
  constexpr int oZero = L::tileBytes, oBucket = oZero + L::zeroBytes, oList = oBucket + L::bucketBytes, oStepCls = oList + L::listBytes,
                oStage = oStepCls + L::stepClsBytes, oCnt = oStage + L::stageBytes;
  constexpr unsigned CEN_ZERO = (unsigned)(oZero / 2), EMPTY = CEN_ZERO | 0x80000000u;     // empty slot: centre in the zero rows, flag in bit 31
  short* tile = reinterpret_cast<short*>(smem);
  unsigned long long* bucket = reinterpret_cast<unsigned long long*>(smem + oBucket);
  unsigned* list = reinterpret_cast<unsigned*>(smem + oList);
  unsigned char* stepCls = smem + oStepCls;
  int* cnt = reinterpret_cast<int*>(smem + oCnt);                          // [32] counts, [32] first step of the class
  int* start = cnt + 32;
  const int tid = threadIdx.x;
  const int x0 = (ctuIdx % a.wCtu) * C, y0 = (ctuIdx / a.wCtu) * C;
  int myKey[S], myPos[S];
  {
    constexpr int NBT = (L::ROWS * (P / 4) + ACT - 1) / ACT;
    pel4 tv[NBT];
    tile_fetch<P, NBT>(tv, a.rec[0], a.rstride[0], a.w, a.h, x0 - 4, y0 - 3, L::ROWS, tid, ACT);
    // the classes of this thread's blocks: requested together with the tile (behind the barrier they were a second memory latency of the set-up)
#pragma unroll
    for (int s = 0; s < S; s++)
    {
      const int blk = tid + s * ACT, bi = blk % BPR, bj = blk / BPR;
      const int bx = x0 + 4 * bj, by = y0 + 4 * bi;
      myKey[s] = -1;
      if (!CLS && blk < NBLK && bx < a.w && by < a.h) myKey[s] = (int)a.cls[(size_t)(by >> 2) * (a.w >> 2) + (bx >> 2)];
    }
    between();                                                              // (the luma tile is on its way into this thread's registers)
    tile_store<P, NBT>(tile, tv, L::ROWS, tid, ACT);
  }
  for (int i = tid; i < L::zeroBytes / 4; i += ACT) reinterpret_cast<unsigned*>(smem + oZero)[i] = 0u;
  if (!CLS) for (int i = tid; i < ALF_CLASSES * ALF_REC7; i += ACT) bucket[i] = 0ull;
  for (int i = tid; i < L::MAXSTEPS * 4; i += ACT) list[i] = EMPTY;
  if (tid < 64) cnt[tid] = 0;
  __syncthreads();
  if (CLS)
  {
    constexpr int QN = BPR + 1;
    static_assert(QN * QN * 16 <= L::bucketBytes, "quad sums fit into the record region");
    int* quad = reinterpret_cast<int*>(smem + oBucket);
    for (int q = tid; q < QN * QN; q += ACT)
    {
      // quad (qi, qj): picture rows y0 + 4 qi - 2 .. + 1, columns x0 + 4 qj - 2 .. + 1; two samples per instruction as in alf_classify_kernel
      const int qi = q / QN, qj = q - qi * QN;                              // row-major: neighbouring lanes read neighbouring 8-byte words of a tile row
      const unsigned* base = reinterpret_cast<const unsigned*>(tile + (4 * qi) * P + 4 * qj);
      constexpr int quadPitch = P;
#include "alf_quad_sums.inc"
      *reinterpret_cast<int4*>(quad + (qi * QN + qj) * 4) = make_int4((int)sv, (int)sh, (int)sd0, (int)sd1);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < S; s++)
    {
      const int blk = tid + s * ACT, bi = blk % BPR, bj = blk / BPR;
      const int bx = x0 + 4 * bj, by = y0 + 4 * bi;
      if (blk < NBLK && bx < a.w && by < a.h)
      {
        const int4 q00 = *reinterpret_cast<const int4*>(quad + (bi * QN + bj) * 4), q01 = *reinterpret_cast<const int4*>(quad + (bi * QN + bj + 1) * 4);
        const int4 q10 = *reinterpret_cast<const int4*>(quad + ((bi + 1) * QN + bj) * 4), q11 = *reinterpret_cast<const int4*>(quad + ((bi + 1) * QN + bj + 1) * 4);
        const int sumV = q00.x + q01.x + q10.x + q11.x, sumH = q00.y + q01.y + q10.y + q11.y;
        const int sumD0 = q00.z + q01.z + q10.z + q11.z, sumD1 = q00.w + q01.w + q10.w + q11.w;
        const int& keyShift = a.clsShift;
#include "alf_class_key.inc"
        myKey[s] = classIdx | (transposeIdx << 8);
        a.clsOut[(size_t)(by >> 2) * (a.w >> 2) + (bx >> 2)] = (uint16_t)myKey[s];
      }
    }
    __syncthreads();
    for (int i = tid; i < ALF_CLASSES * ALF_REC7; i += ACT) bucket[i] = 0ull;        // (two barriers before the first record is added to)
  }
#pragma unroll
  for (int s = 0; s < S; s++)
  {
    // column-major thread -> block map (blk = tid + s ACT, row blk % BPR): the lanes of a wave are vertical neighbours, so the four blocks of a step
    // mostly are too -- their tile rows sit 16 LDS banks apart (4 rows x 68 dwords), while horizontal neighbours (2 banks apart) collide four-way
    // in every tile read
    myPos[s] = 0;
    // position inside the class: one LDS atomic per wave and distinct class (neighbouring blocks mostly share the class, and same-address
    // atomics serialise), the lanes of a class take consecutive positions behind the returned base
    const int myC = myKey[s] < 0 ? -1 : (myKey[s] & 0xff);
    unsigned long long todo = __ballot(myC >= 0);
    while (todo)
    {
      const int leader = __builtin_ctzll(todo);
      const int cc = __shfl(myC, leader);
      const unsigned long long m = __ballot(myC == cc);
      int base = 0;
      if ((tid & 63) == leader) base = atomicAdd(&cnt[cc], (int)__popcll(m));
      base = __shfl(base, leader);
      if (myC == cc) myPos[s] = base + (int)__popcll(m & ((1ull << (tid & 63)) - 1ull));
      todo &= ~m;
    }
  }
  __syncthreads();
  if (tid < 64)                                                             // first step of every class: an exclusive prefix sum over the lanes of one wave
  {
    const int steps = tid < ALF_CLASSES ? (cnt[tid] + 3) >> 2 : 0;
    int incl = steps;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) { const int v = __shfl_up(incl, o); if (tid >= o) incl += v; }
    if (tid <= ALF_CLASSES) start[tid] = incl - steps;                       // (lane ALF_CLASSES: the total)
  }
  __syncthreads();
  const int T = start[ALF_CLASSES];
#pragma unroll
  for (int s = 0; s < S; s++)
    if (myKey[s] >= 0)
    {
      const int blk = tid + s * ACT, bi = blk % BPR, bj = blk / BPR;
      list[start[myKey[s] & 0xff] * 4 + myPos[s]] = (unsigned)((4 * bi + 3) * P + 4 * bj + 4) | (unsigned)((myKey[s] >> 8) & 3) << 16 | (unsigned)(bi * BPR + bj) << 18;
    }
  for (int st = tid; st < T; st += ACT)
  {
    int c = 0;
    while (st >= start[c + 1]) c++;
    stepCls[st] = (unsigned char)c;
  }
  __syncthreads();

  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, c = lane & 15, g = lane >> 4;
  // sample offset of the tap that transposition t puts at coefficient c (geometric tap k sits at coefficient perm_t[k])
  constexpr int geoDy[13] = { 3, 2, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0, 0 }, geoDx[13] = { 0, 1, 0, -1, 2, 1, 0, -1, -2, 3, 2, 1, 0 };
  int offT[4] = { 0, 0, 0, 0 };
#pragma unroll
  for (int t = 0; t < 4; t++)
  {
    const unsigned long long perm = t == 0 ? 0xCBA9876543210ull : t == 1 ? 0xC62037B518A49ull : t == 2 ? 0xCBA9456781230ull : 0xC62015B734A89ull;
#pragma unroll
    for (int k = 0; k < 12; k++)
      if ((int)((perm >> (4 * k)) & 15) == c) offT[t] = geoDy[k] * P + geoDx[k];
  }
  // second operand of the pair sum: + for the taps, 0 for the centre, - for org - rec (first operand = org there)
  const unsigned sgn = c < 12 ? 0x00010001u : (c == 12 ? 0u : 0xFFFFFFFFu);
  const bool isD = c == 13, dead = c >= 14;
  const int s0 = (wv * T) / NW, s1 = ((wv + 1) * T) / NW;
  alf_i4 LLa = { 0, 0, 0, 0 }, HLa = { 0, 0, 0, 0 }, LHa = { 0, 0, 0, 0 }, HHa = { 0, 0, 0, 0 };
  int cur = -1;
  auto flush = [&](int cl)
  {
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
      const int row = 4 * g + r;
      const long long v = (long long)HHa[r] * 65536 + (long long)(HLa[r] + LHa[r]) * 256 + (long long)LLa[r];
      int e = -1;
      if (row < 13 && c < 13) e = row * 13 + c;
      else if (row == 13 && c < 13) e = 169 + c;
      else if (row == 13 && c == 13) e = 182;
      if (e >= 0) atomicAdd(&bucket[cl * ALF_REC7 + e], (unsigned long long)v);
    }
    LLa = HLa = LHa = HHa = alf_i4{ 0, 0, 0, 0 };
  };
  // org rows of a step (four blocks x four rows of 8 bytes) are loaded FOUR steps ahead by lanes 0..15 (lane 4 g + i: row i of block g), kept
  // in registers, and written to the wave's 128-byte LDS stage when their step comes: the org - rec lanes read their first operand there
  // (row pitch 8 bytes) exactly as the other lanes read theirs in the tile (row pitch 2 P bytes)
  const unsigned stageOff = (unsigned)(oStage + wv * 128);
  const Pel* orgRowBase = a.org[0] + (size_t)(y0 + (lane & 3)) * a.ostride[0] + x0;
  const unsigned rowStep = isD ? 8u : (unsigned)(2 * P);
  auto issue = [&](int stp, uint2& dst)
  {
    dst = make_uint2(0u, 0u);
    if (lane < 16 && stp < s1)
    {
      const unsigned e2 = list[stp * 4 + (lane >> 2)];
      if ((int)e2 >= 0)
      {
        const unsigned blk2 = e2 >> 18;
        dst = *reinterpret_cast<const uint2*>(orgRowBase + (size_t)(4 * (blk2 / BPR)) * a.ostride[0] + 4 * (blk2 % BPR));
      }
    }
  };
  auto step = [&](int st, const uint2& orgRow)
  {
    const int cl = __builtin_amdgcn_readfirstlane((int)stepCls[st]);
    if (cl != cur) { if (cur >= 0) flush(cur); cur = cl; }
    if (lane < 16) *reinterpret_cast<uint2*>(smem + stageOff + lane * 8) = orgRow;
    const unsigned e = list[st * 4 + g];
    const int t = (int)(e >> 16) & 3;
    const int offLo = (t & 1) ? offT[1] : offT[0], offHi = (t & 1) ? offT[3] : offT[2];
    const int off = (int)e < 0 ? 0 : ((t & 2) ? offHi : offLo);           // empty slot: both operands in the zero rows
    const int cen = dead ? (int)CEN_ZERO : (int)(e & 0xFFFFu);
    const int ap = cen + off, am = cen - off;                               // first samples of the two 4-sample rows (row i: + i P); cen is even
    const unsigned sh = (unsigned)(off & 1) << 4;
    const unsigned adP = isD ? (stageOff + (unsigned)g * 32u) : (unsigned)(ap >> 1) << 2;
    const unsigned adM = (unsigned)(am >> 1) << 2;
    alf_i4 aL, aH;
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
      const unsigned* dp = reinterpret_cast<const unsigned*>(smem + adP + i * rowStep);
      const unsigned* dm = reinterpret_cast<const unsigned*>(smem + adM + i * 2 * P);
      const unsigned p0 = dp[0], p1 = dp[1], p2 = dp[2], m0 = dm[0], m1 = dm[1], m2 = dm[2];
      const unsigned P01 = __builtin_amdgcn_alignbit(p1, p0, sh), P23 = __builtin_amdgcn_alignbit(p2, p1, sh);
      const unsigned M01 = __builtin_amdgcn_alignbit(m1, m0, sh), M23 = __builtin_amdgcn_alignbit(m2, m1, sh);
      const us2 v01 = __builtin_bit_cast(us2, P01) + __builtin_bit_cast(us2, M01) * __builtin_bit_cast(us2, sgn);
      const us2 v23 = __builtin_bit_cast(us2, P23) + __builtin_bit_cast(us2, M23) * __builtin_bit_cast(us2, sgn);
      const us2 bias = { 128, 128 };
      const us2 h01 = v01 + bias, h23 = v23 + bias;
      aL[i] = (int)__builtin_amdgcn_perm(__builtin_bit_cast(unsigned, v23), __builtin_bit_cast(unsigned, v01), 0x06040200u);   // low bytes, signed
      aH[i] = (int)__builtin_amdgcn_perm(__builtin_bit_cast(unsigned, h23), __builtin_bit_cast(unsigned, h01), 0x07050301u);   // (v + 128) >> 8
    }
    LLa = __builtin_amdgcn_mfma_i32_16x16x64_i8(aL, aL, LLa, 0, 0, 0);
    HHa = __builtin_amdgcn_mfma_i32_16x16x64_i8(aH, aH, HHa, 0, 0, 0);
    HLa = __builtin_amdgcn_mfma_i32_16x16x64_i8(aH, aL, HLa, 0, 0, 0);
    LHa = __builtin_amdgcn_mfma_i32_16x16x64_i8(aL, aH, LHa, 0, 0, 0);
  };
  uint2 ring[4];
#pragma unroll
  for (int u = 0; u < 4; u++) issue(s0 + u, ring[u]);
  for (int st = s0; st < s1; st += 4)
  {
#pragma unroll
    for (int u = 0; u < 4; u++)
    {
      if (st + u < s1)                                                      // wave-uniform
      {
        step(st + u, ring[u]);
        issue(st + u + 4, ring[u]);
      }
    }
  }
  if (cur >= 0) flush(cur);
  __syncthreads();
  // records: 7x7 (13 x 13 + 13 + 1 entries per class) and its 5x5 sub-record (coefficient i of 5x5 = coefficient sig[i] of 7x7)
  unsigned long long* o7 = a.out7 + (size_t)ctuIdx * ALF_CLASSES * ALF_REC7;
  for (int i = tid; i < ALF_CLASSES * ALF_REC7; i += ACT) o7[i] = bucket[i];
  unsigned long long* o5 = a.out5 + (size_t)ctuIdx * ALF_CLASSES * ALF_REC5;
  for (int i = tid; i < ALF_CLASSES * ALF_REC5; i += ACT)
  {
    const int cc = i / ALF_REC5, e = i - cc * ALF_REC5;
    const int sig[7] = { 2, 5, 6, 7, 10, 11, 12 };
    o5[i] = bucket[cc * ALF_REC7 + (e < 49 ? sig[e / 7] * 13 + sig[e % 7] : e < 56 ? 169 + sig[e - 49] : 182)];
  }
}

// Chroma CTU pair, same form: the 16 variables are (six tap pairs, centre, org - rec) of Cb and of Cr at the same pixel, so one Gram matrix holds
// the Cb record in its upper-left and the Cr record in its lower-right 8 x 8 (the cross terms are dropped).  No classes, no transposition.
// what the chroma part of a CTU needs from memory, requested BEFORE the luma part runs: the org rows of every step of this wave
// (lanes 0..31: plane, block, row) and this thread's share of the two reconstruction tiles
template <int C> struct AlfChromaPre
{
  using L = AlfCtuLds<C>;
  static constexpr int NS = (C / 8) * (C / 8) / 4, NW = ACT / 64, NSW = (NS + NW - 1) / NW, NBT = (L::CROWS * (L::CP / 4) + ACT - 1) / ACT;
  uint2 orgR[NSW];
  pel4 tv[2][NBT];
};

template <int C>
__device__ __forceinline__ void alf_chroma_prefetch(const AlfStatsPic& a, int ctuIdx, AlfChromaPre<C>& pre)
{
  using L = AlfCtuLds<C>;
  using PR = AlfChromaPre<C>;
  constexpr int C2 = C / 2, BPR = C2 / 4;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int w2 = a.w >> 1, h2 = a.h >> 1;
  const int x0 = (ctuIdx % a.wCtu) * C2, y0 = (ctuIdx / a.wCtu) * C2;
  const int s0 = (wv * PR::NS) / PR::NW, s1 = ((wv + 1) * PR::NS) / PR::NW;
  const int pl2 = (lane >> 4) & 1, g2 = (lane >> 2) & 3, i2 = lane & 3;
#pragma unroll
  for (int u = 0; u < PR::NSW; u++)
  {
    pre.orgR[u] = make_uint2(0u, 0u);
    const int blk = (s0 + u) * 4 + g2, bi = blk / BPR, bj = blk % BPR;
    if (lane < 32 && s0 + u < s1 && x0 + 4 * bj < w2 && y0 + 4 * bi < h2)
      pre.orgR[u] = *reinterpret_cast<const uint2*>(a.org[1 + pl2] + (size_t)(y0 + 4 * bi + i2) * a.ostride[1 + pl2] + x0 + 4 * bj);
  }
#pragma unroll
  for (int q = 0; q < 2; q++)
    tile_fetch<L::CP, PR::NBT>(pre.tv[q], a.rec[1 + q], a.rstride[1 + q], w2, h2, x0 - 4, y0 - 3, L::CROWS, tid, ACT);
}

template <int C>
__device__ __forceinline__ void alf_ctu_chroma(const AlfStatsPic& a, int ctuIdx, unsigned char* smem, const AlfChromaPre<C>& pre)
{
  using L = AlfCtuLds<C>;
  constexpr int P = L::CP, C2 = C / 2, BPR = C2 / 4, NBLK = BPR * BPR, NS = NBLK / 4, NW = ACT / 64, NSW = (NS + NW - 1) / NW;
  constexpr int oBucket = 2 * L::ctileBytes, oStage = oBucket + 2 * ALF_REC5 * 8 + 16;
  static_assert(NS % NW == 0 || NS < NW, "chroma steps per wave");
  const int tid = threadIdx.x;
  const int w2 = a.w >> 1, h2 = a.h >> 1;
  const int x0 = (ctuIdx % a.wCtu) * C2, y0 = (ctuIdx / a.wCtu) * C2;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, c = lane & 15, g = lane >> 4, pl = c >> 3, cc = c & 7;
  const int s0 = (wv * NS) / NW, s1 = ((wv + 1) * NS) / NW;
  unsigned long long* bucket = reinterpret_cast<unsigned long long*>(smem + oBucket);       // [plane][ALF_REC5]
#pragma unroll
  for (int q = 0; q < 2; q++) tile_store<P, AlfChromaPre<C>::NBT>(reinterpret_cast<short*>(smem + q * L::ctileBytes), pre.tv[q], L::CROWS, tid, ACT);
  for (int i = tid; i < 2 * ALF_REC5; i += ACT) bucket[i] = 0ull;
  __syncthreads();
  constexpr int geoDy[7] = { 2, 1, 1, 1, 0, 0, 0 }, geoDx[7] = { 0, 1, 0, -1, 2, 1, 0 };
  int off = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) if (cc == k) off = geoDy[k] * P + geoDx[k];
  const unsigned sgn = cc < 6 ? 0x00010001u : (cc == 6 ? 0u : 0xFFFFFFFFu);
  const bool isD = cc == 7;
  const unsigned tileOff = (unsigned)(pl * L::ctileBytes), stageOff = (unsigned)(oStage + wv * 256);
  const unsigned rowStep = isD ? 8u : (unsigned)(2 * P);
  const unsigned sh = (unsigned)(off & 1) << 4;
  alf_i4 LLa = { 0, 0, 0, 0 }, HLa = { 0, 0, 0, 0 }, LHa = { 0, 0, 0, 0 }, HHa = { 0, 0, 0, 0 };
#pragma unroll
  for (int u = 0; u < NSW; u++)
  {
    const int st = s0 + u;
    if (st < s1)                                                            // wave-uniform
    {
      if (lane < 32) *reinterpret_cast<uint2*>(smem + stageOff + lane * 8) = pre.orgR[u];
      const int blk = st * 4 + g, bi = blk / BPR, bj = blk % BPR;
      const bool valid = x0 + 4 * bj < w2 && y0 + 4 * bi < h2;
      const int cen = (4 * bi + 3) * P + 4 * bj + 4;
      const int ap = cen + off, am = cen - off;
      const unsigned adP = isD ? stageOff + (unsigned)(pl * 128 + g * 32) : tileOff + ((unsigned)(ap >> 1) << 2);
      const unsigned adM = tileOff + ((unsigned)(am >> 1) << 2);
      alf_i4 aL, aH;
#pragma unroll
      for (int i = 0; i < 4; i++)
      {
        const unsigned* dp = reinterpret_cast<const unsigned*>(smem + adP + i * rowStep);
        const unsigned* dm = reinterpret_cast<const unsigned*>(smem + adM + i * 2 * P);
        const unsigned p0 = dp[0], p1 = dp[1], p2 = dp[2], m0 = dm[0], m1 = dm[1], m2 = dm[2];
        const unsigned P01 = __builtin_amdgcn_alignbit(p1, p0, sh), P23 = __builtin_amdgcn_alignbit(p2, p1, sh);
        const unsigned M01 = __builtin_amdgcn_alignbit(m1, m0, sh), M23 = __builtin_amdgcn_alignbit(m2, m1, sh);
        const us2 v01 = __builtin_bit_cast(us2, P01) + __builtin_bit_cast(us2, M01) * __builtin_bit_cast(us2, sgn);
        const us2 v23 = __builtin_bit_cast(us2, P23) + __builtin_bit_cast(us2, M23) * __builtin_bit_cast(us2, sgn);
        const us2 bias = { 128, 128 };
        const us2 h01 = v01 + bias, h23 = v23 + bias;
        aL[i] = (int)__builtin_amdgcn_perm(__builtin_bit_cast(unsigned, v23), __builtin_bit_cast(unsigned, v01), 0x06040200u);
        aH[i] = (int)__builtin_amdgcn_perm(__builtin_bit_cast(unsigned, h23), __builtin_bit_cast(unsigned, h01), 0x07050301u);
      }
      if (!valid) { aL = alf_i4{ 0, 0, 0, 0 }; aH = alf_i4{ 0, 0, 0, 0 }; }
      LLa = __builtin_amdgcn_mfma_i32_16x16x64_i8(aL, aL, LLa, 0, 0, 0);
      HHa = __builtin_amdgcn_mfma_i32_16x16x64_i8(aH, aH, HHa, 0, 0, 0);
      HLa = __builtin_amdgcn_mfma_i32_16x16x64_i8(aH, aL, HLa, 0, 0, 0);
      LHa = __builtin_amdgcn_mfma_i32_16x16x64_i8(aL, aH, LHa, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++)
  {
    const int row = 4 * g + r, r7 = row & 7;
    const long long v = (long long)HHa[r] * 65536 + (long long)(HLa[r] + LHa[r]) * 256 + (long long)LLa[r];
    int e = -1;
    if ((row >> 3) == pl)
    {
      if (r7 < 7 && cc < 7) e = r7 * 7 + cc;
      else if (r7 == 7 && cc < 7) e = 49 + cc;
      else if (r7 == 7 && cc == 7) e = 56;
    }
    if (e >= 0 && s1 > s0) atomicAdd(&bucket[pl * ALF_REC5 + e], (unsigned long long)v);
  }
  __syncthreads();
  for (int i = tid; i < 2 * ALF_REC5; i += ACT) a.outC[i / ALF_REC5][(size_t)ctuIdx * ALF_REC5 + (i % ALF_REC5)] = bucket[i];
}

// one workgroup per CTU: the CTU's chroma pair, then luma in the same LDS (the chroma tiles and records lie inside the luma tile's bytes, which are
// written behind the barrier that ends the chroma part).
// As workgroups of their own the chroma pairs were a second round of 80 KB workgroups behind the luma round: 10 us of a 56 us launch.
template <int C, bool CLS>
__global__ __launch_bounds__(ACT) void alf_stats_picture_kernel(AlfStatsPic a)
{
  extern __shared__ __align__(16) unsigned char alfSmem[];
  AlfChromaPre<C> pre;
  const int ctuIdx = vvc_xcd_index((int)blockIdx.x, a.nCtu, a.xcd);
  if (ctuIdx < 0) return;
  // the chroma pair FIRST, with the luma tile requested in front of it: the luma tile's trip through the start-up burst (every workgroup of the chip
  // fetches at once) is covered by the chroma part's arithmetic instead of by nothing (58.9 -> 58.0 us; luma first with the chroma loads behind the tile: 59.4)
  alf_chroma_prefetch<C>(a, ctuIdx, pre);
  alf_ctu_luma<C, CLS>(a, ctuIdx, alfSmem, [&]() { alf_ctu_chroma<C>(a, ctuIdx, alfSmem, pre); __syncthreads(); });
}

// The 5x5 diamond is the centre of the 7x7 diamond under every transposition, so the 5x5 covariance record of a class is a sub-matrix of its 7x7
// record: coefficient i of the 5x5 filter is coefficient SIG[i] of the 7x7 filter (tap (2,0) -> 2, (1,1) -> 5, (1,0) -> 6, (1,-1) -> 7, (0,2) -> 10,
// (0,1) -> 11, centre -> 12).  One thread per output entry; also zeroes nothing: every entry of out5 is written.
__global__ __launch_bounds__(256) void alf_stats_5from7_kernel(const unsigned long long* __restrict__ out7, unsigned long long* __restrict__ out5, int nRecords)
{
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= nRecords * ALF_REC5) return;
  const int rec = gid / ALF_REC5, e = gid - rec * ALF_REC5;
  const int sig[7] = { 2, 5, 6, 7, 10, 11, 12 };
  const unsigned long long* r7 = out7 + (size_t)rec * ALF_REC7;
  unsigned long long v;
  if (e < 49) v = r7[sig[e / 7] * 13 + sig[e % 7]];
  else if (e < 56) v = r7[169 + sig[e - 49]];
  else v = r7[182];
  out5[gid] = v;
}

__global__ __launch_bounds__(256) void zero3_kernel(unsigned long long* a, size_t na, unsigned long long* b, size_t nb, unsigned long long* c, size_t nc)
{
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t i = gid; i < na; i += stride) a[i] = 0ull;
  for (size_t i = gid; i < nb; i += stride) b[i] = 0ull;
  for (size_t i = gid; i < nc; i += stride) c[i] = 0ull;
}


}  // namespace

extern "C" {

int vvcgpu_alf_stats(const vvc_pel* org, int org_stride, const vvc_pel* rec, int rec_stride,
                     int width, int height, int ctu_size, const uint16_t* cls, int filter_type,
                     int64_t* out, void* stream)
{
  VVC_CHECK_ARG(org && rec && out, "alf_stats: null pointer");
  VVC_CHECK_ARG(width > 0 && height > 0 && (width & 3) == 0 && (height & 3) == 0, "alf_stats: size must be a multiple of 4");
  VVC_CHECK_ARG(org_stride >= width && rec_stride >= width && (org_stride & 3) == 0 && ((uintptr_t)org & 7) == 0,
                "alf_stats: org needs stride %% 4 == 0 and 8-byte alignment");
  VVC_CHECK_ARG(ctu_size >= AT ? (ctu_size % AT) == 0 : false, "alf_stats: ctu size %d must be a multiple of %d", ctu_size, AT);
  VVC_CHECK_ARG(filter_type == 0 || filter_type == 1, "alf_stats: filter_type %d", filter_type);
  const int nCls = cls ? ALF_CLASSES : 1;
  const int N = filter_type ? 13 : 7;
  const int wCtu = cdiv(width, ctu_size), hCtu = cdiv(height, ctu_size);
  hipStream_t st = (hipStream_t)stream;
  VVC_HIP(hipMemsetAsync(out, 0, sizeof(int64_t) * (size_t)(N * N + N + 1) * nCls * wCtu * hCtu, st));
  dim3 grid(cdiv(width, AT), cdiv(height, AT));
  if (filter_type)
    hipLaunchKernelGGL(alf_stats_kernel<true>, grid, dim3(256), 0, st, org, org_stride, rec, rec_stride, width, height,
                       ctu_size, wCtu, cls, nCls, reinterpret_cast<unsigned long long*>(out));
  else
    hipLaunchKernelGGL(alf_stats_kernel<false>, grid, dim3(256), 0, st, org, org_stride, rec, rec_stride, width, height,
                       ctu_size, wCtu, cls, nCls, reinterpret_cast<unsigned long long*>(out));
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

}  // extern "C"

// cls_out != nullptr: the fused form -- the classes are derived inside the CTU workgroups and written to cls_out (cls is not read)
static int alf_stats_picture_impl(const vvcgpu_planes* org, const vvcgpu_planes* rec, int width, int height, int ctu_size, const uint16_t* cls,
                                  uint16_t* cls_out, int bit_depth, int64_t* out7, int64_t* out5, int64_t* out_cb, int64_t* out_cr, void* stream)
{
  VVC_CHECK_ARG(org && rec && (cls || cls_out) && out7 && out5 && out_cb && out_cr, "alf_stats_picture: null pointer");
  VVC_CHECK_ARG(width > 0 && height > 0 && (width & 7) == 0 && (height & 7) == 0, "alf_stats_picture: size must be a multiple of 8");
  VVC_CHECK_ARG(ctu_size == 64 || (ctu_size >= 2 * AT && (ctu_size % (2 * AT)) == 0), "alf_stats_picture: ctu size %d must be 64 or a multiple of %d", ctu_size, 2 * AT);
  for (int c = 0; c < 3; c++)
  {
    const int w = c ? width >> 1 : width;
    VVC_CHECK_ARG(org->p[c] && rec->p[c] && org->stride[c] >= w && rec->stride[c] >= w && (org->stride[c] & 3) == 0 && ((uintptr_t)org->p[c] & 7) == 0,
                  "alf_stats_picture: plane %d (org needs stride %% 4 == 0 and 8-byte alignment)", c);
  }
  VVC_CHECK_ARG(org->stride[1] == org->stride[2] && rec->stride[1] == rec->stride[2], "alf_stats_picture: Cb and Cr strides must match");
  hipStream_t st = (hipStream_t)stream;
  const int wCtu = cdiv(width, ctu_size), hCtu = cdiv(height, ctu_size), nCtu = wCtu * hCtu;
  unsigned long long* o7 = reinterpret_cast<unsigned long long*>(out7);
  unsigned long long* ocb = reinterpret_cast<unsigned long long*>(out_cb);
  unsigned long long* ocr = reinterpret_cast<unsigned long long*>(out_cr);
  // The classifier inside the CTU workgroups lengthens every workgroup's chain of phases by ~4 us and saves the classifier's launch (~9.5 us at 4K, ~3 us
  // at 1080p): it pays when the CTUs fill the machine about twice (510 CTUs at 4K: 67.5 -> 59.4 us), not for a 1080p picture's 135 CTUs (54.6 -> 61.4 us)
  if (cls_out && nCtu < ALF_CLS_OWN_LAUNCH_CTUS)
  {
    const int rt = vvcgpu_alf_classify(rec->p[0], rec->stride[0], width, height, bit_depth, cls_out, stream);
    if (rt) return rt;
    cls = cls_out; cls_out = nullptr;
  }
  if (ctu_size == 128 || ctu_size == 64)
  {
    // CTU form: one launch, every record written by the workgroup that owns the CTU
    AlfStatsPic a;
    for (int c = 0; c < 3; c++) { a.org[c] = org->p[c]; a.rec[c] = rec->p[c]; a.ostride[c] = org->stride[c]; a.rstride[c] = rec->stride[c]; }
    a.w = width; a.h = height; a.wCtu = wCtu; a.nCtu = nCtu; a.cls = cls; a.clsOut = cls_out; a.clsShift = bit_depth + 4; a.xcd = vvc_xcd_on();
    a.out7 = o7; a.out5 = reinterpret_cast<unsigned long long*>(out5); a.outC[0] = ocb; a.outC[1] = ocr;
    auto launch = [&](auto kernel, int ldsBytes) -> int
    {
      VVC_HIP(vvc_allow_lds(kernel, ldsBytes));
      hipLaunchKernelGGL(kernel, dim3(vvc_xcd_grid(nCtu, a.xcd)), dim3(ACT), ldsBytes, st, a);
      return VVCGPU_OK;
    };
    int rt;
    if (ctu_size == 128) rt = cls_out ? launch(alf_stats_picture_kernel<128, true>, AlfCtuLds<128>::bytes) : launch(alf_stats_picture_kernel<128, false>, AlfCtuLds<128>::bytes);
    else                 rt = cls_out ? launch(alf_stats_picture_kernel<64, true>, AlfCtuLds<64>::bytes) : launch(alf_stats_picture_kernel<64, false>, AlfCtuLds<64>::bytes);
    if (rt) return rt;
    VVC_LAUNCH_CHECK();
    return VVCGPU_OK;
  }
  if (cls_out)                                                              // other CTU sizes: the classifier's own launch in front of the tile form
  {
    const int rt = vvcgpu_alf_classify(rec->p[0], rec->stride[0], width, height, bit_depth, cls_out, stream);
    if (rt) return rt;
    cls = cls_out;
  }
  hipLaunchKernelGGL(zero3_kernel, dim3(512), dim3(256), 0, st, o7, (size_t)nCtu * ALF_CLASSES * ALF_REC7, ocb, (size_t)nCtu * ALF_REC5, ocr, (size_t)nCtu * ALF_REC5);
  hipLaunchKernelGGL(alf_stats_kernel<true>, dim3(cdiv(width, AT), cdiv(height, AT)), dim3(256), 0, st, org->p[0], org->stride[0], rec->p[0], rec->stride[0],
                     width, height, ctu_size, wCtu, cls, ALF_CLASSES, o7);
  hipLaunchKernelGGL(alf_stats_chroma2_kernel, dim3(cdiv(width >> 1, AT), cdiv(height >> 1, AT), 2), dim3(256), 0, st, org->p[1], org->p[2], org->stride[1],
                     rec->p[1], rec->p[2], rec->stride[1], width >> 1, height >> 1, ctu_size >> 1, wCtu, ocb, ocr);
  hipLaunchKernelGGL(alf_stats_5from7_kernel, dim3(cdiv(nCtu * ALF_CLASSES * ALF_REC5, 256)), dim3(256), 0, st, o7, reinterpret_cast<unsigned long long*>(out5), nCtu * ALF_CLASSES);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}

extern "C" {

int vvcgpu_alf_stats_picture(const vvcgpu_planes* org, const vvcgpu_planes* rec, int width, int height, int ctu_size, const uint16_t* cls,
                             int64_t* out7, int64_t* out5, int64_t* out_cb, int64_t* out_cr, void* stream)
{
  VVC_CHECK_ARG(cls, "alf_stats_picture: null pointer");
  return alf_stats_picture_impl(org, rec, width, height, ctu_size, cls, nullptr, 10, out7, out5, out_cb, out_cr, stream);
}

int vvcgpu_alf_classify_stats_picture(const vvcgpu_planes* org, const vvcgpu_planes* rec, int width, int height, int ctu_size, int bit_depth,
                                      uint16_t* cls_out, int64_t* out7, int64_t* out5, int64_t* out_cb, int64_t* out_cr, void* stream)
{
  VVC_CHECK_ARG(cls_out, "alf_classify_stats_picture: null pointer");
  VVC_CHECK_ARG(bit_depth >= 8 && bit_depth <= 10, "alf_classify_stats_picture: bit depth %d outside 8..10", bit_depth);
  return alf_stats_picture_impl(org, rec, width, height, ctu_size, nullptr, cls_out, bit_depth, out7, out5, out_cb, out_cr, stream);
}

}  // extern "C"
