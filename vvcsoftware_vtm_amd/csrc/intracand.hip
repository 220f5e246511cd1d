// intracand.hip -- vvcgpu_intra_mode_cand_batch: the mode pre-selection pass of the intra luma search for a list of independent PUs, in one launch.
//
// Reference behaviour reproduced (bit-exact, the doubles included):
//   IntraSearch::estIntraPredLumaQT, the two SATD rounds, the MPM append and the PBINTRA cut   EncoderLib/IntraSearch.cpp:405-522, 591-618
//   IntraPrediction::useFilteredIntraRefSamples(.., modeSpecific = true, ..)                   CommonLib/IntraPrediction.cpp:1107-1139
//   initIntraPatternChType(.., true): xFillReferenceSamples, xFilterReferenceSamples          :807-1004, :1071-1104 (through intra_dev.h)
//   predIntraAng :251-347 (through intra_dev.h), RdCost::xGetHADs (through dist_dev.h)
//   updateCandList                                                                             CommonLib/UnitTools.h:190-223
//
// Design (docs/KERNELS.md, "The intra mode pre-selection pass"): one owner per PU under the model of owner_dev.h, a wavefront for a PU of at most 256
// samples, a workgroup for a larger one.  The owner checks the PU against the contract, gathers (or loads) the packed references once, stages BOTH
// reference chains (unfiltered, filtered) and the original block in its LDS, and then evaluates a round's modes: each mode is its projection, its
// samples into an LDS tile and the Hadamard of (LDS original, LDS tile).  Blocks of 16 or 32 samples run four or two modes side by side in a wavefront
// (intra_pred_samples<G>, satd_tiles<.., G>); the four wavefronts of a workgroup owner take a round's modes in turn up to 1024 samples, and share
// every mode by quarters of the rows above (32x64, 64x32, 64x64: one tile instead of four keeps the launch's LDS at 21 KB per workgroup).  The SATDs
// land in an LDS table in any order; one lane then replays the updateCandList calls in the reference's visiting order, builds the second round's
// list under the bSatdChecked guard, and after it appends the MPMs and applies the PBINTRA cut.
#include "common.h"
#include "dist_dev.h"
#include "intra_dev.h"
#include "owner_dev.h"
#include "pu_entry_host.h"

static_assert(sizeof(vvcgpu_intra_satd_desc) == 32 && sizeof(vvcgpu_intra_fill_desc) == 40, "descriptor layouts");

namespace {

constexpr int IC_WAVE_MAX = 256;                                          // samples of the largest PU a wavefront owns
constexpr int IC_MODES_ABREAST_MAX = 1024;                                // samples of the largest PU whose workgroup owner gives every wavefront a mode of its own
constexpr int IC_MODES = 67, IC_ROUND1 = 35, IC_RD_MAX = 8, IC_HAD = 3;   // NUM_LUMA_MODE; planar, DC, the even angular modes; numModesForFullRD; uiHadModeList
constexpr int IC_LIST_INTS = 16, IC_COST_DOUBLES = 12;                    // a PU's row of list_out / cost_out
constexpr int IC_SMALL_MAIN = 56, IC_SMALL_NEG = 16;                      // a side-by-side group's share of the wavefront's main reference buffer
static_assert(4 * IC_SMALL_MAIN <= NEG_MAX + REF_MAX && IC_SMALL_NEG >= 8 && IC_SMALL_MAIN - IC_SMALL_NEG >= 8 + 3, "blocks with sides of at most 8");

typedef const __attribute__((address_space(3))) short* IcLdsPel;

// what the owner keeps besides samples
struct __align__(16) IcState
{
  unsigned long long satd[IC_MODES];                                      // uiSad of every evaluated mode, ~0 elsewhere
  double rdCost[IC_RD_MAX], hadCost[IC_HAD];                              // CandCostList, CandHadList
  double outCost[IC_COST_DOUBLES];
  int rdMode[IC_RD_MAX + 3], hadMode[IC_HAD];                             // uiRdModeList (with room for the appended MPMs), uiHadModeList
  int todo[IC_ROUND1], nTodo;                                             // the modes of the round, in visiting order
  int outList[IC_LIST_INTS];
};
constexpr int IC_REF_BYTES = 4 * REF_MAX * 2, IC_PACKED_BYTES = 2 * REF_MAX * 2, IC_MAIN_BYTES = (NEG_MAX + REF_MAX) * 2;
static_assert(sizeof(IcState) % 16 == 0 && IC_MAIN_BYTES >= FILL_UNITS_MAX * 2, "the unit table of the gathering lies in the first main reference buffer");

// LDS of an owner of `lanes` lanes for a PU of w x h: state, both chains, the packed references, per wavefront a main reference buffer, the original,
// per wavefront a tile (at least 64 samples: four 4x4 blocks side by side) -- or ONE tile where the wavefronts share a mode by bands of rows
inline int ic_lds_bytes(int w, int h, int lanes)
{
  const int nw = lanes / 64, tile = w * h < 64 ? 64 : w * h, tiles = w * h > IC_MODES_ABREAST_MAX ? 1 : nw;
  return (int)sizeof(IcState) + IC_REF_BYTES + IC_PACKED_BYTES + nw * IC_MAIN_BYTES + w * h * 2 + tiles * tile * 2;
}

struct IcArgs
{
  const Pel* rec; const unsigned char* flagsBase; const vvcgpu_intra_fill_desc* fill; Pel* refs; const Pel* org;
  const vvcgpu_intra_satd_desc* pus; const int* ctl; const unsigned long long* modeBits; const unsigned long long* interHad;
  unsigned long long* satdOut; int* listOut; double* costOut;
  double sqrtLambda;
  int n, useMpm, noSmoothing, bd, cmin, cmax, waveBytes;
};

inline __host__ __device__ bool ic_side_ok(int v) { return v >= 4 && v <= 64 && (v & (v - 1)) == 0; }

// updateCandList (UnitTools.h:190-223) on lists in LDS; size: the lists' common size, at most fastNum here
__device__ __forceinline__ void ic_update_cand_list(int mode, double cost, int* modes, double* costs, int& size, int fastNum)
{
  const int cur = min(fastNum, size);
  int shift = 0;
  while (shift < fastNum && shift < cur && cost < costs[cur - 1 - shift]) shift++;
  if (size >= fastNum && shift != 0)
  {
    for (int i = 1; i < shift; i++) { modes[cur - i] = modes[cur - 1 - i]; costs[cur - i] = costs[cur - 1 - i]; }
    modes[cur - shift] = mode; costs[cur - shift] = cost;
  }
  else if (cur < fastNum)                                                 // insert at end() - shift
  {
    for (int i = size; i > size - shift; i--) { modes[i] = modes[i - 1]; costs[i] = costs[i - 1]; }
    modes[size - shift] = mode; costs[size - shift] = cost;
    size++;
  }
}

// One mode by a group of G lanes: predIntraAng from the chain the filter rule selects into the group's tile, then the Hadamard against the original.
// write: the group holds a mode of the round (an idle group walks the same code over the round's last mode and keeps its result).
template <int G>
__device__ __forceinline__ void ic_mode(const IcArgs& a, IcState* st, int w, int h, int T, int L, int mode, bool write, const short* refs4, short* mainX,
                                        const short* orgS, short* tile, int lane)
{
  const bool filt = intra_use_filtered(w, h, mode, a.noSmoothing);
  const short* top = refs4 + (filt ? 2 * REF_MAX : 0);
  intra_pred_samples<G>(w, h, mode, T, L, top, top + REF_MAX, mainX, tile, w, a.cmin, a.cmax, lane);
  wave_sync();
  unsigned long long sad;
  if (G == 64) sad = satd_block<64, IcLdsPel, IcLdsPel>((IcLdsPel)orgS, w, (IcLdsPel)tile, w, w, h, lane);
  else if (G == 16) sad = satd_tiles<4, 4, 16, IcLdsPel, IcLdsPel>((IcLdsPel)orgS, w, (IcLdsPel)tile, w, w, h, lane);    // 4x4
  else if (w > h) sad = satd_tiles<8, 4, 32, IcLdsPel, IcLdsPel>((IcLdsPel)orgS, w, (IcLdsPel)tile, w, w, h, lane);      // 8x4
  else sad = satd_tiles<4, 8, 32, IcLdsPel, IcLdsPel>((IcLdsPel)orgS, w, (IcLdsPel)tile, w, w, h, lane);                 // 4x8
  if (lane == 0 && write) st->satd[mode] = sad;
  wave_sync();                                                            // the tile and the main reference buffer are free again
}

// the modes st->todo[0 .. nTodo) of a round, in any order, into st->satd
template <int NT>
__device__ __forceinline__ void ic_round(const IcArgs& a, IcState* st, int w, int h, int T, int L, const short* refs4, short* mainBuf, const short* orgS, short* tile,
                                         int lane, int wv)
{
  constexpr int NW = NT / 64;
  const int nTodo = st->nTodo, samples = w * h;
  if (NT == 64 && samples < 64)
  {
    if (samples == 16)
      for (int k0 = 0; k0 < nTodo; k0 += 4)
      {
        const int g = lane >> 4, k = k0 + g;
        ic_mode<16>(a, st, w, h, T, L, st->todo[min(k, nTodo - 1)], k < nTodo, refs4, mainBuf + g * IC_SMALL_MAIN + IC_SMALL_NEG, orgS, tile + g * 16, lane & 15);
      }
    else
      for (int k0 = 0; k0 < nTodo; k0 += 2)
      {
        const int g = lane >> 5, k = k0 + g;
        ic_mode<32>(a, st, w, h, T, L, st->todo[min(k, nTodo - 1)], k < nTodo, refs4, mainBuf + g * IC_SMALL_MAIN + IC_SMALL_NEG, orgS, tile + g * 32, lane & 31);
      }
    return;
  }
  if (NT == 256 && samples > IC_MODES_ABREAST_MAX)
  {
    // 32x64, 64x32, 64x64: every mode by all four wavefronts, each its quarter of the rows (a multiple of the Hadamard tile's height) from projection
    // to Hadamard; the quarters' sums meet in the table (integer sums: any order)
    const int bandH = h >> 2, y0 = wv * bandH;
    for (int k = (wv << 6) + lane; k < nTodo; k += NT) st->satd[st->todo[k]] = 0ull;
    __syncthreads();
    for (int k = 0; k < nTodo; k++)
    {
      const int mode = st->todo[k];
      const short* top = refs4 + (intra_use_filtered(w, h, mode, a.noSmoothing) ? 2 * REF_MAX : 0);
      intra_pred_samples<64>(w, h, mode, T, L, top, top + REF_MAX, mainBuf + NEG_MAX, tile + y0 * w, w, a.cmin, a.cmax, lane, y0, y0 + bandH);
      wave_sync();
      const unsigned long long sad = satd_block<64, IcLdsPel, IcLdsPel>((IcLdsPel)(orgS + y0 * w), w, (IcLdsPel)(tile + y0 * w), w, w, bandH, lane, 0, h);
      if (lane == 0) atomicAdd(&st->satd[mode], sad);
      wave_sync();                                                        // the band and the main reference buffer are free again
    }
    return;
  }
  for (int k = wv; k < nTodo; k += NW) ic_mode<64>(a, st, w, h, T, L, st->todo[k], true, refs4, mainBuf + NEG_MAX, orgS, tile, lane);
}

// the updateCandList calls of the round's modes in visiting order (one lane)
__device__ __forceinline__ void ic_replay(const IcArgs& a, IcState* st, int p, int m0, int m1, int m2, int numModes, int& rdSize, int& hadSize)
{
  const unsigned long long b0 = a.modeBits[4 * (size_t)p], b1 = a.modeBits[4 * (size_t)p + 1], b2 = a.modeBits[4 * (size_t)p + 2], b3 = a.modeBits[4 * (size_t)p + 3];
  const int nTodo = st->nTodo;
  for (int k = 0; k < nTodo; k++)
  {
    const int mode = st->todo[k];
    const unsigned long long sad = st->satd[mode];
    const unsigned long long bits = mode == m0 ? b0 : mode == m1 ? b1 : mode == m2 ? b2 : b3;
    const double prod = (double)bits * a.sqrtLambda;                      // a product, then a sum (the library is built with -ffp-contract=off)
    const double cost = (double)sad + prod;
    ic_update_cand_list(mode, cost, st->rdMode, st->rdCost, rdSize, numModes);
    ic_update_cand_list(mode, (double)sad, st->hadMode, st->hadCost, hadSize, IC_HAD);
  }
}

template <int NT>
__device__ __forceinline__ void ic_pu(const IcArgs& a, int p, bool sidesOk, unsigned char* smem, int tid)
{
  constexpr int NW = NT / 64;
  const int lane = tid & 63, wv = NT == 256 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  const vvcgpu_intra_satd_desc s = a.pus[p];
  const int w = s.w, h = s.h;
  const int m0 = a.ctl[4 * (size_t)p], m1 = a.ctl[4 * (size_t)p + 1], m2 = a.ctl[4 * (size_t)p + 2], numModes = a.ctl[4 * (size_t)p + 3];

  // ---- the contract, before anything is read or written for the PU
  bool ok = sidesOk && m0 >= 0 && m0 < IC_MODES && m1 >= 0 && m1 < IC_MODES && m2 >= 0 && m2 < IC_MODES && numModes >= 1 && numModes <= IC_RD_MAX;
  vvcgpu_intra_fill_desc f;
  memset(&f, 0, sizeof(f));
  int T = 0, L = 0;
  if (ok)
  {
    intra_ref_lengths(w, h, T, L);
    if (a.fill)
    {
      f = a.fill[p];
      ok = f.w == w && f.h == h && f.ref_off == s.ref_off && f.unit_w >= 1 && f.unit_h >= 1;
      ok = ok && (T + f.unit_w - 1) / f.unit_w + (L + f.unit_h - 1) / f.unit_h + 1 <= FILL_UNITS_MAX;
    }
  }
  if (!ok)
  {
    if (a.satdOut) for (int i = tid; i < IC_MODES; i += NT) a.satdOut[IC_MODES * (size_t)p + i] = ~0ull;
    if (tid < IC_LIST_INTS) a.listOut[IC_LIST_INTS * (size_t)p + tid] = -1;
    if (tid < IC_COST_DOUBLES) a.costOut[IC_COST_DOUBLES * (size_t)p + tid] = __builtin_inf();
    return;
  }

  IcState* st = reinterpret_cast<IcState*>(smem);
  short* refs4 = reinterpret_cast<short*>(smem + sizeof(IcState));       // unfiltered top, left, filtered top, left: REF_MAX each
  short* packed = refs4 + 4 * REF_MAX;                                    // the packed references, T + L + 1 <= 2 REF_MAX
  short* mainAll = packed + 2 * REF_MAX;
  short* orgS = mainAll + NW * (NEG_MAX + REF_MAX);
  const int samples = w * h, tileShorts = samples < 64 ? 64 : samples;
  short* tile = orgS + samples + (samples > IC_MODES_ABREAST_MAX ? 0 : wv * tileShorts);     // one tile where the wavefronts share a mode
  short* mainBuf = mainAll + wv * (NEG_MAX + REF_MAX);

  // ---- once per PU: the references, both chains, the original, the round-1 list
  if (a.fill)
  {
    if (wv == 0) intra_fill_refs_block(a.rec, a.flagsBase, f, a.bd, lane, mainAll, packed);
    owner_sync<NT>();
    if (a.refs) for (int i = tid; i <= T + L; i += NT) a.refs[s.ref_off + i] = packed[i];
  }
  else
  {
    for (int i = tid; i <= T + L; i += NT) packed[i] = a.refs[s.ref_off + i];
    owner_sync<NT>();
  }
  {
    // chain position i: left[L] .. left[1], top-left, top[1] .. top[T]
    auto chain = [&](int i) { return (int)(i <= L ? (i == L ? packed[0] : packed[T + (L - i)]) : packed[i - L]); };
    for (int i = tid; i <= T + L; i += NT)
    {
      const int c = chain(i);
      if (i <= L) refs4[REF_MAX + (L - i)] = (short)c;
      if (i >= L) refs4[i - L] = (short)c;
      if (!a.noSmoothing)                                                 // xFilterReferenceSamples :1071-1104: the two ends stay
      {
        const int v = (i == 0 || i == T + L) ? c : (chain(i - 1) + 2 * c + chain(i + 1) + 2) >> 2;
        if (i <= L) refs4[3 * REF_MAX + (L - i)] = (short)v;
        if (i >= L) refs4[2 * REF_MAX + (i - L)] = (short)v;
      }
    }
  }
  {
    const Pel* org = a.org + s.org_off;
    const int log2W = ilog2(w);
    for (int i = tid; i < samples; i += NT) orgS[i] = org[(ptrdiff_t)(i >> log2W) * s.org_stride + (i & (w - 1))];
  }
  for (int i = tid; i < IC_MODES; i += NT) st->satd[i] = ~0ull;
  for (int k = tid; k < IC_ROUND1; k += NT) st->todo[k] = k < 2 ? k : 2 * (k - 1);      // :405-414: 0, 1, 2, 4, .. 66
  if (tid == 0) st->nTodo = IC_ROUND1;
  owner_sync<NT>();

  // ---- round 1 :405-446
  ic_round<NT>(a, st, w, h, T, L, refs4, mainBuf, orgS, tile, lane, wv);
  owner_sync<NT>();
  int rdSize = 0, hadSize = 0;                                            // (used by lane 0 of the owner)
  if (tid == 0)
  {
    ic_replay(a, st, p, m0, m1, m2, numModes, rdSize, hadSize);
    // round 2 :452-496: the children of the parents 3..65 in list order, -1 before +1, under the bSatdChecked guard
    unsigned long long doneLo = 0x5555555555555557ull;                    // modes 0, 1 and the even modes below 64
    unsigned doneHi = 0x5u;                                               // modes 64, 66
    int n = 0;
    for (int i = 0; i < numModes; i++)
    {
      const int parent = st->rdMode[i];
      if (parent > DC + 1 && parent < IC_MODES - 1)
        for (int sub = -1; sub <= 1; sub += 2)
        {
          const int mode = parent + sub;
          const bool done = mode < 64 ? ((doneLo >> mode) & 1ull) != 0ull : ((doneHi >> (mode - 64)) & 1u) != 0u;
          if (!done)
          {
            st->todo[n++] = mode;
            if (mode < 64) doneLo |= 1ull << mode; else doneHi |= 1u << (mode - 64);
          }
        }
    }
    st->nTodo = n;
  }
  owner_sync<NT>();
  ic_round<NT>(a, st, w, h, T, L, refs4, mainBuf, orgS, tile, lane, wv);
  owner_sync<NT>();

  // ---- the lists' tail: round 2's updates, the MPM append :499-522, the PBINTRA cut :591-618
  if (tid == 0)
  {
    ic_replay(a, st, p, m0, m1, m2, numModes, rdSize, hadSize);
    if (a.useMpm)
      for (int j = 0; j < 3; j++)
      {
        const int mpm = j == 0 ? m0 : j == 1 ? m1 : m2;
        bool included = false;
        for (int i = 0; i < rdSize; i++) included = included || st->rdMode[i] == mpm;
        if (!included) st->rdMode[rdSize++] = mpm;
      }
    int finalSize = rdSize;
    const unsigned long long interHad = a.interHad ? a.interHad[p] : ~0ull;
    if (interHad != ~0ull)
    {
      const double thr = (double)interHad * 1.1;                          // cs.interHad * PBINTRA_RATIO
      if (hadSize < 3 || st->hadCost[2] > thr) finalSize = min(finalSize, 2);
      if (hadSize < 2 || st->hadCost[1] > thr) finalSize = min(finalSize, 1);
      if (hadSize < 1 || st->hadCost[0] > thr) finalSize = 0;             // the early return
    }
    st->outList[0] = finalSize; st->outList[1] = hadSize;
    for (int i = 0; i < IC_HAD; i++) st->outList[2 + i] = i < hadSize ? st->hadMode[i] : -1;
    for (int i = 0; i < IC_RD_MAX + 3; i++) st->outList[5 + i] = i < finalSize ? st->rdMode[i] : -1;
    for (int i = 0; i < IC_RD_MAX; i++) st->outCost[i] = i < numModes ? st->rdCost[i] : __builtin_inf();
    for (int i = 0; i < IC_HAD; i++) st->outCost[IC_RD_MAX + i] = i < hadSize ? st->hadCost[i] : __builtin_inf();
    st->outCost[IC_RD_MAX + IC_HAD] = __builtin_inf();
  }
  owner_sync<NT>();
  if (a.satdOut) for (int i = tid; i < IC_MODES; i += NT) a.satdOut[IC_MODES * (size_t)p + i] = st->satd[i];
  if (tid < IC_LIST_INTS) a.listOut[IC_LIST_INTS * (size_t)p + tid] = st->outList[tid];
  if (tid < IC_COST_DOUBLES) a.costOut[IC_COST_DOUBLES * (size_t)p + tid] = st->outCost[tid];
}

__global__ __launch_bounds__(256) void intra_mode_cand_kernel(const IcArgs a)
{
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the owner split of owner_dev.h with the two kinds in the other order: the workgroup owners' PUs are the long ones of the launch, so they start first
  OwnerSlot o;
  o.waveOwner = (int)blockIdx.x >= a.n;
  o.unit = o.waveOwner ? ((int)blockIdx.x - a.n) * 4 + wave : (int)blockIdx.x;
  o.leave = o.unit >= a.n;
  if (o.leave) return;
  const vvcgpu_intra_satd_desc s = a.pus[o.unit];
  const bool sidesOk = ic_side_ok(s.w) && ic_side_ok(s.h);
  // a PU outside the served sides has no tile: the wavefront owner writes its sentinel rows
  if ((!sidesOk || s.w * s.h <= IC_WAVE_MAX) != o.waveOwner) return;
  if (o.waveOwner) ic_pu<64>(a, o.unit, sidesOk, smem + (size_t)wave * a.waveBytes, tid & 63);
  else ic_pu<256>(a, o.unit, sidesOk, smem, tid);
}

}  // namespace

extern "C" int vvcgpu_intra_mode_cand_batch(const vvc_pel* rec_base, const uint8_t* flags_base, const vvcgpu_intra_fill_desc* fill, vvc_pel* refs_base,
                                            const vvc_pel* org_base, const vvcgpu_intra_satd_desc* pus, int n, const int32_t* pu_ctl,
                                            const uint64_t* pu_mode_bits, const uint64_t* pu_inter_had, int flags, double sqrt_lambda, int bit_depth,
                                            int clp_min, int clp_max, uint64_t* satd_out, int32_t* list_out, double* cost_out, void* stream)
{
  const char* name = "intra_mode_cand_batch";
  VVC_CHECK_ARG(n >= 0, "%s: n %d", name, n);
  if (n == 0) return VVCGPU_OK;
  VVC_CHECK_ARG(org_base && pus && pu_ctl && pu_mode_bits && list_out && cost_out, "%s: null pointer", name);
  VVC_CHECK_ARG((fill != nullptr) == (rec_base != nullptr) && (fill != nullptr) == (flags_base != nullptr),
                "%s: null pointer (rec_base, flags_base and fill go together)", name);
  VVC_CHECK_ARG(fill || refs_base, "%s: null pointer (refs_base without fill)", name);
  VVC_CHECK_ARG((flags & ~(VVCGPU_INTRA_CAND_USE_MPM | VVCGPU_INTRA_CAND_NO_SMOOTHING)) == 0, "%s: unknown flags 0x%x", name, flags);
  VVC_CHECK_ARG(clp_min <= clp_max && clp_min >= -32768 && clp_max <= 32767, "%s: clip range %d..%d", name, clp_min, clp_max);
  VVC_CHECK_ARG(sqrt_lambda >= 0.0 && sqrt_lambda < 1048576.0, "%s: sqrt_lambda out of range", name);
  VVC_CHECK_ARG(((uintptr_t)pus & 15) == 0 && ((uintptr_t)fill & 15) == 0, "%s: descriptor array must be 16-byte aligned", name);
  if (bit_depth > 10 || bit_depth < 8) { vvcgpu_set_error("%s: bit depth %d outside 8..10", name, bit_depth); return VVCGPU_E_UNSUPPORTED; }
  VVC_CHECK_ARG(n < (1 << 27), "%s: n %d", name, n);
  const PuOwnerLds L = pu_owner_lds(4, 64, 64, IC_WAVE_MAX, ic_lds_bytes);
  IcArgs a;
  a.rec = rec_base; a.flagsBase = flags_base; a.fill = fill; a.refs = refs_base; a.org = org_base; a.pus = pus; a.ctl = pu_ctl;
  a.modeBits = reinterpret_cast<const unsigned long long*>(pu_mode_bits); a.interHad = reinterpret_cast<const unsigned long long*>(pu_inter_had);
  a.satdOut = reinterpret_cast<unsigned long long*>(satd_out); a.listOut = list_out; a.costOut = cost_out;
  a.sqrtLambda = sqrt_lambda;
  a.n = n; a.useMpm = (flags & VVCGPU_INTRA_CAND_USE_MPM) ? 1 : 0; a.noSmoothing = (flags & VVCGPU_INTRA_CAND_NO_SMOOTHING) ? 1 : 0;
  a.bd = bit_depth; a.cmin = clp_min; a.cmax = clp_max; a.waveBytes = L.waveBytes;
  VVC_HIP(vvc_allow_lds(intra_mode_cand_kernel, L.lds));
  hipLaunchKernelGGL(intra_mode_cand_kernel, dim3(pu_owner_grid(n, true)), dim3(256), L.lds, (hipStream_t)stream, a);
  VVC_LAUNCH_CHECK();
  return VVCGPU_OK;
}
