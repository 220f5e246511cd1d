/* vvcgpu.h -- C ABI of the MI355X-native pixel hot path for VTM (reference studied: VTM 2.1).
 *
 * This is the drop-in boundary: every entry point replaces one of the reference's function-pointer
 * table slots or picture-level methods; the reference-side binding that
 * installs them is shown in INTEGRATION.md.  Plain C: pointers, sizes, no C++ or torch types.
 *
 * Conventions
 *  - All sample pointers are DEVICE pointers (HBM) unless the parameter name ends in `_host`.
 *    `Pel` = int16_t, `TCoeff` = int32_t (reference: CommonLib/TypeDef.h:370-371).
 *  - Strides are in ELEMENTS, as in the reference's AreaBuf (CommonLib/Buffer.h:78-91).
 *  - A plane pointer addresses sample (0,0) of the valid picture; kernels that need samples outside
 *    the picture (ALF) replicate the border themselves, so no margin is required for those.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous on
 *    that stream; the caller synchronises.  Small parameter tables (`*_host`) are copied into the
 *    kernel argument block at call time and may be reused immediately.
 *  - Return value: 0 on success, negative VVCGPU_E_* otherwise; vvcgpu_last_error() gives text.
 *    The reference convention (CHECK/THROW -> Exception, TypeDef.h:1187-1208) is restored by the shim.
 *  - All entry points are re-entrant (reference may call from OpenMP jobs, EncLib.cpp:94-113).
 */
#ifndef VVCGPU_H
#define VVCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int16_t vvc_pel;
typedef int32_t vvc_coef;

#define VVCGPU_OK            0
#define VVCGPU_E_ARG        -1   /* bad argument (shape, alignment, enum) */
#define VVCGPU_E_DEVICE     -2   /* HIP runtime error */
#define VVCGPU_E_UNSUPPORTED -3  /* outside the precondition (e.g. bit depth > 10) */

/* ---- library ------------------------------------------------------------------------------- */
int         vvcgpu_version(void);                 /* ABI version, currently 1 */
const char* vvcgpu_last_error(void);              /* thread-local text of the last failure */
int         vvcgpu_device_count(void);
int         vvcgpu_set_device(int device);
/* sizeof() of the parameter structs, for binding self-checks: 0 sao_ctu, 1 deblock_cfg, 2 dist_desc, 3 search_blk,
 * 4 mvcost, 5 search_best, 6 if_desc, 7 mc_desc, 8 pelop_desc, 9 pelop_cfg, 10 tr_desc, 11 frac_blk, 12 frac_result,
 * 13 dqtr_desc, 14 afg_desc, 15 afe_desc, 16 tz_pu, 17 tz_cfg, 18 intra_desc, 19 cclm_desc, 20 intra_fill_desc, 21 imv_pu, 22 imv_result, 23 quant_desc,
 * 24 dq_rates, 25 depquant_desc, 26 rdoq_rates, 27 rdoq_desc, 28 intra_satd_desc, 29 affine_iter, 30 me_hier_cfg, 31 wp_param,
 * 32 wp_sad_cand, 33 tile_stats, 34 affine_me_item, 35 affine_me_cfg, 36 affine_me_result, 37 affine_me_step,
 * 38 bipred_me_ref, 39 bipred_me_item, 40 bipred_me_cfg, 41 bipred_me_result, 42 bipred_me_step, 44 affine_bipred_ref, 45 affine_bipred_item,
 * 46 affine_bipred_cfg, 47 affine_bipred_result, 48 affine_bipred_step, 50 unipred_me_ref, 51 unipred_me_item, 52 unipred_me_cfg,
 * 53 unipred_me_search, 54 unipred_me_result, 56 affine_unipred_ref, 57 affine_unipred_item, 58 affine_unipred_cfg, 59 affine_unipred_search,
 * 60 affine_unipred_result, 62 intra_chroma_pu, 63 inter_resi_item; -1 for unknown ids (43, 49, 55 and 61 are not assigned and stay unknown). */
int         vvcgpu_sizeof(int struct_id);

/* ---- device memory helpers for host-side callers (the reference keeps pictures in host memory; the shim stages them).
 *      2-D copies take pitches in BYTES.  All are asynchronous on `stream` except vvcgpu_stream_sync. */
int vvcgpu_malloc(void** dev_ptr, size_t bytes);
int vvcgpu_free(void* dev_ptr);
int vvcgpu_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int vvcgpu_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int vvcgpu_memcpy2d_h2d(void* dst_dev, size_t dst_pitch, const void* src_host, size_t src_pitch, size_t width_bytes,
                        size_t height, void* stream);
int vvcgpu_memcpy2d_d2h(void* dst_host, size_t dst_pitch, const void* src_dev, size_t src_pitch, size_t width_bytes,
                        size_t height, void* stream);
int vvcgpu_memcpy2d_d2d(void* dst_dev, size_t dst_pitch, const void* src_dev, size_t src_pitch, size_t width_bytes,
                        size_t height, void* stream);
int vvcgpu_stream_sync(void* stream);
/* Library-internal per-stream resources (work lists, packed search blocks, counters) are created on the first call that needs them and kept
 * for later calls on the same (device, stream).  A host that creates streams per thread / job calls vvcgpu_stream_release(stream) before it
 * destroys a stream: the call waits for the stream's queued work and frees what the library holds for it (any number of streams may come and
 * go; the stream's slot is found whichever device is current).  vvcgpu_shutdown() does the same for every stream of every device and also
 * releases the table images below (e.g. before unloading the library); whatever is needed afterwards is created again on demand.  Both return
 * VVCGPU_OK when there was nothing to free and VVCGPU_E_DEVICE when a device could not be reached (what could not be freed is kept, not leaked).
 * The scratch of a stream grows geometrically; a buffer it has outgrown is freed once the work queued up to the end of the call that outgrew it
 * has completed.
 * Threads: the entry points are re-entrant; calls on DIFFERENT streams may run at the same time from different host threads (the first calls included,
 * which create the slots and build the table images below), and so may vvcgpu_stream_release of different streams.  ONE host thread drives a stream at a
 * time (per-thread streams for concurrent callers), and that includes its release: no thread is inside an entry point on a stream while another
 * releases it.  Once vvcgpu_stream_release(stream) has returned the library holds nothing for that handle: any thread may drive it from then on (a
 * runtime that hands out streams from a pool may give the handle to another thread), its resources are created anew.  vvcgpu_shutdown() is called while
 * no other thread is inside the library.  vvcgpu_last_error() is per thread: a refused call of one thread never shows in another's text.
 * (tests/test_gpu_threads.py runs this contract with 4 and 8 threads against the oracle.) */
int vvcgpu_stream_release(void* stream);
int vvcgpu_shutdown(void);
/* Per device (and bit depth) the library keeps a few constant table images in device memory: the transform matrices (TrQuant.cpp:72-84, Rom.cpp:245-299)
 * as int32 and as the f16 image of the matrix-core kernels, the Toeplitz tap tables of the matrix-core interpolation (InterpolationFilter.cpp:59-138).
 * They are built by the FIRST call that needs them -- on the NULL stream, with a device synchronisation, under a library mutex: that call must not run
 * inside a stream capture and briefly stalls other threads' streams.  vvcgpu_warmup(bit_depth) builds them all for the current device at a time the host
 * chooses (start-up), after which no entry point synchronises the device until vvcgpu_shutdown() has released them.  Optional; idempotent. */
int vvcgpu_warmup(int bit_depth);

/* ---- A1: ALF classification  (AdaptiveLoopFilter::deriveClassification, AdaptiveLoopFilter.cpp:274-463;
 *          table slot m_deriveClassificationBlk, AdaptiveLoopFilter.h:90) -----------------------
 * src: luma plane after deblock+SAO (W x H valid samples, border replicated by the kernel exactly as
 *      ALFProcess does with extendBorderPel(3), AdaptiveLoopFilter.cpp:90-92).
 * cls: one uint16 per 4x4 luma block, row-major (H/4) x (W/4): low byte classIdx 0..24, high byte
 *      transposeIdx 0..3 (reference stores the same pair per pixel, AdaptiveLoopFilter.h:46-56).
 * W and H must be multiples of 4.                                                              */
int vvcgpu_alf_classify(const vvc_pel* src, int src_stride, int width, int height, int bit_depth,
                        uint16_t* cls, void* stream);

/* ---- A2: ALF filtering  (AdaptiveLoopFilter::ALFProcess CTU loop + filterBlk<5|7>,
 *          AdaptiveLoopFilter.cpp:68-139,465-650; table slots m_filter5x5Blk/m_filter7x7Blk) ------
 * src must not alias dst (reference filters from a copy, AdaptiveLoopFilter.cpp:87-92).
 * filter_type: 0 = 5x5 (7 coeff), 1 = 7x7 (13 coeff)  (AlfFilterType, TypeDef.h).
 * coeff_host: luma: 25 classes x 13 int16 (m_coeffFinal layout, MAX_NUM_ALF_LUMA_COEFF = 13);
 *             chroma: 7 int16.
 * ctu_enable: device array, one byte per CTU in raster order (Picture::getAlfCtuEnableFlag); CTUs with 0
 *             receive the unfiltered src samples, so dst is a complete picture (the reference's dst already
 *             holds them).  NULL = all enabled.
 * For chroma pass the chroma plane, its width/height and ctu_size = luma CTU size >> 1.          */
int vvcgpu_alf_filter_luma(const vvc_pel* src, int src_stride, vvc_pel* dst, int dst_stride,
                           int width, int height, int ctu_size, const uint16_t* cls,
                           int filter_type, const int16_t* coeff_host, const uint8_t* ctu_enable,
                           int clp_min, int clp_max, void* stream);
int vvcgpu_alf_filter_chroma(const vvc_pel* src, int src_stride, vvc_pel* dst, int dst_stride,
                             int width, int height, int ctu_size, const int16_t* coeff_host,
                             const uint8_t* ctu_enable, int clp_min, int clp_max, void* stream);

/* ---- S1: SAO apply  (SampleAdaptiveOffset::SAOProcess/offsetCTU/offsetBlock,
 *          SampleAdaptiveOffset.cpp:292-612) -----------------------------------------------------
 * One call per component.  src = deblocked plane (the reference's m_tempBuf copy), dst = recon plane;
 * samples of CTUs whose mode is OFF and samples skipped at unavailable borders are NOT written (dst is
 * expected to already hold the deblocked picture, as in the reference where dst is the source of the copy).
 * params: device array of vvcgpu_sao_ctu, one per CTU in raster order, already merge-resolved and
 *         de-quantised (xReconstructBlkSAOParams, SampleAdaptiveOffset.cpp:262-290).
 * avail bits (deriveLoopFilterBoundaryAvailibility, :685-760).                                   */
typedef struct vvcgpu_sao_ctu {
  int8_t  type;        /* -1 = off, 0 EO_0, 1 EO_90, 2 EO_135, 3 EO_45, 4 BO  (SAOModeNewTypes) */
  uint8_t avail;       /* bit0 L, 1 R, 2 A, 3 B, 4 AL, 5 AR, 6 BL, 7 BR */
  int16_t offset[32];  /* EO: offset[0..4] = classes (edgeType+2); BO: offset[band]            */
} vvcgpu_sao_ctu;
int vvcgpu_sao_apply(const vvc_pel* src, int src_stride, vvc_pel* dst, int dst_stride,
                     int width, int height, int ctu_w, int ctu_h, int bit_depth,
                     const vvcgpu_sao_ctu* params, int clp_min, int clp_max, void* stream);

/* ---- L1+L2: deblocking  (LoopFilter::loopFilterPic, LoopFilter.cpp:149-230: pass 1 all vertical edges,
 *          pass 2 all horizontal edges; xEdgeFilterLuma :543-681, xEdgeFilterChroma :684-838,
 *          xPelFilterLuma :856-916, xPelFilterChroma :928-949) -------------------------------------------
 * In place on the three reconstruction planes (4:2:0).  The CU/TU/motion walk that decides WHICH edge
 * segments are filtered and with which boundary strength (xDeblockCU :243-369, xGetBoundaryStrengthSingle
 * :419-541) stays on the host; it is handed over as maps with one entry per 4x4 luma unit, row-major
 * (height/4) x (width/4):
 *   edge_ver[u] / edge_hor[u]: the 4-sample segment on the LEFT / TOP border of unit u
 *        bits 0-1  luma   BS (0 = segment not filtered; only 8x8-grid positions may be non-zero)
 *        bits 2-3  chroma BS (chroma is filtered when it is 2 and the edge lies on the 8-sample chroma grid)
 *        bit  4    P side must not be modified (IPCM+pcm_loop_filter_disable / transquant bypass, :640-651)
 *        bit  5    Q side must not be modified
 *   qp_luma[u], qp_chroma[u]: QP of the CU covering unit u in the luma tree / chroma tree (CodingUnit::qp;
 *        identical unless the slice uses the dual tree).
 * width and height must be multiples of 8 (minimum CU size 4 with the 8x8 deblocking grid, TypeDef.h:60). */
typedef struct vvcgpu_deblock_cfg {
  int32_t bit_depth_luma, bit_depth_chroma;
  int32_t beta_offset_div2, tc_offset_div2;     /* slice deblocking offsets            */
  int32_t cb_qp_offset, cr_qp_offset;           /* PPS chroma QP offsets (:809)        */
  int32_t clp_min[3], clp_max[3];               /* ClpRng per component                */
} vvcgpu_deblock_cfg;
int vvcgpu_deblock(vvc_pel* y, int stride_y, vvc_pel* cb, vvc_pel* cr, int stride_c, int width, int height,
                   const uint8_t* edge_ver, const uint8_t* edge_hor, const int8_t* qp_luma,
                   const int8_t* qp_chroma, const vvcgpu_deblock_cfg* cfg_host, void* stream);

/* ---- S2: SAO statistics  (EncSampleAdaptiveOffset::getStatistics / getBlkStats,
 *          EncoderLib/EncSampleAdaptiveOffset.cpp:278-330, 1122-1490; isCalculatePreDeblockSamples == false,
 *          i.e. SAOLcuBoundary 0 as in all shipped cfgs) -------------------------------------------------
 * One call per component.  org = original plane, rec = deblocked plane.
 * out: per CTU (raster) 5 types x { int64 diff[32]; int64 count[32]; }  (SAOStatData, EncSampleAdaptiveOffset.h:53-80);
 *      EO classes use indices 0..4 (edgeType + 2), BO the 32 bands.  320 int64 per CTU.
 * avail: device array, one byte per CTU with the vvcgpu_sao_ctu.avail bit layout; only L (bit0), A (bit2) and
 *      AL (bit4) are read -- right/below/above-right come from the picture geometry exactly as in :300-306.
 * skip_lines_r / skip_lines_b: m_skipLinesR/B of the component (5/4 luma, 3/2 chroma; :122-128).
 * Precondition: org and rec samples within the bit depth (|org - rec| <= 1023: the per-thread accumulators pack count and sum; a band index is
 * taken modulo 32); a plane holds fewer than 2^31 samples.                                               */
int vvcgpu_sao_stats(const vvc_pel* org, int org_stride, const vvc_pel* rec, int rec_stride,
                     int width, int height, int ctu_w, int ctu_h, int bit_depth, const uint8_t* avail,
                     int skip_lines_r, int skip_lines_b, int64_t* out, void* stream);

/* ---- A3: ALF covariance statistics  (EncAdaptiveLoopFilter::deriveStatsForFiltering / getBlkStats /
 *          calcCovariance, EncoderLib/EncAdaptiveLoopFilter.cpp:1317-1515) ---------------------------------
 * One call per (component, filter shape).  rec = deblocked+SAO plane (border replicated by the kernel, :250-252),
 * org = original plane.  cls: A1 output for luma, NULL for chroma (single class).
 * filter_type 0: 5x5 (N = 7 coefficients), 1: 7x7 (N = 13).
 * out: per CTU (raster) x class (25 luma / 1 chroma): int64 E[N][N] (full symmetric), y[N], pixAcc
 *      = N*N + N + 1 values (183 / 57).  The reference accumulates the same integers into doubles
 *      (AlfCovariance, EncAdaptiveLoopFilter.h:46-52); all sums are < 2^53, so int64 is exact and
 *      order-independent.                                                                             */
int vvcgpu_alf_stats(const vvc_pel* org, int org_stride, const vvc_pel* rec, int rec_stride,
                     int width, int height, int ctu_size, const uint16_t* cls, int filter_type,
                     int64_t* out, void* stream);

/* ---- D1/D2/D3: block distortion, batched  (RdCost::m_afpDistortFunc table, RdCost.h:104; scalar bodies
 *          xGetSAD* RdCost.cpp:450-1000, xGetHADs :2855-2974 + xCalcHADs* :2205-2853, xGetSSE* :1820-2200;
 *          SIMD twins x86/RdCostX86.h:215-432, 2292-2436) ------------------------------------------------------
 * One descriptor per reference call `distFunc(DistParam)`: offsets are in elements from org_base / cur_base
 * (two device allocations, e.g. the original picture and a reference picture or a fractional-plane buffer).
 * kind 0 = SAD  (vertical subsampling: rows step 1<<sub_shift, sum <<= sub_shift, RdCost.cpp:466-492)
 *      1 = HAD  (Hadamard SATD, tile selection of xGetHADs with isQtbt = true; rectangular tiles use the
 *                reference's double arithmetic (int)(sad / sqrt(128.0) * 2), RdCost.cpp:2561,2698,2771,2850)
 *      2 = SSE  (sum of squared differences; the chroma distortion weight of getDistPart stays on the host)
 *      3 = MR-SAD  (row D4: xGetMRSAD and its size twins, RdCost.cpp:1008-1815: offset = sum(org - cur) / N over the sub-sampled
 *                block, truncating; sum |org - cur - offset| << sub_shift -- the m_afpDistortFunc[DF_MRSAD..] entries for useMR)
 *      4 = MR-HAD  (xGetMRHADs :3433-3446: kind 1 on org - Pel(meanDiff))
 * out[i] is the Distortion (uint64) of descriptor i.  Bit depth <= 10 (the reference's SIMD precondition). */
typedef struct vvcgpu_dist_desc {
  int64_t org_off, cur_off;
  int32_t org_stride, cur_stride;
  int16_t w, h;
  int16_t sub_shift;          /* SAD / MR-SAD only */
  int16_t reserved;
} vvcgpu_dist_desc;
int vvcgpu_dist_batch(int kind, const vvc_pel* org_base, const vvc_pel* cur_base, const vvcgpu_dist_desc* descs,
                      int n, int bit_depth, uint64_t* out, void* stream);

/* ---- D1 (search form): SAD surface of a block over a regular grid of integer positions
 *          (the distFunc loops of InterSearch::xPatternSearch, InterSearch.cpp:1887-1935, and of the raster stage of
 *          xTZSearch, :2159-2169, both through xTZSearchHelp/distFunc :249-343) --------------------------------
 * All blocks of one call share w, h, sub_shift and the position grid  x = dx0 + i*sx (i < nx), y = dy0 + j*sy (j < ny),
 * relative to (ref_x, ref_y) of the block.  Every probed sample must lie inside the reference plane's allocation
 * (the reference clips MVs to the padded picture, Mv.cpp:64-80).  org samples may be any int16 (bi-pred refinement
 * searches on 2*org - otherPred, InterSearch.cpp:1682-1692).
 * sad_out: nblocks x ny x nx uint32, row-major.  May be NULL when only `best` is wanted (what xPatternSearch and the raster
 *          loop of xTZSearch keep, InterSearch.cpp:1887-1935, 1979-2000): the arg-min is fused into the SAD kernels and no
 *          surface is written.  The fused arg-min packs (cost << 24 | scan index): cost < 2^40 and nx * ny < 2^24 are
 *          preconditions whenever `best` is given (motion lambda * MV bits stays below 2^20 in the reference).
 * best (optional): per block the argmin of  sad + uint64(lambda * bits(x,y))  in the reference's scan order
 *          (y outer, x inner, strict '<': InterSearch.cpp:1913-1925) with the MV-bit cost of RdCost.h:172-199.   */
typedef struct vvcgpu_search_blk { int32_t org_x, org_y, ref_x, ref_y; } vvcgpu_search_blk;
typedef struct vvcgpu_mvcost {
  double  lambda;             /* m_motionLambda                         */
  int32_t pred_hor, pred_ver; /* m_mvPredictor (after setPredictor)     */
  int32_t cost_scale;         /* m_iCostScale                           */
  int32_t imv_shift;          /* imvShift                               */
} vvcgpu_mvcost;
typedef struct vvcgpu_search_best { int32_t x, y; uint64_t cost; uint64_t sad; } vvcgpu_search_best;
int vvcgpu_sad_search(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride,
                      const vvcgpu_search_blk* blocks, int nblocks, int w, int h, int sub_shift,
                      int dx0, int dy0, int nx, int ny, int sx, int sy, uint32_t* sad_out,
                      const vvcgpu_mvcost* mvcost_host, vvcgpu_search_best* best, void* stream);

/* ---- D1 + D5, hierarchical form: the step-5 raster stage of xTZSearch (InterSearch.cpp:2159-2169) AND the +-dense_range full search of
 *          xPatternSearch (:1886-1935) for EVERY 16x16, 32x32 and 64x64 block of a regular block grid, in one launch ---------------------------
 * The blocks of a CU tree that share the displacement grid and the MV predictor: the SAD of a 32x32 / 64x64 block at a displacement is the exact
 * sum of the SADs of its 16x16 sub-blocks at that displacement (same rows under row sub-sampling), so each 16x16 SAD is computed ONCE and the
 * larger blocks are sums.  Per block the result equals vvcgpu_sad_search on that block with
 *   raster: dx0 = dy0 = -5 (raster_range / 5), nx = ny = 2 (raster_range / 5) + 1, sx = sy = 5;   dense: dx0 = dy0 = -dense_range, nx = ny = 2 dense_range + 1,
 * the same sub_shift and mvcost (cost, arg-min in visiting order, strict '<').  Sample range: org samples may be any int16, as for
 * vvcgpu_sad_search (2 org - otherPred of a bi-predictive search and beyond); reference samples are picture samples of at most 10 bits; with these the SAD
 * of a 64x64 block is at most 4096 * 33791 < 2^28 and SAD + lambda * bits stays below the 0x30000000 the raster key is built on (tested at
 * exactly these ends: tests/test_gpu_search_bounds.py).
 * Grid: 16x16 block (i, j), i < n16x, j < n16y, has its origin at (org_x + 16 i, org_y + 16 j) in the original and its zero-vector position at
 * (ref_x + 16 i, ref_y + 16 j) in the reference plane; 32x32 block (i, j) covers 16x16 blocks (2i .. 2i+1, 2j .. 2j+1), i < n16x / 2, j < n16y / 2
 * (whole blocks only), 64x64 likewise with 4.  Results: raster_best[0 / 1 / 2] = arrays of n16x n16y / (n16x/2)(n16y/2) / (n16x/4)(n16y/4) records
 * for the 16 / 32 / 64 blocks, row-major; dense_best[] likewise (NULL with dense_range 0).  Arrays of sizes that have no block may be NULL.
 * Reads of the reference plane: exactly the samples the per-size searches of the existing blocks read (window of +-5 (raster_range / 5) around
 * every block).  Preconditions of the kernel: raster_step 5, raster_range <= 99 (39 x 39 positions), dense_range <= 4, sub_shift 0 or 1, org_stride
 * even, ref_stride a multiple of 8, org 4-byte and ref 16-byte aligned, 0 <= lambda < 4e6; anything else returns VVCGPU_E_UNSUPPORTED (nothing
 * launched) and the caller takes vvcgpu_sad_search per size.                                                                                  */
typedef struct vvcgpu_me_hier_cfg {
  int32_t org_x, org_y;       /* grid origin in the original plane */
  int32_t ref_x, ref_y;       /* zero-vector position of the grid origin in the reference plane */
  int32_t n16x, n16y;         /* 16x16 blocks of the grid */
  int32_t sub_shift;          /* rows step 1 << sub_shift (DistParam::subShift) */
  int32_t raster_range;       /* iSearchRange of the raster stage */
  int32_t raster_step;        /* iRaster: 5 */
  int32_t dense_range;        /* BipredSearchRange of xPatternSearch; 0 = no dense grid */
} vvcgpu_me_hier_cfg;
int vvcgpu_me_hier_search(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_me_hier_cfg* cfg_host,
                          const vvcgpu_mvcost* mvcost_host, vvcgpu_search_best* const* raster_best, vvcgpu_search_best* const* dense_best, void* stream);

/* ---- I1: interpolation filter table slots, batched  (InterpolationFilter::m_filterHor/m_filterVer[N][isFirst][isLast]
 *          and m_filterCopy[isFirst][isLast], InterpolationFilter.h:84-86; bodies InterpolationFilter.cpp:205-379;
 *          SIMD twins x86/InterpolationFilterX86.h:195-1125) ------------------------------------------------------
 * One descriptor per reference call.  taps = 8, 4 or 2 (filter) or 0 (filterCopy, coeff ignored).  src_off addresses
 * the first OUTPUT-aligned sample exactly as the reference's `src` argument does (the kernel steps back taps/2-1). */
typedef struct vvcgpu_if_desc {
  int64_t src_off, dst_off;           /* elements from src_base / dst_base */
  int32_t src_stride, dst_stride;
  int16_t w, h;
  int8_t  taps, is_vertical, is_first, is_last;
  int16_t coeff[8];
  int16_t reserved[4];                /* sizeof == 56 */
} vvcgpu_if_desc;
int vvcgpu_if_batch(const vvc_pel* src_base, vvc_pel* dst_base, const vvcgpu_if_desc* descs, int n,
                    int bit_depth, int clp_min, int clp_max, void* stream);

/* ---- I3 (+B1): motion compensation of prediction blocks, batched  (InterPrediction::xPredInterBlk,
 *          InterPrediction.cpp:480-547, uni: rndRes = true; bi: both lists with rndRes = false followed by
 *          PelBuf::addAvg, :743-760 / Buffer.cpp:114-151).  Affine (xPredAffineBlk :550-722) is the same call with
 *          one descriptor per 4x4 (2x2 chroma) sub-block and the sub-block MVs derived on the host. -----------------
 * ref*_off: element offset (from ref0_base / ref1_base) of the block position displaced by the INTEGER part of the MV
 *           (pu pos + (mv >> shift)); frac_x/frac_y in 1/16 (luma) or 1/32 (chroma) sample units as computed at
 *           :497-504; is_luma selects the 8-tap table m_lumaFilter[16][8] or the 4-tap m_chromaFilter[32][4].
 * bi = 0: dst = clipped uni-prediction from ref0.   bi = 1: dst = addAvg(pred(ref0), pred(ref1)).
 * bi = 2: dst = the unrounded 14-bit intermediate of ref0 (what motionCompensation leaves in m_acYuvPred).
 * Reads: the rows / columns the reference's branch reads ((N - 1) extra rows only when frac_y != 0, columns likewise), as whole ALIGNED
 * 16-byte words (16x16 luma PUs on the matrix-core path, reference strides that are multiples of 8 samples) or aligned dwords (everything else)
 * -- i.e. at most SEVEN samples left of and seven samples right of them IN THE SAME ROW and inside the aligned 16-byte words that hold them (the
 * x86 filters over-read as far: picture margins cover it; a plane whose rows start 16-byte aligned is never read outside its rows).  16x16 luma
 * and 8x8 chroma PUs with bi 0 / 1 and quarter- (chroma: eighth-) sample phases take the matrix-core path (both filter passes as exact f16
 * products); other phases, bi = 2 and reference samples outside the bit depth take the packed vector path; PUs that are grids of such tiles
 * walk it tile by tile; every result is bit-equal to the reference. */
typedef struct vvcgpu_mc_desc {
  int64_t ref0_off, ref1_off, dst_off;
  int32_t ref0_stride, ref1_stride, dst_stride;
  int16_t w, h;
  int8_t  frac_x0, frac_y0, frac_x1, frac_y1;
  int8_t  is_luma, bi;
  int16_t reserved;
} vvcgpu_mc_desc;
int vvcgpu_mc_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base,
                    const vvcgpu_mc_desc* descs, int n, int bit_depth, int clp_min, int clp_max, void* stream);
/* The same call for a list that is (mostly) 16x16 luma / 8x8 chroma PUs -- a picture's PU list under the common partition, as the motion
 * compensation of a whole picture hands it over (InterPrediction::motionCompensation per PU, InterPrediction.cpp:480-547): ONE launch.  vvcgpu_mc_batch
 * runs the matrix-core kernel and, behind it, a launch of the generic kernel for every descriptor the first one left (4.9 us per 4K picture when that
 * list is empty); here a descriptor the matrix-core kernel cannot take -- another shape, phase or stride, reference samples outside the bit depth -- is
 * served by the wavefront that found it, behind its walk, through the same generic body.  Any list is valid and every result is the one
 * vvcgpu_mc_batch gives; a list of mostly other shapes is slower here (they are served by the matrix-core kernel's waves one after the other). */
int vvcgpu_mc_picture_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base,
                            const vvcgpu_mc_desc* descs, int n, int bit_depth, int clp_min, int clp_max, void* stream);
/* "predict a candidate -> distortion against the original" in one pass: the cost of an AMVP candidate (InterSearch::xGetTemplateCost,
 * EncoderLib/InterSearch.cpp:1606-1640: motionCompensation of the candidate vector, then getDistPart(DF_SAD)) and of a merge candidate
 * (EncCu::xCheckRDCostMerge2Nx2N, EncoderLib/EncCu.cpp:1565-1592: motionCompensation of the candidate, then the Hadamard distParam.distFunc).
 * Descriptors as vvcgpu_mc_batch with bi = 0 or 1, EXCEPT that dst_off / dst_stride address the ORIGINAL block in org_base and `reserved` is the
 * row sub-sampling shift of the SAD (DistParam::subShift; 0 for the other kinds).  kind: 0 SAD, 1 Hadamard (xGetHADs), 2 SSE.  out[i] = what
 * vvcgpu_mc_batch followed by vvcgpu_dist_batch(kind) returns for the pair; the prediction stays in LDS.  w, h <= 128.  The vector bits of
 * the candidates (getCostOfVectorWithPredictor) and the candidate lists stay with the caller.  Descriptors live in device memory, so the library
 * cannot validate them on the host: a descriptor outside the contract (w or h outside 1..128, bi outside 0..1) is skipped and its out[i] is the
 * sentinel ~0 (UINT64_MAX); the same sentinel convention holds for vvcgpu_intra_satd_batch (w, h outside 1..64) and for the distortion output of
 * vvcgpu_affine_me_iter_batch (w, h outside 1..128).  The descriptor array of vvcgpu_mc_batch / vvcgpu_mc_dist_batch is 16-byte aligned.       */
int vvcgpu_mc_dist_batch(int kind, const vvc_pel* ref0_base, const vvc_pel* ref1_base, const vvc_pel* org_base, const vvcgpu_mc_desc* descs, int n,
                         int bit_depth, int clp_min, int clp_max, uint64_t* out, void* stream);
/* Explicit weighted prediction of a slice's PUs (InterPrediction::xPredInterBi / motionCompensation, InterPrediction.cpp:418-477, 762-800, with
 * WeightPrediction::addWeightUni / addWeightBi, WeightPrediction.cpp:46-60, 157-300): the prediction of vvcgpu_mc_picture_batch (ONE launch, the same
 * matrix-core / generic split) with the weighted epilogue in place of rndRes / addAvg.  P = the 14-bit intermediate that bi = 2 stores
 * ((src << headRoom) - 8192 at full-sample positions, not clipped); shiftNum = max(2, 14 - bit_depth), S = shift + shiftNum, clip to [clp_min, clp_max]:
 *   bi = 0, w0 != 1 << shift   clip(((w0 (P0 + 8192) + (1 << (S - 1))) >> S) + offset)
 *   bi = 0, w0 == 1 << shift   clip((((P0 + 8192) + (1 << (shiftNum - 1))) >> shiftNum) + offset)
 *   bi = 1                     clip((w0 (P0 + 8192) + w1 (P1 + 8192) + (1 << (S - 1)) + (offset << (S - 1))) >> S)
 * Descriptors as vvcgpu_mc_batch EXCEPT: bi = 0 is weighted uni-prediction from ref0 (a PU predicted from list 1 only is passed as ref0 with list 1's
 * entry), bi = 1 weighted bi-prediction, and `reserved` is the index of the PU's entry in wp.  wp: device memory, 16-byte aligned, n_wp (1..32767)
 * entries, typically built once per slice from its (refIdx pair, component) combinations.  Like the sentinel of vvcgpu_mc_dist_batch, a descriptor
 * outside the contract is skipped and its dst left untouched: bi outside 0..1, reserved outside [0, n_wp), w or h outside 1..128, or an entry
 * outside the range a WPScalingParam takes (|w0| <= 255, |w1| <= 255 for bi = 1, 0 <= shift <= 8, |offset| <= 2^(bit_depth + 1)).  n == 0 is a
 * no-op; null pointers (ref1_base may be null for a list without bi = 1), n_wp outside 1..32767 and descriptor or table arrays that are not
 * 16-byte aligned return VVCGPU_E_ARG, a bit depth outside 8..10 VVCGPU_E_UNSUPPORTED, before any device work. */
typedef struct {                      /* WPScalingParam fields AFTER WeightPrediction::getWpScaling (WeightPrediction.cpp:77-156)       */
  int32_t w0, w1;                     /* .w of list 0 / list 1 (w1 unused when bi == 0)                                                    */
  int32_t offset;                     /* .offset: uni = iOffset * (1 << (bd - 8)); bi = o0 + o1                                            */
  int32_t shift;                      /* .shift:  uni = log2WeightDenom;            bi = log2WeightDenom + 1;  sizeof == 16               */
} vvcgpu_wp_param;
int vvcgpu_mc_wp_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base, const vvcgpu_mc_desc* descs, int n,
                       const vvcgpu_wp_param* wp, int n_wp, int bit_depth, int clp_min, int clp_max, void* stream);

/* ---- B1-B4: PelBuffer element-wise operations, batched  (g_pelBufOP table, Buffer.h:57-73: addAvg4/8, reco4/8,
 *          linTf4/8; cores Buffer.cpp:50-94; plus AreaBuf::subtract Buffer.h:321-339, removeHighFreq :389-416,
 *          copyClip Buffer.cpp:197-222) --------------------------------------------------------------------------
 * op: 0 addAvg   dst = clip((s0 + s1 + offset) >> shift)
 *     1 reco     dst = clip(s0 + s1)                      (dst may alias s0, DecCu.cpp:188)
 *     2 linTf    dst = (scale*s0 >> shift) + offset, clipped when clip != 0   (shift < 0 shifts left)
 *     3 subtract dst = s0 - s1
 *     4 removeHighFreq  dst = 2*s0 - s1, clipped when clip != 0
 *     5 copyClip dst = clip(s0)                                                                           */
typedef struct vvcgpu_pelop_desc {
  int64_t src0_off, src1_off, dst_off;
  int32_t src0_stride, src1_stride, dst_stride;
  int16_t w, h;
} vvcgpu_pelop_desc;
typedef struct vvcgpu_pelop_cfg { int32_t scale, shift, offset, clip, clp_min, clp_max; } vvcgpu_pelop_cfg;
int vvcgpu_pelop_batch(int op, const vvc_pel* src0_base, const vvc_pel* src1_base, vvc_pel* dst_base,
                       const vvcgpu_pelop_desc* descs, int n, const vvcgpu_pelop_cfg* cfg_host, void* stream);

/* ---- T1/T2/T3: 2-D separable transforms, batched  (free functions xTrMxN_EMT / xITrMxN_EMT, TrQuant.cpp:138-310, as
 *          called by TrQuant::xT / xIT :694-791 through the fastFwdTrans/fastInvTrans tables :72-84; transform skip
 *          xTransformSkip / xITransformSkip :795-847, 1112-1163) ------------------------------------------------------
 * tr_hor / tr_ver: 0 DCT-II (sizes 2..64), 1 DCT-VIII, 2 DST-VII (sizes 4..32) (TransType, TypeDef.h:402-410);
 * tr_hor = 3 selects transform skip (tr_ver ignored).  Coefficients are W x H int32, contiguous (stride W), as the
 * reference's CoeffBuf.  Zero-out as with useQTBT/m_rectTUs: columns/rows >= 32 are not computed and written as 0
 * (forward, TrQuant.cpp:157-162) / not read (inverse, :755-759).  maxLog2TrDynamicRange is 15 (no extended precision).
 * The integer matrices are the reference's run-time generated tables shipped as golden data (csrc/tr_tables.inc).   */
typedef struct vvcgpu_tr_desc {
  int64_t resi_off, coeff_off;          /* elements from resi_base (Pel) / coeff_base (TCoeff) */
  int32_t resi_stride;
  int16_t w, h;
  int8_t  tr_hor, tr_ver;
  int16_t reserved;
  int32_t reserved2;                    /* sizeof == 32 */
} vvcgpu_tr_desc;
int vvcgpu_tr_fwd_batch(const vvc_pel* resi_base, vvc_coef* coeff_base, const vvcgpu_tr_desc* descs, int n,
                        int bit_depth, void* stream);
int vvcgpu_tr_inv_batch(const vvc_coef* coeff_base, vvc_pel* resi_base, const vvcgpu_tr_desc* descs, int n,
                        int bit_depth, void* stream);
/* ---- N1 (first "next" row): de-quantisation fused with the inverse transform at the ABI
 *          (TrQuant::invTransformNxN = m_quant->dequant + xIT, TrQuant.cpp:559-571; Quant::dequant, Quant.cpp:277-428 with
 *          flat scaling; dependent quantisation DQIntern::Quantizer::dequantBlock, DepQuant.cpp:708-785) ---------------
 * One descriptor per TU; binary compatible with vvcgpu_tr_desc (level_off sits where coeff_off does).  level_base holds
 * the entropy-decoded levels, W x H int32 contiguous.  qp = QpParam::Qp of the component (bit-depth offset included).
 * dep_quant = 1 replays the 4-state machine over the diagonal 4x4-grouped scan (state transitions 32040, :782).
 * ONE launch: the de-quantiser and the inverse transform of a TU run in the same wave, the de-quantised coefficients stay in LDS.
 * coeff_out (optional, may be NULL; same offsets as level_base; the reference's m_plTempCoeff) additionally receives the de-quantised
 * coefficients.  Intermediate products are formed in 64 bits (the reference's `int` cannot overflow for levels in
 * the entropy-coding range +-32768, which is the precondition).                                                          */
typedef struct vvcgpu_dqtr_desc {
  int64_t resi_off, level_off;          /* elements from resi_base (Pel) / level_base (TCoeff) */
  int32_t resi_stride;
  int16_t w, h;
  int8_t  tr_hor, tr_ver;               /* as vvcgpu_tr_desc; tr_hor = 3: transform skip */
  int8_t  dep_quant;                    /* 0: Quant::dequant, 1: dependent quantisation */
  int8_t  reserved;
  int32_t qp;                           /* sizeof == 32 */
} vvcgpu_dqtr_desc;
int vvcgpu_dequant_tr_inv_batch(const vvc_coef* level_base, vvc_pel* resi_base, const vvcgpu_dqtr_desc* descs, int n,
                                int bit_depth, vvc_coef* coeff_out, void* stream);
/* ---- fused residual chain of one TU  (InterSearch::xEstimateInterResidualQT, EncoderLib/InterSearch.cpp:4254-4504:
 *          residual = org - pred (CodingStructure::getResiBuf / subtract, CommonLib/Buffer.h:321-339), TrQuant::transformNxN :4409
 *          = xT (TrQuant.cpp:694-739) + Quant::quant (Quant.cpp:721-834, sign bit hiding :142-273), TrQuant::invTransformNxN :4497
 *          = Quant::dequant (Quant.cpp:277-428) + xIT (TrQuant.cpp:743-791), reconstruction clip(pred + resi') (Buffer.cpp:66-79)) ----
 * What vvcgpu_pelop_batch(subtract) -> vvcgpu_tr_fwd_batch -> vvcgpu_quant_batch -> vvcgpu_dequant_tr_inv_batch -> vvcgpu_pelop_batch(reco)
 * compute for the same TUs, in ONE pass: the residual, the coefficients and the de-quantised coefficients never leave the chip; per TU the
 * levels (W x H int32 contiguous at level_off, zero outside the kept 32 x 32 low-frequency region), their absolute sum (abs_sum[i], as
 * Quant::quant's uiAbsSum) and the reconstructed samples are written once.  Bit-exact with that sequence (tests/test_gpu_resichain.py).
 * Preconditions: org / pred samples within the bit depth (|residual| <= 1023), tr_hor / tr_ver in 0..2 (transform skip and RDPCM TUs go
 * through the separate entry points), qp as vvcgpu_quant_desc.  TUs with both sides in 16 / 32 / 64 run their four 1-D stages on the matrix cores
 * (v_mfma_f32_16x16x32_f16 on exact integer limbs), one wave per TU; a 16- / 32- / 64-point side with an 8- or 4-point one as well, two or four
 * TUs packed into one multi-tile with block-diagonal short stages; 8x8 / 8x4 / 4x8 / 4x4 in lane groups; 2-wide (chroma) TUs on a generic
 * wave-per-TU path.  Results do not depend on the path.                                                                                      */
typedef struct vvcgpu_resi_chain_desc {
  int64_t org_off, pred_off, rec_off;   /* elements from org_base / pred_base / rec_base (Pel) */
  int64_t level_off;                    /* elements from level_base (TCoeff) */
  int32_t org_stride, pred_stride, rec_stride;
  int16_t w, h;                         /* 2..64, powers of two */
  int8_t  tr_hor, tr_ver;               /* 0 DCT-II, 1 DCT-VIII, 2 DST-VII */
  int8_t  intra_slice;                  /* quantiser rounding offset 171 (I slice) or 85, as vvcgpu_quant_desc */
  int8_t  sign_hiding;
  int32_t qp;                           /* QpParam::Qp of the component (bit-depth offset included) */
  int32_t reserved[2];                  /* sizeof == 64 */
} vvcgpu_resi_chain_desc;
int vvcgpu_resi_chain_batch(const vvc_pel* org_base, const vvc_pel* pred_base, vvc_pel* rec_base, vvc_coef* level_base,
                            const vvcgpu_resi_chain_desc* descs, int n, int bit_depth, int clp_min, int clp_max, uint32_t* abs_sum,
                            void* stream);
/* The same for descriptors the caller has GROUPED BY SHAPE (an encoder knows its TU shapes when it builds the list): runs_host holds n_runs triples
 * (w, h, count) -- descs[] is run 0's TUs, then run 1's, ...; every descriptor of a run has the run's w x h; a shape appears in at most one run.  The
 * library then needs no classification pass over the list (one launch fewer: 8.7 us of a 3840x2160 picture).  Same outputs, same preconditions; in
 * addition the descriptors must be valid (tr_hor / tr_ver in 0..2, DCT-II on a 64-point side): the un-grouped entry marks an invalid TU with
 * abs_sum = 0xFFFFFFFF and skips it, this one does not look.  A call that holds a shape with a side of 2 is served as vvcgpu_resi_chain_batch.     */
int vvcgpu_resi_chain_runs_batch(const vvc_pel* org_base, const vvc_pel* pred_base, vvc_pel* rec_base, vvc_coef* level_base,
                                 const vvcgpu_resi_chain_desc* descs, int n, const int32_t* runs_host, int n_runs,
                                 int bit_depth, int clp_min, int clp_max, uint32_t* abs_sum, void* stream);
/* ---- T3: residual DPCM of transform-skipped / lossless TUs  (TrQuant::applyForwardRDPCM, CommonLib/TrQuant.cpp:991-1045, with
 *          Quant::transformSkipQuantOneSample / invTrSkipDeQuantOneSample, Quant.cpp:911-1090; TrQuant::invRdpcmNxN, TrQuant.cpp:632-688).
 *          A range-extension tool (CU::isRDPCMEnabled, UnitTools.cpp:105-108): off in the shipped cfgs, here for completeness of row T3. --------
 * mode: 0 off, 1 horizontal, 2 vertical (RDPCMMode).  fwd: per sample delta = residual - reconstructed running sum of its line, level =
 * transform-skip quantiser of the delta (rounding offset 256 when mode != 0, else 171 / 85 by slice type), coefficient index reversed when
 * `rotate` (TU::isNonTransformedResidualRotated); lossless: level = delta.  abs_sum[i] = sum |level| (32-bit, as the reference's uiAbsSum).
 * inv: in place, every sample after the first of a line becomes the clipped running sum of the line.                                        */
typedef struct vvcgpu_rdpcm_desc {
  int64_t resi_off, coeff_off;          /* elements from resi_base (Pel) / coeff_base (TCoeff, W x H contiguous) */
  int32_t resi_stride;
  int16_t w, h;
  int8_t  mode, lossless, rotate, intra_slice;
  int32_t qp;                           /* QpParam::Qp */
  int32_t reserved;                     /* sizeof == 40 */
} vvcgpu_rdpcm_desc;
int vvcgpu_rdpcm_fwd_batch(const vvc_pel* resi_base, vvc_coef* coeff_base, const vvcgpu_rdpcm_desc* descs, int n, int bit_depth, uint32_t* abs_sum,
                           void* stream);
int vvcgpu_rdpcm_inv_batch(vvc_pel* resi_base, const vvcgpu_rdpcm_desc* descs, int n, void* stream);
/* ---- I3: affine sub-block motion vectors on the device  (InterPrediction::xPredAffineBlk, CommonLib/InterPrediction.cpp:550-722: the per
 *          4x4 (chroma 2x2) sub-block vector from the control-point vectors, roundAffineMv (Mv.cpp:56-61), the clip of :675-676, the split into
 *          integer position and 1/16 (chroma 1/32) phase :681-701) -------------------------------------------------------------------------
 * One vvcgpu_affine_pu per PU; the kernel writes one vvcgpu_mc_desc per sub-block (w/4 x h/4 of them, row-major, starting at first_desc), ready for
 * vvcgpu_mc_batch: the caller no longer derives sub-block vectors on the host.  Control-point vectors are in 1/16 luma sample units (Mv::setHighPrec).
 * comp 0: luma descriptors (4x4), 1: chroma descriptors (2x2, phase in 1/32).  ref_origin: position of picture sample (0,0) inside the reference
 * plane of that component (its margin), so that ref offsets address the padded plane.  bi = 1: both lists (ref0 / ref1), else list 0 only
 * (bi field of the descriptors: 1 / 0).                                                                                                     */
typedef struct vvcgpu_affine_pu {
  int32_t pos_x, pos_y;                 /* luma position of the PU */
  int16_t w, h;                         /* luma size */
  int16_t six_param, bi;
  int32_t mv[2][3][2];                  /* [list][LT, RT, LB][hor, ver] */
  int64_t dst_off;                      /* elements from dst_base of the component */
  int32_t dst_stride, first_desc;       /* sizeof == 80 */
} vvcgpu_affine_pu;
int vvcgpu_affine_subblock_descs(const vvcgpu_affine_pu* pus, int n, int comp, int pic_w, int pic_h, int max_cu_w, int max_cu_h,
                                 int ref_origin_x, int ref_origin_y, int ref0_stride, int ref1_stride, vvcgpu_mc_desc* out, void* stream);
/* The whole of xPredAffineBlk for a list of PUs in one call: vvcgpu_affine_subblock_descs into subblock_ws (n_subblocks = sum of the PUs' sub-block
 * counts, device memory the call overwrites), then their interpolation as vvcgpu_mc_batch does it -- for luma with four 4x4 sub-blocks per wavefront
 * through the packed filter code (a list of 4x4 descriptors handed to vvcgpu_mc_batch itself goes one sub-block per wavefront: 0.6 ms instead of
 * 0.15 for the 518 k sub-blocks of a 4K picture).  Arguments as the two calls it bundles; ref1_base may be NULL when no PU has bi = 1.          */
int vvcgpu_affine_pred_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, vvc_pel* dst_base, const vvcgpu_affine_pu* pus, int n, int n_subblocks,
                             vvcgpu_mc_desc* subblock_ws, int comp, int pic_w, int pic_h, int max_cu_w, int max_cu_h, int ref_origin_x, int ref_origin_y,
                             int ref0_stride, int ref1_stride, int bit_depth, int clp_min, int clp_max, void* stream);
/* ---- picture-level forms of the in-loop entry points: the three planes of a 4:2:0 picture in ONE launch each.  A chroma plane of a 4K picture is
 *          about one workgroup per CU, so a launch of its own costs its latency floor; these are also the forms a binding uses that keeps the
 *          reconstruction resident on the device across loopFilterPic -> SAOProcess -> ALFProcess (EncGOP.cpp:2122-2153, DecLib.cpp:506-533).
 * Same arithmetic and preconditions as the per-plane entry points they bundle (vvcgpu_sao_apply, vvcgpu_sao_stats, vvcgpu_alf_filter_luma /
 * _chroma, vvcgpu_alf_stats); width / height are the luma size, chroma planes are half size, ctu_size is the luma CTU size.            */
typedef struct vvcgpu_planes { vvc_pel* p[3]; int32_t stride[3]; } vvcgpu_planes;     /* Y, Cb, Cr: device pointers, strides in samples */
int vvcgpu_sao_apply_picture(const vvcgpu_planes* src, const vvcgpu_planes* dst, int width, int height, int ctu_size, int bit_depth,
                             const vvcgpu_sao_ctu* params_y, const vvcgpu_sao_ctu* params_cb, const vvcgpu_sao_ctu* params_cr,
                             int clp_min, int clp_max, void* stream);
/* out_y / out_cb / out_cr as vvcgpu_sao_stats' out (nCtu x 5 x 2 x 32 int64 each); skip lines: luma (r, b), chroma (r, b) */
int vvcgpu_sao_stats_picture(const vvcgpu_planes* org, const vvcgpu_planes* rec, int width, int height, int ctu_size, int bit_depth,
                             const uint8_t* avail, int skip_r_luma, int skip_b_luma, int skip_r_chroma, int skip_b_chroma,
                             int64_t* out_y, int64_t* out_cb, int64_t* out_cr, void* stream);
/* luma with the per-4x4 classifier and filter_type (0: 5x5, 1: 7x7), chroma always 5x5 with one filter; enable_* may be NULL (all CTUs on) */
int vvcgpu_alf_filter_picture(const vvcgpu_planes* src, const vvcgpu_planes* dst, int width, int height, int ctu_size, const uint16_t* cls,
                              int filter_type, const int16_t* luma_coeff_host, const int16_t* chroma_coeff_host, const uint8_t* enable_y,
                              const uint8_t* enable_cb, const uint8_t* enable_cr, int clp_min, int clp_max, void* stream);
/* the four covariance sets EncAdaptiveLoopFilter::deriveStatsForFiltering builds per picture (EncAdaptiveLoopFilter.cpp:1317-1392): luma 7x7
 * (out7: nCtu x 25 x 183) and luma 5x5 (out5: nCtu x 25 x 57) per class, Cb and Cr 5x5 (nCtu x 1 x 57 each).  The 5x5 diamond is a sub-diamond of
 * the 7x7 one under every transposition, so the luma 5x5 set is gathered from the 7x7 sums instead of being accumulated a second time.   */
int vvcgpu_alf_stats_picture(const vvcgpu_planes* org, const vvcgpu_planes* rec, int width, int height, int ctu_size, const uint16_t* cls,
                             int64_t* out7, int64_t* out5, int64_t* out_cb, int64_t* out_cr, void* stream);
/* The encoder's ALF front end for a picture in ONE launch: ALFProcess derives the block classes of the SAO output
 * (AdaptiveLoopFilter::deriveClassification, EncAdaptiveLoopFilter.cpp:1218-1226) and then accumulates the covariances over them
 * (deriveStatsForFiltering, :1317-1392).  cls_out (one uint16 per 4x4 luma block, as vvcgpu_alf_classify writes it) is an OUTPUT here:
 * the CTU workgroups of vvcgpu_alf_stats_picture classify their blocks from the tile they hold anyway.  Results are those of
 * vvcgpu_alf_classify followed by vvcgpu_alf_stats_picture, bit for bit (CTU sizes other than 64 / 128 and pictures of fewer than 320 CTUs --
 * where a classifier launch of its own is the faster form -- run exactly these two).  */
int vvcgpu_alf_classify_stats_picture(const vvcgpu_planes* org, const vvcgpu_planes* rec, int width, int height, int ctu_size, int bit_depth,
                                      uint16_t* cls_out, int64_t* out7, int64_t* out5, int64_t* out_cb, int64_t* out_cr, void* stream);
/* ---- what EncAdaptiveLoopFilter::alfEncoder (EncAdaptiveLoopFilter.cpp:333-461) reads of the per-CTU records, so that they never leave the device:
 * the frame sums (48 KB per set) and two doubles per CTU are all a binding downloads per decision round.
 * vvcgpu_alf_frame_stats = getFrameStat (:1303-1315): frame_out[class][val] (+)= the sum over the CTUs whose enable byte is not 0.
 *   ctu_stats: device array n_ctu x n_classes x n_vals exactly as the statistics entries above write it; n_classes 25 or 1, n_vals 183 or 57.
 *   enable: device array, one byte per CTU (the array vvcgpu_alf_filter_picture takes), NULL = every CTU is on; a disabled CTU's record is not read.
 *   frame_out: device array n_classes x n_vals; accumulate == 0 overwrites it, != 0 adds to it -- the chroma frame record of getFrameStats
 *   (:1285-1301) is the Cb call followed by the Cr call with accumulate = 1 (:1298-1299).
 *   Arithmetic is int64 (integer atomics: the result does not depend on scheduling).  As for vvcgpu_alf_stats this equals the reference's double
 *   accumulation as long as every sum stays below 2^53 in magnitude: then int64 is exact and order-independent.
 *   n_ctu == 0 returns VVCGPU_OK and writes nothing.                                                                                              */
int vvcgpu_alf_frame_stats(const int64_t* ctu_stats, int n_ctu, int n_classes, int n_vals, const uint8_t* enable, int accumulate,
                           int64_t* frame_out, void* stream);
/* vvcgpu_alf_ctu_dist = the two per-CTU distortions of deriveCtbAlfEnableFlags (:272-331): dist_out[i][0] = getUnfilteredDistortion(cov, numClasses)
 *   (:618-626, the sum of pixAcc in class order), dist_out[i][1] = getFilteredDistortion (:628-639): calcErrorForCoeffs (:1157-1174) of every class
 *   record under the quantised filter its class is assigned, summed in class order.  Both are the reference's doubles BIT FOR BIT: IEEE double
 *   arithmetic in the reference's order, no contraction.
 *   filter_type 0: N = 7, 1: N = 13 (a class record is N*N + N + 1 values); coeff_set_host: n_filters x N quantised coefficients (m_filterCoeffSet),
 *   1 <= n_filters <= 25; filter_idx_host: n_classes entries in 0 .. n_filters - 1 (the row of m_filterIndices in use; NULL with n_classes == 1 =
 *   filter 0); coeff_bits: m_NUM_BITS (10 in the reference; 2..16), factor = 1 << (coeff_bits - 1).  Both host tables travel in the kernel argument:
 *   no copy, no synchronisation.  dist_out: device array n_ctu x 2 doubles.
 *   Precondition: every record value is below 2^53 in magnitude, so that its conversion to double is exact.                                     */
int vvcgpu_alf_ctu_dist(const int64_t* ctu_stats, int n_ctu, int n_classes, int filter_type, const int32_t* coeff_set_host, int n_filters,
                        const int16_t* filter_idx_host, int coeff_bits, double* dist_out, void* stream);
/* The coefficient scan the library replays (host copy, out[scanIdx] = raster position; w, h in 2..64 powers of two). */
int vvcgpu_scan_order_host(int w, int h, uint16_t* out);
/* ---- N3 ("next" row): affine gradient search kernels  (AffineGradientSearch table slots m_HorizontalSobelFilter /
 *          m_VerticalSobelFilter / m_EqualCoeffComputer, AffineGradientSearch.h:50-54; bodies AffineGradientSearch.cpp:66-174;
 *          called per iteration of xAffineMotionEstimation, InterSearch.cpp:3456-3534) --------------------------------
 * sobel: deriv = 3x3 Sobel response of the W x H prediction block (horizontal: [-1 0 1; -2 0 2; -1 0 1], vertical its
 *        transpose); the outermost ring repeats the nearest interior value (:83-96, :116-129).  w, h >= 3.
 * equal_coeff: out[col+1][row] = sum iC[col]*iC[row], out[col+1][P] = sum (iC[col]*resi) << 3 over the block, P = 4 or 6
 *        parameters, iC built from the two derivative planes and the sample position (:139-157); out is n x 7 x 7 int64
 *        (row 0 and unused columns are written as 0; the reference ACCUMULATES into a zeroed matrix, the caller adds).
 *        The residue is indexed with the DERIVATIVE stride, as the reference does (:144 uses `idx` for both).           */
typedef struct vvcgpu_afg_desc {
  int64_t pred_off, deriv_off;          /* elements from pred_base (Pel) / deriv_base (int32) */
  int32_t pred_stride, deriv_stride;
  int16_t w, h;
  int32_t reserved;                     /* sizeof == 32 */
} vvcgpu_afg_desc;
int vvcgpu_affine_sobel_batch(int vertical, const vvc_pel* pred_base, int32_t* deriv_base, const vvcgpu_afg_desc* descs, int n,
                              void* stream);
typedef struct vvcgpu_afe_desc {
  int64_t resi_off, deriv_off;          /* elements from resi_base (Pel) / derivx_base, derivy_base (int32, same offset) */
  int32_t deriv_stride;                 /* also the stride of the residue block */
  int16_t w, h;
  int32_t six_param;                    /* 0: 4-parameter model, 1: 6-parameter model */
  int32_t reserved;                     /* sizeof == 32 */
} vvcgpu_afe_desc;
int vvcgpu_affine_equal_coeff_batch(const vvc_pel* resi_base, const int32_t* derivx_base, const int32_t* derivy_base,
                                    const vvcgpu_afe_desc* descs, int n, int64_t* out, void* stream);

/* One iteration of the affine gradient search behind its prediction (the loop body of InterSearch::xAffineMotionEstimation, InterSearch.cpp:3456-3534:
 * xPredAffineBlk with the current control-point vectors, error = org - pred, the two Sobel planes, the normal-equation sums, and the distortion of
 * that prediction for the cost check) in one call: sub-block vectors (as vvcgpu_affine_subblock_descs, luma, list 0 only: pu.bi must be 0), the
 * sub-block prediction (as vvcgpu_mc_batch, left in pred_base at pu.dst_off / pu.dst_stride), then ONE pass over the PU that writes neither a
 * residue nor a derivative plane.  PUs: both sides 16..128 (AFFINE_MIN_BLOCK_SIZE sub-blocks of 4x4).  For a bi-predictive search org_base holds the
 * caller's "2 org - other prediction" block, as in the reference.  pu.first_desc: index of the PU's first sub-block in subblock_ws (n_subblocks
 * entries = sum of (w / 4) (h / 4), device memory the call may overwrite).  coeff_out: n x 7 x 7 int64 as vvcgpu_affine_equal_coeff_batch;
 * dist_out (may be NULL): n x uint64, dist_kind 0 SAD / 1 Hadamard (what xAffineMotionEstimation's cost uses) of org against the prediction.
 * The caller solves the 4 x 4 / 6 x 6 system and updates the vectors on the host (double arithmetic, InterSearch.cpp:3536-3600);
 * vvcgpu_affine_me_batch below runs the whole loop on the device.                                                                                 */
typedef struct vvcgpu_affine_iter {
  vvcgpu_affine_pu pu;
  int64_t org_off;                      /* elements from org_base */
  int32_t org_stride, reserved;         /* sizeof == 96 */
} vvcgpu_affine_iter;
int vvcgpu_affine_me_iter_batch(const vvc_pel* org_base, const vvc_pel* ref_base, vvc_pel* pred_base, const vvcgpu_affine_iter* items, int n,
                                int n_subblocks, vvcgpu_mc_desc* subblock_ws, int dist_kind, int pic_w, int pic_h, int max_cu_w, int max_cu_h,
                                int ref_origin_x, int ref_origin_y, int ref_stride, int bit_depth, int clp_min, int clp_max, int64_t* coeff_out,
                                uint64_t* dist_out, void* stream);

/* The WHOLE affine gradient search of a PU against one reference picture (InterSearch::xAffineMotionEstimation, InterSearch.cpp:3286-3743; solveEqual
 * :3102-3179; clipMv Mv.cpp:64-80; Mv::roundMV2SignalPrecision Mv.h:242-247; RdCost::getBitsOfVectorWithPredictor / getCost RdCost.h:172-199) for a list
 * of independent searches in ONE launch with no host synchronisation inside: the owner of a PU (a wavefront up to 1024 samples, a workgroup above)
 * carries it from the start vectors through every iteration -- sub-block vectors, 4x4 sub-block prediction (kept in LDS, never written out), error,
 * Sobel and equation sums, the 4 x 4 / 6 x 6 solve in IEEE double arithmetic (the double -> int conversions give what x86 cvttsd2si gives: truncation,
 * 0x80000000 for NaN or out of range), vector update, Hadamard cost, vector bits, keep-if-strictly-better -- to the reference's termination rule.
 * Every result is the one the reference computes.  Start (:3362-3415): the start vectors are clipped, predicted and costed as step 0.
 * items, results, trace: device memory.  The library cannot validate device-resident items on the host: an item outside the contract (a side outside
 * 16..128 or no multiple of 4, pu.bi != 0) is skipped and gets cost = ~0 (UINT64_MAX), steps = 0 and zero vectors / bits (the sentinel convention of
 * vvcgpu_mc_dist_batch).  n == 0 is a no-op; null pointers (trace may be NULL), non-positive picture / CTU sizes or ref_stride, clp_min > clp_max and a
 * lambda outside [0, 2^20) return VVCGPU_E_ARG, a bit depth outside 8..10 VVCGPU_E_UNSUPPORTED, before any device work.  Reference samples: the
 * contract of vvcgpu_affine_me_iter_batch (sub-block vectors are clipped to the picture + 8 samples / - CTU - 8 samples; the 8-tap window reaches 4
 * samples further, so a margin of max_cu + 12 readable samples around the picture serves every search).                                          */
#define VVCGPU_AFFINE_ME_MAX_STEPS 8    /* the start vectors + at most 7 iterations */
typedef struct {                        /* one (PU, reference picture) search               sizeof == 128 */
  vvcgpu_affine_pu pu;    /* pos_x/pos_y = pu.cu->lumaPos(), w, h (16..128, multiples of 4), six_param = cu->affineType; bi must be 0;
                             mv[0][k] = acMv[k] on entry in 1/16 sample units (after Mv::setHighPrec); mv[1], dst_off, dst_stride, first_desc: 0 */
  int64_t  org_off;       /* elements from org_base; for a bi-predictive search the caller's "2 org - other prediction" block, any int16 */
  int32_t  org_stride;
  int32_t  half_weight;   /* bBi: cost weight 0.5 and the shorter iteration limits */
  int32_t  mvp[3][2];     /* acMvPred[k] in 1/16 units (setHighPrec applied by the caller; exact for a low-precision predictor) */
  uint32_t bits;          /* ruiBits on entry */
  int32_t  reserved;
} vvcgpu_affine_me_item;
typedef struct {                        /* host struct                                      sizeof == 64 */
  double  lambda;         /* RdCost::m_motionLambda */
  int32_t pic_w, pic_h, max_cu_w, max_cu_h;        /* clipMv, sub-block vector clip */
  int32_t ref_origin_x, ref_origin_y, ref_stride;  /* as vvcgpu_affine_me_iter_batch */
  int32_t bit_depth, clp_min, clp_max;
  int32_t affine_type;    /* sps.getSpsNext().getUseAffineType(): iteration limits 3/4 (6-param), 3/5 (4-param) for bi/uni; 0: 5/7 */
  int32_t reserved[3];
} vvcgpu_affine_me_cfg;
typedef struct {                        /* sizeof == 40 */
  int32_t  mv[3][2];      /* acMv on return (1/16 units); mv[2] of a 4-parameter search = the input, untouched */
  uint32_t bits;          /* ruiBits on return */
  uint32_t steps;         /* predictions evaluated: 1 + iterations that reached the second xPredAffineBlk */
  uint64_t cost;          /* ruiCost */
} vvcgpu_affine_me_result;
typedef struct { int32_t mv[3][2]; uint64_t cost; } vvcgpu_affine_me_step;   /* sizeof == 32 */
/* trace (may be NULL): n x VVCGPU_AFFINE_ME_MAX_STEPS entries, entry s of a search = the vectors and the cost of its evaluated prediction s, unused
 * entries zero. */
int vvcgpu_affine_me_batch(const vvc_pel* org_base, const vvc_pel* ref_base, const vvcgpu_affine_me_item* items, int n,
                           const vvcgpu_affine_me_cfg* cfg_host, vvcgpu_affine_me_result* results, vvcgpu_affine_me_step* trace, void* stream);

/* The WHOLE bi-predictive refinement of a PU (the loop of InterSearch::predInterSearch, InterSearch.cpp:1058-1164, with every
 * xMotionEstimation(..., bBi = true) :1668-1816 and xCheckBestMVP :1537-1603 inside it) for a list of independent PUs in ONE launch with no host
 * synchronisation inside.  The owner of a PU (a wavefront up to 1024 samples, a workgroup above) carries it through every dependent step; per iteration
 * and reference index, in the reference's order:
 *   other prediction  luma motionCompensation of the other list's current vector (xPredInterUni: clipMv, 8-tap DCTIF, rounded and clipped -- the uni
 *                     form of vvcgpu_mc_batch), formed when the iteration starts (the reference forms it at :1077-1084 and again after each accepted
 *                     improvement, :1130-1138; an iteration only ever reads the prediction of the OTHER list's current vector, so both give the same);
 *   search key        2 org - otherPred, clipped when clip_for_bipred_me (Buffer.h:389-416; op 4 of vvcgpu_pelop_batch); it lives in LDS;
 *   xSetSearchRange   (:1820-1854) around the entry vector cMvTemp[list][ref]: clipMv, +-bipred_search_range, clipMv of both corners, divideByPowerOf2;
 *   xPatternSearch    (:1887-1941) SAD with the item's sub_shift, vector cost at scale 2 against cMvPredBi[list][ref], y outer, x inner, strict '<';
 *   xPatternSearchFracDIF   half then quarter stage, Hadamard when use_hadamard: exactly vvcgpu_frac_refine;
 *   cost              vector (int << 2) + (half << 1) + qter; uiMvBits at scale 0; ruiBits += uiMvBits;
 *                     ruiCost = (uint64)(floor(0.5 ((double)cost - (double)getCost(uiMvBits))) + (double)getCost(ruiBits)), getCost(b) = (uint64)(lambda b);
 *   xCheckBestMVP     over the candidates of that (list, ref); then keep-if-strictly-better against uiCostBi (:1119-1139), which starts at UINT64_MAX.
 * After a pass without change (:1142-1163) the two closing xCheckBestMVP calls are made when uiCostBi <= uiCost[0] && uiCostBi <= uiCost[1].  The
 * reference hands them amvp[eRefPicList] -- the candidate set last copied for the list of the CURRENT iteration, not that of the list being checked --
 * and so does this.  An item on which the reference's own CHECK in xCheckBestMVP throws ("Invalid MV prediction candidate") is outside the contract:
 * the device ignores the CHECK, does not fault, and the result is unspecified.
 * Loop control (host cfg): num_iter 4 or 1 (iNumIter); pick_list_by_cost (FASTINTERSEARCH_MODE1/2, :1062-1072); mvd_l1_zero: list 1 is fixed and list 0
 * searched -- the caller has done :1009-1023 and passes ref_idx[1] = bestBiPRefIdxL1, that record's mvp_idx = bestBiPMvpL1 and mv[1] = the candidate;
 * the device derives uiMotBits[1] by :1024-1036 and forms the list-1 prediction like any other.  Not served: weighted prediction, composite reference.
 * AMVR passes (cfg.imv = cu.imv of every PU of the call, 1: integer-sample, 2: four-sample vectors; the encoder runs one pass per value,
 * EncCu::xCheckRDCostInterIMV): with imvShift = imv << 1, xPatternSearch takes its vector bits with >> imvShift (:1913); xPatternSearchIntRefine
 * (:2408-2500) replaces xPatternSearchFracDIF and the cost line: the integer vector and its 8 neighbours at 1 << imvShift quarter units, each against
 * every candidate i < num_cand at test_i = testPos (1 << imvShift) + roundMV(mv - cand_i, imvShift) + cand_i, the full block at clipMv(test_i) >> 2 (no
 * interpolation, no row sub-sampling), SATD when use_hadamard else SAD, (uint64)(0.5 d) + getCost(vector bits), strict '<' in the reference's visiting
 * order; the step's vector, predictor index, predictor, bits (the vector bits counted twice, :2494-2497) and cost are as the refinement leaves them;
 * xCheckBestMVP returns at once (:1543-1546), per step and in the closing calls (result.closing still reports that the condition of :1142-1163 held).
 * Contract of an AMVR pass: every candidate vector of every (list, reference) is a multiple of 1 << imvShift quarter units (PU::fillMvpCand rounds
 * them), and item.mv / ref[][].mv on entry are results of a pass with the same imv, hence aligned.  The reference's own CHECKs (:2437-2438: integer-sample
 * differences to BOTH candidates) throw otherwise; an item that breaks this is outside the contract like one that fails the CHECK of xCheckBestMVP: no
 * fault, result unspecified.  With num_cand == 1 candidate 1 is not read.  cfg.imv == 0 is the quarter-sample pass described above, bit for bit.
 * Reference planes: up to 16 luma planes of one stride; ref_planes[i] points to sample (0, 0) of picture i inside its padded allocation.  Readable
 * margin (a stated margin, as vvcgpu_affine_me_batch): vectors are clipped to the picture + 8 / - CTU - 8 samples, the block, the +-1 sample of the
 * refinement and the 8 taps reach further: max_cu + 12 readable samples around the picture on every side serve every search.
 * items, results, trace: device memory.  Items cannot be validated on the host: an item outside the contract (a side not in {4, 8, 16, 32, 64, 128} or
 * larger than the CTU or than cfg.max_pu_w / max_pu_h, a PU not inside the picture, sub_shift outside 0..1 or h >> sub_shift == 0, n_ref outside 1..4,
 * ref_idx outside the list, a plane index outside [0, n_planes), num_cand outside 1..2, mvp_idx outside the candidates, org_stride <= 0) is skipped and
 * gets cost = ~0 (UINT64_MAX) with everything else zero (the sentinel of vvcgpu_affine_me_batch); its trace entries are zero.  n == 0 is a no-op;
 * null pointers (trace may be NULL), n < 0, geometry, clp_min > clp_max, lambda outside [0, 2^20), bipred_search_range outside 1..8, num_iter other
 * than 1 or 4, imv outside 0..2, n_planes outside 1..16 and max_pu sides that are no served side return VVCGPU_E_ARG, a bit depth outside 8..10 VVCGPU_E_UNSUPPORTED,
 * before any device work. */
#define VVCGPU_BIPRED_ME_MAX_STEPS  16  /* num_iter 4 x at most 4 reference indices */
#define VVCGPU_BIPRED_ME_MAX_REFS   4
#define VVCGPU_BIPRED_ME_MAX_PLANES 16
typedef struct {                        /* one (list, reference index) of a PU                sizeof == 32 */
  int32_t plane;          /* index into cfg.ref_planes */
  int32_t mv[2];          /* cMvTemp[list][ref] on entry (quarter units): the uni-predictive result for this reference */
  int32_t mv_cand[2][2];  /* aacAMVPInfo[list][ref].mvCand[0..1] */
  int16_t num_cand;       /* .numCand: 1..2 */
  int16_t mvp_idx;        /* aaiMvpIdx[list][ref]; cMvPred[list][ref] = mv_cand[mvp_idx] */
} vvcgpu_bipred_me_ref;
typedef struct {                        /* one PU                                             sizeof == 360 */
  int32_t  pos_x, pos_y;  /* pu.cu->lumaPos() == the PU's position */
  int16_t  w, h;          /* 4, 8, 16, 32, 64 or 128 each */
  int16_t  sub_shift;     /* DistParam::subShift of the integer search: 0 or 1 */
  int16_t  reserved0;
  int64_t  org_off;       /* elements from org_base */
  int32_t  org_stride;
  int32_t  n_ref[2];      /* getNumRefIdx(list): 1..4 */
  int32_t  ref_idx[2];    /* iRefIdx[list]: the uni-predictive choice */
  int32_t  mv[2][2];      /* cMv[list] (quarter units) */
  int32_t  reserved1;
  uint64_t cost[2];       /* uiCost[0..1] */
  uint32_t bits[2];       /* uiBits[0..1] */
  uint32_t mb_bits[3];    /* uiMbBits[0..2] */
  int32_t  reserved2;
  vvcgpu_bipred_me_ref ref[2][VVCGPU_BIPRED_ME_MAX_REFS];
} vvcgpu_bipred_me_item;
typedef struct {                        /* host struct                                        sizeof == 224 */
  double  lambda;         /* RdCost::m_motionLambda */
  const vvc_pel* ref_planes[VVCGPU_BIPRED_ME_MAX_PLANES];   /* device pointers; entries from n_planes on are ignored */
  int32_t n_planes, ref_stride;
  int32_t pic_w, pic_h, max_cu_w, max_cu_h;                 /* clipMv */
  int32_t bit_depth, clp_min, clp_max;
  int32_t num_iter;             /* iNumIter: 4 or 1 */
  int32_t pick_list_by_cost;    /* FASTINTERSEARCH_MODE1/2: the list of every iteration is the one with the larger uni cost (:1062-1072) */
  int32_t mvd_l1_zero;          /* slice.getMvdL1ZeroFlag() */
  int32_t bipred_search_range;  /* m_bipredSearchRange: 1..8 */
  int32_t clip_for_bipred_me;   /* getClipForBiPredMeEnabled() */
  int32_t use_hadamard;         /* getUseHADME() (no lossless CUs) */
  uint32_t mvp_idx_cost[3];     /* m_auiMVPIdxCost[0..2][AMVP_MAX_NUM_CANDS] */
  int32_t max_pu_w, max_pu_h;   /* the caller states that no item is wider / higher (0: 128): LDS per owner is sized by it, so that small PUs keep many
                                   owners per compute unit; an item beyond it is skipped */
  int32_t imv;                  /* cu.imv of every PU of the call: 0 (quarter-sample), 1 (integer-sample) or 2 (four-sample vectors) */
  int32_t reserved;
} vvcgpu_bipred_me_cfg;
typedef struct {                        /* sizeof == 80 */
  int32_t  mv[2][2];      /* cMvBi[0..1] */
  int32_t  ref_idx[2];    /* iRefIdxBi[0..1] */
  int32_t  mvp_idx[2];    /* aaiMvpIdxBi[list][iRefIdxBi[list]] */
  int32_t  mvp[2][2];     /* cMvPredBi[list][iRefIdxBi[list]] */
  uint32_t bits;          /* uiBits[2] */
  uint32_t mot_bits[2];   /* uiMotBits[0..1] */
  uint32_t me_calls;      /* xMotionEstimation calls made */
  uint32_t closing;       /* 1: the closing xCheckBestMVP calls ran */
  uint32_t reserved;
  uint64_t cost;          /* uiCostBi; ~0 with everything else zero: item skipped */
} vvcgpu_bipred_me_result;
typedef struct {                        /* one xMotionEstimation + xCheckBestMVP              sizeof == 48 */
  int32_t  list, ref;
  int32_t  int_mv[2];     /* the integer vector xPatternSearch found */
  int32_t  mv[2];         /* cMvTemp[list][ref] after the refinement (quarter units) */
  uint32_t bits;          /* uiBitsTemp after xCheckBestMVP */
  int32_t  mvp_idx;       /* aaiMvpIdxBi[list][ref] after xCheckBestMVP */
  int32_t  accepted;      /* uiCostTemp < uiCostBi */
  int32_t  reserved;
  uint64_t cost;          /* uiCostTemp after xCheckBestMVP */
} vvcgpu_bipred_me_step;
/* trace (may be NULL): n x VVCGPU_BIPRED_ME_MAX_STEPS entries, entry s of an item = its s-th xMotionEstimation call, unused entries zero. */
int vvcgpu_bipred_me_batch(const vvc_pel* org_base, const vvcgpu_bipred_me_item* items, int n, const vvcgpu_bipred_me_cfg* cfg_host,
                           vvcgpu_bipred_me_result* results, vvcgpu_bipred_me_step* trace, void* stream);

/* The WHOLE affine bi-predictive search of a PU (the bi-predictive part of InterSearch::xPredAffineInterSearch, InterSearch.cpp:2823-2997, with every
 * xAffineMotionEstimation(..., bBi = true) :3286-3743 and xCheckBestAffineMVP :3181-3284 inside it) for a list of independent PUs in ONE launch with
 * no host synchronisation inside.  The owner of a PU (a wavefront up to 1024 samples, a workgroup above) carries it through every dependent step; per
 * iteration and reference index, in the reference's order:
 *   set-up            (:2831-2882) uiMotBits, uiBits[2]; with mvd_l1_zero list 1 is fixed: the caller passes ref_idx[1] = bestBiPRefIdxL1 and that record's
 *                     mvp_idx = bestBiPMvpL1, the device sets cMvBi[1] = cMvTemp[1][ref] = cMvPredBi[1][ref] = that candidate (:2847-2853) and derives
 *                     uiMotBits[1] by :2864-2874;
 *   list              (:2895-2928) iIter % 2, list 0 first; pick_list_by_cost: the list with the larger uni cost; mvd_l1_zero: list 0;
 *   other prediction  luma motionCompensation of an affine PU (InterPrediction::xPredInterUni, InterPrediction.cpp:377-407): the control-point vectors
 *                     PU::setAllAffineMv leaves in the corners of the motion buffer (UnitTools.cpp:2319-2330), no clipMv of them, xPredAffineBlk
 *                     (:550-722) with bi = false, rounded and clipped -- of the other list's current cMvBi at iRefIdxBi, formed when the iteration
 *                     starts (the reference forms it at :2913-2920 and again after each acceptance, :2970-2977; an iteration only ever reads the
 *                     prediction of the OTHER list, so both give the same);
 *   search key        2 org - otherPred, clipped when clip_for_bipred_me (Buffer.h:389-416; op 4 of vvcgpu_pelop_batch); it lives in LDS;
 *   per reference     skipped when only_ref says so (:2936-2941); the bits of :2944-2953; xAffineMotionEstimation(bBi = true) from cMvTemp[list][ref]
 *                     against cMvPredBi[list][ref] -- what vvcgpu_affine_me_batch does for an item with half_weight = 1, the original being the key;
 *                     xCheckBestAffineMVP over the candidates of that (list, ref): nothing when num_cand < 2, the second-predictor rule for vectors 1
 *                     and 2, uint32 bits, wrapping uint64 cost; then keep-if-strictly-better against uiCostBi (:2960-2978), which starts at UINT64_MAX.
 * After a pass without change (:2981-2995) the two closing xCheckBestAffineMVP calls are made when uiCostBi <= uiCost[0] && uiCostBi <= uiCost[1]; each
 * gets the candidate set of the list it checks (unlike the translational loop).  All vectors are in 1/16 sample units (after Mv::setHighPrec; the
 * convention of vvcgpu_affine_me_item.mvp).  The uni-predictive stage (:2651-2814) is vvcgpu_affine_unipred_me_batch, whose out-items are this
 * entry's items.  Not served: the final mode choice (:3017-3099; host), weighted prediction.
 * Reference planes and readable margin: as vvcgpu_bipred_me_batch -- ref_planes[i] points to sample (0, 0) of picture i inside its padded allocation;
 * sub-block vectors are clipped to the picture + 8 / - CTU - 8 samples and the 8 taps reach 4 further: max_cu + 12 readable samples around the picture
 * on every side serve every search.
 * items, results, trace: device memory.  Items cannot be validated on the host: an item outside the contract (a side not in {16, 32, 64, 128} or larger
 * than the CTU or than cfg.max_pu_w / max_pu_h, a PU not inside the picture, n_ref outside 1..4, ref_idx outside the list, only_ref outside -1 ..
 * n_ref - 1, a plane index outside [0, n_planes), num_cand outside 1..2, mvp_idx outside the candidates, org_stride <= 0) is skipped and gets
 * cost = ~0 (UINT64_MAX) with everything else zero; its trace entries are zero; it reads no sample.  n == 0 is a no-op; null pointers (trace may be
 * NULL), n < 0, geometry, clp_min > clp_max, lambda outside [0, 2^20), num_iter other than 1 or 4, n_planes outside 1..16 and max_pu sides that are
 * no served side return VVCGPU_E_ARG, a bit depth outside 8..10 VVCGPU_E_UNSUPPORTED, before any device work. */
#define VVCGPU_AFFINE_BIPRED_MAX_STEPS 16  /* num_iter 4 x at most 4 reference indices */
#define VVCGPU_AFFINE_BIPRED_MAX_REFS 4
typedef struct {                        /* one (list, reference index) of a PU                sizeof == 80 */
  int32_t plane;             /* index into cfg.ref_planes */
  int32_t mv[3][2];          /* cMvTemp[list][ref] on entry: the uni-predictive affine result for this reference */
  int32_t mv_cand[2][3][2];  /* aacAffineAMVPInfo[list][ref]: mvCandLT / RT / LB of candidates 0 and 1 */
  int16_t num_cand;          /* .numCand: 1..2 */
  int16_t mvp_idx;           /* aaiMvpIdx[list][ref]; cMvPred[list][ref] = mv_cand[mvp_idx] */
} vvcgpu_affine_bipred_ref;
typedef struct {                        /* one PU                                             sizeof == 784 */
  int32_t  pos_x, pos_y;     /* pu.cu->lumaPos() */
  int16_t  w, h;             /* 16, 32, 64 or 128 each */
  int16_t  six_param;        /* cu->affineType */
  int16_t  reserved0;
  int64_t  org_off;          /* elements from org_base */
  int32_t  org_stride;
  int32_t  n_ref[2];         /* getNumRefIdx(list): 1..4 */
  int32_t  ref_idx[2];       /* iRefIdx[list] */
  int32_t  mv[2][3][2];      /* aacMv[list] */
  int32_t  reserved1;
  uint64_t cost[2];          /* uiCost[0..1] */
  uint32_t bits[2];          /* uiBits[0..1] */
  uint32_t mb_bits[3];       /* uiMbBits[0..2] */
  int32_t  only_ref[2];      /* refIdx4Para[list] of a 6-parameter PU: -1 every index, r >= 0 only index r (< n_ref[list]) is searched (:2936-2941) */
  int32_t  reserved2;
  vvcgpu_affine_bipred_ref ref[2][VVCGPU_AFFINE_BIPRED_MAX_REFS];
} vvcgpu_affine_bipred_item;
typedef struct {                        /* host struct                                        sizeof == 224 */
  double  lambda;            /* RdCost::m_motionLambda */
  const vvc_pel* ref_planes[16];   /* device pointers; entries from n_planes on are ignored */
  int32_t n_planes, ref_stride;
  int32_t pic_w, pic_h, max_cu_w, max_cu_h;                 /* clipMv, sub-block vector clip */
  int32_t bit_depth, clp_min, clp_max;
  int32_t num_iter;             /* iNumIter: 4 or 1 */
  int32_t pick_list_by_cost;    /* FASTINTERSEARCH_MODE1/2 (:2896-2906) */
  int32_t mvd_l1_zero;          /* slice.getMvdL1ZeroFlag() */
  int32_t clip_for_bipred_me;   /* getClipForBiPredMeEnabled() */
  int32_t affine_type;          /* sps.getSpsNext().getUseAffineType(): iteration limit 3 per search; 0: 5 (as vvcgpu_affine_me_cfg) */
  uint32_t mvp_idx_cost[3];     /* m_auiMVPIdxCost[0..2][AMVP_MAX_NUM_CANDS] */
  int32_t max_pu_w, max_pu_h;   /* the caller states that no item is wider / higher (0: 128): LDS per owner is sized by it; an item beyond it is skipped */
  int32_t reserved[3];
} vvcgpu_affine_bipred_cfg;
typedef struct {                        /* sizeof == 144 */
  int32_t  mv[2][3][2];      /* cMvBi[0..1] */
  int32_t  ref_idx[2];       /* iRefIdxBi[0..1] */
  int32_t  mvp_idx[2];       /* aaiMvpIdxBi[list][iRefIdxBi[list]] */
  int32_t  mvp[2][3][2];     /* cMvPredBi[list][iRefIdxBi[list]] */
  uint32_t bits;             /* uiBits[2] */
  uint32_t mot_bits[2];      /* uiMotBits[0..1] */
  uint32_t me_calls;         /* xAffineMotionEstimation calls made */
  uint32_t closing;          /* 1: the closing xCheckBestAffineMVP calls ran */
  uint32_t reserved;
  uint64_t cost;             /* uiCostBi; ~0 with everything else zero: item skipped */
} vvcgpu_affine_bipred_result;
typedef struct {                        /* one xAffineMotionEstimation + xCheckBestAffineMVP  sizeof == 56 */
  int32_t  list, ref;
  int32_t  mv[3][2];         /* cMvTemp[list][ref] after the search */
  uint32_t steps;            /* predictions evaluated, as vvcgpu_affine_me_result.steps */
  uint32_t bits;             /* uiBitsTemp after xCheckBestAffineMVP */
  int32_t  mvp_idx;          /* aaiMvpIdxBi[list][ref] after xCheckBestAffineMVP */
  int32_t  accepted;         /* uiCostTemp < uiCostBi */
  uint64_t cost;             /* uiCostTemp after xCheckBestAffineMVP */
} vvcgpu_affine_bipred_step;
/* trace (may be NULL): n x VVCGPU_AFFINE_BIPRED_MAX_STEPS entries, entry s of an item = its s-th xAffineMotionEstimation call, unused entries zero. */
int vvcgpu_affine_bipred_me_batch(const vvc_pel* org_base, const vvcgpu_affine_bipred_item* items, int n, const vvcgpu_affine_bipred_cfg* cfg_host,
                                  vvcgpu_affine_bipred_result* results, vvcgpu_affine_bipred_step* trace, void* stream);

/* The WHOLE uni-predictive stage of the translational inter search of a PU (the loop of InterSearch::predInterSearch, InterSearch.cpp:877-964, with
 * xEstimateMvPredAMVP :1443-1483 / xGetTemplateCost :1606-1642, xMotionEstimation(bBi = false) :1668-1816 and xCheckBestMVP :1537-1603 inside it) for
 * a list of independent PUs of mixed sizes, with no host synchronisation inside: two launches on the stream.  The first gives every (PU, list, reference
 * index) search an owner of its own (a wavefront up to 1024 samples, a workgroup above), the second makes the per-PU decisions.  Results are bit-exact,
 * the double arithmetic of the costs included.  Per PU and per (list, reference index), in the reference's order:
 *   bits              uiBitsTemp = mb_bits[list] + the reference-index bits of :883-890 (cfg.n_ref[list]);
 *   xEstimateMvPredAMVP   with the caller's candidates (bFilled = true; PU::fillMvpCand stays on the host): per candidate clipMv, luma xPredInterBlk
 *                     (uni, rounded and clipped: the uni form of vvcgpu_mc_batch), full SAD (no row sub-sampling) + getCost(mvp_idx_cost[i]); the best by
 *                     uiBestCost > uiTmpCost in candidate order; its cost is biPDistTemp;
 *   :896-901          bestBiPDist / bestBiPMvpL1 / bestBiPRefIdxL1 when cfg.mvd_l1_zero (list 1, strict '<');
 *   xMotionEstimation (bBi = false), diamond searches only.  Normal path: rcMv = rcMvPred, xTZSearch under the contract of vvcgpu_tz_search_batch
 *                     (cost scale 2; VVCGPU_TZ_EXTENDED per item = MESEARCH_DIAMOND_ENHANCED; the 2Nx2N predictor m_integerMv2Nx2N[list][ref] per
 *                     (list, reference) when VVCGPU_UNIPRED_PRED2), xPatternSearchFracDIF under the contract of vvcgpu_frac_refine (Hadamard when
 *                     use_hadamard), then :1795-1805: vector (int << 2) + (half << 1) + qter, uiMvBits at scale 0, ruiBits += uiMvBits,
 *                     ruiCost = (uint64)(floor((double)cost - (double)getCost(uiMvBits)) + (double)getCost(ruiBits)), getCost(b) = (uint64)(lambda b).
 *                     Cached-start path (:1759-1766; VVCGPU_UNIPRED_CACHED: the block cache holds an integer vector for this (list, reference)): the
 *                     search starts from that vector with the fast settings, not the extended ones, and without the 2Nx2N predictor.  The search range
 *                     is cfg.search_range[list][ref] (m_aaiAdaptSR);
 *   xCheckBestMVP     over that (list, reference)'s candidates;
 *   list-1 shortcut   with cfg.fast_me_gen_b_low_delay and cfg.list1_to_list0[ref] >= 0 a list-1 reference takes list 0's vector instead of searching
 *                     and corrects the cost as :909-921 do (uint64 subtraction, then addition), then xCheckBestMVP;
 *   :944-962          keep-if-strictly-better per list, and the "valid list 1" record (list-1 references with list1_to_list0 < 0).
 * AMVR passes (cfg.imv = cu.imv of every PU of the call, 1: integer-sample, 2: four-sample vectors; the encoder runs one pass per value,
 * EncCu::xCheckRDCostInterIMV): with imvShift = imv << 1, xTZSearch takes its vector cost with imvShift on both paths (vvcgpu_tz_cfg.imv_shift);
 * xPatternSearchIntRefine (:2408-2500) replaces xPatternSearchFracDIF and :1795-1805, as described for vvcgpu_bipred_me_batch with weight 1.0 on the
 * original; xCheckBestMVP returns at once (:1543-1546); the list-1 shortcut takes its vector bits with >> imvShift (:916).  mv is the refined vector,
 * int_mv still the xTZSearch result, mvp_idx / bits / cost as the refinement leaves them, and the out-items carry that mvp_idx; bestBiP* still come from
 * the template costs and the mvd_l1_zero preparation is unchanged.  The affine search is skipped by the encoder when imv != 0 (:969).  Contract of an
 * AMVR pass: every candidate vector of every (list, reference) is a multiple of 1 << imvShift quarter units (PU::fillMvpCand rounds them); the
 * reference's own CHECKs (:2437-2438) throw otherwise, and an item that breaks this is outside the contract: no fault, result unspecified.  With
 * num_cand == 1 candidate 1 is not read.  cfg.imv == 0 is the quarter-sample pass described above, bit for bit.
 * Not served: weighted prediction, composite reference, MESEARCH_FULL and MESEARCH_SELECTIVE, affine.
 * bipred_items_out (may be NULL): n complete vvcgpu_bipred_me_item records, exactly what vvcgpu_bipred_me_batch asks of its caller -- n_ref, planes,
 * cMvTemp, candidates and aaiMvpIdx per (list, reference), iRefIdx, cMv, uiCost, uiBits, mb_bits -- with the mvd_l1_zero preparation of :1009-1023 and
 * :1038 done when cfg.mvd_l1_zero (ref_idx[1] = bestBiPRefIdxL1, that record's mvp_idx = bestBiPMvpL1, its mv and mv[1] = that candidate), so that
 * the buffer can be handed to vvcgpu_bipred_me_batch on the same stream as it is.  On a P slice (n_ref[1] == 0) the records carry n_ref[1] = 0, which
 * the bi-predictive entry skips.
 * Reference planes: up to 16 luma planes of one stride; ref_planes[i] points to sample (0, 0) of picture i inside its padded allocation.  Readable
 * margin (a stated margin, as vvcgpu_bipred_me_batch): max_cu + 16 readable samples around the picture on every side.  Vectors are clipped to the picture
 * + 8 / - CTU - 8 samples, and the block, the +-1 sample of the refinement and the 8 taps reach max_cu + 12 samples; the zero-neighbourhood rounds of the
 * extended TZ search probe up to search_range / 2 around the zero vector whatever the clipped range is: a probe whose block would leave the picture by
 * more than max_cu + 14 samples is clamped to that rectangle (a wrong SAD where the reference would read its own margin, never a fault).  Reference
 * rows are read as aligned dwords; reference and original samples of the integer search must be non-negative (picture samples).
 * items, results, bipred_items_out: device memory.  Items cannot be validated on the host: an item outside the contract (a side not in {4, 8, 16, 32,
 * 64, 128} or larger than the CTU or than cfg.max_pu_w / max_pu_h, a PU not inside the picture, sub_shift outside 0..1 or h >> sub_shift == 0,
 * org_stride <= 0, tz_flags other than 0 or VVCGPU_TZ_EXTENDED, and for a (list, reference) of the slice num_cand outside 1..2 or flags outside 0..3) is
 * skipped: it reads no sample, its result has cost[0] = cost[1] = ~0 (UINT64_MAX) with everything else zero, its out-item is all zero.  n == 0 is a
 * no-op; null pointers (bipred_items_out may be NULL), n < 0, geometry, clp_min > clp_max, lambda outside [0, 2^20), n_planes outside 1..16, n_ref[0]
 * outside 1..4, n_ref[1] outside 0..4, a ref_plane outside [0, n_planes), a search_range outside 1..256, a list1_to_list0 outside [-1, n_ref[0]), imv outside 0..2 and
 * max_pu sides that are no served side return VVCGPU_E_ARG, a bit depth outside 8..10 VVCGPU_E_UNSUPPORTED, before any device work. */
#define VVCGPU_UNIPRED_ME_MAX_REFS   4
#define VVCGPU_UNIPRED_ME_MAX_PLANES 16
enum { VVCGPU_UNIPRED_PRED2 = 1, VVCGPU_UNIPRED_CACHED = 2 };
typedef struct {                        /* one (list, reference index) of a PU                sizeof == 40 */
  int32_t mv_cand[2][2];  /* amvp.mvCand[0..1] (quarter units) */
  int32_t pred2[2];       /* m_integerMv2Nx2N[list][ref] (integer units), used when VVCGPU_UNIPRED_PRED2 */
  int32_t cached_mv[2];   /* the block cache's integer vector (integer units), used when VVCGPU_UNIPRED_CACHED */
  int16_t num_cand;       /* amvp.numCand: 1..2 */
  int16_t flags;          /* VVCGPU_UNIPRED_* */
  int32_t reserved;
} vvcgpu_unipred_me_ref;
typedef struct {                        /* one PU                                             sizeof == 360 */
  int32_t  pos_x, pos_y;  /* pu.cu->lumaPos() == the PU's position */
  int16_t  w, h;          /* 4, 8, 16, 32, 64 or 128 each */
  int16_t  sub_shift;     /* DistParam::subShift of the integer search: 0 or 1 */
  int16_t  tz_flags;      /* 0 or VVCGPU_TZ_EXTENDED (normal path) */
  int64_t  org_off;       /* elements from org_base */
  int32_t  org_stride;
  uint32_t mb_bits[3];    /* uiMbBits[0..2] */
  vvcgpu_unipred_me_ref ref[2][VVCGPU_UNIPRED_ME_MAX_REFS];
} vvcgpu_unipred_me_item;
typedef struct {                        /* host struct                                        sizeof == 304 */
  double  lambda;         /* RdCost::m_motionLambda */
  const vvc_pel* ref_planes[VVCGPU_UNIPRED_ME_MAX_PLANES];  /* device pointers; entries from n_planes on are ignored */
  int32_t n_planes, ref_stride;
  int32_t pic_w, pic_h, max_cu_w, max_cu_h;                 /* clipMv */
  int32_t bit_depth, clp_min, clp_max;
  int32_t n_ref[2];                                         /* slice.getNumRefIdx(list): 1..4, list 1 also 0 (P slice) */
  int32_t ref_plane[2][VVCGPU_UNIPRED_ME_MAX_REFS];         /* index into ref_planes of (list, reference index) */
  int32_t search_range[2][VVCGPU_UNIPRED_ME_MAX_REFS];      /* m_aaiAdaptSR[list][ref]: 1..256 */
  int32_t list1_to_list0[VVCGPU_UNIPRED_ME_MAX_REFS];       /* slice.getList1IdxToList0Idx(ref): -1 or a list-0 reference index */
  int32_t fast_me_gen_b_low_delay;  /* getFastMEForGenBLowDelayEnabled() */
  int32_t mvd_l1_zero;              /* slice.getMvdL1ZeroFlag() */
  int32_t first_search_stop;        /* getFastMEAssumingSmootherMVEnabled() */
  int32_t use_hadamard;             /* getUseHADME() (no lossless CUs) */
  uint32_t mvp_idx_cost[3];         /* m_auiMVPIdxCost[0..2][AMVP_MAX_NUM_CANDS] */
  int32_t max_pu_w, max_pu_h;       /* as in vvcgpu_bipred_me_cfg: no item is wider / higher (0: 128); an item beyond it is skipped */
  int32_t imv;                      /* cu.imv of every PU of the call: 0 (quarter-sample), 1 (integer-sample) or 2 (four-sample vectors) */
  int32_t reserved;
} vvcgpu_unipred_me_cfg;
typedef struct {                        /* one (list, reference index) of a result            sizeof == 48 */
  int32_t  mv[2];         /* cMvTemp[list][ref] (quarter units) */
  int32_t  int_mv[2];     /* the integer vector xTZSearch found: what m_integerMv2Nx2N / the block cache are updated with (zero where the list-1
                             shortcut took list 0's vector) */
  int32_t  mvp_idx;       /* aaiMvpIdx[list][ref] after xCheckBestMVP */
  uint32_t bits;          /* uiBitsTemp after xCheckBestMVP */
  uint64_t cost;          /* uiCostTemp after xCheckBestMVP */
  uint64_t tmpl_cost[2];  /* xGetTemplateCost of candidate 0..1 (0 beyond num_cand) */
} vvcgpu_unipred_me_search;
typedef struct {                        /* one PU                                             sizeof == 472 */
  vvcgpu_unipred_me_search s[2][VVCGPU_UNIPRED_ME_MAX_REFS];   /* entries beyond cfg.n_ref[list] are zero */
  int32_t  ref_idx[2];    /* iRefIdx[0..1] */
  int32_t  mv[2][2];      /* cMv[0..1] */
  uint64_t cost[2];       /* uiCost[0..1]; both ~0 with everything else zero: item skipped.  cost[1] = ~0 on a P slice */
  uint32_t bits[2];       /* uiBits[0..1] (0 for a list without references) */
  int32_t  best_bip_ref_idx_l1, best_bip_mvp_l1;   /* bestBiPRefIdxL1, bestBiPMvpL1 (0 unless mvd_l1_zero) */
  uint64_t best_bip_dist; /* bestBiPDist (~0 unless mvd_l1_zero set it) */
  int32_t  valid_l1_ref_idx;   /* refIdxValidList1 */
  int32_t  valid_l1_mv[2];     /* mvValidList1 */
  uint32_t valid_l1_bits;      /* bitsValidList1 (0xFFFFFFFF: no valid list-1 reference) */
  uint64_t valid_l1_cost;      /* costValidList1 (~0: no valid list-1 reference) */
} vvcgpu_unipred_me_result;
int vvcgpu_unipred_me_batch(const vvc_pel* org_base, const vvcgpu_unipred_me_item* items, int n, const vvcgpu_unipred_me_cfg* cfg_host,
                            vvcgpu_unipred_me_result* results, vvcgpu_bipred_me_item* bipred_items_out, void* stream);

/* The WHOLE uni-predictive stage of the affine inter search of a PU (the uni-predictive part of InterSearch::xPredAffineInterSearch,
 * InterSearch.cpp:2651-2814, with xEstimateAffineAMVP :3745-3794 / xGetAffineTemplateCost :1645-1665, xAffineMotionEstimation(bBi = false) :3286-3743
 * and xCheckBestAffineMVP :3181-3284 inside it) for a list of independent PUs of mixed sizes and mixed 4- / 6-parameter type, with no host
 * synchronisation inside: two launches on the stream.  The first gives every (PU, list, reference index) search an owner of its own (a wavefront up to
 * 1024 samples, a workgroup above), the second makes the per-PU decisions.  Results are bit-exact, the double arithmetic of the costs included.  All
 * vectors are in 1/16 sample units, after Mv::setHighPrec (the convention of vvcgpu_affine_me_item.mvp and of vvcgpu_affine_bipred_me_batch): the
 * reference holds hevcMv as quarter-sample vectors and mvAffine4Para, the output of an earlier xAffineMotionEstimation, as 1/16-sample ones;
 * xPredAffineBlk and xAffineMotionEstimation raise what they get to 1/16 sample (InterPrediction.cpp:579-581, InterSearch.cpp:3327-3329), and
 * :2700-2706 work on the raw components of mvFour, which are 1/16-sample values, so hevc_mv = hevcMv << 2 and mv4 = mvAffine4Para as they are give
 * what the reference computes.  Per PU and per (list, reference index), in the reference's order:
 *   bits              uiBitsTemp = mb_bits[list] + the reference-index bits of :2658-2666 (cfg.n_ref[list]);
 *   xEstimateAffineAMVP   with the caller's candidates (PU::fillAffineMvpCand stays on the host): per candidate xGetAffineTemplateCost -- luma
 *                     xPredAffineBlk with bi = false on the candidate's three vectors as they are (no clipMv of them), rounded and clipped, full SAD
 *                     against the original + getCost(mvp_idx_cost[i]); the best by uiBestCost > uiTmpCost in candidate order; its cost is biPDistTemp;
 *   :2673-2677        a 6-parameter PU whose only_ref[list] (refIdx4Para) differs from this index stops here: only aaiMvpIdx and the candidate set are
 *                     kept, cMvTemp stays zero; this happens before the bestBiP* update;
 *   start vectors     (:2681-2727) the template cost of hevc_mv used for all three control points, with the chosen index's cost; for a 6-parameter PU
 *                     also that of the inherited 4-parameter result mvFour: mv4[0..1] and mvFour[2] by :2700-2706 ((mv4[0] << 7) -+ ((mv4[1] - mv4[0])
 *                     swapped << (7 + log2 h - log2 w)), >> 7, roundMV2SignalPrecision), taken on strict '<'; the search starts from that vector when
 *                     its cost is < biPDistTemp, otherwise from the predictor;
 *   :2730-2735        bestBiPDist / bestBiPMvpL1 / bestBiPRefIdxL1 when cfg.mvd_l1_zero (list 1, strict '<');
 *   search            (:2738-2783) bits += mvp_idx_cost[mvp_idx]; then xAffineMotionEstimation(bBi = false) -- exactly what vvcgpu_affine_me_batch does
 *                     for an item with half_weight = 0 -- or the list-1 shortcut: with cfg.fast_me_gen_b_low_delay, list1_to_list0[ref] >= 0 and, for a
 *                     6-parameter PU, list1_to_list0[ref] == only_ref[0], a list-1 reference copies list 0's vectors, subtracts getCost(bits) of list 0
 *                     (uint64), adds the vector bits of :2753-2770 (second-predictor rule for vectors 1 and 2) and adds getCost again;
 *   xCheckBestAffineMVP   over that (list, reference)'s candidates;
 *   :2788-2812        the uiCostTempL0 / uiBitsTempL0 record, keep-if-strictly-better per list, and the "valid list 1" record.
 * Not served: weighted prediction (the bi branch of xGetAffineTemplateCost), composite reference.  Affine AMVP derivation and the final mode choice
 * (:3017-3099) stay on the host.
 * bipred_items_out (may be NULL): n complete vvcgpu_affine_bipred_item records, exactly what vvcgpu_affine_bipred_me_batch asks of its caller --
 * geometry, n_ref, planes, cMvTemp, candidates and aaiMvpIdx per (list, reference), iRefIdx, aacMv, uiCost, uiBits, mb_bits, only_ref -- with the
 * mvd_l1_zero preparation of :2840-2853 done when cfg.mvd_l1_zero (ref_idx[1] = bestBiPRefIdxL1, that record's mvp_idx = bestBiPMvpL1, its mv and
 * mv[1] = that candidate), so that the buffer can be handed to vvcgpu_affine_bipred_me_batch on the same stream as it is.  On a P slice
 * (n_ref[1] == 0) the records carry n_ref[1] = 0, which the bi-predictive entry skips.
 * Reference planes and readable margin: as vvcgpu_affine_bipred_me_batch -- ref_planes[i] points to sample (0, 0) of picture i inside its padded
 * allocation; sub-block vectors are clipped to the picture + 8 / - CTU - 8 samples and the 8 taps reach 4 further: max_cu + 12 readable samples around
 * the picture on every side serve every prediction of every search.
 * items, results, bipred_items_out: device memory.  Items cannot be validated on the host: an item outside the contract (a side not in {16, 32, 64,
 * 128} or larger than the CTU or than cfg.max_pu_w / max_pu_h, a PU not inside the picture, org_stride <= 0, only_ref[l] outside -1 .. n_ref[l] - 1 for
 * a list that has references, num_cand outside 1..2 for a (list, reference) of the slice) is skipped: it reads no sample, its result has cost[0] =
 * cost[1] = ~0 (UINT64_MAX) with everything else zero, its out-item is all zero.  n == 0 is a no-op; null pointers (bipred_items_out may be NULL),
 * n < 0, geometry, clp_min > clp_max, lambda outside [0, 2^20), n_planes outside 1..16, n_ref[0] outside 1..4, n_ref[1] outside 0..4, a ref_plane
 * outside [0, n_planes), a list1_to_list0 outside [-1, n_ref[0]) and max_pu sides that are no served side return VVCGPU_E_ARG, a bit depth outside
 * 8..10 VVCGPU_E_UNSUPPORTED, before any device work. */
#define VVCGPU_AFFINE_UNIPRED_MAX_REFS 4
typedef struct {                        /* one (list, reference index) of a PU                sizeof == 80 */
  int32_t mv_cand[2][3][2];  /* affiAMVPInfo: mvCandLT / RT / LB of candidates 0 and 1 */
  int32_t hevc_mv[2];        /* hevcMv[list][ref] << 2: the translational result */
  int32_t mv4[2][2];         /* mvAffine4Para[list][ref][0..1]: read for a 6-parameter PU */
  int16_t num_cand;          /* .numCand: 1..2 */
  int16_t reserved0;
  int32_t reserved1;
} vvcgpu_affine_unipred_ref;
typedef struct {                        /* one PU                                             sizeof == 688 */
  int32_t  pos_x, pos_y;     /* pu.cu->lumaPos() */
  int16_t  w, h;             /* 16, 32, 64 or 128 each */
  int16_t  six_param;        /* cu->affineType */
  int16_t  reserved0;
  int64_t  org_off;          /* elements from org_base */
  int32_t  org_stride;
  uint32_t mb_bits[3];       /* uiMbBits[0..2] */
  int32_t  only_ref[2];      /* refIdx4Para[list]: a 6-parameter PU searches only this index of the list (-1: none); copied to the out-item */
  vvcgpu_affine_unipred_ref ref[2][VVCGPU_AFFINE_UNIPRED_MAX_REFS];
} vvcgpu_affine_unipred_item;
typedef struct {                        /* host struct                                        sizeof == 264 */
  double  lambda;            /* RdCost::m_motionLambda */
  const vvc_pel* ref_planes[16];   /* device pointers; entries from n_planes on are ignored */
  int32_t n_planes, ref_stride;
  int32_t pic_w, pic_h, max_cu_w, max_cu_h;                 /* clipMv, sub-block vector clip */
  int32_t bit_depth, clp_min, clp_max;
  int32_t n_ref[2];                                         /* slice.getNumRefIdx(list): 1..4, list 1 also 0 (P slice) */
  int32_t ref_plane[2][VVCGPU_AFFINE_UNIPRED_MAX_REFS];     /* index into ref_planes of (list, reference index) */
  int32_t list1_to_list0[VVCGPU_AFFINE_UNIPRED_MAX_REFS];   /* slice.getList1IdxToList0Idx(ref): -1 or a list-0 reference index */
  int32_t fast_me_gen_b_low_delay;  /* getFastMEForGenBLowDelayEnabled() */
  int32_t mvd_l1_zero;              /* slice.getMvdL1ZeroFlag() */
  int32_t affine_type;              /* sps.getSpsNext().getUseAffineType(): iteration limit 4 (6-param) / 5 (4-param); 0: 7 (as vvcgpu_affine_me_cfg) */
  uint32_t mvp_idx_cost[3];         /* m_auiMVPIdxCost[0..2][AMVP_MAX_NUM_CANDS] */
  int32_t max_pu_w, max_pu_h;       /* as in vvcgpu_affine_bipred_cfg: no item is wider / higher (0: 128); an item beyond it is skipped */
  int32_t reserved;
} vvcgpu_affine_unipred_cfg;
typedef struct {                        /* one (list, reference index) of a result            sizeof == 88 */
  int32_t  mv[3][2];         /* cMvTemp[list][ref]: what the caller stores as mvAffine4Para (zero where skipped by only_ref) */
  int32_t  mvp_idx;          /* aaiMvpIdx[list][ref] after xCheckBestAffineMVP */
  uint32_t bits;             /* uiBitsTemp after xCheckBestAffineMVP (0 where skipped) */
  uint64_t cost;             /* uiCostTemp after xCheckBestAffineMVP (0 where skipped) */
  uint64_t tmpl_cost[2];     /* xGetAffineTemplateCost of candidate 0..1 (0 beyond num_cand) */
  uint64_t start_cost;       /* template cost of the translational start; 0 unless searched == 1 */
  uint64_t inherit_cost;     /* template cost of the inherited 4-parameter start; 0 unless searched == 1 of a 6-parameter PU */
  int32_t  start;            /* 0 the predictor, 1 the translational vector, 2 the inherited vectors; 0 unless searched == 1 */
  uint32_t steps;            /* as vvcgpu_affine_me_result.steps; 0 where nothing was searched */
  int32_t  searched;         /* 0 skipped by only_ref, 1 searched, 2 the list-1 shortcut */
  int32_t  reserved;
} vvcgpu_affine_unipred_search;
typedef struct {                        /* one PU                                             sizeof == 840 */
  vvcgpu_affine_unipred_search s[2][VVCGPU_AFFINE_UNIPRED_MAX_REFS];   /* entries beyond cfg.n_ref[list] are zero */
  int32_t  ref_idx[2];       /* iRefIdx[0..1] */
  int32_t  mv[2][3][2];      /* aacMv[0..1] */
  uint64_t cost[2];          /* uiCost[0..1]; both ~0 with everything else zero: item skipped.  cost[1] = ~0 on a P slice */
  uint32_t bits[2];          /* uiBits[0..1] (0 for a list in which nothing was searched) */
  int32_t  best_bip_ref_idx_l1, best_bip_mvp_l1;   /* bestBiPRefIdxL1, bestBiPMvpL1 (0 unless mvd_l1_zero) */
  uint64_t best_bip_dist;    /* bestBiPDist (~0 unless mvd_l1_zero set it) */
  int32_t  valid_l1_ref_idx;    /* refIdxValidList1 */
  int32_t  valid_l1_mv[3][2];   /* mvValidList1 */
  uint32_t valid_l1_bits;       /* bitsValidList1 (0xFFFFFFFF: no valid list-1 reference) */
  uint64_t valid_l1_cost;       /* costValidList1 (~0: no valid list-1 reference) */
} vvcgpu_affine_unipred_result;
int vvcgpu_affine_unipred_me_batch(const vvc_pel* org_base, const vvcgpu_affine_unipred_item* items, int n, const vvcgpu_affine_unipred_cfg* cfg_host,
                                   vvcgpu_affine_unipred_result* results, vvcgpu_affine_bipred_item* bipred_items_out, void* stream);

/* ---- the merge candidate pass of a CU, on the device  (EncCu::xCheckRDCostMerge2Nx2N, first pass, EncoderLib/EncCu.cpp:1537-1612: per merge candidate
 *          InterPrediction::motionCompensation of all components into acMergeBuffer[] -- xSubPuMC, CommonLib/InterPrediction.cpp:265-345, for an ATMVP
 *          candidate --, the Hadamard (lossless: SAD) distFunc of the luma prediction, cost = (double)sad + (double)bits * sqrtLambda, updateCandList
 *          (CommonLib/UnitTools.h:190-223) into RdModeList and the MRG_FAST_RATIO cut) -----------------------------------------------------------
 * One call serves the pass for n_pu independent PUs: two launches on the caller's stream, no host synchronisation inside, every output bit for bit
 * the reference's, the doubles included.  It is built from the two descriptor types of vvcgpu_mc_batch and vvcgpu_dist_batch and plain index arrays.
 * Every array is device memory; descriptor arrays are 16-byte aligned.
 *   pu_cand_first[n_pu + 1]   PU p owns candidates pu_cand_first[p] .. pu_cand_first[p + 1] - 1 in merge order: candidate k of the PU is uiMergeCand = k;
 *                             their number is mergeCtx.numValidMergeCand, 1..7
 *   cand_dist[n_comp c + comp]  the DistParam / getDistPart pair of candidate c and component comp (0 Y, 1 Cb, 2 Cr); n_comp is 1 (luma only) or 3.
 *                             org_off / org_stride address the original block in org_base, cur_off / cur_stride the candidate's prediction block of the
 *                             component in pred_base (the caller's layout of m_acMergeBuffer[c]); w, h its size, sub_shift 0.  Luma sides are 4, 8, .. 128;
 *                             a chroma block is no larger than the luma block; cur_stride >= w
 *   cand_mc_first[n_cand + 1]   candidate c is predicted by mc_descs[cand_mc_first[c] .. cand_mc_first[c + 1] - 1]: descriptors as vvcgpu_mc_batch takes
 *                             them (bi 0 or 1, the vector clipped and split into integer offset and phase by the caller -- 1/16 luma, 1/32 chroma, so
 *                             high-precision merge vectors are served; a list-1-only candidate is passed as ref0), EXCEPT that `reserved` is the component
 *                             (0, 1, 2) and dst_off / dst_stride address pred_base.  A MRG_TYPE_DEFAULT_N candidate is one descriptor per component, an
 *                             ATMVP candidate (MRG_TYPE_SUBPU_ATMVP) one per sub-block (1 << getSubPuMvpSubblkLog2Size() luma samples: chroma blocks go
 *                             down to 2x2) per component; xSubPuMC joins neighbours of equal motion before it predicts, which changes no sample, so the
 *                             caller need not.  Within a candidate every descriptor's destination rectangle lies inside the cur block of its component,
 *                             with dst_stride == cur_stride, and together the rectangles of a component tile that block
 *   max_num_merge_cand        slice.getMaxNumMergeCand(), 1..7;  use_hadamard: !lossless (:1564), 0 = full SAD without row sub-sampling;
 *   sqrt_lambda               getMotionLambda(), in [0, 2^20)
 *   pred_base                 may be NULL: a cost-only call, nothing is written and the offsets still place the blocks;  sse_out may be NULL
 * Outputs:
 *   dist_out[c]               what vvcgpu_mc_batch of the luma run followed by vvcgpu_dist_batch(kind = use_hadamard ? 1 : 0) on cand_dist[n_comp c] returns
 *   sse_out[n_comp c + comp]  what vvcgpu_dist_batch(kind 2) returns for the component: the DF_SSE of the no-residual leg of the second pass
 *                             (InterSearch.cpp:4762-4790); the chroma distortion weight stays on the host, as for vvcgpu_dist_batch
 *   cost_out[c]               (double)dist + (double)bits * sqrt_lambda with bits = k + 1 - (k == max_num_merge_cand - 1) (:1594-1599): a product, then
 *                             a sum, no fused multiply-add
 *   rd_list_out[8 p]          uiNumMrgSATDCand after :1605-1612;  rd_list_out[8 p + 1 + i] = RdModeList[i] for i < min(NUM_MRG_SATD_CAND, count), -1
 *                             beyond (entries 5..7 are always -1).  updateCandList is followed literally with uiFastCandNum = 4 (strict '<': of two equal
 *                             costs the earlier candidate stays ahead).  With fewer than four candidates the reference's pruning loop indexes its cost
 *                             list beyond its size; the entry stops at the list's size there: uiNumMrgSATDCand starts from min(4, count)
 *   the predictions           of every component of every candidate, in pred_base (unless NULL): the samples vvcgpu_mc_batch writes for the descriptors
 * Reads of reference samples are exactly those vvcgpu_mc_batch states.
 * Descriptors cannot be validated on the host.  A candidate is SKIPPED -- it writes no sample, its dist_out and sse_out are ~0 -- if its run is empty or
 * leaves [0, n_mc); if one of its descriptors has w or h outside 1..128, bi outside 0..1, `reserved` outside [0, n_comp) or a phase outside the filter
 * table (0..15 luma, 0..31 chroma); if a destination rectangle leaves its cur block (or dst_stride differs from cur_stride); if its luma block has a
 * side outside {4, 8, .. 128}, or a chroma block is empty, larger than the luma block or wider than its cur_stride.  A PU is skipped -- its rd_list_out
 * row is all -1 -- if it has a skipped candidate (then the cost_out of all its candidates is +infinity), fewer than 1 or more than 7 candidates, or a
 * candidate range that leaves [0, n_cand) (then no cost_out is written for it).  A PU outside the contract is never a fault.
 * VVCGPU_E_ARG before any device work: a null pointer (ref1_base, pred_base and sse_out may be null), a negative count, n_comp outside {1, 3},
 * max_num_merge_cand outside 1..7, clp_min > clp_max, sqrt_lambda negative, not finite or >= 2^20, a descriptor array that is not 16-byte aligned;
 * VVCGPU_E_UNSUPPORTED: a bit depth outside 8..10.  n_pu == 0 is a no-op.
 * Not served, i.e. the caller's: PU::getInterMergeCandidates, clipMv, xCheckIdenticalMotion (a bi candidate of identical motion is handed over as a
 * uni-predictive one), the bestIsSkip gate and the second pass; weighted prediction; the single affine merge candidate, which has no SATD pass in
 * this reference (:1722-1803).                                                                                                                      */
int vvcgpu_merge_cand_batch(const vvc_pel* ref0_base, const vvc_pel* ref1_base, const vvc_pel* org_base, vvc_pel* pred_base,
                            const vvcgpu_mc_desc* mc_descs, int n_mc, const int32_t* cand_mc_first,
                            const vvcgpu_dist_desc* cand_dist, int n_cand, int n_comp, const int32_t* pu_cand_first, int n_pu,
                            int max_num_merge_cand, int use_hadamard, double sqrt_lambda, int bit_depth, int clp_min, int clp_max,
                            uint64_t* dist_out, uint64_t* sse_out, double* cost_out, int32_t* rd_list_out, void* stream);

/* ---- the inter residual pixel pass  (InterSearch::encodeResAndCalcRdInterCU, EncoderLib/InterSearch.cpp:4752-4909, with the "check full" part of
 *          xEstimateInterResidualQT :4254-4634; reached from xCheckRDCostMerge2Nx2N's second pass and from xEncodeInterResidual after predInterSearch) ----
 * One call serves n independent transform blocks -- an item is a (TU, component) pair of an inter CU, sides powers of two 2..64: a 4:2:0 CU is three
 * items, a 128-sample CU its four 64x64 luma TUs and its 32x32 chroma TUs as items of their own (for inter CUs they do not depend on each other) -- in
 * ONE launch on the caller's stream, no host synchronisation inside.  Per item
 *   orgResi   = org - pred, formed once (cs.getResiBuf().copyFrom(org); subtract(pred), :4816-4822);
 *   zero_dist = xGetSSE(0, orgResi) = sum orgResi^2: nonCoeffDist of :4424, the CU's zeroDistortion and the skip leg's distortion (the prediction is
 *               already clipped);
 *   and for each of the up to VVCGPU_INTER_RESI_SLOTS transform candidates tr[k] of the TU
 *   transformNxN :4409 (xT TrQuant.cpp:694-739 or xTransformSkip :1112-1163, Quant::quant Quant.cpp:721-834 with rounding 171 / 85 by intra_slice and
 *               xSignBitHidingHDQ :142-273 by sign_hiding), invTransformNxN :4497 (Quant::dequant :277-428, xIT :743-791 or xITransformSkip :795-847);
 *   dist_resi = xGetSSE(orgResi, resi') on the UNCLIPPED resi': currCompDist of :4504 -- the loop decides in the residual domain ("previously unclipped
 *               reconstruction values were used", :4882), and rec - pred is not resi' wherever the clip bites;
 *   dist_rec  = xGetSSE(org, clip(pred + resi')): the CU's finalDistortion term (:4880-4900).
 * orgResi, the coefficients and the de-quantised coefficients never go through device memory; the original and the prediction of an item are read once
 * for all its slots.
 *
 * items[i]     org_off / org_stride: the original block in org_base.  pred_off / pred_stride: the prediction block in pred_base -- the output of
 *              vvcgpu_mc_batch, or a merge candidate's block.  list_row >= 0 (a LIST item): the prediction is that of merge candidate
 *              c = rd_list[8 list_row + 1 + list_slot] at pred_off + c pred_cand_pitch, rd_list being rd_list_out of vvcgpu_merge_cand_batch, consumed
 *              where it lies (same stream, no download); the item is served when 0 <= list_slot < rd_list[8 list_row] and 0 <= c <= 6, else skipped.
 *              list_row < 0: pred_off as given.  w, h: powers of two 2..64.  qp: QpParam::Qp of the component; intra_slice / sign_hiding as
 *              vvcgpu_quant_desc.  tr[k], k = 0..5: -1 unused; tr_hor + 3 tr_ver with 0 DCT-II, 1 DCT-VIII, 2 DST-VII (0 = DCT-II both ways; 4, 5, 7, 8 the
 *              four pairs of g_aiTrSubsetInter under cu.emtFlag); VVCGPU_INTER_RESI_TS transform skip.  Transform skip is served on blocks with BOTH
 *              SIDES <= 4 (Log2MaxTransformSkipBlockSize 2, the shipped cfgs' value; 2-wide chroma blocks included), on no larger block.
 *              cand_off / level_off, both multiples of 4: slot k owns the w h contiguous samples at cand_off + k w h of resi_base (and of rec_base) and
 *              the w h levels at level_off + k w h of level_base.
 * flags        VVCGPU_INTER_RESI_*.  bit_depth 8..10 (else VVCGPU_E_UNSUPPORTED).  clp_min / clp_max: the clip range of the reconstruction.
 * Outputs per (item, slot), index 6 i + k: abs_sum as vvcgpu_resi_chain_batch's; dist_resi and dist_rec, each what vvcgpu_dist_batch kind 2 returns for
 * the two blocks (64-bit sums; one squared term stays below 2^31: |orgResi - resi'| <= 1023 + 32768).  Per item: zero_dist[i].  The levels (the zeroed
 * region of a 64-point side included) and resi' go to the slot's candidate buffers, the reconstruction to rec_base only under
 * VVCGPU_INTER_RESI_WRITE_REC (rec_base may be NULL otherwise).
 * A slot whose levels are all zero is still finished: resi' is stored as zeros, dist_resi == zero_dist, dist_rec == xGetSSE(org, clip(pred)); the
 * reference takes its else branch at :4521, the host does the same from abs_sum == 0.
 *
 * A skipped item or slot has abs_sum = 0xFFFFFFFF and both distortions ~0, a skipped item zero_dist = ~0 as well; nothing is touched in the three
 * buffers.  An ITEM is skipped when a side is outside 2..64 or not a power of two, when it is a list item and rd_list is NULL or the slot or the
 * candidate is out of range, when cand_off or level_off is not a multiple of 4.  A SLOT is skipped when it is -1, its code is outside -1..9, it puts a
 * transform other than DCT-II on a 64-point side or DCT-VIII / DST-VII on a side of 2, or it is a transform-skip slot on a block with a side above 4.
 * Candidate regions of different items must not overlap.  Samples must lie within the bit depth.  Offsets cannot be validated; an item outside the
 * contract is never a fault.
 * VVCGPU_E_ARG before any device work: a null required pointer (rd_list may be NULL; rec_base may be NULL without WRITE_REC), negative n, unknown flag
 * bits, a bad clip range, an item array that is not 16-byte aligned.  n == 0 is a no-op.
 * With the caller: every CABAC rate (cbf_comp, residual_coding, rqt_root_cbf, xGetSymbolFracBitsInter), the cost compares and the forced-null rule
 * (:4531-4568), the root-cbf decision (:4853) and the copy of the winner, the chroma distortion weight and DF_SSE_WTD.
 * Not served: cross-component prediction, RDPCM and lossless (range extensions, off in the shipped cfgs), RDOQ (vvcgpu_rdoq_batch; this is the
 * Quant::quant chain, as in every fused entry).  The DepQuant trellis is vvcgpu_inter_resi_code_dq_batch's, below.                                 */
#define VVCGPU_INTER_RESI_SLOTS      6
#define VVCGPU_INTER_RESI_TS         9     /* tr[k]: transform skip */
#define VVCGPU_INTER_RESI_WRITE_REC  1     /* flags: every served slot also stores clip(pred + resi') in rec_base */
typedef struct vvcgpu_inter_resi_item {
  int64_t org_off, pred_off;               /* samples from org_base / pred_base */
  int64_t pred_cand_pitch;                 /* list items: samples between the blocks of successive merge candidates of this component in pred_base */
  int64_t cand_off, level_off;             /* slot k: w h samples at cand_off + k w h of resi_base (and rec_base), w h levels at level_off + k w h */
  int32_t org_stride, pred_stride;
  int32_t qp;                              /* QpParam::Qp of the component */
  int32_t list_row;                        /* < 0: pred_off as given; >= 0: a row of rd_list */
  int16_t w, h;
  int8_t  list_slot, intra_slice, sign_hiding, reserved;
  int8_t  tr[VVCGPU_INTER_RESI_SLOTS];     /* -1 unused; tr_hor + 3 tr_ver (each 0 DCT-II, 1 DCT-VIII, 2 DST-VII); 9 transform skip */
  int8_t  reserved1[2];
  int32_t reserved2[2];                    /* sizeof == 80 */
} vvcgpu_inter_resi_item;
int vvcgpu_inter_resi_code_batch(const vvc_pel* org_base, const vvc_pel* pred_base, const vvcgpu_inter_resi_item* items, int n,
                                 const int32_t* rd_list,                 /* rd_list_out of vvcgpu_merge_cand_batch, may be NULL */
                                 vvc_pel* resi_base, vvc_pel* rec_base, vvc_coef* level_base,
                                 int flags, int bit_depth, int clp_min, int clp_max,
                                 uint32_t* abs_sum, uint64_t* dist_resi, uint64_t* dist_rec, uint64_t* zero_dist, void* stream);

/* ---- the inter residual pixel pass with the quantiser of the shipped cfgs (DepQuant 1) ----
 * vvcgpu_inter_resi_code_batch as above -- the same items, the same list look-up through rd_list, the same outputs at the same indices, the same skip
 * markers -- with what transformNxN (InterSearch.cpp:4409) and invTransformNxN (:4497) do under slice->getDepQuantEnabledFlag():
 *   the quantiser is DQIntern::DepQuant::quant (CommonLib/DepQuant.cpp:1323-1387), the trellis of vvcgpu_depquant_batch, its early return when no
 *               coefficient exceeds getLastThreshold() included (abs_sum 0, all levels zero);
 *   the de-quantiser is DQIntern::Quantizer::dequantBlock (:708-785), the dep_quant = 1 path of vvcgpu_dequant_tr_inv_batch.
 * intra_slice and sign_hiding of the item are IGNORED: the trellis has no rounding offset, and sign bit hiding is off with dependent quantisation
 * (JVET_K0072).  orgResi, zero_dist, dist_resi on the unclipped resi', dist_rec and the all-zero rule are those of vvcgpu_inter_resi_code_batch.
 * At most three launches on the caller's stream (forward transforms, trellis, de-quantiser + inverse transforms + distortions), no host
 * synchronisation inside; validity and the list look-up are decided on the device, so the call can be submitted behind vvcgpu_merge_cand_batch
 * without a download.
 *
 * dq[i]        parallel to items[i]: lambda = Quant::m_dLambda of the component (> 0), rates_idx and luma as in vvcgpu_depquant_desc.
 * rates        n_rates tables (vvcgpu_dq_rates), in device memory; shim/vtm_rates.h (vtmref_dq_rates_from_ctx) shows how the reference fills one.
 * quantiser    VVCGPU_INTER_RESI_Q_DEPQUANT, the one served value; any other returns VVCGPU_E_UNSUPPORTED before any device work.
 * level_extent the extent of level_base, in levels, that the items address (at least 16).
 * ws           device workspace of vvcgpu_inter_resi_code_dq_workspace_bytes(level_extent, n) bytes, 16-byte aligned: the coefficients, the trellis
 *              decisions and level histories -- all indexed by the slot's level offset -- and per slot a trellis record and a work-list entry.  It may hold anything on
 *              entry; nothing in it survives the call by contract.
 * flags        VVCGPU_INTER_RESI_WRITE_REC as above, and VVCGPU_INTER_RESI_DQ_TS (this entry's alone; vvcgpu_inter_resi_code_batch refuses it): a slot
 *              with code VVCGPU_INTER_RESI_TS on an item with w == 4 && h == 4 -- the transform-skip candidate the reference tests on every 4x4 block it
 *              codes under TransformSkip 1 (InterSearch.cpp:4340-4386: luma without cu.emtFlag, chroma 4x4) -- is served like any other slot.  In this
 *              reference TrQuant::transformNxN (TrQuant.cpp:966-977) hands the output of xTransformSkip to the same DepQuant::quant, and DepQuant.cpp
 *              reads tu.transformSkip for extended precision only (:663, :755; off), so with shift = 15 - bit_depth - 2 (getTransformShift of 4x4):
 *                coefficients = orgResi << shift (xTransformSkip :1140-1148), the trellis and dequantBlock unchanged,
 *                resi' = (coef' + (1 << (shift - 1))) >> shift (xITransformSkip :823-833), unclipped;
 *              levels, abs_sum, both distortions, the reconstruction and the all-zero rule as for every slot.  The kernels of a call with the flag
 *              are instantiations of their own: a call without it runs what it ran before the flag existed.
 * Served: sides 4..64, DCT-II and the four inter-EMT pairs (DCT-II only on a 64-point side), with VVCGPU_INTER_RESI_DQ_TS transform skip on 4x4 (on no
 * other size: TU::hasTransformSkipFlag with Log2MaxTransformSkipBlockSize 2 allows an area of at most 16, and sides of 2 are not served here), bit depth 8..10.
 * An ITEM is skipped, beside the rules above, when a side is 2, when level_off is negative or not a multiple of 16 (the trellis workspace is indexed by
 * it), when rates_idx is outside [0, n_rates) or lambda is not above zero.  A SLOT is skipped, beside the rules above, when it is a transform-skip slot
 * and the call does not carry VVCGPU_INTER_RESI_DQ_TS or the block is not 4x4, or when its levels do not lie inside level_extent.
 * VVCGPU_E_ARG before any device work: the cases of vvcgpu_inter_resi_code_batch, a null dq, rates or ws, n_rates < 1, level_extent < 16, a workspace
 * that is too small or not 16-byte aligned, a dq array that is not 8-byte aligned.  n == 0 is a no-op.
 * With the caller: as for vvcgpu_inter_resi_code_batch, and the rate tables (one per component and TU size class, refreshed when the CABAC contexts move).
 * Not served: blocks with a side of 2 (vvcgpu_depquant_batch does not serve them either: the binding keeps them on the host), transform skip with
 * rotation or RDPCM (range extensions, off), RDOQ, cross-component prediction, RDPCM and lossless.  Transform skip itself is no limit of
 * vvcgpu_depquant_batch: it takes the scaled residual as coefficients like any others, and the stand-alone chain is vvcgpu_tr_fwd_batch with tr_hor = 3,
 * vvcgpu_depquant_batch, vvcgpu_dequant_tr_inv_batch with tr_hor = 3 and dep_quant = 1 (sides of 4 and up).                                        */
#define VVCGPU_INTER_RESI_Q_DEPQUANT 1     /* quantiser: DQIntern::DepQuant::quant */
#define VVCGPU_INTER_RESI_DQ_TS      8     /* flags of vvcgpu_inter_resi_code_dq_batch: a VVCGPU_INTER_RESI_TS slot of a 4x4 item is served */
typedef struct vvcgpu_inter_resi_dq {
  double  lambda;                          /* Quant::m_dLambda of the component */
  int32_t rates_idx;                       /* index into the rates array */
  int8_t  luma;
  int8_t  reserved[3];                     /* sizeof == 16 */
} vvcgpu_inter_resi_dq;
struct vvcgpu_dq_rates;                    /* the rate tables of the trellis, defined with vvcgpu_depquant_batch below */
size_t vvcgpu_inter_resi_code_dq_workspace_bytes(size_t level_extent, int n);
int vvcgpu_inter_resi_code_dq_batch(const vvc_pel* org_base, const vvc_pel* pred_base, const vvcgpu_inter_resi_item* items,
                                    const vvcgpu_inter_resi_dq* dq, int n,
                                    const int32_t* rd_list,              /* rd_list_out of vvcgpu_merge_cand_batch, may be NULL */
                                    const struct vvcgpu_dq_rates* rates, int n_rates, int quantiser,
                                    vvc_pel* resi_base, vvc_pel* rec_base, vvc_coef* level_base, size_t level_extent,
                                    int flags, int bit_depth, int clp_min, int clp_max,
                                    uint32_t* abs_sum, uint64_t* dist_resi, uint64_t* dist_rec, uint64_t* zero_dist,
                                    void* ws, size_t ws_bytes, void* stream);

/* ---- the rate half of the RD loops: CABACWriter::residual_coding under the bit estimator, for n level blocks in one launch ----
 * What getEstFracBits() returns after `getCtx() = ctxStart; resetBits(); residual_coding(tu, compID)` (InterSearch.cpp:4380-4381, :4490-4492;
 * IntraSearch.cpp xGetIntraFracBitsQT) on a BitEstimator_Std, for every level block that the RD pass entries above leave in level_base:
 *   residual_coding EncoderLib/CABACWriter.cpp:1970-2087 (HEVC_TOOLS 0, JVET_K0072, JVET_K1000_SIMPLIFIED_EMT, ENABLE_BMS: one scan, diagonal in 4x4
 *               groups, 2x2 groups when a side is 2), transform_skip_flag :2090-2103, emt_tu_index :2106-2133, last_sig_coeff :2202-2255,
 *               residual_coding_subblock :2260-2383 (group flag; sig / par / gt1; gt2; Go-Rice remainders; signs with hideSign, SBH_THRESHOLD 4);
 *   the context of every bin: CoeffCodingContext CommonLib/ContextModelling.cpp:217-393 (rectCUs: the luma prefix_ctx table, the chroma
 *               Clip3(0, 2, side >> 3) shifts), sigCtxIdAbs / ctxOffsetAbs / GoRiceParAbs ContextModelling.h:135-220 -- the offset of an inferred
 *               significance is the one ctxOffsetAbs finds left over from the position coded before it, as in the reference;
 *   the estimator: b += m_EstFracBits[state ^ bin]; state = m_NextState[state][bin] per context (Contexts.h:91-96, BinEncoder.h:300), whole bits
 *               for bypass bins (BinEncoder.h:266-267), encodeRemAbsEP with useLimitedPrefixLength false (BinEncoder.cpp:452-503).
 * The bins and their contexts depend on the levels alone, the fractional bits are a sum, and only bins of ONE context are ordered: one wavefront
 * takes an item, lays the levels into LDS, finds every position's bins and context offsets with its lanes as scan positions, and walks them with
 * its lanes as contexts.  One launch, no host synchronisation; behind an RD pass on the same stream with gate = that pass' abs_sum, nothing is
 * downloaded between the two.
 *
 * items[i]     level_off: the w h levels of the block in level_base, row-major with pitch w -- what the RD passes write at level_off + k w h.
 *              ctx_idx: the row of ctx.  w, h: powers of two 2..64.  luma: channel type.  dep_quant: stateTab 32040 or 0 (:2034).  sign_hiding:
 *              cctx.hideSign.  ts_flag: -1 no transform_skip_flag bin, 0 / 1 the bin of that value (the host decides presence, :2093).
 *              emt_idx: -1 none, 0..3 the emt_tu_index; emt_inter: context pair 2, 3 instead of 0, 1; emt_thr: 1 codes the two bins only when
 *              numSig > g_EmtSigNumThr (the intra rule :2070-2079), 0 always (the inter rule).  reserved: 0.
 * gate         may be NULL; gate[i] == 0xFFFFFFFF (the skip marker of the RD passes' abs_sum) skips item i.
 * ctx          n_ctx rows of VVCGPU_RESI_RATE_CTX_BYTES bytes, device: the BinProbModel_Std states (getState()) of one (snapshot, channel type) at
 *              the offsets below, a chroma row from the shorter chroma sets; shim/vtm_rates.h (vtmref_resi_ctx_row) fills one.
 * est_bits     128 words, device: ProbModelTables::m_EstFracBits.  next_state: 256 bytes, device: m_NextState[s][bin] at 2 s + bin.  They are the
 *              reference's data, handed in as the quantisers' rate tables are (shim/vtm_rates.h: vtmref_cabac_model).
 * Outputs per item: frac_bits[i] as above; num_sig[i], the count of non-zero levels (numSig of :2056); ctx_out (may be NULL), row i: the item's
 * row after its block, for the copy of the winner (the re-walk of InterSearch.cpp:4607-4624).  A block without a level returns 0 and 0 and its row
 * unchanged: the reference never codes one, and the cbf bin is the caller's (vvcgpu_inter_resi_choose_batch takes its bits).
 * A skipped item has frac_bits = ~0, num_sig = 0xFFFFFFFF and its ctx_out row untouched: gate[i] == 0xFFFFFFFF, a side outside 2..64 or not a power
 * of two, ctx_idx outside [0, n_ctx), a negative level_off, a flag field out of range or a reserved byte that is not 0.  |level| <= 32767 (larger
 * values are outside the contract and are clamped).  Offsets cannot be validated; an item outside the contract is never a fault.
 * VVCGPU_E_ARG before any device work: a null required pointer (gate and ctx_out may be NULL), negative n, n_ctx < 1, an item array that is not
 * 8-byte aligned.  n == 0 is a no-op.
 * With the caller: the cbf and header bins, the context snapshot (one row per channel type), the copy of the winner's row.                        */
#define VVCGPU_RESI_RATE_CTX_BYTES   192
#define VVCGPU_RESI_RATE_LAST_X      0     /* 25: Ctx::LastX[chType] */
#define VVCGPU_RESI_RATE_LAST_Y      25    /* 25: Ctx::LastY[chType] */
#define VVCGPU_RESI_RATE_SIG_GROUP   50    /* 2: Ctx::SigCoeffGroup[chType] */
#define VVCGPU_RESI_RATE_SIG         52    /* 3 x 20: Ctx::SigFlag[chType + 0 / 2 / 4] */
#define VVCGPU_RESI_RATE_PAR         112   /* 21: Ctx::ParFlag[chType] */
#define VVCGPU_RESI_RATE_GT2         133   /* 21: Ctx::GtxFlag[chType] */
#define VVCGPU_RESI_RATE_GT1         154   /* 21: Ctx::GtxFlag[chType + 2] */
#define VVCGPU_RESI_RATE_TS          175   /* 1: Ctx::TransformSkipFlag(chType) */
#define VVCGPU_RESI_RATE_EMT         176   /* 4: Ctx::EMTTuIndex */
#define VVCGPU_RESI_RATE_CTX_USED    180   /* zero padding from here */
struct vvcgpu_resi_rate_item {
  int64_t level_off;                       /* levels from level_base */
  int32_t ctx_idx;                         /* row of ctx */
  int16_t w, h;
  int8_t  luma, dep_quant, sign_hiding;
  int8_t  ts_flag;                         /* -1 none, 0 / 1 */
  int8_t  emt_idx;                         /* -1 none, 0..3 */
  int8_t  emt_inter, emt_thr;
  int8_t  reserved[9];                     /* sizeof == 32 */
};
int vvcgpu_resi_rate_batch(const vvc_coef* level_base, const struct vvcgpu_resi_rate_item* items, int n,
                           const uint32_t* gate,                         /* may be NULL */
                           const uint8_t* ctx, int n_ctx, const uint32_t* est_bits, const uint8_t* next_state,
                           uint64_t* frac_bits, uint32_t* num_sig,
                           uint8_t* ctx_out,                             /* may be NULL */
                           void* stream);

/* ---- the compare of xEstimateInterResidualQT (InterSearch.cpp:4395-4568) over the outputs of the two calls before it ----
 * Third call of the chain vvcgpu_inter_resi_code_batch / _dq_batch -> vvcgpu_resi_rate_batch (items 6 i + k on the levels at level_off + k w h,
 * gate = abs_sum) -> this one: every input is a device array, so nothing is downloaded before the winner is known.  For item i, with
 * D(x) = (uint64_t)(dist_weight[i] * (double)x) (RdCost::getDistPart :406-409; 1.0 for luma), cost(d, b) = dist_scale * (double)d + (double)b
 * (RdCost::calcRdCost, a multiply then an add) and p the cbf of the Cb item of a Cr item (prev[i], else 0):
 *   nonCoeffDist = D(zero_dist[i]), nonCoeffBits = cbf_bits[4 i + 2 p], nonCoeffCost = cost(nonCoeffDist, nonCoeffBits)             :4424-4455
 *   the slots in ascending order: abs_sum > 0: bits = cbf_bits[4 i + 2 p + 1] + frac_bits[6 i + k], dist = D(dist_resi[6 i + k]), cbf 1  :4463-4509;
 *               abs_sum == 0 on the transform-skip slot: cost DBL_MAX, bits and dist 0 (:4517-4520); else the non-coefficient triple, cbf 0;
 *   a slot is taken when cost < min, or when it is the transform-skip slot and cost == min (:4531);
 *   on slot 0 the forced null when nonCoeffCost < cost or abs_sum == 0: abs_sum 0, cbf 0, the non-coefficient triple (:4534-4544).
 * A slot is a candidate when tr[k] is not -1, abs_sum[6 i + k] is not 0xFFFFFFFF and, with abs_sum > 0, frac_bits[6 i + k] is not ~0; other
 * slots are passed over.  prev[i]: the index of the Cb item of a Cr item, else -1; the thread of a Cr item re-derives the Cb decision itself (with
 * p = 0), so items need no order.
 * Outputs per item: slot (the winner), cbf (0 after a forced null), abs_sum_out, dist, bits, min_cost.  An item comes back as slot -1 (cbf 0,
 * abs_sum_out 0xFFFFFFFF, dist and bits ~0, min_cost DBL_MAX) when slot 0 is no candidate, when a transform-skip code is not the last code of tr[]
 * that is not -1, when zero_dist[i] is ~0, when prev[i] is outside [-1, n) or the item it names comes back as slot -1.
 * VVCGPU_E_ARG before any device work: a null pointer, negative n, an item array that is not 16-byte aligned.  n == 0 is a no-op.
 * Not served: lossless (nonCoeffCost = MAX_DOUBLE, :4512) and cross-component prediction.
 * With the caller: the cbf bins' bits (two contexts' estFracBits per item), the copy of the winner, the root-cbf decision (:4853).               */
int vvcgpu_inter_resi_choose_batch(const vvcgpu_inter_resi_item* items, int n,
                                   const uint32_t* abs_sum, const uint64_t* dist_resi, const uint64_t* zero_dist,
                                   const uint64_t* frac_bits, const uint64_t* cbf_bits, const int32_t* prev,
                                   const double* dist_weight, double dist_scale,
                                   int32_t* slot, int32_t* cbf, uint32_t* abs_sum_out, uint64_t* dist, uint64_t* bits, double* min_cost,
                                   void* stream);

/* ---- N2 ("next" row): integer-sample TZ search of whole PUs, on the device  (InterSearch::xTZSearch,
 *          EncoderLib/InterSearch.cpp:1971-2252, with xTZSearchHelp :249-343, xTZ2PointSearch :349-374,
 *          xTZ8PointDiamondSearch :431-632, xSetSearchRange :1820-1883, clipMv CommonLib/Mv.cpp:64-80) -----------------
 * One wavefront walks one PU through the complete reference control flow (start point / zero vector / 2Nx2N predictor,
 * search range, first diamond rounds, zero neighbourhood, 2-point search, raster, star refinement); the up-to-16 candidates
 * of one diamond round (64 raster points) are evaluated together, and the arg-min keeps the reference's visiting order
 * and strict '<' rule, so position, cost and SAD are those of the sequential search.
 * Per PU: start_x/start_y = rcMv on entry (quarter units, before clipMv); pred2_x/pred2_y = *pIntegerMv2Nx2NPred (integer
 * units) when flag VVCGPU_TZ_PRED2; pos_x/pos_y = pu.cu->lumaPos(); pred_hor/pred_ver = m_mvPredictor (quarter units);
 * sub_shift = DistParam::subShift as set by RdCost::setDistParam for subShiftMode 0/2 (RdCost.cpp:256-283; mode 1 is
 * MESEARCH_SELECTIVE only and not served); VVCGPU_TZ_EXTENDED / VVCGPU_TZ_FAST = bExtendedSettings / bFastSettings.
 * cfg: lambda, cost_scale (2 in xMotionEstimation), imv_shift, search_range (m_iSearchRange), first_search_stop
 * (FastMEAssumingSmootherMV), picture and CTU size for clipMv, and the rectangle of reference samples that may be read
 * [ref_x0, ref_x1) x [ref_y0, ref_y1) in plane coordinates: the reference probes positions up to search_range / 2 beyond
 * the clipped range (zero-neighbourhood test) and relies on the picture margin; probes are clamped to the rectangle here,
 * so a too small margin gives a wrong SAD, never a fault; the plane allocation must extend 4 bytes beyond the rectangle's last sample
 * (reference rows are read as aligned dwords) and reference samples must be non-negative (picture samples).  Composite reference (JVET_K0157 inCtuSearch) and MR-SAD
 * (weighted prediction) are not served.  results: x, y = rcMv (integer units), cost = uiBestSad, sad = ruiSAD.          */
enum { VVCGPU_TZ_PRED2 = 1, VVCGPU_TZ_EXTENDED = 2, VVCGPU_TZ_FAST = 4 };
typedef struct vvcgpu_tz_pu {
  int32_t org_x, org_y, ref_x, ref_y;
  int32_t start_x, start_y, pred2_x, pred2_y;
  int32_t pos_x, pos_y, pred_hor, pred_ver;
  int16_t w, h, sub_shift, flags;
  int32_t reserved[2];                  /* reserved[0] > 0: this PU's own search range (m_aaiAdaptSR[list][refIdx]: the adaptive search range is per
                                           reference picture), 0: cfg.search_range; a batch may then mix the (list, reference) searches of one PU.  Must not exceed
                                           cfg.search_range (the caller passes the maximum over the batch there); a larger value is clamped to it.
                                           reserved[1]: 0.  sizeof == 64 */
} vvcgpu_tz_pu;
typedef struct vvcgpu_tz_cfg {
  double  lambda;
  int32_t cost_scale, imv_shift;
  int32_t search_range, first_search_stop;
  int32_t pic_w, pic_h, max_cu_w, max_cu_h;
  int32_t ref_x0, ref_y0, ref_x1, ref_y1;
  int32_t wg_per_pu;                    /* 0: one wavefront per PU (PUs up to about 32x32); 1: one workgroup of four per PU   */
  int32_t uniform_pu;                   /* 0: PUs of any size.  h << 16 | w (16 / 32 / 64 each): the caller states that the PUs of the batch are w x h with
                                           2:1 row sub-sampling; the raster stage (iRaster 5, InterSearch.cpp:2159-2169) then runs as its own launch
                                           between two launches of the search (a PU that does not match, or whose raster touches the border of the
                                           readable rectangle, keeps the one-launch form: results are identical either way).  sizeof == 64 */
} vvcgpu_tz_cfg;
int vvcgpu_tz_search_batch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride,
                           const vvcgpu_tz_pu* pus, int n, const vvcgpu_tz_cfg* cfg_host,
                           vvcgpu_search_best* results, void* stream);

/* ---- N4 ("next" row, picture-level passes): border extension and picture hash --------------------------------------------
 * vvcgpu_extend_border: Picture::extendPicBorder (CommonLib/Picture.cpp:996-1041) for one plane: every sample of the margin
 *   becomes the nearest picture sample (left/right columns replicated, then whole rows replicated upwards/downwards).
 *   plane points to sample (0,0) INSIDE the padded allocation; margins are in samples of this plane (the reference shifts the
 *   luma margin by the chroma scale, :1010-1011).
 * vvcgpu_picture_hash: the per-plane digests of CommonLib/PicYuvMD5.cpp -- method 1 (HASHTYPE_CRC): compCRC :83-125, CRC-16
 *   CCITT over the low byte then (bit depth > 8) the high byte of every sample in raster order, 16 zero bits appended;
 *   method 2 (HASHTYPE_CHECKSUM): compChecksum :143-169.  The CRC is linear over GF(2): every lane reduces 8 samples, lane and
 *   block remainders are shifted to their position by multiplication with x^n mod P and XORed.  out: one uint32 on the device
 *   (CRC in the low 16 bits).  method 0 (MD5, calcMD5 :181-207) is a serial chain of 64-byte blocks per plane and is NOT
 *   offered on the device (VVCGPU_E_UNSUPPORTED).                                                                          */
int vvcgpu_extend_border(vvc_pel* plane, int stride, int w, int h, int margin_x, int margin_y, void* stream);
int vvcgpu_picture_hash(int method, const vvc_pel* plane, int stride, int w, int h, int bit_depth, uint32_t* out, void* stream);

/* ---- N4 ("next" row): intra sample prediction  (IntraPrediction::predIntraAng, CommonLib/IntraPrediction.cpp:251-347 =
 *          xPredIntraPlanar :424-477 | xPredIntraDc :482-493 | xPredIntraAng :540-773 with wide-angle mapping :213-231, followed by
 *          the simplified PDPC; optional xFilterReferenceSamples :1071-1104 in front) ---------------------------------------
 * One descriptor per prediction block (a TU of the intra PU), any mix of sizes and modes in one call.  The caller gathers the
 * reference samples (xFillReferenceSamples, :807-1004: availability and substitution are control logic over the coding
 * structure) and hands them over PACKED:  refs[0] = top-left, refs[1 .. T] = the row above, refs[T + 1 .. T + L] = the column to
 * the left, with T / L = m_topRefLength / m_leftRefLength of setReferenceArrayLengths (:233-249; vvcgpu_intra_ref_lengths).
 * mode = PU::getFinalIntraMode (0 planar, 1 DC, 2..66 angular; the wide-angle remapping happens inside, as in the reference).
 * filter_refs = the decision of useFilteredIntraRefSamples (:1107-1150).  w, h: powers of two 4..64 (the reference predicts per
 * TU, <= 64; its DC divisor table g_aucLog2 ends at 128).  clp_min / clp_max: slice clip range of the component.  CCLM
 * (predIntraChromaLM, JVET_K0190) is not built.                                                                             */
typedef struct vvcgpu_intra_desc {
  int64_t ref_off, dst_off;             /* samples, relative to refs_base / dst_base */
  int32_t dst_stride;
  int16_t w, h;
  int8_t  mode, filter_refs;
  int16_t reserved;
  int32_t reserved2;                    /* sizeof == 32 */
} vvcgpu_intra_desc;
int vvcgpu_intra_ref_lengths(int w, int h, int* top_len, int* left_len);
int vvcgpu_intra_pred_batch(const vvc_pel* refs_base, vvc_pel* dst_base, const vvcgpu_intra_desc* descs, int n, int clp_min, int clp_max,
                            void* stream);

/* N4, intra mode pre-selection  (IntraSearch::estIntraPredLumaQT, EncoderLib/IntraSearch.cpp:397-480: for every candidate mode
 *          predIntraAng into the prediction buffer, then distParam.distFunc = the Hadamard distortion RdCost::xGetHADs against the
 *          original, :423-433 and the second round :470-480) -- one descriptor per (block, candidate mode): the prediction of
 *          vvcgpu_intra_pred_batch goes into LDS and only out[i] = xGetHADs(org, pred) (what vvcgpu_dist_batch kind 1 returns for the
 *          same two blocks) leaves the chip.  The mode bits and the candidate lists (xFracModeBitsIntra, updateCandList) stay with
 *          the caller.  refs as vvcgpu_intra_desc; org_off / org_stride: the block in the original plane.                            */
typedef struct vvcgpu_intra_satd_desc {
  int64_t ref_off, org_off;             /* samples, relative to refs_base / org_base */
  int32_t org_stride;
  int16_t w, h;                         /* powers of two 4..64 */
  int8_t  mode, filter_refs;
  int16_t reserved;
  int32_t reserved2;                    /* sizeof == 32 */
} vvcgpu_intra_satd_desc;
int vvcgpu_intra_satd_batch(const vvc_pel* refs_base, const vvc_pel* org_base, const vvcgpu_intra_satd_desc* descs, int n, int clp_min,
                            int clp_max, uint64_t* out, void* stream);

/* N4, reference sample gathering: IntraPrediction::xFillReferenceSamples (:807-1004) for the packed layout above.  rec_off: the
 * block's top-left sample in the reconstruction plane; flags_off: the reference's neighborFlags of the block in flags_base, one
 * byte per unit in chain order  below-left (bottom first) ... left ... top-left ... above ... above-right,
 * ceil(L / unit_h) + 1 + ceil(T / unit_w) entries (the availability walk over the coding structure, :853-858, stays with the
 * caller); unit_w / unit_h: pcv.minCUWidth / Height shifted by the component scale (:824-826).  Unavailable units are padded
 * exactly like the reference's line buffer; with nothing available every sample is 1 << (bit_depth - 1).  ref_off: where the
 * T + L + 1 packed samples go in refs_base -- feed them to vvcgpu_intra_pred_batch.                                         */
typedef struct vvcgpu_intra_fill_desc {
  int64_t rec_off, flags_off, ref_off;
  int32_t rec_stride;
  int16_t w, h;
  int8_t  unit_w, unit_h;
  int16_t reserved;
  int32_t reserved2;                    /* sizeof == 40 */
} vvcgpu_intra_fill_desc;
int vvcgpu_intra_fill_refs_batch(const vvc_pel* rec_base, const uint8_t* flags_base, vvc_pel* refs_base, const vvcgpu_intra_fill_desc* descs,
                                 int n, int bit_depth, void* stream);

/* N4, the intra mode pre-selection PASS: what IntraSearch::estIntraPredLumaQT does between initIntraPatternChType and its RD loop
 * (EncoderLib/IntraSearch.cpp:383-522, 591-618) for n independent luma PUs of mixed sizes, in one launch with no host synchronisation inside.
 * Per PU: the reference sample gathering (optional; xFillReferenceSamples, CommonLib/IntraPrediction.cpp:807-1004), both reference chains of
 * initIntraPatternChType(.., true) (xFilterReferenceSamples :1071-1104), round 1 (:405-446: planar, DC and the even angular modes), round 2
 * (:452-496: mode -1 / +1 of every parent 3..65 of the round-1 list, in list order, under the bSatdChecked guard), the MPM append (:499-522) and the
 * PBINTRA cut with its early return (:591-618).  Every mode is predicted from the chain that useFilteredIntraRefSamples(.., modeSpecific = true, ..)
 * selects (:1107-1139: the wide-angle rule, planar iff w h > 32, m_aucIntraFilter with HM_MDIS_AS_IN_JEM = 1), costs
 * (double)uiSad + (double)bits * sqrt_lambda with the Hadamard distFunc (the product first, then the sum, not fused), and goes through the two
 * updateCandList calls of :440-442 / :489-490 (CommonLib/UnitTools.h:190-223; strict '<': of two equal costs the earlier visited mode stays ahead).
 *
 * pus[p]       org_off, org_stride, w, h (powers of two 4..64) and ref_off: the PU's T + L + 1 packed references in refs_base, laid out as for
 *              vvcgpu_intra_pred_batch; mode, filter_refs and the reserved fields are ignored.
 * fill[p]      with rec_base and flags_base, all three or none: exactly what vvcgpu_intra_fill_refs_batch takes, with w, h and ref_off equal to
 *              pus[p]'s.  The references are gathered first and, unless refs_base is NULL, also written there.  Without fill, refs_base holds them.
 * pu_ctl       [4 p .. 4 p + 3]: the three MPMs of PU::getIntraMPMs (each 0..66), then numModesForFullRD (1..8; the caller's table lookup, :356-368).
 * pu_mode_bits [4 p + k]: what xFracModeBitsIntra returns for a mode equal to mpm[k] (the first match, k = 0..2), k = 3: for every other mode
 *              (CABACWriter::intra_luma_pred_mode, EncoderLib/CABACWriter.cpp:867-935, yields these four values under a fixed ctxStartIntraMode).
 * pu_inter_had [p]: cs.interHad of the PBINTRA gate; ~0 switches the gate off for the PU, a NULL array for all.  The gate's condition (getUsePbIntraFast,
 *              the slice type, the part size, the EMT pass) is the caller's; the device compares CandHadList[k] > (double)interHad * 1.1.
 * flags        VVCGPU_INTRA_CAND_*.  sqrt_lambda: getMotionLambda() / (1 << SCALE_BITS), in [0, 2^20).  bit_depth: 8..10 (else VVCGPU_E_UNSUPPORTED).
 * satd_out     [67 p + m]: uiSad of every evaluated mode m, ~0 for the others; may be NULL.
 * list_out     [16 p ..]: [0] the final uiRdModeList.size() (0: the early return of :604-617), [1] the size of uiHadModeList, [2..4] uiHadModeList,
 *              [5..15] uiRdModeList; -1 beyond each list's size.
 * cost_out     [12 p ..]: [0..7] CandCostList (numModesForFullRD entries: an appended MPM carries none), [8..10] CandHadList; +infinity elsewhere.
 *
 * A PU outside the contract -- a side outside 4..64 (a 128-sample side is not served, as by the other intra entries), fill[p] disagreeing with pus[p]
 * (or with a unit size below 1, or more than 192 units), an MPM outside 0..66, numModesForFullRD outside 1..8 -- is skipped: nothing is read or
 * predicted for it, its list_out row is all -1, its cost_out row all +infinity, its satd_out row all ~0.  Offsets cannot be validated.
 * VVCGPU_E_ARG before any device work: a null required pointer, fill / rec_base / flags_base not all set or all NULL, neither fill nor refs_base,
 * negative n, unknown flag bits, a bad clip range, sqrt_lambda negative, not finite or >= 2^20, a descriptor array that is not 16-byte aligned.
 * n == 0 is a no-op.
 * Not served: lossless DPCM (useDPCMForFirstPassIntraEstimation), INTRA_FULL_SEARCH, the emtUsageFlag == 2 reuse of a saved list (:541-581), chroma
 * (vvcgpu_intra_chroma_code_batch), and the RD loop that follows (:620-; its pixel pass: vvcgpu_intra_tu_code_batch).                                                             */
#define VVCGPU_INTRA_CAND_USE_MPM       1   /* getFastUDIUseMPMEnabled(): the append of :499-522 */
#define VVCGPU_INTRA_CAND_NO_SMOOTHING  2   /* sps intraSmoothingDisabledFlag: no mode predicts from filtered references */
int vvcgpu_intra_mode_cand_batch(
    const vvc_pel* rec_base, const uint8_t* flags_base, const vvcgpu_intra_fill_desc* fill,  /* all three NULL: refs_base holds the references */
    vvc_pel* refs_base,                        /* read when fill == NULL; with fill: where the gathered references are also written, may be NULL */
    const vvc_pel* org_base, const vvcgpu_intra_satd_desc* pus, int n,
    const int32_t* pu_ctl, const uint64_t* pu_mode_bits, const uint64_t* pu_inter_had,       /* pu_inter_had may be NULL */
    int flags, double sqrt_lambda, int bit_depth, int clp_min, int clp_max,
    uint64_t* satd_out, int32_t* list_out, double* cost_out, void* stream);                   /* satd_out may be NULL */

/* N4, the pixel pass of the intra RD loop: what IntraSearch::xIntraCodingTUBlock (EncoderLib/IntraSearch.cpp:1147-1316) does for one surviving mode or
 * one EMT candidate -- predIntraAng, org - pred, transformNxN, the numSig count (:1257-1280), invTransformNxN, reconstruct, getDistPart(DF_SSE) -- for
 * n independent luma TUs of mixed sizes, in ONE launch with no host synchronisation inside.  The prediction is formed in LDS and never goes through
 * device memory; the rate (xGetIntraFracBitsQT) and the cost compare stay with the caller.
 *
 * Item i is the pair preds[i] + tus[i] (both device arrays, 16-byte aligned); w, h must agree between the two: powers of two 4..64.
 * preds[i]     ref_off: the packed references in refs_base, as for vvcgpu_intra_pred_batch.  dst_off / dst_stride are ignored: the prediction's place is
 *              tus[i].pred_off / pred_stride in pred_base.  mode 0..66 with filter_refs: used as given.  mode VVCGPU_INTRA_TU_FROM_LIST: the mode is
 *              mode_list[16 row + 5 + slot] with row = tus[i].reserved[0], slot = tus[i].reserved[1] -- mode_list being list_out of
 *              vvcgpu_intra_mode_cand_batch, consumed where it lies -- when slot < mode_list[16 row], else the item is skipped; the filter decision is
 *              then the device's (useFilteredIntraRefSamples(.., modeSpecific = true, ..) for luma, CommonLib/IntraPrediction.cpp:1107-1139).
 *              mode VVCGPU_INTRA_TU_PRED_GIVEN: no prediction, it is read from pred_base (chroma and CCLM through vvcgpu_cclm_pred_batch, the reload of
 *              default0Save1Load2 == 2).
 * tus[i]       as for vvcgpu_resi_chain_batch (Quant::quant with rounding 171 / 85 by intra_slice, xSignBitHidingHDQ by sign_hiding, Quant::dequant,
 *              tr_hor / tr_ver 0..2, the 64-point zero-out, the reconstruction clip), same alignment contract for offsets and strides.  Levels go to
 *              level_off, the zeroed region included.  reserved[0] / reserved[1]: row and slot of a FROM_LIST item, for this entry only.
 * flags        VVCGPU_INTRA_TU_*.  bit_depth: 8..10 (else VVCGPU_E_UNSUPPORTED).  clp_min / clp_max: the clip range of prediction and reconstruction.
 * abs_sum[i]   as vvcgpu_resi_chain_batch's.  num_sig[i]: the number of non-zero levels as stored (what :1262-1274 counts, uncapped; the comparison
 *              with g_EmtSigNumThr and the early return of :1276 are the caller's, the entry always finishes the item).
 * dist[i]      xGetSSE(org, rec), what vvcgpu_dist_batch kind 2 returns for the two blocks, from the reconstruction the item has just formed (64-bit
 *              sums; the chroma distortion weight and DF_SSE_WTD are the caller's).  mode_out[i]: the mode used, -1 for PRED_GIVEN.
 *
 * An item is skipped -- abs_sum = num_sig = 0xFFFFFFFF, dist = ~0, mode_out = -1, nothing touched in pred_base / rec_base / level_base -- when it is a
 * FROM_LIST slot beyond its list (or mode_list is NULL, or the list holds no mode 0..66 there), a side is outside 4..64, the pair disagrees on w / h,
 * the mode is outside -2..66, tr_hor / tr_ver is outside 0..2, a 64-point side is not DCT-II, or it is PRED_GIVEN without pred_base.
 * The rec / pred / level regions of different items must not overlap (candidates of one PU go to candidate buffers of their own), nor an item's rec
 * region its own pred region.  Samples must lie within the bit depth.  Offsets cannot be validated.
 * VVCGPU_E_ARG before any device work: a null required pointer (pred_base may be NULL when no item is PRED_GIVEN and WRITE_PRED is off; mode_list may
 * be NULL), negative n, unknown flag bits, a bad clip range, a descriptor array that is not 16-byte aligned.  n == 0 is a no-op.
 * Not served: transform skip and RDPCM (their own entries), RDOQ (vvcgpu_rdoq_batch; this is the Quant::quant chain; the DepQuant trellis is
 * vvcgpu_intra_tu_code_dq_batch's, below), cross-component prediction, TUs split below the PU (the 64x64 TUs of a 128-sample CU depend on each other's reconstruction),
 * chroma and CCLM prediction (they come in through PRED_GIVEN; whole chroma PUs: vvcgpu_intra_chroma_code_batch), the rate and the cost.          */
#define VVCGPU_INTRA_TU_PRED_GIVEN  (-1)   /* preds[i].mode: the prediction is read from pred_base */
#define VVCGPU_INTRA_TU_FROM_LIST   (-2)   /* preds[i].mode: taken from mode_list */
#define VVCGPU_INTRA_TU_WRITE_PRED    1    /* flags: predicted items also store their prediction at tus[i].pred_off (the "save" of default0Save1Load2 == 1) */
#define VVCGPU_INTRA_TU_NO_SMOOTHING  2    /* flags: as VVCGPU_INTRA_CAND_NO_SMOOTHING, for FROM_LIST items */
int vvcgpu_intra_tu_code_batch(
    const vvc_pel* refs_base, const vvcgpu_intra_desc* preds,
    const vvc_pel* org_base, vvc_pel* pred_base, vvc_pel* rec_base, vvc_coef* level_base,
    const vvcgpu_resi_chain_desc* tus, int n,
    const int32_t* mode_list,
    int flags, int bit_depth, int clp_min, int clp_max,
    uint32_t* abs_sum, uint32_t* num_sig, uint64_t* dist, int32_t* mode_out, void* stream);

/* ---- the pixel pass of the intra RD loop with the quantiser of the shipped cfgs (DepQuant 1) ----
 * vvcgpu_intra_tu_code_batch as above -- the same items (preds[i] + tus[i]), the same three mode kinds (0..66 as given, VVCGPU_INTRA_TU_FROM_LIST from
 * mode_list with the device's filter decision, VVCGPU_INTRA_TU_PRED_GIVEN), the same flags, the same outputs at the same indices, the same skip
 * markers -- with what transformNxN (IntraSearch.cpp:1253, called with the estimator's contexts) and invTransformNxN (:1289) of
 * IntraSearch::xIntraCodingTUBlock (EncoderLib/IntraSearch.cpp:1147-1316) do under slice->getDepQuantEnabledFlag():
 *   the quantiser is DQIntern::DepQuant::quant (CommonLib/DepQuant.cpp:1323-1387), the trellis of vvcgpu_depquant_batch over all w h coefficients (the
 *               zeroed region of a 64-point side holds zeros), its early return when no coefficient exceeds getLastThreshold() included (abs_sum 0, all
 *               levels zero);
 *   the de-quantiser is DQIntern::Quantizer::dequantBlock (:708-785), the dep_quant = 1 path of vvcgpu_dequant_tr_inv_batch.
 * Transform, trellis, de-quantiser and inverse transform are those of vvcgpu_inter_resi_code_dq_batch.  intra_slice and sign_hiding of tus[i] are
 * IGNORED: the trellis has no rounding offset, and sign bit hiding is off with dependent quantisation (JVET_K0072).
 * The trellis of an intra CU differs from an inter CU's only in RateEstimator::xSetLastCoeffOffset (DepQuant.cpp:379-396): an intra luma TU takes the
 * QtCbf bits where a depth-0 inter luma TU takes QtRootCbf.  That lives in the rate table: AN INTRA CALLER FILLS vvcgpu_dq_rates.cbf FROM QtCbf
 * (shim/vtm_rates.h branches on CU::isIntra).
 * Per served item: the prediction is formed in LDS and stored at tus[i].pred_off only under WRITE_PRED; org - pred goes through the forward transform
 * of tr_hor / tr_ver; the levels go to level_off; num_sig[i] is the number of non-zero stored levels, uncapped (the compare with g_EmtSigNumThr and
 * the early return of :1276 stay with the caller, the entry always finishes the item); with abs_sum == 0 the reconstruction is clip(pred) (the
 * piResi.fill(0) branch of :1293); dist[i] = xGetSSE(org, rec) from the reconstruction just formed; mode_out[i] as above.
 * At most three launches on the caller's stream (prediction + forward transforms, trellis, de-quantiser + inverse transforms + reconstruction +
 * distortion), no host synchronisation inside; validity and the list look-up are decided on the device, so the call can be submitted behind
 * vvcgpu_intra_mode_cand_batch without a download.
 *
 * dq[i]        parallel to the items, 8-byte aligned: lambda = Quant::m_dLambda of the component (> 0), rates_idx and luma as in vvcgpu_depquant_desc.
 * rates        n_rates tables (vvcgpu_dq_rates), in device memory.
 * quantiser    VVCGPU_INTRA_TU_Q_DEPQUANT, the one served value; any other returns VVCGPU_E_UNSUPPORTED before any device work.
 * level_extent the extent of level_base, in levels, that the items address (at least 16).
 * ws           device workspace of vvcgpu_intra_tu_code_dq_workspace_bytes(level_extent, n) bytes, 16-byte aligned: the coefficients, the trellis
 *              decisions and level histories, the predictions between the first and the last launch -- all indexed by the item's level offset -- and
 *              per item a trellis record and a work-list entry.  It may hold anything on entry; nothing in it survives the call by contract.
 * flags        VVCGPU_INTRA_TU_WRITE_PRED and VVCGPU_INTRA_TU_NO_SMOOTHING as above, and VVCGPU_INTRA_TU_DQ_TS (this entry's alone;
 *              vvcgpu_intra_tu_code_batch refuses it): an item with tus[i].tr_hor == 3 and w == h == 4 is the checkTransformSkip candidate of
 *              xRecurIntraCodingLumaQT (IntraSearch.cpp:1347-1412: intra luma 4x4 without cu.emtFlag); tr_ver is ignored, as in vvcgpu_tr_desc.  All
 *              three mode kinds are served: the reference reloads the prediction it saved (default0Save1Load2, :1182-1217), the same prediction the
 *              item forms or is given.  The arithmetic is that of VVCGPU_INTER_RESI_DQ_TS: coefficients = (org - pred) << shift with
 *              shift = 15 - bit_depth - 2, the trellis and dequantBlock unchanged, resi' = (coef' + (1 << (shift - 1))) >> shift.  num_sig, dist,
 *              mode_out, WRITE_PRED and the abs_sum == 0 branch work as for every item.  The kernels of a call with the flag are instantiations of
 *              their own: a call without it runs what it ran before the flag existed.
 * An item is skipped, beside the rules of vvcgpu_intra_tu_code_batch, when level_off is negative or not a multiple of 16 (the trellis workspace is
 * indexed by it), when its w h levels do not lie inside level_extent, when rates_idx is outside [0, n_rates) or lambda is not above zero.  An item with
 * tr_hor == 3 is skipped (the rule of vvcgpu_intra_tu_code_batch: tr_hor outside 0..2) unless the call carries VVCGPU_INTRA_TU_DQ_TS and the block is
 * 4x4.  An item outside the contract is never a fault.
 * VVCGPU_E_ARG before any device work: the cases of vvcgpu_intra_tu_code_batch, a null dq, rates or ws, n_rates < 1, level_extent < 16, a workspace
 * that is too small or not 16-byte aligned, a dq array that is not 8-byte aligned.  n == 0 is a no-op.
 * With the caller: as for vvcgpu_intra_tu_code_batch, and the rate tables (one per component and TU size class, refreshed when the CABAC contexts move).
 * Not served: RDOQ, transform skip on any block but 4x4 (Log2MaxTransformSkipBlockSize 2) or with rotation, RDPCM, cross-component prediction, TUs
 * split below the PU.  The chroma mode pass under DepQuant is vvcgpu_intra_chroma_code_dq_batch (below; the chroma transform-skip loop of
 * xRecurIntraChromaCodingQT :1751-1819 is not served); single chroma blocks also reach this entry through PRED_GIVEN.                           */
#define VVCGPU_INTRA_TU_Q_DEPQUANT 1       /* quantiser: DQIntern::DepQuant::quant */
#define VVCGPU_INTRA_TU_DQ_TS      8       /* flags of vvcgpu_intra_tu_code_dq_batch: a 4x4 item with tr_hor == 3 is the transform-skip candidate */
size_t vvcgpu_intra_tu_code_dq_workspace_bytes(size_t level_extent, int n);
int vvcgpu_intra_tu_code_dq_batch(
    const vvc_pel* refs_base, const vvcgpu_intra_desc* preds,
    const vvc_pel* org_base, vvc_pel* pred_base, vvc_pel* rec_base, vvc_coef* level_base, size_t level_extent,
    const vvcgpu_resi_chain_desc* tus, const vvcgpu_inter_resi_dq* dq, int n,
    const int32_t* mode_list,
    const struct vvcgpu_dq_rates* rates, int n_rates, int quantiser,
    int flags, int bit_depth, int clp_min, int clp_max,
    uint32_t* abs_sum, uint32_t* num_sig, uint64_t* dist, int32_t* mode_out,
    void* ws, size_t ws_bytes, void* stream);

/* N4, the intra chroma mode pass: what the mode loop of IntraSearch::estIntraPredChromaQT (EncoderLib/IntraSearch.cpp:704-852) does in pixels for n
 * independent chroma PUs of mixed sizes, each one TU per component, 4:2:0, with no host synchronisation inside: per PU up to six candidate modes
 * (PU::getIntraChromaCandModes, CommonLib/UnitTools.cpp:466-491), each through xRecurIntraChromaCodingQT (:1657-1843) = xIntraCodingTUBlock
 * (:1147-1316) for Cb and for Cr.  Per PU the references of both components (gathered as by vvcgpu_intra_fill_refs_batch, or given), the two original
 * blocks and -- when a slot holds the linear model -- the down-sampled luma block (xGetLumaRecPixels, CommonLib/IntraPrediction.cpp:1283-1581) are
 * staged once; every slot's prediction is formed on the chip (predIntraAng :251-354 from unfiltered references: useFilteredIntraRefSamples :1114 never
 * filters chroma outside 4:4:4; xGetLMParameters :1597-1857 + predIntraChromaLM :390-403 for LM_CHROMA_IDX, the chroma neighbours being row 0 / column 0
 * of the references) and goes through the residual chain of vvcgpu_resi_chain_batch (DCT-II both ways, Quant::quant, the 64-point zero-out, the
 * reconstruction clip) and xGetSSE(org, rec).
 *
 * pus[p]       org_off[c] (c = 0 Cb, 1 Cr): the component's original block in org_base, rows org_stride apart.  ref_off[c]: its T + L + 1 packed references
 *              in refs_base, laid out as for vvcgpu_intra_pred_batch.  luma_off / luma_stride: the co-located luma block in luma_base, the luma
 *              RECONSTRUCTION, as vvcgpu_cclm_desc's; above_avail / left_avail: as vvcgpu_cclm_desc's (the caller's two flags).  w, h: the chroma block,
 *              powers of two 2..64.  mode[k], k = 0..5: 0..66 = PU::getFinalIntraMode of the slot (DM resolved by the caller), 67 = LM_CHROMA_IDX,
 *              -1 = unused (LM disabled, or pruned by the caller).  qp[c]: QpParam::Qp of the component; intra_slice / sign_hiding as vvcgpu_quant_desc.
 *              cand_off / level_off: the PU's candidate buffers, both multiples of 4: item (k, c) owns the contiguous w x h block at
 *              cand_off + (2 k + c) w h of pred_base and of cand_rec_base, and at level_off + (2 k + c) w h of level_base.
 * fill[2 p + c] with rec_base and flags_base, all three or none: exactly what vvcgpu_intra_fill_refs_batch takes (rec_base: the chroma reconstruction), with
 *              w, h and ref_off equal to the PU's.  The references are gathered once per component and, unless refs_base is NULL, also written there.
 *              Without fill, refs_base holds them.
 * runs_host    the PU list is GROUPED BY SHAPE: n_runs triples (w, h, count) as vvcgpu_resi_chain_runs_batch takes them (w, h powers of two 2..64), the
 *              counts summing to n; a shape appears in at most one run.  The library picks a kernel per shape class on the host (both sides <= 16; a
 *              side of 32 or 64): at most two launches, all on `stream`.
 * flags        VVCGPU_INTRA_CHROMA_*.  bit_depth: 8..10, ONE value for luma and chroma (the shipped cfgs have them equal), else VVCGPU_E_UNSUPPORTED.
 *              clp_min / clp_max: the clip range of prediction and reconstruction.
 * Outputs per (PU, slot, component), index 12 p + 2 k + c: abs_sum as vvcgpu_resi_chain_batch's; dist = xGetSSE(org, rec) from the reconstruction just
 * formed, 64-bit; the levels (the zeroed region included) and the reconstruction in the candidate buffers; the prediction too under WRITE_PRED.
 *
 * An unused slot has abs_sum = 0xFFFFFFFF and dist = ~0 for both components and nothing touched in the buffers.  So has every slot of a PU outside the
 * contract: a side outside 2..64 or not a power of two, w x h not its run's, a mode outside -1..67, a slot with 67 and no luma_base, cand_off or level_off not
 * a multiple of 4, fill[2 p + c] disagreeing with the PU (or with a unit size below 1, or more than 192 units).  Candidate regions of different PUs must
 * not overlap.  Samples must lie within the bit depth.  Offsets cannot be validated.
 * VVCGPU_E_ARG before any device work: a null required pointer (pred_base may be NULL without WRITE_PRED, luma_base may be NULL), fill / rec_base /
 * flags_base not all set or all NULL, neither fill nor refs_base, negative n, n_runs below 1, a run whose shape is not one of the 36 or appears twice, a
 * negative count, counts not summing to n, unknown flag bits, a bad clip range, a descriptor array that is not 16-byte aligned.  n == 0 is a no-op.
 * With the caller: getIntraChromaCandModes and the resolution of DM through getFinalIntraMode, isLMCModeEnabled, the rate (xGetIntraFracBitsQT), the cost
 * compare, the chroma distortion weight and DF_SSE_WTD, the copy of the winner.
 * Not served: transform-skip candidates (checkTransformSkip: their own entries), cross-component prediction, RDOQ, 4:2:2 and 4:4:4, TUs split below
 * the PU.  The DepQuant trellis is vvcgpu_intra_chroma_code_dq_batch's (below).                                                                      */
#define VVCGPU_INTRA_CHROMA_LM          67   /* mode[k]: LM_CHROMA_IDX */
#define VVCGPU_INTRA_CHROMA_WRITE_PRED   1   /* flags: every served item also stores its prediction in pred_base */
typedef struct vvcgpu_intra_chroma_pu {
  int64_t org_off[2], ref_off[2];       /* samples, relative to org_base / refs_base */
  int64_t luma_off, cand_off, level_off;
  int32_t org_stride, luma_stride;
  int32_t qp[2];
  int16_t w, h;
  int8_t  above_avail, left_avail, intra_slice, sign_hiding;
  int8_t  mode[6];
  int16_t reserved;
  int32_t reserved2[2];                 /* sizeof == 96 */
} vvcgpu_intra_chroma_pu;
int vvcgpu_intra_chroma_code_batch(
    const vvc_pel* rec_base, const uint8_t* flags_base, const vvcgpu_intra_fill_desc* fill,  /* all three NULL: refs_base holds the references */
    vvc_pel* refs_base,                        /* read when fill == NULL; with fill: where the gathered references are also written, may be NULL */
    const vvc_pel* luma_base,                  /* may be NULL: a PU with an LM slot is then skipped */
    const vvc_pel* org_base, const vvcgpu_intra_chroma_pu* pus, int n, const int32_t* runs_host, int n_runs,
    vvc_pel* pred_base, vvc_pel* cand_rec_base, vvc_coef* level_base,
    int flags, int bit_depth, int clp_min, int clp_max,
    uint32_t* abs_sum, uint64_t* dist, void* stream);

/* ---- the intra chroma mode pass with the quantiser of the shipped cfgs (DepQuant 1) ----
 * vvcgpu_intra_chroma_code_batch as above -- the same PUs grouped by shape, the same fill / refs_base / luma_base, the same six slots and mode values,
 * VVCGPU_INTRA_CHROMA_WRITE_PRED, the same outputs at index 12 p + 2 k + c, the same candidate buffer layout, the same markers of unused slots and of
 * PUs outside the contract -- with what transformNxN and invTransformNxN of xIntraCodingTUBlock do under slice->getDepQuantEnabledFlag(), exactly as
 * in vvcgpu_intra_tu_code_dq_batch:
 *   the quantiser is DQIntern::DepQuant::quant (CommonLib/DepQuant.cpp:1323-1387) over all w h coefficients (the zeroed region of a 64-point side holds
 *               zeros), its early return when no coefficient exceeds getLastThreshold() included (abs_sum 0, all levels zero);
 *   the de-quantiser is DQIntern::Quantizer::dequantBlock (:708-785); the transform is DCT-II both ways;
 *   abs_sum == 0 gives rec = clip(pred) (the piResi.fill(0) branch); intra_slice and sign_hiding of the PU are IGNORED.
 * THE RATE TABLE OF A Cr BLOCK DEPENDS ON THE Cb BLOCK OF THE SAME CANDIDATE MODE.  RateEstimator::xSetLastCoeffOffset (CommonLib/DepQuant.cpp:379-396)
 * takes the cbf bits of a chroma TU from Ctx::QtCbf[compID](DeriveCtx::CtxQtCbf(compID, tu.depth, tu.cbf[COMPONENT_Cb])); DeriveCtx::CtxQtCbf
 * (CommonLib/ContextModelling.cpp:519-549) returns prevCbCbf ? 1 : 0 for Cr; xRecurIntraChromaCodingQT (EncoderLib/IntraSearch.cpp:1722-1843) codes Cb
 * first, and xIntraCodingTUBlock sets tu.cbf[Cb] from Cb's uiAbsSum before Cr's transformNxN runs.  The choice is made here on the device, per slot,
 * from the Cb result of that slot in the same call:
 * dq[3 p + 0]  the record of the PU's Cb blocks;
 * dq[3 p + 1]  the record of Cr in a slot whose Cb block has abs_sum == 0: THE CALLER FILLS ITS TABLE'S cbf FROM Ctx::QtCbf[Cr](0);
 * dq[3 p + 2]  the record of Cr in a slot whose Cb block has abs_sum > 0: its table's cbf from Ctx::QtCbf[Cr](1).
 *              Each record has its own lambda (selectLambda(compID), > 0) and rates_idx; luma must be 0.  The array is 8-byte aligned.
 * rates        n_rates tables (vvcgpu_dq_rates), in device memory.
 * quantiser    VVCGPU_INTRA_CHROMA_Q_DEPQUANT, the one served value; any other returns VVCGPU_E_UNSUPPORTED before any device work.
 * level_extent the extent of level_base, in levels, that the PUs address (at least 16).
 * ws           device workspace of vvcgpu_intra_chroma_code_dq_workspace_bytes(level_extent, n) bytes, 16-byte aligned: the coefficients, the trellis
 *              decisions and level histories, the predictions between the first and the last launch -- all indexed by the item's level offset -- and
 *              per item (twelve per PU) a trellis record and a work-list entry.  It may hold anything on entry; nothing in it survives the call by
 *              contract.
 * Five launches on the caller's stream, for every list (one kernel design serves all shapes): staging + prediction + forward transforms; the trellis of
 * the Cb blocks; the choice of the Cr records; the trellis of the Cr blocks; de-quantiser + inverse transforms + reconstruction + distortion.  No host
 * synchronisation inside: the call can be submitted behind the luma passes.
 * Contract differences from vvcgpu_intra_chroma_code_batch, all decided on the device and never a fault: sides are 4..64 (vvcgpu_depquant_batch serves
 * no 2-sample side); a RUN with a 2-sample side is accepted, so that the sibling's list can be handed over, and every PU of it gets the markers;
 * level_off must be a non-negative multiple of 16 (the trellis workspace is indexed by level offsets; w h >= 16 keeps every item of a PU on that grid);
 * all twelve blocks of the PU must lie inside level_extent; all three records must have rates_idx in [0, n_rates), lambda > 0 and luma == 0.  Any
 * violation skips the whole PU: markers for all twelve items, buffers untouched.
 * VVCGPU_E_ARG before any device work: the cases of vvcgpu_intra_chroma_code_batch, a null dq, rates or ws, n_rates < 1, level_extent < 16, a dq array
 * that is not 8-byte aligned, a workspace that is too small or not 16-byte aligned, n above (2^31 - 1) / 12, level_extent of 2^40 or more.  A bit depth outside 8..10 returns
 * VVCGPU_E_UNSUPPORTED.  n == 0 is a no-op.
 * With the caller: as for vvcgpu_intra_chroma_code_batch, and the three tables and lambdas per PU (shim/vtm_rates.h fills either Cr table from tu.cbf[Cb]).
 * Not served: transform-skip candidates, cross-component prediction, RDOQ, 4:2:2 and 4:4:4, TUs split below the PU, 2-sample sides, the rate and the cost. */
#define VVCGPU_INTRA_CHROMA_Q_DEPQUANT 1   /* quantiser: DQIntern::DepQuant::quant */
size_t vvcgpu_intra_chroma_code_dq_workspace_bytes(size_t level_extent, int n);
int vvcgpu_intra_chroma_code_dq_batch(
    const vvc_pel* rec_base, const uint8_t* flags_base, const vvcgpu_intra_fill_desc* fill, vvc_pel* refs_base,
    const vvc_pel* luma_base, const vvc_pel* org_base, const vvcgpu_intra_chroma_pu* pus, const vvcgpu_inter_resi_dq* dq, int n,
    const int32_t* runs_host, int n_runs,
    const struct vvcgpu_dq_rates* rates, int n_rates, int quantiser,
    vvc_pel* pred_base, vvc_pel* cand_rec_base, vvc_coef* level_base, size_t level_extent,
    int flags, int bit_depth, int clp_min, int clp_max,
    uint32_t* abs_sum, uint64_t* dist, void* ws, size_t ws_bytes, void* stream);

/* ---- the compares of the intra RD loops and the commit of the winner ----
 * vvcgpu_intra_luma_choose_batch: the transform loop of IntraSearch::xRecurIntraCodingLumaQT (EncoderLib/IntraSearch.cpp:1429-1588) inside the mode loop
 * of estIntraPredLumaQT (:637-697) for n_pu PUs coded as one TU, over the outputs of ONE vvcgpu_intra_tu_code_batch / _dq_batch call (the same tus
 * array; abs_sum, num_sig, dist, mode_out) and of a vvcgpu_resi_rate_batch call whose items are parallel to it (gate = abs_sum; frac_bits and,
 * optionally, ctx_out).  One launch, a wavefront per PU, no host synchronisation: behind those calls on one stream nothing is downloaded before the
 * winner's reconstruction lies in the picture plane, where vvcgpu_intra_chroma_code_batch (luma_base) and the next CU's vvcgpu_intra_fill_refs_batch
 * read it.
 *
 * pus[p]       cand_first, n_modes (1..16), n_tr (1..5): candidate (mode slot m, transform index t) is item j = cand_first + m n_tr + t.
 *              mpm[3], mode_bits[4]: the fractional bits of everything xEncIntraHeader codes (:1047-1063, the CU header bins included) for a mode equal
 *              to mpm[0] / mpm[1] / mpm[2] / none of them, the four-value scheme of vvcgpu_intra_mode_cand_batch.  cbf_bits[2]: the cbf_comp bin 0 / 1
 *              under QtCbf luma.  emt_cu_bits: emt_cu_flag as coded at :1049, 0 where it is not coded.  flags VVCGPU_INTRA_CHOOSE_*: EMT_FLAG =
 *              cu.emtFlag; TS_LAST = checkTransformSkip, index n_tr - 1 is the transform-skip candidate; FAST_EMT = getFastIntraEMT() && isAllIntra.
 *              rec_dst_off / rec_dst_stride: the PU's block in rec_dst_base; level_dst_off: its w h levels, pitch w, in level_dst_base.  reserved: 0.
 * Per candidate j, every context involved being distinct and every candidate starting from ctxStart (:646, :1465):
 *   valid       abs_sum[j] != 0xFFFFFFFF and, with abs_sum[j] > 0, frac_bits[j] != ~0.  A mode slot whose t = 0 candidate is not valid is passed over
 *               whole (the FROM_LIST slots beyond the list); an invalid candidate at t > 0 is passed over alone.
 *   bits        cbf = abs_sum[j] > 0; mode_bits[class of mode_out[j]] + cbf_bits[cbf] + (cbf ? emt_cu_bits + frac_bits[j] : 0): xGetIntraFracBitsQT(.., true,
 *               false) (:1109-1128, :1047-1063, :1102).
 *   cost        dist_scale * (double)dist[j] + (double)bits (RdCost::calcRdCost: a multiply, then an add), or MAX_DOUBLE by the rule of :1501-1502: the
 *               transform-skip candidate with cbf 0; EMT_FLAG and t > 0 and not the transform-skip candidate and num_sig[j] <= 2 (g_EmtSigNumThr).
 * Within a mode slot the candidates run in ascending t and are taken on cost < dSingleCost (:1524, start MAX_DOUBLE) with cbfBestMode tracked; under
 * FAST_EMT a candidate with t > 0 that is not the transform-skip one is passed over while !cbfBestMode (:1449).  The slots run in ascending m and are
 * taken on cost < csBest->cost (:664, start MAX_DOUBLE): of equal costs the earlier stays, and a slot whose candidates all cost MAX_DOUBLE never wins.
 * cand_cost[j] the cost of every candidate that was evaluated (MAX_DOUBLE included); VVCGPU_INTRA_CHOOSE_PASSED, a NaN pattern to be compared as 64
 *              bits, for a candidate that was passed over or is invalid.  m_modeCostStore[m] is the minimum over t.  Entries outside the range of
 *              every PU inside the contract are not written.
 * result[p]    best_cand (the winner's j, or -1), best_mode (its mode_out), best_tr (its t), cbf, dist, bits, cost.  Without a winner: -1, -1, -1, 0,
 *              ~0, ~0, MAX_DOUBLE and nothing committed (the early return).
 * Commit, for a PU with a winner j*: the w x h reconstruction at tus[j*].rec_off / rec_stride of rec_base goes to rec_dst_base (:1650, the copy into the
 * picture), the w h levels at tus[j*].level_off of level_base to level_dst_base, and -- when ctx_out and ctx_best are given -- row j* of ctx_out
 * (VVCGPU_RESI_RATE_CTX_BYTES bytes) to row p of ctx_best (ctxBest of :1555).  Nothing else in the destinations is touched.  Rows are moved in 8-byte
 * words where source and destination row are both 8-byte aligned (luma blocks lie at multiples of 4 samples), else in 4-byte or 2-byte ones.
 * A PU outside the contract comes back without a winner and is never a fault: n_modes / n_tr out of range, a candidate range leaving [0, n), candidates
 * disagreeing on w / h, a side outside 4..64 or not a power of two, unknown flag bits, a reserved word that is not 0.  Offsets cannot be validated.
 * The destination blocks of different PUs must not overlap, nor the destinations the candidate buffers.
 * VVCGPU_E_ARG before any device work: a null required pointer (ctx_out and ctx_best may be NULL, both or none), negative n_pu or n, pus / tus / result
 * not 16-byte aligned, a 64-bit array not 8-byte aligned.  n_pu == 0 is a no-op.
 * With the caller: the header and cbf bits (estFracBits of the contexts at ctxStart), the context snapshot, reading result[].
 * Not served: TUs split below the PU, checkInitTrDepthTransformSkipWinner, lossless, DF_SSE_WTD.                                                   */
#define VVCGPU_INTRA_CHOOSE_EMT_FLAG  1
#define VVCGPU_INTRA_CHOOSE_TS_LAST   2
#define VVCGPU_INTRA_CHOOSE_FAST_EMT  4
#define VVCGPU_INTRA_CHOOSE_PASSED    0x7FF8000000564356ull   /* cand_cost / slot_cost of a candidate that was not evaluated */
struct vvcgpu_intra_choose_pu {
  int64_t  rec_dst_off, level_dst_off;
  uint64_t mode_bits[4], cbf_bits[2], emt_cu_bits;
  int32_t  cand_first, rec_dst_stride;
  int16_t  n_modes, n_tr;
  int8_t   mpm[3], flags;
  int32_t  reserved[2];                    /* sizeof == 96 */
};
struct vvcgpu_intra_choose_result {
  int32_t  best_cand, best_mode, best_tr, cbf;
  uint64_t dist, bits;
  double   cost;
  int64_t  reserved;                       /* 0; sizeof == 48 */
};
int vvcgpu_intra_luma_choose_batch(
    const struct vvcgpu_intra_choose_pu* pus, int n_pu,
    const vvcgpu_resi_chain_desc* tus, int n,
    const uint32_t* abs_sum, const uint32_t* num_sig, const uint64_t* dist, const int32_t* mode_out, const uint64_t* frac_bits, double dist_scale,
    const vvc_pel* rec_base, const vvc_coef* level_base,
    const uint8_t* ctx_out,                    /* may be NULL */
    vvc_pel* rec_dst_base, vvc_coef* level_dst_base,
    uint8_t* ctx_best,                         /* may be NULL */
    double* cand_cost, struct vvcgpu_intra_choose_result* result, void* stream);

/* vvcgpu_intra_chroma_choose_batch: the mode loop of IntraSearch::estIntraPredChromaQT (EncoderLib/IntraSearch.cpp:773-847) over the outputs of ONE
 * vvcgpu_intra_chroma_code_batch / _dq_batch call -- the same pus array, abs_sum / dist at 12 p + 2 k + c -- and of the rate of its level blocks at the
 * same index.  The Cr block of a slot is coded behind its Cb block (:1122-1123), so its contexts start from Cb's.  Two vvcgpu_resi_rate_batch calls
 * over 12 n items each (gate = abs_sum) do it: the first serves the Cb items from the ctxStart row with ctx_out (its Cr items carry w = 0 and are
 * skipped) and gives frac_bits_cb; the second serves the Cr items with ctx = that ctx_out and ctx_idx = 12 p + 2 k, the Cb item's index (its Cb
 * items are skipped) and gives frac_bits_cr and, on request, the ctx_out this entry takes.  A Cb block without a level leaves its row as it was, so
 * the Cr block behind it starts from ctxStart, as in the reference.  One launch, a wavefront per PU, no host synchronisation.
 *
 * cpus[p]      mode_bits[6]: intra_chroma_pred_mode of each slot.  cbf_cb_bits[2]: the cbf_comp bin 0 / 1 of Cb.  cbf_cr_bits[4]: index 2 cbf_cb + cbf_cr,
 *              the context CtxQtCbf selects from Cb's cbf (:1003).  dist_weight[2]: the chroma distortion weight of Cb / Cr.  rec_dst_off[c] /
 *              rec_dst_stride: the component's block in rec_dst_base; level_dst_off[c]: its w h levels in level_dst_base.  reserved: 0.
 * pus[p]       what the pixel pass took: w, h (powers of two 2..64), mode[6], cand_off, level_off -- item (k, c) owns the w x h block at
 *              cand_off + (2 k + c) w h of cand_rec_base and at level_off + (2 k + c) w h of level_base.
 * A slot k is a candidate when mode[k] != -1, neither abs_sum is 0xFFFFFFFF and a component with levels has frac_bits != ~0.  With cbf_c = abs_sum > 0:
 *   bits = mode_bits[k] + cbf_cb_bits[cbf_cb] + cbf_cr_bits[2 cbf_cb + cbf_cr] + the frac_bits of the components with levels   (xGetIntraFracBitsQT(.., false, true) :798)
 *   dist = D_cb + D_cr, D_c = (uint64_t)(dist_weight[c] * (double)dist[..])                                             (RdCost::getDistPart :408)
 *   cost = dist_scale * (double)dist + (double)bits                                                                     (:800, uiDist - baseDist)
 * The slots run in ascending k and are taken on cost < dBestCost (:803, start MAX_DOUBLE).
 * slot_cost[6 p + k] the cost of a candidate slot, VVCGPU_INTRA_CHOOSE_PASSED otherwise.
 * result[p]    best_slot, best_mode (mode[best_slot]), cbf[2], dist, bits, cost; without a winner -1, -1, 0, 0, ~0, ~0, MAX_DOUBLE, nothing committed.
 * Commit (:828-838): both components' reconstruction (rows of the candidate block are w apart) to rec_dst_base and levels to level_dst_base, and with
 * ctx_out and ctx_best row 12 p + 2 k* + 1 of ctx_out, the contexts behind the Cr block, to row p of ctx_best.  Chroma blocks lie at multiples of 2
 * samples: rows move in 8-byte words where both rows allow it, else in 4-byte or 2-byte ones.
 * A PU outside the contract -- a side outside 2..64 or not a power of two, a reserved word that is not 0 -- comes back without a winner, never a fault.
 * VVCGPU_E_ARG before any device work: a null required pointer (ctx_out and ctx_best may be NULL, both or none), negative n, n above (2^31 - 1) / 12,
 * cpus / pus / result not 16-byte aligned, a 64-bit array not 8-byte aligned.  n == 0 is a no-op.
 * With the caller: the mode and cbf bits, the weights, the context snapshot, reading result[].  4:2:0.
 * Not served: transform-skip and cross-component candidates (the loop of :1751-1819).                                                              */
struct vvcgpu_intra_chroma_choose_pu {
  uint64_t mode_bits[6], cbf_cb_bits[2], cbf_cr_bits[4];
  double   dist_weight[2];
  int64_t  rec_dst_off[2], level_dst_off[2];
  int32_t  rec_dst_stride;
  int32_t  reserved[3];                    /* sizeof == 160 */
};
struct vvcgpu_intra_chroma_choose_result {
  int32_t  best_slot, best_mode, cbf[2];
  uint64_t dist, bits;
  double   cost;
  int64_t  reserved;                       /* 0; sizeof == 48 */
};
int vvcgpu_intra_chroma_choose_batch(
    const struct vvcgpu_intra_chroma_choose_pu* cpus, const vvcgpu_intra_chroma_pu* pus, int n,
    const uint32_t* abs_sum, const uint64_t* dist, const uint64_t* frac_bits_cb, const uint64_t* frac_bits_cr, double dist_scale,
    const vvc_pel* cand_rec_base, const vvc_coef* level_base,
    const uint8_t* ctx_out,                    /* may be NULL */
    vvc_pel* rec_dst_base, vvc_coef* level_dst_base,
    uint8_t* ctx_best,                         /* may be NULL */
    double* slot_cost, struct vvcgpu_intra_chroma_choose_result* result, void* stream);

/* N4, CCLM: cross-component linear model prediction of a chroma block  (IntraPrediction::xGetLumaRecPixels :1283-1581, the
 * JVET_K0190 branch, + xGetLMParameters :1597-1857 + predIntraChromaLM :390-403).  4:2:0 only.  luma_off: the co-located luma
 * block's top-left sample in the luma RECONSTRUCTION plane (rows -2, -1 are read when above_avail, columns -3 .. -1 when left_avail);
 * nb_off: reconstructed chroma neighbours of this component in nb_base, the w samples above followed by the h samples to the left
 * (what getPredictorPtr(compID) holds in row 0 / column 0); above_avail / left_avail: the reference's bAboveAvaillable /
 * bLeftAvaillable (ALL units of that side available, :1633-1637 -- control logic over the coding structure, decided by the
 * caller); w, h: chroma block, powers of two 2..64.                                                                        */
typedef struct vvcgpu_cclm_desc {
  int64_t luma_off, nb_off, dst_off;
  int32_t luma_stride, dst_stride;
  int16_t w, h;
  int8_t  above_avail, left_avail;
  int16_t reserved;
  int32_t reserved2[2];                 /* sizeof == 48 */
} vvcgpu_cclm_desc;
int vvcgpu_cclm_pred_batch(const vvc_pel* luma_base, const vvc_pel* nb_base, vvc_pel* dst_base, const vvcgpu_cclm_desc* descs, int n,
                           int bit_depth_luma, int bit_depth_chroma, int clp_min, int clp_max, void* stream);

/* N1, forward direction without RDOQ: scalar quantisation of transform coefficients  (Quant::quant, Quant.cpp:721-834: level =
 * (|c| * g_quantScales[qp % 6] * whScale + add) >> qBits with add = (intra slice ? 171 : 85) << (qBits - 9), flat scaling) and,
 * when the slice enables it, sign bit hiding per 4x4 coefficient group (xSignBitHidingHDQ :142-273, JVET_K0072 keeps it for
 * slices without dependent quantisation).  abs_sum[i] = uiAbsSum of TU i (sum of the magnitudes before hiding).  The rate-
 * distortion optimised quantisers (QuantRDOQ, the DepQuant trellis) walk CABAC context state sequentially and are NOT built.  */
typedef struct vvcgpu_quant_desc {
  int64_t coeff_off, level_off;         /* in elements of coeff_base / level_base; both blocks are w x h, row pitch w */
  int16_t w, h;                         /* powers of two 2..64 */
  int8_t  intra_slice, sign_hiding;
  int16_t reserved;
  int32_t qp;                           /* QpParam::Qp (bit-depth offset included) */
  int32_t reserved2;                    /* sizeof == 32 */
} vvcgpu_quant_desc;
int vvcgpu_quant_batch(const vvc_coef* coeff_base, vvc_coef* level_base, const vvcgpu_quant_desc* descs, int n, int bit_depth, uint32_t* abs_sum,
                       void* stream);

/* N1, the rate-distortion optimised quantiser of the default configuration: dependent quantisation as a 4-state trellis
 * (DQIntern::DepQuant::quant, CommonLib/DepQuant.cpp:1323-1391 with xDecideAndUpdate :1252-1320, State :861-1102, CommonCtx::update
 * :1104-1164, Quantizer::initQuantBlock / preQuantCoeff :647-706, :786-808).  The trellis is sequential along the scan but
 * independent between TUs.  The CABAC side enters as RATE TABLES: what DQIntern::RateEstimator (:335-485) derives from the
 * current context states -- last-position bits per column / row (incl. the cbf bit difference), coded-sub-block flag bits,
 * significance bits of the three state-dependent context sets, and the greater-than / parity bit sums -- in 2^-15 bit units
 * (SCALE_BITS); the caller fills one vvcgpu_dq_rates per (component, TU width x height class) and points TUs at it.
 * luma != 0 selects the luma template context offsets (:566-577).  lambda = Quant::m_dLambda of the component.
 * level_out receives the signed levels (row pitch w), abs_sum[i] the sum of absolute levels.  total_coeffs: extent of the
 * coefficient buffer the descriptors address (coeff_off + w * h <= total_coeffs, coeff_off a multiple of 16, blocks disjoint);
 * ws: device workspace of vvcgpu_depquant_workspace_bytes(total_coeffs, n) bytes, 16-byte aligned (trellis decisions and the
 * per-state level histories, both indexed by coeff_off).                                                                                                */
typedef struct vvcgpu_dq_rates {
  int32_t last_x[64], last_y[64];       /* m_lastBitsX / m_lastBitsY                                     */
  int32_t sig_sbb[2][2];                /* m_sigSbbFracBits[ctx].intBits[bin]                            */
  int32_t sig[3][18][2];                /* m_sigFracBits[ctxSet][ctx].intBits[bin]                       */
  int32_t gtx[21][7];                   /* m_gtxFracBits[ctx].bits[0..6]                                 */
} vvcgpu_dq_rates;
typedef struct vvcgpu_depquant_desc {
  int64_t coeff_off, level_off;         /* elements of coeff_base / level_base, blocks are w x h with row pitch w */
  double  lambda;
  int32_t qp;                           /* QpParam::Qp                                                   */
  int32_t rates_idx;                    /* index into the rates array                                    */
  int16_t w, h;                         /* powers of two 4..64 (2-wide chroma blocks are not served)     */
  int8_t  luma;
  int8_t  reserved[3];                  /* sizeof == 40 */
} vvcgpu_depquant_desc;
size_t vvcgpu_depquant_workspace_bytes(size_t total_coeffs, int n);
int vvcgpu_depquant_batch(const vvc_coef* coeff_base, vvc_coef* level_base, const vvcgpu_depquant_desc* descs, int n,
                          const vvcgpu_dq_rates* rates, int bit_depth, uint32_t* abs_sum, size_t total_coeffs, void* ws, size_t ws_bytes,
                          void* stream);

/* N1, the rate-distortion optimised quantiser used when dependent quantisation is off (DepQuant::quant hands the TU over,
 * CommonLib/DepQuant.cpp:1411-1421): QuantRDOQ::xRateDistOptQuant, CommonLib/QuantRDOQ.cpp:694-1409 with xGetCodedLevel :107-162, xGetICRate :235-313,
 * xGetRateLast :407-421, xGetErrScaleCoeff :482-506 and the JVET_K0072 template contexts (CommonLib/ContextModelling.h:135-219);
 * what QuantRDOQ::quant :652-690 dispatches to for blocks wider and higher than 2.  The decision chain of one TU is sequential (each
 * level changes the contexts of the following ones); TUs are independent.  All costs are IEEE doubles evaluated in the reference's
 * order.  The CABAC side enters as the fractional-bit tables (FracBitsAccess, 2^-15 bit units) the function reads:
 *   sig[ofs]      Ctx::SigFlag[chType]( ofs )                 (sigCtxIdAbs with state 0; 18 luma / 12 chroma offsets)
 *   par/gt1/gt2   Ctx::ParFlag[chType], Ctx::GtxFlag[2 + chType], Ctx::GtxFlag[chType] ( ctxOffsetAbs: 21 luma / 11 chroma offsets )
 *   sig_group[c]  Ctx::SigCoeffGroup[chType]( c )
 *   last_x/last_y the prefix tables lastBitsX / lastBitsY as built at :1172-1200
 *   cbf           Ctx::QtRootCbf() (luma of an inter CU at depth 0) or Ctx::QtCbf[compID]( CtxQtCbf ) :1134-1160
 * sign_hiding = slice->getSignDataHidingEnabledFlag().  lambda = Quant::m_dLambda.  Layout rules, abs_sum and the workspace as
 * for vvcgpu_depquant_batch (workspace: the per-coefficient cost / rate-delta arrays m_pdCostCoeff ... m_deltaU of the reference). */
typedef struct vvcgpu_rdoq_rates {
  int32_t sig[18][2];
  int32_t par[21][2], gt1[21][2], gt2[21][2];
  int32_t sig_group[2][2];
  int32_t last_x[14], last_y[14];
  int32_t cbf[2];                       /* sizeof == 784 */
} vvcgpu_rdoq_rates;
typedef struct vvcgpu_rdoq_desc {
  int64_t coeff_off, level_off;         /* elements of coeff_base / level_base, blocks are w x h with row pitch w */
  double  lambda;
  int32_t qp;                           /* QpParam::Qp                                                   */
  int32_t rates_idx;                    /* index into the rates array                                    */
  int16_t w, h;                         /* powers of two 4..64                                           */
  int8_t  luma, sign_hiding;
  int8_t  reserved[2];                  /* sizeof == 40 */
} vvcgpu_rdoq_desc;
size_t vvcgpu_rdoq_workspace_bytes(size_t total_coeffs, int n);
int vvcgpu_rdoq_batch(const vvc_coef* coeff_base, vvc_coef* level_base, const vvcgpu_rdoq_desc* descs, int n,
                      const vvcgpu_rdoq_rates* rates, int bit_depth, uint32_t* abs_sum, size_t total_coeffs, void* ws, size_t ws_bytes,
                      void* stream);

/* The shipped matrix [type][log2(N)-1] as N x N int16 (host copy; for the shim's table check against initROM()). */
const int16_t* vvcgpu_tr_matrix_host(int type, int n);

/* ---- I2 (+D2, D5): fractional-sample refinement of a PU, fused  (InterSearch::xPatternSearchFracDIF,
 *          EncoderLib/InterSearch.cpp:2503-2552 = xExtDIFUpSamplingH :3813-3869 -> xPatternRefinement(half) :634-689 ->
 *          xExtDIFUpSamplingQ :3882-4093 -> xPatternRefinement(quarter)) ------------------------------------------------
 * The reference materialises up to 12 fractional planes (m_filteredBlock[4][4]) per PU and reference picture and then
 * evaluates 9 half-sample and 9 quarter-sample candidates with distFunc (Hadamard when HadamardME is on) + MV cost.
 * Here the planes never exist in HBM: every candidate block is interpolated in LDS (horizontal first-stage filter, then
 * vertical last-stage filter, the exact stage flags of the reference) and consumed by the distortion directly.
 * All blocks of one call share w, h.  ref_x/ref_y: block position displaced by the integer MV; mv_x/mv_y: that integer
 * MV (rcMvInt, integer-sample units) for the MV cost.  mvcost_host: lambda and predictor (m_mvPredictor, quarter units);
 * cost_scale/imv_shift are ignored (the reference uses scale 1 for the half stage and 0 for the quarter stage, shift 0).
 * result: half_x/half_y in {-1,0,1} (rcMvHalf), qter_x/qter_y in {-1,0,1} (rcMvQter), cost = ruiCost of the quarter stage,
 * cost_half = best cost of the half stage.  Candidate order and strict '<' tie rule as s_acMvRefineH/Q (:59-83).        */
typedef struct vvcgpu_frac_blk { int32_t org_x, org_y, ref_x, ref_y, mv_x, mv_y; } vvcgpu_frac_blk;
typedef struct vvcgpu_frac_result { int32_t half_x, half_y, qter_x, qter_y; uint64_t cost_half, cost; } vvcgpu_frac_result;
int vvcgpu_frac_refine(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride,
                       const vvcgpu_frac_blk* blocks, int nblocks, int w, int h, int bit_depth, int clp_min, int clp_max,
                       int use_hadamard, const vvcgpu_mvcost* mvcost_host, vvcgpu_frac_result* results, void* stream);

/* N2, AMVR: integer / 4-sample refinement of the integer search result with both AMVP candidates
 * (InterSearch::xPatternSearchIntRefine, InterSearch.cpp:2408-2501; taken instead of the fractional refinement when cu.imv != 0).
 * 9 positions (the input vector and its 8 neighbours at distance 1 << imv_shift) x num_cand predictors; distortion = SATD
 * (use_hadamard: getUseHADME() && !transQuantBypass) or SAD at the clipped position, times `weight` in double precision and
 * truncated (:2456), + the MV cost against that predictor; strict '<' in visiting order.  Per PU: mv = rcMv on entry (integer
 * units), cand = amvpInfo.mvCand[0..1] (quarter units), idx_cost = m_auiMVPIdxCost[0..1][AMVP_MAX_NUM_CANDS], mvp_idx / bits =
 * riMVPIdx / ruiBits on entry.  Result: mv (quarter units), mvp_idx, bits = ruiBits, cost = ruiCost on exit.  cfg: the fields
 * lambda, imv_shift (1 or 2 + ...: 2 for integer, 4 for 4-sample in quarter units), picture geometry and readable rectangle of
 * vvcgpu_tz_cfg are used.                                                                                                  */
typedef struct vvcgpu_imv_pu {
  int32_t org_x, org_y, ref_x, ref_y;
  int32_t mv_x, mv_y;
  int32_t cand_x[2], cand_y[2];
  int32_t pos_x, pos_y;
  uint32_t idx_cost[2];
  uint32_t bits;
  int16_t w, h;
  int8_t  num_cand, mvp_idx;
  int16_t reserved;
  int32_t reserved2;                    /* sizeof == 72 */
} vvcgpu_imv_pu;
typedef struct vvcgpu_imv_result { int32_t mv_x, mv_y, mvp_idx; uint32_t bits; uint64_t cost; } vvcgpu_imv_result;
int vvcgpu_imv_refine_batch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_imv_pu* pus, int n,
                            const vvcgpu_tz_cfg* cfg_host, int use_hadamard, double weight, vvcgpu_imv_result* results, void* stream);

/* N2, chained: integer TZ search followed by the fused fractional refinement (I2) of the same PUs, on one stream with no host
 * round trip -- the device form of InterSearch::xMotionEstimation's  xPatternSearchFast -> xPatternSearchFracDIF  sequence
 * (InterSearch.cpp:1775-1816).  All PUs of one call share w x h (the refinement kernel's rule); every PU keeps its own
 * predictor (pred_hor / pred_ver) in both stages.  int_results as vvcgpu_tz_search_batch, frac_results as vvcgpu_frac_refine;
 * the final vector is  (int << 2) + (half << 1) + qter  (:1813-1815).                                                     */
int vvcgpu_me_batch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, const vvcgpu_tz_pu* pus, int n, int w, int h,
                    const vvcgpu_tz_cfg* cfg_host, int bit_depth, int clp_min, int clp_max, int use_hadamard,
                    vvcgpu_search_best* int_results, vvcgpu_frac_result* frac_results, void* stream);

/* ---- encoder picture analysis: the per-picture scalars the reference computes OUTSIDE its CTU loop, from planes already in HBM --------------
 * (the same reason vvcgpu_picture_hash exists: a 4K 10-bit picture is 24.9 MB, its download costs more than its whole hot path).  Every device
 * result is an INTEGER, bit-exact with the reference; where the reference goes on in double, the *_host helpers below finish the integers with the
 * reference's operations in the reference's order (no floating-point sum is formed on the device).  Picture forms take vvcgpu_planes (Y, Cb, Cr;
 * 4:2:0, chroma at half size) and n_planes in {1, 3} (1: only p[0] / stride[0] are read, at width x height -- a chroma plane may be passed that way).
 * Precondition of every entry: samples within the bit depth (0 .. 2^bd - 1, bd 8..10).  Null pointers and bad sizes return VVCGPU_E_ARG, a bit depth
 * outside 8..10 VVCGPU_E_UNSUPPORTED, before any device work.  Base pointers and strides are free: 16-byte row loads where both allow, sample-wise
 * loads otherwise (views into padded pictures, odd strides).  Each entry is at most one zeroing launch and one kernel; none synchronises.
 *
 * vvcgpu_tile_stats_picture: per plane, the plane is cut into tile x tile tiles (tile / 2 for the chroma planes of n_planes = 3), raster order, partial
 *   tiles at the right and at the bottom: ceil(w / t) * ceil(h / t) records per plane, written to out_y / out_cb / out_cr (the chroma outputs may be
 *   null for n_planes = 1).  Per tile:
 *     sa_act  sum |f| of the high-pass filter  f = 12 c - 2 (l + r + u + d) - (the four diagonal neighbours)  over the tile's samples EXCEPT those on the
 *             plane's outer row or column; neighbours are read across tile borders;
 *     sum     sum of the samples of the whole tile;
 *     ss_err  sum (org - rec)^2 over the whole tile; 0 when rec_or_null is null.
 *   tile: a multiple of 4 (n_planes = 1) or of 8 (n_planes = 3) up to 128.  Two reference computations are this definition:
 *   (a) perceptual QP adaptation per CTU (EncSlice.cpp:1405-1448, filterAndCalculateAverageEnergies :156-184): with tile = CTU size, the interior of the
 *       reference's fltArea (the CTU grown by one sample and clipped to the picture, whose own border row and column the filter skips) is exactly the
 *       CTU's samples minus the picture's outer row and column, so sa_act is the reference's saAct of that CTU and its sample count is
 *       (iFltWidth - 2) * (iFltHeight - 2); m_iOffsetCtu = (sum + (n >> 1)) / n with n the CTU's clipped area.  The whole-plane activity of
 *       applyQPAdaptationChroma (:219, luma and both chroma planes) is the integer sum of a plane's sa_act, the luma mean of :237-244 the sum of its sum fields.
 *   (b) WPSNR (EncGOP.cpp:2661-2717, calcWeightedSquaredError): with tile = B, the block size of :2741-2742 (vvcgpu_wpsnr_block_size_host), xAct, yAct,
 *       wAct and hAct select the same samples, ss_err is ssErr and sa_act is saAct; org is the ORIGINAL (the reference passes it as its pic1).  One tile
 *       size per call, halved for chroma: when the chroma B is not half the luma B (the table of a plane's own B: 3840x2160 128 / 64, 1920x1080 64 / 32,
 *       416x240 16 / 8, 64x64 4 / none), call per plane with n_planes = 1.
 * vvcgpu_picture_sse: sum (a - b)^2 per plane, out3[0..2] (the planes beyond n_planes: 0) -- xFindDistortionPlane without WPSNR (EncGOP.cpp:2812-2825)
 *   and its fall-back for planes too small for WPSNR (:2746-2760).  No filter reads.
 * vvcgpu_wpsnr_block_size_host: B of :2741-2742 in the reference's types from the PLANE's own width and height and its chroma shift (0 luma, 1 chroma of
 *   4:2:0); 0 when the reference falls back to the plain SSE (B < 4).
 * vvcgpu_wpsnr_finish_host: :2762-2794 from the tile records of one plane (tile = that plane's B, host copy): wmse += ss_err * pow(msAct^2, -0.5) in raster
 *   order with the lower limit of :2709, the GLOBAL_AVERAGING scaling by picture size, uint64(wmse * pow(sumAct, 0.5) + 0.5).  VVCGPU_E_ARG for a plane
 *   whose B is 0.
 *
 * vvcgpu_picture_histogram: xCalcHistogram (WeightPredAnalysis.cpp:79-99, values clamped into [0, 2^bd)) of every plane: hist[c * 2^bd + v], uint32,
 *   3 * 2^bd entries (planes beyond n_planes: 0).
 * vvcgpu_wp_acdc_host: xCalcACDCParamSlice (:267-297) of one plane from its histogram (host copy, 2^bd entries, n_samples = width * height of the plane):
 *   orgDC = sum v * h[v]; orgNormDC and *dc with the roundings of :280, 296 (fixed_shift: RExt__PREDICTION_WEIGHTING_ANALYSIS_DC_PRECISION with
 *   high-precision offsets, else 0); *ac = sum h[v] * |v - orgNormDC|.  One device pass for the reference's two dependent ones; exact because the samples
 *   are within the bit depth (the histogram's clamp changes nothing).
 * vvcgpu_wp_sad_batch: the weighted SADs of ONE (original plane, reference plane) pair for n_cand (0..16; 0: a no-op) candidates in one pass over the two
 *   planes; out: n_cand int64 on the device.  flags bit 0: high-precision offsets; bit 1: the clipped form.  Unclipped: xCalcSADvalueWP (:653-682) =
 *   the unclipped branch of xCalcSADvalueWPOptionalClip (:718-733); clipped: :699-717.  Accumulation in 64 bits as the reference.  Candidates are
 *   accepted within log2_denom 0..7, |weight| <= 1024, offset -32768..32767 (else VVCGPU_E_ARG): every term then fits 32 bits.  Covers the four SADs
 *   per (list, reference, component) of xUpdatingWPParameters (:513-545) and the pairs of xSelectWP (:620-630).
 *   xSearchHistogram / xCalcHistDistortion (:102-219) are NOT offered: the reference's loop reads one element past its vectors (i <= numElements, :110),
 *   so there is nothing defined to be exact against.
 *
 * vvcgpu_intra_cost_ctus: rate control's intra cost (EncSlice::calCostSliceI, EncSlice.cpp:1163-1204): per CTU in raster order
 *   m_costIntra = (sumHad + offset) >> shift with shift = bit_depth - 8, offset = shift ? 1 << (shift - 1) : 0 (:1172-1173) and sumHad the sum over the
 *   whole 8 x 8 blocks inside the clipped CTU (EncCu::updateCtuDataISlice, EncCu.cpp:468-485) of the 8 x 8 Hadamard of the original samples without its DC
 *   term, (s + 2) >> 2 (xCalcHADs8x8_ISlice :374-466).  cost: ceil(width / ctu) * ceil(height / ctu) int32; the picture's total is the host's sum.
 *   ctu_size: 16, 32, 64 or 128.                                                                                                                  */
typedef struct { uint64_t sa_act, sum, ss_err; } vvcgpu_tile_stats;                     /* sizeof == 24 */
typedef struct { int32_t log2_denom, weight, offset, flags; } vvcgpu_wp_sad_cand;        /* sizeof == 16 */
int vvcgpu_tile_stats_picture(const vvcgpu_planes* org, const vvcgpu_planes* rec_or_null, int width, int height, int tile, int n_planes,
                              vvcgpu_tile_stats* out_y, vvcgpu_tile_stats* out_cb, vvcgpu_tile_stats* out_cr, void* stream);
int vvcgpu_picture_sse(const vvcgpu_planes* a, const vvcgpu_planes* b, int width, int height, int n_planes, uint64_t* out3, void* stream);
int vvcgpu_wpsnr_block_size_host(int plane_w, int plane_h, int chroma_shift, int* block_size);
int vvcgpu_wpsnr_finish_host(const vvcgpu_tile_stats* tiles_host, int plane_w, int plane_h, int chroma_shift, int bit_depth, uint64_t* ssd);
int vvcgpu_picture_histogram(const vvcgpu_planes* pic, int width, int height, int n_planes, int bit_depth, uint32_t* hist, void* stream);
int vvcgpu_wp_acdc_host(const uint32_t* hist_host, int bit_depth, int n_samples, int fixed_shift, int64_t* dc, int64_t* ac);
int vvcgpu_wp_sad_batch(const vvc_pel* org, int org_stride, const vvc_pel* ref, int ref_stride, int w, int h, int bit_depth,
                        const vvcgpu_wp_sad_cand* cands_host, int n_cand, int64_t* out, void* stream);
int vvcgpu_intra_cost_ctus(const vvc_pel* org_y, int stride, int width, int height, int ctu_size, int bit_depth, int32_t* cost, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VVCGPU_H */
