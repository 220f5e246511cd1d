"""Host-side operator mirrors of the reference call sites, over torch CUDA tensors (torch is plumbing:
device memory + streams).  Every function goes through the C ABI (capi) -- no CPU fallback exists.

Planes are 2-D int16 CUDA tensors (rows may be strided views into a padded picture buffer)."""
import ctypes as C
import numpy as np
import torch

from . import capi
# the struct mirrors live in abi; bench.py, the tests and the tools read them as ops.<NAME>
from .abi import (AFE_DESC, AFFINE_ITER, AFFINE_ME_ITEM, AFFINE_ME_MAX_STEPS, AFFINE_ME_RESULT, AFFINE_ME_STEP, AFFINE_PU, AFG_DESC, CCLM_DESC, DEPQUANT_DESC, DIST_DESC, DQ_RATES, DQTR_DESC, FRAC_BLK,  # noqa: F401
                  FRAC_RESULT, IF_DESC, IMV_PU, IMV_RESULT, INTER_RESI_DQ, INTER_RESI_ITEM, INTER_RESI_Q_DEPQUANT, INTER_RESI_SLOTS, INTER_RESI_TS, INTER_RESI_WRITE_REC, INTRA_DESC, INTRA_FILL_DESC, INTRA_SATD_DESC, INTRA_CHROMA_LM, INTRA_CHROMA_PU, INTRA_CHROMA_Q_DEPQUANT, INTRA_CHROMA_WRITE_PRED, INTRA_CHOOSE_PU, INTRA_CHOOSE_RESULT, INTRA_CHROMA_CHOOSE_PU, INTRA_CHROMA_CHOOSE_RESULT, INTRA_CHOOSE_PASSED, INTRA_TU_FROM_LIST, INTRA_TU_NO_SMOOTHING, INTRA_TU_PRED_GIVEN, INTRA_TU_Q_DEPQUANT, INTRA_TU_WRITE_PRED, MC_DESC, PELOP_DESC, QUANT_DESC, RC_DESC, RESI_RATE_CTX_BYTES, RESI_RATE_ITEM,
                  RDOQ_DESC, RDOQ_RATES, RDPCM_DESC, SAO_DTYPE, SEARCH_BEST, SEARCH_BLK, TR_DESC, TZ_CFG, TZ_PU, DeblockCfg, MeHierCfg, MvCost,
                  PelopCfg, Planes, AffineMeCfg, BipredMeCfg, BIPRED_ME_ITEM, BIPRED_ME_MAX_PLANES, BIPRED_ME_MAX_REFS, BIPRED_ME_MAX_STEPS, BIPRED_ME_REF,
                  BIPRED_ME_RESULT, BIPRED_ME_STEP, AffineBipredCfg, AFFINE_BIPRED_ITEM, AFFINE_BIPRED_MAX_REFS, AFFINE_BIPRED_MAX_STEPS,
                  AFFINE_BIPRED_REF, AFFINE_BIPRED_RESULT, AFFINE_BIPRED_STEP, AffineUnipredCfg, AFFINE_UNIPRED_MAX_REFS, AFFINE_UNIPRED_RESULT,
                  UnipredMeCfg, UNIPRED_ME_MAX_PLANES, UNIPRED_ME_MAX_REFS, UNIPRED_ME_RESULT, WP_PARAM, TILE_STATS, WP_SAD_CAND, WP_SAD_HIGH_PRECISION, WP_SAD_CLIPPED)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plane(t, name="plane"):
    assert t.is_cuda and t.dtype == torch.int16 and t.dim() == 2 and t.stride(1) == 1, "%s: need 2-D int16 CUDA plane" % name
    return capi.ptr(t), t.stride(0), t.shape[1], t.shape[0]


# ---- ALF (AdaptiveLoopFilter.cpp) ---------------------------------------------------------------
def alf_classify(src, bit_depth):
    """A1: returns (H/4, W/4) int16 tensor holding classIdx | transposeIdx << 8 (uint16 bit pattern)."""
    p, st, w, h = _plane(src)
    cls = torch.empty((h // 4, w // 4), dtype=torch.int16, device=src.device)
    capi.call("vvcgpu_alf_classify", p, st, w, h, bit_depth, capi.ptr(cls), _stream())
    return cls


def alf_filter_luma(src, dst, ctu, cls, filter_type, coeff, ctu_enable=None, clp=(0, 1023)):
    p, st, w, h = _plane(src)
    q, dt, w2, h2 = _plane(dst, "dst")
    assert (w, h) == (w2, h2)
    cf = np.ascontiguousarray(coeff, dtype=np.int16)
    assert cf.size == 25 * 13
    capi.call("vvcgpu_alf_filter_luma", p, st, q, dt, w, h, ctu, capi.ptr(cls), filter_type,
              C.c_void_p(cf.ctypes.data), capi.ptr(ctu_enable), clp[0], clp[1], _stream())
    return dst


def alf_filter_chroma(src, dst, ctu_c, coeff, ctu_enable=None, clp=(0, 1023)):
    p, st, w, h = _plane(src)
    q, dt, w2, h2 = _plane(dst, "dst")
    assert (w, h) == (w2, h2)
    cf = np.ascontiguousarray(coeff, dtype=np.int16)
    assert cf.size == 7
    capi.call("vvcgpu_alf_filter_chroma", p, st, q, dt, w, h, ctu_c, C.c_void_p(cf.ctypes.data),
              capi.ptr(ctu_enable), clp[0], clp[1], _stream())
    return dst


# ---- SAO (SampleAdaptiveOffset.cpp) -------------------------------------------------------------
def sao_params_to_device(params, device="cuda"):
    """params: numpy structured array of SAO_DTYPE (one per CTU, raster order)."""
    assert params.dtype == SAO_DTYPE
    return torch.from_numpy(params.view(np.uint8).copy()).to(device)


def sao_apply(src, dst, ctu_w, ctu_h, bit_depth, params_dev, clp=(0, 1023)):
    p, st, w, h = _plane(src)
    q, dt, w2, h2 = _plane(dst, "dst")
    assert (w, h) == (w2, h2)
    capi.call("vvcgpu_sao_apply", p, st, q, dt, w, h, ctu_w, ctu_h, bit_depth, capi.ptr(params_dev),
              clp[0], clp[1], _stream())
    return dst


# ---- Deblocking (LoopFilter.cpp) ----------------------------------------------------------------
def deblock_cfg(bd=10, beta_off=0, tc_off=0, cb_off=0, cr_off=0):
    mx = (1 << bd) - 1
    return DeblockCfg(bd, bd, beta_off, tc_off, cb_off, cr_off, (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(mx, mx, mx))


def deblock(Y, Cb, Cr, edge_ver, edge_hor, qp_luma, qp_chroma, cfg):
    """In place.  Maps are uint8/int8 CUDA tensors of shape (H/4, W/4)."""
    p, st, w, h = _plane(Y)
    if Cb is not None:
        pb, sc, _, _ = _plane(Cb)
        pr, sc2, _, _ = _plane(Cr)
        assert sc == sc2
    else:
        pb = pr = None
        sc = 0
    capi.call("vvcgpu_deblock", p, st, pb, pr, sc, w, h, capi.ptr(edge_ver), capi.ptr(edge_hor),
              capi.ptr(qp_luma), capi.ptr(qp_chroma), C.byref(cfg), _stream())


# ---- encoder-side statistics ----------------------------------------------------------------------
def sao_stats(org, rec, ctu_w, ctu_h, bit_depth, avail=None, skip_r=5, skip_b=4):
    """S2: returns int64 tensor (nCtu, 5 types, 2 {diff,count}, 32 classes)."""
    po, so, w, h = _plane(org, "org")
    pr, sr, w2, h2 = _plane(rec, "rec")
    assert (w, h) == (w2, h2)
    n = ((w + ctu_w - 1) // ctu_w) * ((h + ctu_h - 1) // ctu_h)
    out = torch.empty((n, 5, 2, 32), dtype=torch.int64, device=org.device)
    capi.call("vvcgpu_sao_stats", po, so, pr, sr, w, h, ctu_w, ctu_h, bit_depth, capi.ptr(avail), skip_r, skip_b,
              capi.ptr(out), _stream())
    return out


def alf_stats(org, rec, ctu, cls, filter_type):
    """A3: returns int64 tensor (nCtu, nClasses, N*N+N+1)."""
    po, so, w, h = _plane(org, "org")
    pr, sr, w2, h2 = _plane(rec, "rec")
    assert (w, h) == (w2, h2)
    n = ((w + ctu - 1) // ctu) * ((h + ctu - 1) // ctu)
    N = 13 if filter_type else 7
    ncls = 25 if cls is not None else 1
    out = torch.empty((n, ncls, N * N + N + 1), dtype=torch.int64, device=org.device)
    capi.call("vvcgpu_alf_stats", po, so, pr, sr, w, h, ctu, capi.ptr(cls), filter_type, capi.ptr(out), _stream())
    return out


# ---- block distortion (RdCost) ---------------------------------------------------------------------
SAD, HAD, SSE, MRSAD, MRHAD = 0, 1, 2, 3, 4


def struct_to_device(arr, device="cuda"):
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(device)


def dist_batch(kind, org_base, cur_base, descs_dev, n, bit_depth=10):
    """D1-D3: org_base / cur_base are int16 CUDA tensors (any shape, offsets are in elements from element 0)."""
    out = torch.empty(n, dtype=torch.int64, device=org_base.device)
    capi.call("vvcgpu_dist_batch", kind, capi.ptr(org_base), capi.ptr(cur_base), capi.ptr(descs_dev), n, bit_depth,
              capi.ptr(out), _stream())
    return out


def sad_search(org, ref, blocks_dev, nblocks, w, h, sub_shift, dx0, dy0, nx, ny, sx, sy, mvcost=None, want_sad=True):
    """D1 search form.  org/ref: 2-D int16 planes (ref may be a view into a padded buffer; positions are relative to
    the view's origin and may be negative as long as they stay inside the allocation).  Returns (sad[nblocks,ny,nx]
    int32 tensor, best uint8 tensor or None).  want_sad=False asks for the best candidate only (sad_out = NULL in the
    C ABI, what xPatternSearch / xTZSearch keep); the first return value is then None."""
    po, so, _, _ = _plane(org, "org")
    pr, sr, _, _ = _plane(ref, "ref")
    sad = torch.empty((nblocks, ny, nx), dtype=torch.int32, device=org.device) if want_sad else None
    best = None
    mv = None
    if mvcost is not None:
        best = torch.empty(nblocks * SEARCH_BEST.itemsize, dtype=torch.uint8, device=org.device)
        mv = C.byref(mvcost)
    capi.call("vvcgpu_sad_search", po, so, pr, sr, capi.ptr(blocks_dev), nblocks, w, h, sub_shift, dx0, dy0, nx, ny,
              sx, sy, capi.ptr(sad), mv, capi.ptr(best), _stream())
    return sad, best


def me_hier_search(org, ref, org_xy, ref_xy, n16x, n16y, sub_shift, raster_range, dense_range, mvcost, raster_step=5):
    """D1 + D5 hierarchical form (vvcgpu_me_hier_search): the step-5 raster and the +-dense_range grid of every 16x16 / 32x32 / 64x64 block of the grid
    in one launch.  Returns (raster, dense): two lists of three SEARCH_BEST uint8 tensors (16, 32, 64; None where the grid has no block of the size,
    dense = None with dense_range 0)."""
    po, so, _, _ = _plane(org, "org")
    pr, sr, _, _ = _plane(ref, "ref")
    cfg = MeHierCfg(org_xy[0], org_xy[1], ref_xy[0], ref_xy[1], n16x, n16y, sub_shift, raster_range, raster_step, dense_range)
    counts = [n16x * n16y, (n16x // 2) * (n16y // 2), (n16x // 4) * (n16y // 4)]
    mk = lambda: [torch.empty(n * SEARCH_BEST.itemsize, dtype=torch.uint8, device=org.device) if n else None for n in counts]
    raster, dense = mk(), (mk() if dense_range else None)
    arr = lambda ts: (C.c_void_p * 3)(*[capi.ptr(t) for t in ts])
    capi.call("vvcgpu_me_hier_search", po, so, pr, sr, C.byref(cfg), C.byref(mvcost), arr(raster), arr(dense) if dense else None, _stream())
    return raster, dense


# ---- N2: integer TZ search of whole PUs (InterSearch::xTZSearch) ---------------------------------------------
def tz_search_batch(org, ref, pus_dev, n, cfg):
    """N2: xTZSearch for n PUs (one wavefront each).  org/ref: 2-D int16 planes (ref = the whole padded reference plane,
    PU positions in plane coordinates); pus_dev: TZ_PU records on the device; cfg: one-element TZ_CFG numpy record (host).
    Returns SEARCH_BEST records as a uint8 tensor: x, y (integer MV), cost (uiBestSad), sad (ruiSAD)."""
    po, so, _, _ = _plane(org, "org")
    pr, sr, _, _ = _plane(ref, "ref")
    cfg = np.ascontiguousarray(cfg)
    assert cfg.dtype == TZ_CFG and cfg.size == 1
    best = torch.empty(n * SEARCH_BEST.itemsize, dtype=torch.uint8, device=org.device)
    capi.call("vvcgpu_tz_search_batch", po, so, pr, sr, capi.ptr(pus_dev), n, C.c_void_p(cfg.ctypes.data), capi.ptr(best), _stream())
    return best


def me_batch(org, ref, pus_dev, n, w, h, cfg, bit_depth, use_hadamard=True):
    """N2 chained: TZ search + fused fractional refinement of the same PUs (xPatternSearchFast -> xPatternSearchFracDIF).
    Returns (SEARCH_BEST uint8 tensor, FRAC_RESULT uint8 tensor)."""
    po, so, _, _ = _plane(org, "org")
    pr, sr, _, _ = _plane(ref, "ref")
    cfg = np.ascontiguousarray(cfg)
    assert cfg.dtype == TZ_CFG and cfg.size == 1
    best = torch.empty(n * SEARCH_BEST.itemsize, dtype=torch.uint8, device=org.device)
    frac = torch.empty(n * FRAC_RESULT.itemsize, dtype=torch.uint8, device=org.device)
    capi.call("vvcgpu_me_batch", po, so, pr, sr, capi.ptr(pus_dev), n, w, h, C.c_void_p(cfg.ctypes.data), bit_depth, 0, (1 << bit_depth) - 1,
              1 if use_hadamard else 0, capi.ptr(best), capi.ptr(frac), _stream())
    return best, frac


# ---- N4 picture-level passes: border extension, picture hash -------------------------------------------------
HASH_CRC, HASH_CHECKSUM = 1, 2


def extend_border(padded, margin_x, margin_y):
    """Picture::extendPicBorder for one plane.  padded: 2-D int16 tensor holding the picture with its margins."""
    assert padded.dim() == 2 and padded.dtype == torch.int16 and padded.stride(1) == 1
    h, w = padded.shape[0] - 2 * margin_y, padded.shape[1] - 2 * margin_x
    origin = padded.data_ptr() + (margin_y * padded.stride(0) + margin_x) * 2
    capi.call("vvcgpu_extend_border", C.c_void_p(origin), padded.stride(0), w, h, margin_x, margin_y, _stream())


def picture_hash(method, plane, bit_depth):
    """compCRC (method 1) / compChecksum (method 2) of one plane -> 1-element int32 tensor (device), bits as uint32."""
    pp, sp, w, h = _plane(plane, "plane")
    out = torch.zeros(1, dtype=torch.int32, device=plane.device)
    capi.call("vvcgpu_picture_hash", method, pp, sp, w, h, bit_depth, capi.ptr(out), _stream())
    return out


# ---- N4 intra sample prediction ----------------------------------------------------------------------------
def intra_ref_lengths(w, h):
    t, l = C.c_int(), C.c_int()
    capi.call("vvcgpu_intra_ref_lengths", w, h, C.byref(t), C.byref(l))
    return t.value, l.value


def intra_satd_batch(refs_base, org_base, descs_dev, n, clp=(0, 1023)):
    """N4: intra mode pre-selection -- Hadamard distortion of predIntraAng(mode) against the original, one value per (block, mode)."""
    out = torch.empty(n, dtype=torch.int64, device=org_base.device)
    capi.call("vvcgpu_intra_satd_batch", capi.ptr(refs_base), capi.ptr(org_base), capi.ptr(descs_dev), n, clp[0], clp[1], capi.ptr(out), _stream())
    return out


def intra_pred_batch(refs_base, dst_base, descs_dev, n, clp=(0, 1023)):
    """N4: IntraPrediction::predIntraAng for n blocks (packed reference samples in, prediction blocks out)."""
    capi.call("vvcgpu_intra_pred_batch", capi.ptr(refs_base), capi.ptr(dst_base), capi.ptr(descs_dev), n, clp[0], clp[1], _stream())


def cclm_pred_batch(luma_base, nb_base, dst_base, descs_dev, n, bd_luma=10, bd_chroma=10, clp=(0, 1023)):
    """N4: CCLM chroma prediction (xGetLumaRecPixels + xGetLMParameters + predIntraChromaLM) for n chroma blocks."""
    capi.call("vvcgpu_cclm_pred_batch", capi.ptr(luma_base), capi.ptr(nb_base), capi.ptr(dst_base), capi.ptr(descs_dev), n, bd_luma, bd_chroma,
              clp[0], clp[1], _stream())


def intra_fill_refs_batch(rec_base, flags_base, refs_base, descs_dev, n, bit_depth=10):
    """N4: xFillReferenceSamples for n blocks: reconstruction + unit availability flags -> packed reference samples."""
    capi.call("vvcgpu_intra_fill_refs_batch", capi.ptr(rec_base), capi.ptr(flags_base), capi.ptr(refs_base), capi.ptr(descs_dev), n, bit_depth, _stream())


INTRA_CAND_USE_MPM, INTRA_CAND_NO_SMOOTHING = 1, 2


def intra_mode_cand_batch(org_base, pus_dev, n, pu_ctl, pu_mode_bits, sqrt_lambda, refs_base=None, fill=None, pu_inter_had=None,
                          flags=INTRA_CAND_USE_MPM, bit_depth=10, clp=(0, 1023), want_satd=True):
    """the intra mode pre-selection pass of n luma PUs (vvcgpu_intra_mode_cand_batch): pus_dev a device copy of an INTRA_SATD_DESC array, pu_ctl int32
    [n][4] (three MPMs, numModesForFullRD), pu_mode_bits int64 [n][4], pu_inter_had int64 [n] or None.  fill = (rec_base, flags_base, a device copy
    of an INTRA_FILL_DESC array) gathers the references first (refs_base, if given, receives them); without fill, refs_base holds them.
    -> (satd int64 [n][67] or None, lists int32 [n][16], costs float64 [n][12])"""
    dv = org_base.device
    satd = torch.empty((n, 67), dtype=torch.int64, device=dv) if want_satd else None
    lists = torch.empty((n, 16), dtype=torch.int32, device=dv)
    costs = torch.empty((n, 12), dtype=torch.float64, device=dv)
    rec, flg, fd = fill if fill is not None else (None, None, None)
    capi.call("vvcgpu_intra_mode_cand_batch", capi.ptr(rec), capi.ptr(flg), capi.ptr(fd), capi.ptr(refs_base), capi.ptr(org_base), capi.ptr(pus_dev), n,
              capi.ptr(pu_ctl), capi.ptr(pu_mode_bits), capi.ptr(pu_inter_had), flags, float(sqrt_lambda), bit_depth, clp[0], clp[1], capi.ptr(satd),
              capi.ptr(lists), capi.ptr(costs), _stream())
    return satd, lists, costs


def intra_tu_code_batch(refs_base, preds_dev, org_base, pred_base, rec_base, level_base, tus_dev, n, mode_list=None, flags=0, bit_depth=10, clp=(0, 1023)):
    """the pixel pass of the intra RD loop for n luma TUs (vvcgpu_intra_tu_code_batch): preds_dev / tus_dev device copies of an INTRA_DESC and an RC_DESC
    array (item i is the pair), mode_list the lists tensor of intra_mode_cand_batch for INTRA_TU_FROM_LIST items, pred_base None when no item is
    INTRA_TU_PRED_GIVEN and INTRA_TU_WRITE_PRED is off.
    -> (abs_sum int32 [n] (bits as uint32), num_sig int32 [n] (bits as uint32), dist int64 [n] (bits as uint64), mode_out int32 [n])"""
    dv = org_base.device
    abs_sum = torch.empty(n, dtype=torch.int32, device=dv)                 # every entry is written by the library
    num_sig = torch.empty(n, dtype=torch.int32, device=dv)
    dist = torch.empty(n, dtype=torch.int64, device=dv)
    mode_out = torch.empty(n, dtype=torch.int32, device=dv)
    capi.call("vvcgpu_intra_tu_code_batch", capi.ptr(refs_base), capi.ptr(preds_dev), capi.ptr(org_base), capi.ptr(pred_base), capi.ptr(rec_base),
              capi.ptr(level_base), capi.ptr(tus_dev), n, capi.ptr(mode_list), flags, bit_depth, clp[0], clp[1], capi.ptr(abs_sum), capi.ptr(num_sig),
              capi.ptr(dist), capi.ptr(mode_out), _stream())
    return abs_sum, num_sig, dist, mode_out


def intra_tu_code_dq_workspace(level_extent, n, device="cuda"):
    """a workspace for intra_tu_code_dq_batch (vvcgpu_intra_tu_code_dq_workspace_bytes); its contents never matter"""
    return torch.empty(capi.lib().vvcgpu_intra_tu_code_dq_workspace_bytes(level_extent, n), dtype=torch.uint8, device=device)


def intra_tu_code_dq_batch(refs_base, preds_dev, org_base, pred_base, rec_base, level_base, tus_dev, dq_dev, n, rates_dev, n_rates, mode_list=None, flags=0,
                           bit_depth=10, clp=(0, 1023), ws=None, quantiser=INTRA_TU_Q_DEPQUANT):
    """the pixel pass of the intra RD loop with the DepQuant trellis (vvcgpu_intra_tu_code_dq_batch): as intra_tu_code_batch, with dq_dev a device copy of
    an INTER_RESI_DQ array parallel to the items, rates_dev one of a DQ_RATES array of n_rates tables (cbf from QtCbf), ws a workspace of
    intra_tu_code_dq_workspace for level_base's extent (allocated here when None).
    -> (abs_sum int32 [n] (bits as uint32), num_sig int32 [n] (bits as uint32), dist int64 [n] (bits as uint64), mode_out int32 [n])"""
    dv = org_base.device
    extent = int(level_base.numel())
    if ws is None:
        ws = intra_tu_code_dq_workspace(extent, n, dv)
    abs_sum = torch.empty(n, dtype=torch.int32, device=dv)                 # every entry is written by the library
    num_sig = torch.empty(n, dtype=torch.int32, device=dv)
    dist = torch.empty(n, dtype=torch.int64, device=dv)
    mode_out = torch.empty(n, dtype=torch.int32, device=dv)
    capi.call("vvcgpu_intra_tu_code_dq_batch", capi.ptr(refs_base), capi.ptr(preds_dev), capi.ptr(org_base), capi.ptr(pred_base), capi.ptr(rec_base),
              capi.ptr(level_base), C.c_size_t(extent), capi.ptr(tus_dev), capi.ptr(dq_dev), n, capi.ptr(mode_list), capi.ptr(rates_dev), n_rates, quantiser,
              flags, bit_depth, clp[0], clp[1], capi.ptr(abs_sum), capi.ptr(num_sig), capi.ptr(dist), capi.ptr(mode_out), capi.ptr(ws), C.c_size_t(ws.numel()),
              _stream())
    return abs_sum, num_sig, dist, mode_out


def intra_chroma_code_batch(org_base, pus_dev, n, runs, cand_rec_base, level_base, refs_base=None, fill=None, luma_base=None, pred_base=None, flags=0,
                            bit_depth=10, clp=(0, 1023)):
    """the intra chroma mode pass of n chroma PUs grouped by shape (vvcgpu_intra_chroma_code_batch): pus_dev a device copy of an INTRA_CHROMA_PU array, runs
    the (w, h, count) triples of the list.  fill = (rec_base, flags_base, a device copy of an INTRA_FILL_DESC array, two per PU) gathers the references
    first (refs_base, if given, receives them); without fill, refs_base holds them.  luma_base: the luma reconstruction, for PUs with an LM slot.
    -> (abs_sum int32 [n][6][2] (bits as uint32), dist int64 [n][6][2] (bits as uint64))"""
    dv = org_base.device
    abs_sum = torch.empty((n, 6, 2), dtype=torch.int32, device=dv)         # every entry is written by the library
    dist = torch.empty((n, 6, 2), dtype=torch.int64, device=dv)
    r = np.ascontiguousarray(np.asarray(runs, np.int32).reshape(-1, 3))
    rec, flg, fd = fill if fill is not None else (None, None, None)
    capi.call("vvcgpu_intra_chroma_code_batch", capi.ptr(rec), capi.ptr(flg), capi.ptr(fd), capi.ptr(refs_base), capi.ptr(luma_base), capi.ptr(org_base),
              capi.ptr(pus_dev), n, r.ctypes.data_as(C.c_void_p), len(r), capi.ptr(pred_base), capi.ptr(cand_rec_base), capi.ptr(level_base), flags,
              bit_depth, clp[0], clp[1], capi.ptr(abs_sum), capi.ptr(dist), _stream())
    return abs_sum, dist


def intra_chroma_code_dq_workspace(level_extent, n, device="cuda"):
    """a workspace for intra_chroma_code_dq_batch (vvcgpu_intra_chroma_code_dq_workspace_bytes); its contents never matter"""
    return torch.empty(capi.lib().vvcgpu_intra_chroma_code_dq_workspace_bytes(level_extent, n), dtype=torch.uint8, device=device)


def intra_chroma_code_dq_batch(org_base, pus_dev, dq_dev, n, runs, rates_dev, n_rates, cand_rec_base, level_base, refs_base=None, fill=None, luma_base=None,
                               pred_base=None, flags=0, bit_depth=10, clp=(0, 1023), ws=None, quantiser=INTRA_CHROMA_Q_DEPQUANT):
    """the intra chroma mode pass with the DepQuant trellis (vvcgpu_intra_chroma_code_dq_batch): as intra_chroma_code_batch, with dq_dev a device copy of an
    INTER_RESI_DQ array, three per PU (Cb; Cr behind a Cb block without a level; Cr behind one with a level), rates_dev one of a DQ_RATES array of n_rates
    tables, ws a workspace of intra_chroma_code_dq_workspace for level_base's extent (allocated here when None).
    -> (abs_sum int32 [n][6][2] (bits as uint32), dist int64 [n][6][2] (bits as uint64))"""
    dv = org_base.device
    extent = int(level_base.numel())
    if ws is None:
        ws = intra_chroma_code_dq_workspace(extent, n, dv)
    abs_sum = torch.empty((n, 6, 2), dtype=torch.int32, device=dv)         # every entry is written by the library
    dist = torch.empty((n, 6, 2), dtype=torch.int64, device=dv)
    r = np.ascontiguousarray(np.asarray(runs, np.int32).reshape(-1, 3))
    rec, flg, fd = fill if fill is not None else (None, None, None)
    capi.call("vvcgpu_intra_chroma_code_dq_batch", capi.ptr(rec), capi.ptr(flg), capi.ptr(fd), capi.ptr(refs_base), capi.ptr(luma_base), capi.ptr(org_base),
              capi.ptr(pus_dev), capi.ptr(dq_dev), n, r.ctypes.data_as(C.c_void_p), len(r), capi.ptr(rates_dev), n_rates, quantiser, capi.ptr(pred_base),
              capi.ptr(cand_rec_base), capi.ptr(level_base), C.c_size_t(extent), flags, bit_depth, clp[0], clp[1], capi.ptr(abs_sum), capi.ptr(dist),
              capi.ptr(ws), C.c_size_t(ws.numel()), _stream())
    return abs_sum, dist


def inter_resi_code_batch(org_base, pred_base, items_dev, n, resi_base, level_base, rec_base=None, rd_list=None, flags=0, bit_depth=10, clp=(0, 1023)):
    """the inter residual pixel pass of n transform blocks (vvcgpu_inter_resi_code_batch): items_dev a device copy of an INTER_RESI_ITEM array, rd_list the
    rd_list tensor of merge_cand_batch for list items (consumed where it lies), rec_base None unless INTER_RESI_WRITE_REC is set.
    -> (abs_sum int32 [n][6] (bits as uint32), dist_resi, dist_rec int64 [n][6] (bits as uint64), zero_dist int64 [n] (bits as uint64))"""
    dv = org_base.device
    abs_sum = torch.empty((n, INTER_RESI_SLOTS), dtype=torch.int32, device=dv)   # every entry is written by the library
    dist_resi = torch.empty((n, INTER_RESI_SLOTS), dtype=torch.int64, device=dv)
    dist_rec = torch.empty((n, INTER_RESI_SLOTS), dtype=torch.int64, device=dv)
    zero_dist = torch.empty(n, dtype=torch.int64, device=dv)
    capi.call("vvcgpu_inter_resi_code_batch", capi.ptr(org_base), capi.ptr(pred_base), capi.ptr(items_dev), n, capi.ptr(rd_list), capi.ptr(resi_base),
              capi.ptr(rec_base), capi.ptr(level_base), flags, bit_depth, clp[0], clp[1], capi.ptr(abs_sum), capi.ptr(dist_resi), capi.ptr(dist_rec),
              capi.ptr(zero_dist), _stream())
    return abs_sum, dist_resi, dist_rec, zero_dist


def inter_resi_code_dq_workspace(level_extent, n, device="cuda"):
    """a workspace for inter_resi_code_dq_batch (vvcgpu_inter_resi_code_dq_workspace_bytes); its contents never matter"""
    return torch.empty(capi.lib().vvcgpu_inter_resi_code_dq_workspace_bytes(level_extent, n), dtype=torch.uint8, device=device)


def inter_resi_code_dq_batch(org_base, pred_base, items_dev, dq_dev, n, rates_dev, n_rates, resi_base, level_base, rec_base=None, rd_list=None, flags=0,
                             bit_depth=10, clp=(0, 1023), ws=None, quantiser=INTER_RESI_Q_DEPQUANT):
    """the inter residual pixel pass with the DepQuant trellis (vvcgpu_inter_resi_code_dq_batch): as inter_resi_code_batch, with dq_dev a device copy of
    an INTER_RESI_DQ array parallel to the items, rates_dev one of a DQ_RATES array of n_rates tables, ws a workspace of inter_resi_code_dq_workspace
    for level_base's extent (allocated here when None).
    -> (abs_sum int32 [n][6] (bits as uint32), dist_resi, dist_rec int64 [n][6] (bits as uint64), zero_dist int64 [n] (bits as uint64))"""
    dv = org_base.device
    extent = int(level_base.numel())
    if ws is None:
        ws = inter_resi_code_dq_workspace(extent, n, dv)
    abs_sum = torch.empty((n, INTER_RESI_SLOTS), dtype=torch.int32, device=dv)   # every entry is written by the library
    dist_resi = torch.empty((n, INTER_RESI_SLOTS), dtype=torch.int64, device=dv)
    dist_rec = torch.empty((n, INTER_RESI_SLOTS), dtype=torch.int64, device=dv)
    zero_dist = torch.empty(n, dtype=torch.int64, device=dv)
    capi.call("vvcgpu_inter_resi_code_dq_batch", capi.ptr(org_base), capi.ptr(pred_base), capi.ptr(items_dev), capi.ptr(dq_dev), n, capi.ptr(rd_list),
              capi.ptr(rates_dev), n_rates, quantiser, capi.ptr(resi_base), capi.ptr(rec_base), capi.ptr(level_base), C.c_size_t(extent), flags, bit_depth,
              clp[0], clp[1], capi.ptr(abs_sum), capi.ptr(dist_resi), capi.ptr(dist_rec), capi.ptr(zero_dist), capi.ptr(ws), C.c_size_t(ws.numel()), _stream())
    return abs_sum, dist_resi, dist_rec, zero_dist


def resi_rate_batch(level_base, items_dev, n, ctx, est_bits, next_state, gate=None, ctx_out=None):
    """the CABAC rate of residual_coding for n level blocks (vvcgpu_resi_rate_batch): items_dev a device copy of a RESI_RATE_ITEM array, ctx a uint8
    [n_ctx][RESI_RATE_CTX_BYTES] tensor of context rows, est_bits int32 [128] and next_state uint8 [256] the reference's two model tables, gate the
    abs_sum tensor of an RD pass (0xFFFFFFFF skips the item) or None, ctx_out a uint8 [n][RESI_RATE_CTX_BYTES] tensor for the rows after the blocks (the
    rows of skipped items stay as they are) or None.
    -> (frac_bits int64 [n] (bits as uint64), num_sig int32 [n] (bits as uint32))"""
    dv = level_base.device
    assert ctx.dtype == torch.uint8 and ctx.dim() == 2 and ctx.shape[1] == RESI_RATE_CTX_BYTES and ctx.is_contiguous()
    frac_bits = torch.empty(n, dtype=torch.int64, device=dv)                # every entry is written by the library
    num_sig = torch.empty(n, dtype=torch.int32, device=dv)
    assert ctx_out is None or (ctx_out.dtype == torch.uint8 and ctx_out.numel() == n * RESI_RATE_CTX_BYTES and ctx_out.is_contiguous())
    capi.call("vvcgpu_resi_rate_batch", capi.ptr(level_base), capi.ptr(items_dev), n, capi.ptr(gate), capi.ptr(ctx), int(ctx.shape[0]), capi.ptr(est_bits),
              capi.ptr(next_state), capi.ptr(frac_bits), capi.ptr(num_sig), capi.ptr(ctx_out), _stream())
    return frac_bits, num_sig


def inter_resi_choose_batch(items_dev, n, abs_sum, dist_resi, zero_dist, frac_bits, cbf_bits, prev, dist_weight, dist_scale):
    """the compare of xEstimateInterResidualQT (vvcgpu_inter_resi_choose_batch) over the outputs of inter_resi_code_batch / _dq_batch (items_dev, abs_sum,
    dist_resi, zero_dist) and of resi_rate_batch (frac_bits [6 n]); cbf_bits int64 [n][4], prev int32 [n], dist_weight float64 [n], all on the device.
    -> (slot, cbf int32 [n], abs_sum int32 [n] (bits as uint32), dist, bits int64 [n] (bits as uint64), min_cost float64 [n])"""
    dv = abs_sum.device
    slot, cbf, abs_out = (torch.empty(n, dtype=torch.int32, device=dv) for _ in range(3))
    dist, bits = (torch.empty(n, dtype=torch.int64, device=dv) for _ in range(2))
    min_cost = torch.empty(n, dtype=torch.float64, device=dv)
    capi.call("vvcgpu_inter_resi_choose_batch", capi.ptr(items_dev), n, capi.ptr(abs_sum), capi.ptr(dist_resi), capi.ptr(zero_dist), capi.ptr(frac_bits),
              capi.ptr(cbf_bits), capi.ptr(prev), capi.ptr(dist_weight), C.c_double(dist_scale), capi.ptr(slot), capi.ptr(cbf), capi.ptr(abs_out),
              capi.ptr(dist), capi.ptr(bits), capi.ptr(min_cost), _stream())
    return slot, cbf, abs_out, dist, bits, min_cost


def intra_luma_choose_batch(pus_dev, n_pu, tus_dev, n, abs_sum, num_sig, dist, mode_out, frac_bits, dist_scale, rec_base, level_base, rec_dst_base,
                            level_dst_base, ctx_out=None, ctx_best=None, cand_cost=None):
    """the compare of the intra luma RD loops and the commit of the winner (vvcgpu_intra_luma_choose_batch) over the outputs of intra_tu_code_batch /
    _dq_batch (tus_dev, abs_sum, num_sig, dist, mode_out, rec_base, level_base) and of resi_rate_batch (frac_bits [n]; ctx_out, its rows, with ctx_best
    uint8 [n_pu][RESI_RATE_CTX_BYTES]): pus_dev a device copy of an INTRA_CHOOSE_PU array; the winners go to rec_dst_base / level_dst_base / ctx_best.
    -> (cand_cost float64 [n] (INTRA_CHOOSE_PASSED where no cost was formed; entries outside the range of every PU inside the contract are not written:
    they keep what a given cand_cost tensor holds), result: uint8 tensor of n_pu INTRA_CHOOSE_RESULT records)"""
    dv = abs_sum.device
    if cand_cost is None:
        cand_cost = torch.empty(n, dtype=torch.float64, device=dv)
    assert cand_cost.dtype == torch.float64 and cand_cost.numel() == n and cand_cost.is_contiguous()
    result = torch.empty(n_pu * INTRA_CHOOSE_RESULT.itemsize, dtype=torch.uint8, device=dv)
    capi.call("vvcgpu_intra_luma_choose_batch", capi.ptr(pus_dev), n_pu, capi.ptr(tus_dev), n, capi.ptr(abs_sum), capi.ptr(num_sig), capi.ptr(dist),
              capi.ptr(mode_out), capi.ptr(frac_bits), C.c_double(dist_scale), capi.ptr(rec_base), capi.ptr(level_base), capi.ptr(ctx_out),
              capi.ptr(rec_dst_base), capi.ptr(level_dst_base), capi.ptr(ctx_best), capi.ptr(cand_cost), capi.ptr(result), _stream())
    return cand_cost, result


def intra_chroma_choose_batch(cpus_dev, pus_dev, n, abs_sum, dist, frac_bits_cb, frac_bits_cr, dist_scale, cand_rec_base, level_base, rec_dst_base,
                              level_dst_base, ctx_out=None, ctx_best=None, slot_cost=None):
    """the compare of the intra chroma mode loop and the commit of the winner (vvcgpu_intra_chroma_choose_batch) over the outputs of
    intra_chroma_code_batch / _dq_batch (pus_dev, abs_sum, dist [n][6][2], cand_rec_base, level_base) and of the two resi_rate_batch calls over its 12 n
    level blocks (frac_bits_cb, frac_bits_cr [12 n]; ctx_out, the rows of the second, with ctx_best uint8 [n][RESI_RATE_CTX_BYTES]): cpus_dev a device copy
    of an INTRA_CHROMA_CHOOSE_PU array.
    -> (slot_cost float64 [n][6] (INTRA_CHOOSE_PASSED where the slot is no candidate), result: uint8 tensor of n INTRA_CHROMA_CHOOSE_RESULT records)"""
    dv = abs_sum.device
    if slot_cost is None:
        slot_cost = torch.empty((n, 6), dtype=torch.float64, device=dv)
    assert slot_cost.dtype == torch.float64 and slot_cost.numel() == 6 * n and slot_cost.is_contiguous()
    result = torch.empty(n * INTRA_CHROMA_CHOOSE_RESULT.itemsize, dtype=torch.uint8, device=dv)
    capi.call("vvcgpu_intra_chroma_choose_batch", capi.ptr(cpus_dev), capi.ptr(pus_dev), n, capi.ptr(abs_sum), capi.ptr(dist), capi.ptr(frac_bits_cb),
              capi.ptr(frac_bits_cr), C.c_double(dist_scale), capi.ptr(cand_rec_base), capi.ptr(level_base), capi.ptr(ctx_out), capi.ptr(rec_dst_base),
              capi.ptr(level_dst_base), capi.ptr(ctx_best), capi.ptr(slot_cost), capi.ptr(result), _stream())
    return slot_cost, result


def imv_refine_batch(org, ref, pus_dev, n, cfg, use_hadamard=True, weight=1.0):
    """N2 (AMVR): xPatternSearchIntRefine for n PUs -> IMV_RESULT records (uint8 tensor)."""
    po, so, _, _ = _plane(org, "org")
    pr, sr, _, _ = _plane(ref, "ref")
    cfg = np.ascontiguousarray(cfg)
    assert cfg.dtype == TZ_CFG and cfg.size == 1
    out = torch.empty(n * IMV_RESULT.itemsize, dtype=torch.uint8, device=org.device)
    capi.call("vvcgpu_imv_refine_batch", po, so, pr, sr, capi.ptr(pus_dev), n, C.c_void_p(cfg.ctypes.data), 1 if use_hadamard else 0, C.c_double(weight),
              capi.ptr(out), _stream())
    return out


def quant_batch(coeff_base, level_base, descs_dev, n, bit_depth=10):
    """N1 forward: Quant::quant without RDOQ (+ sign bit hiding) for n TUs -> abs-sum int32 tensor [n] (bits as uint32)."""
    out = torch.zeros(n, dtype=torch.int32, device=coeff_base.device)
    capi.call("vvcgpu_quant_batch", capi.ptr(coeff_base), capi.ptr(level_base), capi.ptr(descs_dev), n, bit_depth, capi.ptr(out), _stream())
    return out


def depquant_batch(coeff_base, level_base, descs_dev, n, rates_dev, total_coeffs, bit_depth=10):
    """N1: dependent-quantisation trellis (DQIntern::DepQuant::quant) for n TUs -> abs-sum int32 tensor [n] (bits as uint32)."""
    nbytes = capi.lib().vvcgpu_depquant_workspace_bytes(total_coeffs, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=coeff_base.device)
    out = torch.zeros(n, dtype=torch.int32, device=coeff_base.device)
    capi.call("vvcgpu_depquant_batch", capi.ptr(coeff_base), capi.ptr(level_base), capi.ptr(descs_dev), n, capi.ptr(rates_dev), bit_depth,
              capi.ptr(out), C.c_size_t(total_coeffs), capi.ptr(ws), C.c_size_t(nbytes), _stream())
    return out


def rdoq_batch(coeff_base, level_base, descs_dev, n, rates_dev, total_coeffs, bit_depth=10):
    """N1: rate-distortion optimised quantiser (QuantRDOQ::xRateDistOptQuant) for n TUs -> abs-sum int32 tensor [n] (bits as uint32)."""
    nbytes = capi.lib().vvcgpu_rdoq_workspace_bytes(total_coeffs, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=coeff_base.device)
    out = torch.zeros(n, dtype=torch.int32, device=coeff_base.device)
    capi.call("vvcgpu_rdoq_batch", capi.ptr(coeff_base), capi.ptr(level_base), capi.ptr(descs_dev), n, capi.ptr(rates_dev), bit_depth,
              capi.ptr(out), C.c_size_t(total_coeffs), capi.ptr(ws), C.c_size_t(nbytes), _stream())
    return out


# ---- interpolation / MC / PelBuffer ops -------------------------------------------------------------
def if_batch(src_base, dst_base, descs_dev, n, bit_depth=10, clp=(0, 1023)):
    capi.call("vvcgpu_if_batch", capi.ptr(src_base), capi.ptr(dst_base), capi.ptr(descs_dev), n, bit_depth, clp[0], clp[1], _stream())


def mc_batch(ref0_base, ref1_base, dst_base, descs_dev, n, bit_depth=10, clp=(0, 1023)):
    capi.call("vvcgpu_mc_batch", capi.ptr(ref0_base), capi.ptr(ref1_base), capi.ptr(dst_base), capi.ptr(descs_dev), n,
              bit_depth, clp[0], clp[1], _stream())


def mc_picture_batch(ref0_base, ref1_base, dst_base, descs_dev, n, bit_depth=10, clp=(0, 1023)):
    """mc_batch for a picture's list of (mostly) 16x16 luma / 8x8 chroma PUs: one launch (vvcgpu_mc_picture_batch)"""
    capi.call("vvcgpu_mc_picture_batch", capi.ptr(ref0_base), capi.ptr(ref1_base), capi.ptr(dst_base), capi.ptr(descs_dev), n,
              bit_depth, clp[0], clp[1], _stream())


def mc_wp_batch(ref0_base, ref1_base, dst_base, descs_dev, n, wp_dev, n_wp, bit_depth=10, clp=(0, 1023)):
    """explicit weighted prediction of a picture's PUs (vvcgpu_mc_wp_batch): descriptors as mc_picture_batch, bi = 0 weighted uni- / 1 weighted
    bi-prediction, reserved = index into wp_dev (a device copy of a WP_PARAM array with n_wp entries, see wp_param)"""
    capi.call("vvcgpu_mc_wp_batch", capi.ptr(ref0_base), capi.ptr(ref1_base), capi.ptr(dst_base), capi.ptr(descs_dev), n, capi.ptr(wp_dev), n_wp,
              bit_depth, clp[0], clp[1], _stream())


def wp_param(bit_depth, log2_denom, weight0, offset0, weight1=None, offset1=None, high_precision_offsets=False):
    """one WP_PARAM record (w0, w1, offset, shift) from the slice header's values of ONE component, as WeightPrediction::getWpScaling derives it
    (WeightPrediction.cpp:77-156): uni-prediction when weight1 is None (a list-1-only PU passes list 1's values as weight0 / offset0), else
    bi-prediction.  Offsets are scaled to the bit depth unless the range extension's high-precision offsets are on."""
    sc = 1 if high_precision_offsets else 1 << (bit_depth - 8)
    if weight1 is None:
        return (weight0, 0, offset0 * sc, log2_denom)
    return (weight0, weight1, offset0 * sc + offset1 * sc, log2_denom + 1)


def mc_dist_batch(kind, ref0_base, ref1_base, org_base, descs_dev, n, bit_depth=10, clp=(0, 1023)):
    """predict a candidate (descriptors as mc_batch, dst_off / dst_stride = the original block, reserved = SAD row sub-sampling shift) and return
    its distortion against the original: int64 tensor [n]."""
    out = torch.empty(n, dtype=torch.int64, device=org_base.device)
    capi.call("vvcgpu_mc_dist_batch", kind, capi.ptr(ref0_base), capi.ptr(ref1_base), capi.ptr(org_base), capi.ptr(descs_dev), n, bit_depth,
              clp[0], clp[1], capi.ptr(out), _stream())
    return out


def merge_cand_batch(ref0_base, ref1_base, org_base, pred_base, mc_descs_dev, n_mc, cand_mc_first, cand_dist_dev, n_cand, n_comp, pu_cand_first, n_pu,
                     max_num_merge_cand, sqrt_lambda, use_hadamard=True, bit_depth=10, clp=(0, 1023), want_sse=True):
    """the merge candidate pass of n_pu PUs (vvcgpu_merge_cand_batch): mc_descs_dev / cand_dist_dev are device copies of MC_DESC / DIST_DESC arrays,
    cand_mc_first [n_cand + 1] and pu_cand_first [n_pu + 1] int32 tensors; pred_base may be None (cost only).  -> (dist int64 [n_cand], sse int64
    [n_cand][n_comp] or None, cost float64 [n_cand], rd_list int32 [n_pu][8]: uiNumMrgSATDCand, then RdModeList)"""
    dv = org_base.device
    dist = torch.empty(n_cand, dtype=torch.int64, device=dv)
    sse = torch.empty((n_cand, n_comp), dtype=torch.int64, device=dv) if want_sse else None
    cost = torch.empty(n_cand, dtype=torch.float64, device=dv)
    rd_list = torch.empty((n_pu, 8), dtype=torch.int32, device=dv)
    capi.call("vvcgpu_merge_cand_batch", capi.ptr(ref0_base), capi.ptr(ref1_base), capi.ptr(org_base), capi.ptr(pred_base), capi.ptr(mc_descs_dev), n_mc,
              capi.ptr(cand_mc_first), capi.ptr(cand_dist_dev), n_cand, n_comp, capi.ptr(pu_cand_first), n_pu, max_num_merge_cand, 1 if use_hadamard else 0,
              float(sqrt_lambda), bit_depth, clp[0], clp[1], capi.ptr(dist), capi.ptr(sse), capi.ptr(cost), capi.ptr(rd_list), _stream())
    return dist, sse, cost, rd_list


def pelop_batch(op, src0_base, src1_base, dst_base, descs_dev, n, cfg):
    capi.call("vvcgpu_pelop_batch", op, capi.ptr(src0_base), capi.ptr(src1_base), capi.ptr(dst_base), capi.ptr(descs_dev), n,
              C.byref(cfg), _stream())


# ---- transforms (TrQuant) ----------------------------------------------------------------------------
def tr_fwd_batch(resi_base, coeff_base, descs_dev, n, bit_depth=10):
    capi.call("vvcgpu_tr_fwd_batch", capi.ptr(resi_base), capi.ptr(coeff_base), capi.ptr(descs_dev), n, bit_depth, _stream())


def tr_inv_batch(coeff_base, resi_base, descs_dev, n, bit_depth=10):
    capi.call("vvcgpu_tr_inv_batch", capi.ptr(coeff_base), capi.ptr(resi_base), capi.ptr(descs_dev), n, bit_depth, _stream())


# ---- fused fractional refinement (InterSearch::xPatternSearchFracDIF) ---------------------------------------
def affine_sobel_batch(vertical, pred_base, deriv_base, descs_dev, n):
    """N3: Sobel derivative planes of prediction blocks (table slots m_HorizontalSobelFilter / m_VerticalSobelFilter)."""
    capi.call("vvcgpu_affine_sobel_batch", int(vertical), capi.ptr(pred_base), capi.ptr(deriv_base), capi.ptr(descs_dev), n, _stream())


def affine_equal_coeff_batch(resi_base, gx_base, gy_base, descs_dev, n):
    """N3: normal-equation sums of the affine model (table slot m_EqualCoeffComputer) -> int64 tensor [n, 7, 7]."""
    out = torch.empty((n, 7, 7), dtype=torch.int64, device=resi_base.device)
    capi.call("vvcgpu_affine_equal_coeff_batch", capi.ptr(resi_base), capi.ptr(gx_base), capi.ptr(gy_base), capi.ptr(descs_dev), n,
              capi.ptr(out), _stream())
    return out


def dequant_tr_inv_batch(level_base, resi_base, descs_dev, n, bit_depth, coeff_out=None):
    """N1: de-quantisation + inverse transform in one launch.  coeff_out (optional): int32, same offsets as level_base, receives the de-quantised
    coefficients (the reference's m_plTempCoeff); None: they never leave the chip."""
    capi.call("vvcgpu_dequant_tr_inv_batch", capi.ptr(level_base), capi.ptr(resi_base), capi.ptr(descs_dev), n, bit_depth,
              capi.ptr(coeff_out) if coeff_out is not None else None, _stream())


def frac_refine(org, ref, blocks_dev, nblocks, w, h, bit_depth, mvcost, use_hadamard=True, clp=(0, 1023)):
    """I2+D2+D5: returns a uint8 CUDA tensor holding nblocks FRAC_RESULT records."""
    po, so, _, _ = _plane(org, "org")
    pr, sr, _, _ = _plane(ref, "ref")
    res = torch.empty(nblocks * FRAC_RESULT.itemsize, dtype=torch.uint8, device=org.device)
    capi.call("vvcgpu_frac_refine", po, so, pr, sr, capi.ptr(blocks_dev), nblocks, w, h, bit_depth, clp[0], clp[1],
              1 if use_hadamard else 0, C.byref(mvcost), capi.ptr(res), _stream())
    return res


# ---- fused residual chain (InterSearch::xEstimateInterResidualQT per TU) ------------------------------------
def resi_chain_batch(org_base, pred_base, rec_base, level_base, descs_dev, n, bit_depth=10, clp=(0, 1023)):
    """subtract -> forward transform -> Quant::quant -> Quant::dequant -> inverse transform -> reconstruction of n TUs in one pass.
    Returns the abs-sum int32 tensor [n] (bits as uint32; 0xFFFFFFFF marks a TU outside the entry point's preconditions)."""
    out = torch.empty(n, dtype=torch.int32, device=org_base.device)       # every entry is written by the library
    capi.call("vvcgpu_resi_chain_batch", capi.ptr(org_base), capi.ptr(pred_base), capi.ptr(rec_base), capi.ptr(level_base), capi.ptr(descs_dev), n,
              bit_depth, clp[0], clp[1], capi.ptr(out), _stream())
    return out


def resi_chain_runs_batch(org_base, pred_base, rec_base, level_base, descs_dev, n, runs, bit_depth=10, clp=(0, 1023)):
    """the same for descriptors grouped by shape: runs = [(w, h, count), ...] in the order of the list (vvcgpu_resi_chain_runs_batch)"""
    r = np.ascontiguousarray(np.asarray(runs, dtype=np.int32).reshape(-1, 3))
    out = torch.empty(n, dtype=torch.int32, device=org_base.device)
    capi.call("vvcgpu_resi_chain_runs_batch", capi.ptr(org_base), capi.ptr(pred_base), capi.ptr(rec_base), capi.ptr(level_base), capi.ptr(descs_dev), n,
              C.c_void_p(r.ctypes.data), int(r.shape[0]), bit_depth, clp[0], clp[1], capi.ptr(out), _stream())
    return out


# ---- picture-level forms of the in-loop entry points (three planes, one launch each) ------------------------
def planes(ts):
    """three 2-D int16 CUDA tensors (Y, Cb, Cr) -> vvcgpu_planes"""
    pl = Planes()
    for i, t in enumerate(ts):
        assert t.is_cuda and t.dtype == torch.int16 and t.dim() == 2 and t.stride(1) == 1
        pl.p[i] = t.data_ptr()
        pl.stride[i] = t.stride(0)
    return pl


def sao_apply_picture(src, dst, ctu, bit_depth, params_dev, clp=(0, 1023)):
    h, w = src[0].shape
    capi.call("vvcgpu_sao_apply_picture", C.byref(planes(src)), C.byref(planes(dst)), w, h, ctu, bit_depth, capi.ptr(params_dev[0]),
              capi.ptr(params_dev[1]), capi.ptr(params_dev[2]), clp[0], clp[1], _stream())
    return dst


def sao_stats_picture(org, rec, ctu, bit_depth, avail=None, skip_luma=(5, 4), skip_chroma=(3, 2)):
    """-> [int64 tensor (nCtu, 5, 2, 32)] x 3"""
    h, w = org[0].shape
    n = ((w + ctu - 1) // ctu) * ((h + ctu - 1) // ctu)
    outs = [torch.empty((n, 5, 2, 32), dtype=torch.int64, device=org[0].device) for _ in range(3)]
    capi.call("vvcgpu_sao_stats_picture", C.byref(planes(org)), C.byref(planes(rec)), w, h, ctu, bit_depth, capi.ptr(avail), skip_luma[0], skip_luma[1],
              skip_chroma[0], skip_chroma[1], capi.ptr(outs[0]), capi.ptr(outs[1]), capi.ptr(outs[2]), _stream())
    return outs


def alf_filter_picture(src, dst, ctu, cls, filter_type, luma_coeff, chroma_coeff, enable=(None, None, None), clp=(0, 1023)):
    h, w = src[0].shape
    lc = np.ascontiguousarray(luma_coeff, dtype=np.int16)
    cc = np.ascontiguousarray(chroma_coeff, dtype=np.int16)
    assert lc.size == 25 * 13 and cc.size == 7
    capi.call("vvcgpu_alf_filter_picture", C.byref(planes(src)), C.byref(planes(dst)), w, h, ctu, capi.ptr(cls), filter_type,
              C.c_void_p(lc.ctypes.data), C.c_void_p(cc.ctypes.data), capi.ptr(enable[0]), capi.ptr(enable[1]), capi.ptr(enable[2]), clp[0], clp[1], _stream())
    return dst


def alf_stats_picture(org, rec, ctu, cls):
    """-> (luma 7x7 (nCtu, 25, 183), luma 5x5 (nCtu, 25, 57), [Cb (nCtu, 1, 57), Cr (nCtu, 1, 57)]) int64 tensors"""
    h, w = org[0].shape
    n = ((w + ctu - 1) // ctu) * ((h + ctu - 1) // ctu)
    dev = org[0].device
    a7 = torch.empty((n, 25, 183), dtype=torch.int64, device=dev)
    a5 = torch.empty((n, 25, 57), dtype=torch.int64, device=dev)
    ac = [torch.empty((n, 1, 57), dtype=torch.int64, device=dev) for _ in range(2)]
    capi.call("vvcgpu_alf_stats_picture", C.byref(planes(org)), C.byref(planes(rec)), w, h, ctu, capi.ptr(cls), capi.ptr(a7), capi.ptr(a5),
              capi.ptr(ac[0]), capi.ptr(ac[1]), _stream())
    return a7, a5, ac


def alf_classify_stats_picture(org, rec, ctu, bit_depth):
    """The encoder's ALF front end in one launch (vvcgpu_alf_classify_stats_picture): -> (cls as alf_classify returns it, then alf_stats_picture's tuple)"""
    h, w = org[0].shape
    n = ((w + ctu - 1) // ctu) * ((h + ctu - 1) // ctu)
    dev = org[0].device
    cls = torch.empty((h // 4, w // 4), dtype=torch.int16, device=dev)
    a7 = torch.empty((n, 25, 183), dtype=torch.int64, device=dev)
    a5 = torch.empty((n, 25, 57), dtype=torch.int64, device=dev)
    ac = [torch.empty((n, 1, 57), dtype=torch.int64, device=dev) for _ in range(2)]
    capi.call("vvcgpu_alf_classify_stats_picture", C.byref(planes(org)), C.byref(planes(rec)), w, h, ctu, bit_depth, capi.ptr(cls), capi.ptr(a7), capi.ptr(a5),
              capi.ptr(ac[0]), capi.ptr(ac[1]), _stream())
    return cls, a7, a5, ac


def alf_frame_stats(ctu_stats, enable=None, out=None, accumulate=False):
    """getFrameStat on the device: ctu_stats int64 (nCtu, nClasses, nVals) as the statistics entries return it, enable uint8 (nCtu,) or None (all on)
    -> int64 (nClasses, nVals); with `out` and accumulate the sum is added to it (chroma: Cb, then Cr with accumulate)"""
    n, ncls, nv = ctu_stats.shape
    assert ctu_stats.dtype == torch.int64 and ctu_stats.is_contiguous()
    assert enable is None or (enable.dtype == torch.uint8 and enable.numel() == n and enable.is_contiguous())
    if out is None:
        assert not accumulate, "accumulate needs the record to add to"
        out = torch.empty((ncls, nv), dtype=torch.int64, device=ctu_stats.device)
    assert out.dtype == torch.int64 and out.numel() == ncls * nv and out.is_contiguous()
    capi.call("vvcgpu_alf_frame_stats", capi.ptr(ctu_stats), n, ncls, nv, capi.ptr(enable), 1 if accumulate else 0, capi.ptr(out), _stream())
    return out


def alf_ctu_dist(ctu_stats, coeff_set, filter_idx=None, coeff_bits=10):
    """per CTU (getUnfilteredDistortion, getFilteredDistortion) of deriveCtbAlfEnableFlags -> float64 (nCtu, 2), the reference's doubles bit for bit.
    coeff_set: (nFilters, N) quantised coefficients, filter_idx: per class the filter in use (None with one class: filter 0)"""
    n, ncls, nv = ctu_stats.shape
    assert ctu_stats.dtype == torch.int64 and ctu_stats.is_contiguous() and nv in (57, 183)
    N = 13 if nv == 183 else 7
    cs = np.ascontiguousarray(coeff_set, dtype=np.int32).reshape(-1, N)
    fi = None if filter_idx is None else np.ascontiguousarray(filter_idx, dtype=np.int16).reshape(-1)
    assert fi is None or fi.size == ncls
    out = torch.empty((n, 2), dtype=torch.float64, device=ctu_stats.device)
    capi.call("vvcgpu_alf_ctu_dist", capi.ptr(ctu_stats), n, ncls, 1 if N == 13 else 0, C.c_void_p(cs.ctypes.data), cs.shape[0],
              None if fi is None else C.c_void_p(fi.ctypes.data), coeff_bits, capi.ptr(out), _stream())
    return out


# ---- T3 residual DPCM, I3 affine sub-block vectors -------------------------------------------------------------
def rdpcm_fwd_batch(resi_base, coeff_base, descs_dev, n, bit_depth=10):
    """TrQuant::applyForwardRDPCM for n TUs -> abs-sum int32 tensor [n] (bits as uint32)"""
    out = torch.zeros(n, dtype=torch.int32, device=resi_base.device)
    capi.call("vvcgpu_rdpcm_fwd_batch", capi.ptr(resi_base), capi.ptr(coeff_base), capi.ptr(descs_dev), n, bit_depth, capi.ptr(out), _stream())
    return out


def rdpcm_inv_batch(resi_base, descs_dev, n):
    """TrQuant::invRdpcmNxN, in place"""
    capi.call("vvcgpu_rdpcm_inv_batch", capi.ptr(resi_base), capi.ptr(descs_dev), n, _stream())


def affine_me_iter_batch(org_base, ref_base, pred_base, items_dev, n, n_subblocks, dist_kind, pic_w, pic_h, ref_origin, ref_stride,
                         bit_depth=10, clp=(0, 1023), max_cu=128, want_dist=True):
    """one iteration of the affine gradient search behind its prediction (loop body of xAffineMotionEstimation): the prediction is left in
    pred_base; -> (equation sums int64 [n, 7, 7], distortion int64 [n] or None)"""
    ws = torch.empty(n_subblocks * MC_DESC.itemsize, dtype=torch.uint8, device=org_base.device)
    coeff = torch.empty((n, 7, 7), dtype=torch.int64, device=org_base.device)
    dist = torch.empty(n, dtype=torch.int64, device=org_base.device) if want_dist else None
    capi.call("vvcgpu_affine_me_iter_batch", capi.ptr(org_base), capi.ptr(ref_base), capi.ptr(pred_base), capi.ptr(items_dev), n, n_subblocks,
              capi.ptr(ws), dist_kind, pic_w, pic_h, max_cu, max_cu, ref_origin[0], ref_origin[1], ref_stride, bit_depth, clp[0], clp[1],
              capi.ptr(coeff), capi.ptr(dist) if want_dist else None, _stream())
    return coeff, dist


def affine_me_cfg(lambda_, pic_w, pic_h, ref_origin, ref_stride, bit_depth=10, clp=(0, 1023), affine_type=1, max_cu=128):
    """vvcgpu_affine_me_cfg of one (slice, reference picture): motion lambda, picture / CTU size, the reference plane's margin and stride"""
    return AffineMeCfg(lambda_, pic_w, pic_h, max_cu, max_cu, ref_origin[0], ref_origin[1], ref_stride, bit_depth, clp[0], clp[1], affine_type)


def affine_me_batch(org_base, ref_base, items_dev, n, cfg, want_trace=True):
    """xAffineMotionEstimation for n independent (PU, reference picture) searches in one launch: items_dev = AFFINE_ME_ITEM records on the device,
    cfg = affine_me_cfg(...).  -> (AFFINE_ME_RESULT records, AFFINE_ME_STEP records [n x AFFINE_ME_MAX_STEPS] or None), uint8 tensors"""
    assert isinstance(cfg, AffineMeCfg)
    res = torch.empty(n * AFFINE_ME_RESULT.itemsize, dtype=torch.uint8, device=org_base.device)
    trace = torch.empty(n * AFFINE_ME_MAX_STEPS * AFFINE_ME_STEP.itemsize, dtype=torch.uint8, device=org_base.device) if want_trace else None
    capi.call("vvcgpu_affine_me_batch", capi.ptr(org_base), capi.ptr(ref_base), capi.ptr(items_dev), n, C.byref(cfg), capi.ptr(res),
              capi.ptr(trace) if want_trace else None, _stream())
    return res, trace


def _pu_frame(cfg, lambda_, ref_planes, ref_origin, pic_w, pic_h, bit_depth, clp, max_cu, mvp_idx_cost, max_pu):
    """the fields every whole-PU search cfg begins and ends with (pu_entry_host.h checks them as one frame)"""
    cfg.lambda_ = lambda_
    assert 1 <= len(ref_planes) <= len(cfg.ref_planes)                   # the entry's MAX_PLANES
    for i, t in enumerate(ref_planes):
        ptr, stride, _, _ = _plane(t, "ref_planes[%d]" % i)
        assert stride == ref_planes[0].stride(0), "reference planes of one stride"
        cfg.ref_planes[i] = ptr.value + 2 * (ref_origin[1] * stride + ref_origin[0])
    cfg.n_planes, cfg.ref_stride = len(ref_planes), ref_planes[0].stride(0)
    cfg.pic_w, cfg.pic_h, cfg.max_cu_w, cfg.max_cu_h = pic_w, pic_h, max_cu, max_cu
    cfg.bit_depth, cfg.clp_min, cfg.clp_max = bit_depth, clp[0], clp[1]
    cfg.mvp_idx_cost[:] = mvp_idx_cost
    cfg.max_pu_w, cfg.max_pu_h = max_pu
    return cfg


def _unipred_refs(cfg, n_ref, ref_plane, list1_to_list0):
    """the reference lists of a uni-predictive cfg: counts, the plane of every reference index, list 1's twins in list 0"""
    max_refs = len(cfg.list1_to_list0)                                   # the entry's MAX_REFS
    cfg.n_ref[:] = n_ref
    for l in range(2):
        for r in range(min(n_ref[l], max_refs)):
            cfg.ref_plane[l][r] = ref_plane[l][r]
    cfg.list1_to_list0[:] = (tuple(list1_to_list0) + (-1,) * max_refs)[:max_refs]


def bipred_me_cfg(lambda_, ref_planes, ref_origin, pic_w, pic_h, bit_depth=10, clp=(0, 1023), num_iter=4, pick_list_by_cost=False, mvd_l1_zero=False,
                  search_range=4, clip_key=True, use_hadamard=True, mvp_idx_cost=(1, 1, 0), max_cu=128, max_pu=(0, 0), imv=0):
    """vvcgpu_bipred_me_cfg of one slice (imv: cu.imv of the pass, 0..2).  ref_planes: the PADDED reference luma planes (2-D int16 CUDA tensors of one stride; keep them alive while
    calls that use the cfg run); ref_origin = (x, y) of picture sample (0, 0) inside each of them"""
    cfg = _pu_frame(BipredMeCfg(), lambda_, ref_planes, ref_origin, pic_w, pic_h, bit_depth, clp, max_cu, mvp_idx_cost, max_pu)
    cfg.num_iter, cfg.pick_list_by_cost, cfg.mvd_l1_zero = num_iter, int(pick_list_by_cost), int(mvd_l1_zero)
    cfg.bipred_search_range, cfg.clip_for_bipred_me, cfg.use_hadamard, cfg.imv = search_range, int(clip_key), int(use_hadamard), imv
    return cfg


def bipred_me_batch(org_base, items_dev, n, cfg, want_trace=True):
    """The bi-predictive refinement loop of predInterSearch for n independent PUs in one launch: items_dev = BIPRED_ME_ITEM records on the device,
    cfg = bipred_me_cfg(...).  -> (BIPRED_ME_RESULT records, BIPRED_ME_STEP records [n x BIPRED_ME_MAX_STEPS] or None), uint8 tensors"""
    assert isinstance(cfg, BipredMeCfg)
    res = torch.empty(n * BIPRED_ME_RESULT.itemsize, dtype=torch.uint8, device=org_base.device)
    trace = torch.empty(n * BIPRED_ME_MAX_STEPS * BIPRED_ME_STEP.itemsize, dtype=torch.uint8, device=org_base.device) if want_trace else None
    capi.call("vvcgpu_bipred_me_batch", capi.ptr(org_base), capi.ptr(items_dev), n, C.byref(cfg), capi.ptr(res),
              capi.ptr(trace) if want_trace else None, _stream())
    return res, trace


def unipred_me_cfg(lambda_, ref_planes, ref_origin, pic_w, pic_h, n_ref, ref_plane, search_range, bit_depth=10, clp=(0, 1023), list1_to_list0=(-1, -1, -1, -1),
                   fast_me_gen_b_low_delay=False, mvd_l1_zero=False, first_search_stop=False, use_hadamard=True, mvp_idx_cost=(1, 1, 0), max_cu=128,
                   max_pu=(0, 0), imv=0):
    """vvcgpu_unipred_me_cfg of one slice (imv: cu.imv of the pass, 0..2).  ref_planes: the PADDED reference luma planes (2-D int16 CUDA tensors of one stride; keep them alive while
    calls that use the cfg run); ref_origin = (x, y) of picture sample (0, 0) inside each of them; n_ref = (list 0, list 1) reference counts, ref_plane
    and search_range = per list the plane index / m_aaiAdaptSR of every reference index"""
    cfg = _pu_frame(UnipredMeCfg(), lambda_, ref_planes, ref_origin, pic_w, pic_h, bit_depth, clp, max_cu, mvp_idx_cost, max_pu)
    _unipred_refs(cfg, n_ref, ref_plane, list1_to_list0)
    for l in range(2):
        for r in range(min(n_ref[l], UNIPRED_ME_MAX_REFS)):
            cfg.search_range[l][r] = search_range[l][r]
    cfg.fast_me_gen_b_low_delay, cfg.mvd_l1_zero = int(fast_me_gen_b_low_delay), int(mvd_l1_zero)
    cfg.first_search_stop, cfg.use_hadamard, cfg.imv = int(first_search_stop), int(use_hadamard), imv
    return cfg


def unipred_me_batch(org_base, items_dev, n, cfg, want_bipred_items=True):
    """The uni-predictive stage of predInterSearch for n independent PUs, two launches and no host synchronisation: items_dev = UNIPRED_ME_ITEM records
    on the device, cfg = unipred_me_cfg(...).  -> (UNIPRED_ME_RESULT records, BIPRED_ME_ITEM records ready for bipred_me_batch or None), uint8 tensors"""
    assert isinstance(cfg, UnipredMeCfg)
    res = torch.empty(n * UNIPRED_ME_RESULT.itemsize, dtype=torch.uint8, device=org_base.device)
    out = torch.empty(n * BIPRED_ME_ITEM.itemsize, dtype=torch.uint8, device=org_base.device) if want_bipred_items else None
    capi.call("vvcgpu_unipred_me_batch", capi.ptr(org_base), capi.ptr(items_dev), n, C.byref(cfg), capi.ptr(res),
              capi.ptr(out) if want_bipred_items else None, _stream())
    return res, out


def affine_bipred_cfg(lambda_, ref_planes, ref_origin, pic_w, pic_h, bit_depth=10, clp=(0, 1023), num_iter=4, pick_list_by_cost=False, mvd_l1_zero=False,
                      clip_key=True, affine_type=1, mvp_idx_cost=(1, 1, 0), max_cu=128, max_pu=(0, 0)):
    """vvcgpu_affine_bipred_cfg of one slice.  ref_planes: the PADDED reference luma planes (2-D int16 CUDA tensors of one stride; keep them alive while
    calls that use the cfg run); ref_origin = (x, y) of picture sample (0, 0) inside each of them"""
    cfg = _pu_frame(AffineBipredCfg(), lambda_, ref_planes, ref_origin, pic_w, pic_h, bit_depth, clp, max_cu, mvp_idx_cost, max_pu)
    cfg.num_iter, cfg.pick_list_by_cost, cfg.mvd_l1_zero = num_iter, int(pick_list_by_cost), int(mvd_l1_zero)
    cfg.clip_for_bipred_me, cfg.affine_type = int(clip_key), int(affine_type)
    return cfg


def affine_bipred_me_batch(org_base, items_dev, n, cfg, want_trace=True):
    """The bi-predictive part of xPredAffineInterSearch for n independent PUs in one launch: items_dev = AFFINE_BIPRED_ITEM records on the device,
    cfg = affine_bipred_cfg(...).  -> (AFFINE_BIPRED_RESULT records, AFFINE_BIPRED_STEP records [n x AFFINE_BIPRED_MAX_STEPS] or None), uint8 tensors"""
    assert isinstance(cfg, AffineBipredCfg)
    res = torch.empty(n * AFFINE_BIPRED_RESULT.itemsize, dtype=torch.uint8, device=org_base.device)
    trace = torch.empty(n * AFFINE_BIPRED_MAX_STEPS * AFFINE_BIPRED_STEP.itemsize, dtype=torch.uint8, device=org_base.device) if want_trace else None
    capi.call("vvcgpu_affine_bipred_me_batch", capi.ptr(org_base), capi.ptr(items_dev), n, C.byref(cfg), capi.ptr(res),
              capi.ptr(trace) if want_trace else None, _stream())
    return res, trace


def affine_unipred_cfg(lambda_, ref_planes, ref_origin, pic_w, pic_h, n_ref, ref_plane, bit_depth=10, clp=(0, 1023), list1_to_list0=(-1, -1, -1, -1),
                       fast_me_gen_b_low_delay=False, mvd_l1_zero=False, affine_type=1, mvp_idx_cost=(1, 1, 0), max_cu=128, max_pu=(0, 0)):
    """vvcgpu_affine_unipred_cfg of one slice.  ref_planes: the PADDED reference luma planes (2-D int16 CUDA tensors of one stride; keep them alive while
    calls that use the cfg run); ref_origin = (x, y) of picture sample (0, 0) inside each of them; n_ref = (list 0, list 1) reference counts,
    ref_plane = per list the plane index of every reference index"""
    cfg = _pu_frame(AffineUnipredCfg(), lambda_, ref_planes, ref_origin, pic_w, pic_h, bit_depth, clp, max_cu, mvp_idx_cost, max_pu)
    _unipred_refs(cfg, n_ref, ref_plane, list1_to_list0)
    cfg.fast_me_gen_b_low_delay, cfg.mvd_l1_zero, cfg.affine_type = int(fast_me_gen_b_low_delay), int(mvd_l1_zero), int(affine_type)
    return cfg


def affine_unipred_me_batch(org_base, items_dev, n, cfg, want_bipred_items=True):
    """The uni-predictive stage of xPredAffineInterSearch for n independent PUs, two launches and no host synchronisation: items_dev =
    AFFINE_UNIPRED_ITEM records on the device, cfg = affine_unipred_cfg(...).  -> (AFFINE_UNIPRED_RESULT records, AFFINE_BIPRED_ITEM records ready for
    affine_bipred_me_batch or None), uint8 tensors"""
    assert isinstance(cfg, AffineUnipredCfg)
    res = torch.empty(n * AFFINE_UNIPRED_RESULT.itemsize, dtype=torch.uint8, device=org_base.device)
    out = torch.empty(n * AFFINE_BIPRED_ITEM.itemsize, dtype=torch.uint8, device=org_base.device) if want_bipred_items else None
    capi.call("vvcgpu_affine_unipred_me_batch", capi.ptr(org_base), capi.ptr(items_dev), n, C.byref(cfg), capi.ptr(res),
              capi.ptr(out) if want_bipred_items else None, _stream())
    return res, out


def affine_pred_batch(ref0_base, ref1_base, dst_base, pus_dev, n, n_subblocks, comp, pic_w, pic_h, ref_origin, ref0_stride, ref1_stride,
                      bit_depth=10, clp=(0, 1023), max_cu=128):
    """xPredAffineBlk for a list of PUs: sub-block vectors + their interpolation in one call (luma: four 4x4 sub-blocks per wavefront)"""
    ws = torch.empty(n_subblocks * MC_DESC.itemsize, dtype=torch.uint8, device=dst_base.device)
    capi.call("vvcgpu_affine_pred_batch", capi.ptr(ref0_base), capi.ptr(ref1_base), capi.ptr(dst_base), capi.ptr(pus_dev), n, n_subblocks, capi.ptr(ws),
              comp, pic_w, pic_h, max_cu, max_cu, ref_origin[0], ref_origin[1], ref0_stride, ref1_stride, bit_depth, clp[0], clp[1], _stream())


def affine_subblock_descs(pus_dev, n, n_descs, comp, pic_w, pic_h, ref_origin, ref0_stride, ref1_stride, max_cu=128):
    """sub-block MC descriptors (uint8 tensor of n_descs vvcgpu_mc_desc) of n affine PUs, on the device"""
    out = torch.zeros(n_descs * MC_DESC.itemsize, dtype=torch.uint8, device=pus_dev.device)
    capi.call("vvcgpu_affine_subblock_descs", capi.ptr(pus_dev), n, comp, pic_w, pic_h, max_cu, max_cu, ref_origin[0], ref_origin[1], ref0_stride,
              ref1_stride, capi.ptr(out), _stream())
    return out


# ---- encoder picture analysis (PSNR / WPSNR, QPA activity, weighted-prediction statistics, rate control's intra cost) ----------------------------
def _planes_n(ts):
    """1 or 3 planes (a 2-D tensor or a sequence of them) -> (vvcgpu_planes, n_planes, width, height)"""
    ts = [ts] if torch.is_tensor(ts) else list(ts)
    assert len(ts) in (1, 3), "1 or 3 planes"
    return planes(ts), len(ts), ts[0].shape[1], ts[0].shape[0]


def tile_stats_picture(org, rec, tile):
    """per plane an int64 tensor (tiles_y, tiles_x, 3) holding sa_act, sum, ss_err (uint64 bit patterns) of its tile x tile tiles (tile / 2 for the chroma
    planes of a 3-plane call); rec may be None (ss_err = 0)"""
    po, n, w, h = _planes_n(org)
    pr = _planes_n(rec)[0] if rec is not None else None
    dev = (org if torch.is_tensor(org) else org[0]).device
    outs = []
    for c in range(n):
        t = tile >> 1 if c else tile
        pw, ph = (w >> 1, h >> 1) if c else (w, h)
        outs.append(torch.empty((-(-ph // t), -(-pw // t), 3), dtype=torch.int64, device=dev))
    capi.call("vvcgpu_tile_stats_picture", C.byref(po), C.byref(pr) if pr is not None else None, w, h, tile, n, capi.ptr(outs[0]),
              capi.ptr(outs[1]) if n == 3 else None, capi.ptr(outs[2]) if n == 3 else None, _stream())
    return outs


def picture_sse(a, b):
    """sum (a - b)^2 per plane -> int64 tensor (3,) on the device"""
    pa, n, w, h = _planes_n(a)
    pb = _planes_n(b)[0]
    out = torch.empty(3, dtype=torch.int64, device=(a if torch.is_tensor(a) else a[0]).device)
    capi.call("vvcgpu_picture_sse", C.byref(pa), C.byref(pb), w, h, n, capi.ptr(out), _stream())
    return out


def picture_histogram(pic, bit_depth):
    """xCalcHistogram of every plane -> int32 tensor (3, 2^bd) on the device"""
    pp, n, w, h = _planes_n(pic)
    out = torch.empty((3, 1 << bit_depth), dtype=torch.int32, device=(pic if torch.is_tensor(pic) else pic[0]).device)
    capi.call("vvcgpu_picture_histogram", C.byref(pp), w, h, n, bit_depth, capi.ptr(out), _stream())
    return out


def wp_sad_cands(cands):
    """[(log2_denom, weight, offset, flags)] -> WP_SAD_CAND array"""
    return np.array([tuple(c) for c in cands], dtype=WP_SAD_CAND)


def wp_sad_batch(org, ref, bit_depth, cands):
    """weighted SADs of one (original, reference) plane pair for up to 16 candidates (WP_SAD_CAND array or tuples) -> int64 tensor (n_cand,)"""
    po, so, w, h = _plane(org, "org")
    pr, sr, wr, hr = _plane(ref, "ref")
    assert (w, h) == (wr, hr)
    cands = np.ascontiguousarray(cands if isinstance(cands, np.ndarray) else wp_sad_cands(cands))
    assert cands.dtype == WP_SAD_CAND
    out = torch.empty(len(cands), dtype=torch.int64, device=org.device)
    capi.call("vvcgpu_wp_sad_batch", po, so, pr, sr, w, h, bit_depth, cands.ctypes.data_as(C.c_void_p), len(cands), capi.ptr(out), _stream())
    return out


def intra_cost_ctus(org_y, ctu_size, bit_depth):
    """m_costIntra of every CTU -> int32 tensor (ctus_y, ctus_x)"""
    p, st, w, h = _plane(org_y, "org_y")
    out = torch.empty((-(-h // ctu_size), -(-w // ctu_size)), dtype=torch.int32, device=org_y.device)
    capi.call("vvcgpu_intra_cost_ctus", p, st, w, h, ctu_size, bit_depth, capi.ptr(out), _stream())
    return out


def wpsnr_block_size(plane_w, plane_h, chroma_shift):
    """the WPSNR block size of a plane (0: the reference takes the plain SSE)"""
    b = C.c_int()
    capi.call("vvcgpu_wpsnr_block_size_host", plane_w, plane_h, chroma_shift, C.byref(b))
    return b.value


def wpsnr_finish(tiles, plane_w, plane_h, chroma_shift, bit_depth):
    """tiles: the plane's tile statistics at its own block size (host array, TILE_STATS records or (.., 3) 64-bit integers) -> the reference's weighted SSD"""
    t = np.ascontiguousarray(np.asarray(tiles)).view(np.uint64).reshape(-1)
    ssd = C.c_uint64()
    capi.call("vvcgpu_wpsnr_finish_host", t.ctypes.data_as(C.c_void_p), plane_w, plane_h, chroma_shift, bit_depth, C.byref(ssd))
    return ssd.value


def wp_acdc(hist, bit_depth, n_samples, fixed_shift=0):
    """(iDC, iAC) of xCalcACDCParamSlice from one plane's histogram (host array of 2^bd counts)"""
    hh = np.ascontiguousarray(np.asarray(hist).astype(np.uint32))
    assert hh.size == 1 << bit_depth
    dc, ac = C.c_int64(), C.c_int64()
    capi.call("vvcgpu_wp_acdc_host", hh.ctypes.data_as(C.c_void_p), bit_depth, n_samples, fixed_shift, C.byref(dc), C.byref(ac))
    return dc.value, ac.value
