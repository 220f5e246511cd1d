"""Python mirrors of the structs in include/vvcgpu.h: one numpy dtype (records built in arrays) or ctypes Structure (one record passed by
pointer from the host) per struct, both where both are used.  Field names, order and types follow the header;
tests/test_abi.py compares every field's offset and size with the C compiler's.

numpy and ctypes only: workload.py and the CPU checkers load this without torch or a GPU."""
import ctypes as C

import numpy as np

# ---- in-loop filters ------------------------------------------------------------------------------------------
SAO_DTYPE = np.dtype([("type", "i1"), ("avail", "u1"), ("offset", "<i2", (32,))])


class SaoCtu(C.Structure):
    """vvcgpu_sao_ctu"""
    _fields_ = [("type", C.c_int8), ("avail", C.c_uint8), ("offset", C.c_int16 * 32)]


class DeblockCfg(C.Structure):
    """vvcgpu_deblock_cfg"""
    _fields_ = [("bit_depth_luma", C.c_int32), ("bit_depth_chroma", C.c_int32),
                ("beta_offset_div2", C.c_int32), ("tc_offset_div2", C.c_int32),
                ("cb_qp_offset", C.c_int32), ("cr_qp_offset", C.c_int32),
                ("clp_min", C.c_int32 * 3), ("clp_max", C.c_int32 * 3)]


class Planes(C.Structure):
    """vvcgpu_planes"""
    _fields_ = [("p", C.c_void_p * 3), ("stride", C.c_int32 * 3)]


# ---- block distortion and integer motion search -------------------------------------------------------------------
DIST_DESC = np.dtype([("org_off", "<i8"), ("cur_off", "<i8"), ("org_stride", "<i4"), ("cur_stride", "<i4"),
                      ("w", "<i2"), ("h", "<i2"), ("sub_shift", "<i2"), ("reserved", "<i2")])
SEARCH_BLK = np.dtype([("org_x", "<i4"), ("org_y", "<i4"), ("ref_x", "<i4"), ("ref_y", "<i4")])
SEARCH_BEST = np.dtype([("x", "<i4"), ("y", "<i4"), ("cost", "<u8"), ("sad", "<u8")])


class MvCost(C.Structure):
    """vvcgpu_mvcost"""
    _fields_ = [("lambda_", C.c_double), ("pred_hor", C.c_int32), ("pred_ver", C.c_int32),
                ("cost_scale", C.c_int32), ("imv_shift", C.c_int32)]


class MeHierCfg(C.Structure):
    """vvcgpu_me_hier_cfg"""
    _fields_ = [("org_x", C.c_int32), ("org_y", C.c_int32), ("ref_x", C.c_int32), ("ref_y", C.c_int32), ("n16x", C.c_int32), ("n16y", C.c_int32),
                ("sub_shift", C.c_int32), ("raster_range", C.c_int32), ("raster_step", C.c_int32), ("dense_range", C.c_int32)]


TZ_PU = np.dtype([("org_x", "<i4"), ("org_y", "<i4"), ("ref_x", "<i4"), ("ref_y", "<i4"), ("start_x", "<i4"), ("start_y", "<i4"),
                  ("pred2_x", "<i4"), ("pred2_y", "<i4"), ("pos_x", "<i4"), ("pos_y", "<i4"), ("pred_hor", "<i4"), ("pred_ver", "<i4"),
                  ("w", "<i2"), ("h", "<i2"), ("sub_shift", "<i2"), ("flags", "<i2"), ("reserved", "<i4", (2,))])
TZ_CFG = np.dtype([("lambda", "<f8"), ("cost_scale", "<i4"), ("imv_shift", "<i4"), ("search_range", "<i4"), ("first_search_stop", "<i4"),
                   ("pic_w", "<i4"), ("pic_h", "<i4"), ("max_cu_w", "<i4"), ("max_cu_h", "<i4"),
                   ("ref_x0", "<i4"), ("ref_y0", "<i4"), ("ref_x1", "<i4"), ("ref_y1", "<i4"), ("wg_per_pu", "<i4"), ("reserved", "<i4")])   # "reserved" = vvcgpu_tz_cfg.uniform_pu (the field keeps its name: the golden fixtures store this dtype)
TZ_PRED2, TZ_EXTENDED, TZ_FAST = 1, 2, 4          # TZ_PU.flags

IMV_PU = np.dtype([("org_x", "<i4"), ("org_y", "<i4"), ("ref_x", "<i4"), ("ref_y", "<i4"), ("mv_x", "<i4"), ("mv_y", "<i4"),
                   ("cand_x", "<i4", (2,)), ("cand_y", "<i4", (2,)), ("pos_x", "<i4"), ("pos_y", "<i4"), ("idx_cost", "<u4", (2,)), ("bits", "<u4"),
                   ("w", "<i2"), ("h", "<i2"), ("num_cand", "i1"), ("mvp_idx", "i1"), ("reserved", "<i2"), ("reserved2", "<i4")])
IMV_RESULT = np.dtype([("mv_x", "<i4"), ("mv_y", "<i4"), ("mvp_idx", "<i4"), ("bits", "<u4"), ("cost", "<u8")])

# ---- fractional refinement --------------------------------------------------------------------------------------------
FRAC_BLK = np.dtype([("org_x", "<i4"), ("org_y", "<i4"), ("ref_x", "<i4"), ("ref_y", "<i4"), ("mv_x", "<i4"), ("mv_y", "<i4")])
FRAC_RESULT = np.dtype([("half_x", "<i4"), ("half_y", "<i4"), ("qter_x", "<i4"), ("qter_y", "<i4"), ("cost_half", "<u8"), ("cost", "<u8")])

# ---- intra prediction -----------------------------------------------------------------------------------------------------
INTRA_DESC = np.dtype([("ref_off", "<i8"), ("dst_off", "<i8"), ("dst_stride", "<i4"), ("w", "<i2"), ("h", "<i2"), ("mode", "i1"),
                       ("filter_refs", "i1"), ("reserved", "<i2"), ("reserved2", "<i4")])
INTRA_SATD_DESC = np.dtype([("ref_off", "<i8"), ("org_off", "<i8"), ("org_stride", "<i4"), ("w", "<i2"), ("h", "<i2"), ("mode", "i1"),
                            ("filter_refs", "i1"), ("reserved", "<i2"), ("reserved2", "<i4")])
CCLM_DESC = np.dtype([("luma_off", "<i8"), ("nb_off", "<i8"), ("dst_off", "<i8"), ("luma_stride", "<i4"), ("dst_stride", "<i4"), ("w", "<i2"),
                      ("h", "<i2"), ("above_avail", "i1"), ("left_avail", "i1"), ("reserved", "<i2"), ("reserved2", "<i4", (2,))])
INTRA_FILL_DESC = np.dtype([("rec_off", "<i8"), ("flags_off", "<i8"), ("ref_off", "<i8"), ("rec_stride", "<i4"), ("w", "<i2"), ("h", "<i2"),
                            ("unit_w", "i1"), ("unit_h", "i1"), ("reserved", "<i2"), ("reserved2", "<i4")])
# vvcgpu_intra_tu_code_batch: INTRA_DESC.mode values beside 0..66, and the flags
INTRA_TU_PRED_GIVEN, INTRA_TU_FROM_LIST = -1, -2
INTRA_TU_WRITE_PRED, INTRA_TU_NO_SMOOTHING = 1, 2
INTRA_TU_Q_DEPQUANT = 1                                                     # vvcgpu_intra_tu_code_dq_batch: the served quantiser
INTRA_TU_DQ_TS = 8                                                          # its flag: a 4x4 item with tr_hor == TSKIP is the transform-skip candidate
# vvcgpu_intra_chroma_code_batch: one chroma PU (vvcgpu_intra_chroma_pu), the mode value of LM_CHROMA_IDX and the flag
INTRA_CHROMA_PU = np.dtype([("org_off", "<i8", (2,)), ("ref_off", "<i8", (2,)), ("luma_off", "<i8"), ("cand_off", "<i8"), ("level_off", "<i8"),
                            ("org_stride", "<i4"), ("luma_stride", "<i4"), ("qp", "<i4", (2,)), ("w", "<i2"), ("h", "<i2"), ("above_avail", "i1"),
                            ("left_avail", "i1"), ("intra_slice", "i1"), ("sign_hiding", "i1"), ("mode", "i1", (6,)), ("reserved", "<i2"),
                            ("reserved2", "<i4", (2,))])
INTRA_CHROMA_LM, INTRA_CHROMA_WRITE_PRED = 67, 1
INTRA_CHROMA_Q_DEPQUANT = 1                                                 # vvcgpu_intra_chroma_code_dq_batch: the served quantiser

# ---- quantisers ---------------------------------------------------------------------------------------------------------------
QUANT_DESC = np.dtype([("coeff_off", "<i8"), ("level_off", "<i8"), ("w", "<i2"), ("h", "<i2"), ("intra_slice", "i1"), ("sign_hiding", "i1"),
                       ("reserved", "<i2"), ("qp", "<i4"), ("reserved2", "<i4")])
DQ_RATES = np.dtype([("last_x", "<i4", (64,)), ("last_y", "<i4", (64,)), ("sig_sbb", "<i4", (2, 2)), ("sig", "<i4", (3, 18, 2)), ("gtx", "<i4", (21, 7))])
DEPQUANT_DESC = np.dtype([("coeff_off", "<i8"), ("level_off", "<i8"), ("lambda", "<f8"), ("qp", "<i4"), ("rates_idx", "<i4"), ("w", "<i2"), ("h", "<i2"),
                          ("luma", "i1"), ("reserved", "i1", (3,))])
RDOQ_RATES = np.dtype([("sig", "<i4", (18, 2)), ("par", "<i4", (21, 2)), ("gt1", "<i4", (21, 2)), ("gt2", "<i4", (21, 2)), ("sig_group", "<i4", (2, 2)),
                       ("last_x", "<i4", (14,)), ("last_y", "<i4", (14,)), ("cbf", "<i4", (2,))])
RDOQ_DESC = np.dtype([("coeff_off", "<i8"), ("level_off", "<i8"), ("lambda", "<f8"), ("qp", "<i4"), ("rates_idx", "<i4"), ("w", "<i2"), ("h", "<i2"),
                      ("luma", "i1"), ("sign_hiding", "i1"), ("reserved", "i1", (2,))])

# ---- interpolation, motion compensation, PelBuffer ops --------------------------------------------------------------------
IF_DESC = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("src_stride", "<i4"), ("dst_stride", "<i4"),
                    ("w", "<i2"), ("h", "<i2"), ("taps", "i1"), ("is_vertical", "i1"), ("is_first", "i1"),
                    ("is_last", "i1"), ("coeff", "<i2", (8,)), ("reserved", "<i2", (4,))])
MC_DESC = np.dtype([("ref0_off", "<i8"), ("ref1_off", "<i8"), ("dst_off", "<i8"), ("ref0_stride", "<i4"),
                    ("ref1_stride", "<i4"), ("dst_stride", "<i4"), ("w", "<i2"), ("h", "<i2"), ("frac_x0", "i1"),
                    ("frac_y0", "i1"), ("frac_x1", "i1"), ("frac_y1", "i1"), ("is_luma", "i1"), ("bi", "i1"),
                    ("reserved", "<i2")])
# vvcgpu_wp_param: one entry of the weight table of vvcgpu_mc_wp_batch (WPScalingParam after WeightPrediction::getWpScaling)
WP_PARAM = np.dtype([("w0", "<i4"), ("w1", "<i4"), ("offset", "<i4"), ("shift", "<i4")])
PELOP_DESC = np.dtype([("src0_off", "<i8"), ("src1_off", "<i8"), ("dst_off", "<i8"), ("src0_stride", "<i4"),
                       ("src1_stride", "<i4"), ("dst_stride", "<i4"), ("w", "<i2"), ("h", "<i2")])


class PelopCfg(C.Structure):
    """vvcgpu_pelop_cfg"""
    _fields_ = [("scale", C.c_int32), ("shift", C.c_int32), ("offset", C.c_int32), ("clip", C.c_int32),
                ("clp_min", C.c_int32), ("clp_max", C.c_int32)]


# ---- transforms and the residual chain -------------------------------------------------------------------------------------
TR_DESC = np.dtype([("resi_off", "<i8"), ("coeff_off", "<i8"), ("resi_stride", "<i4"), ("w", "<i2"), ("h", "<i2"),
                    ("tr_hor", "i1"), ("tr_ver", "i1"), ("reserved", "<i2"), ("reserved2", "<i4")])
DCT2, DCT8, DST7, TSKIP = 0, 1, 2, 3              # tr_hor / tr_ver
DQTR_DESC = np.dtype([("resi_off", "<i8"), ("level_off", "<i8"), ("resi_stride", "<i4"), ("w", "<i2"), ("h", "<i2"),
                      ("tr_hor", "i1"), ("tr_ver", "i1"), ("dep_quant", "i1"), ("reserved", "i1"), ("qp", "<i4")])
RC_DESC = np.dtype([("org_off", "<i8"), ("pred_off", "<i8"), ("rec_off", "<i8"), ("level_off", "<i8"), ("org_stride", "<i4"), ("pred_stride", "<i4"),
                    ("rec_stride", "<i4"), ("w", "<i2"), ("h", "<i2"), ("tr_hor", "i1"), ("tr_ver", "i1"), ("intra_slice", "i1"), ("sign_hiding", "i1"),
                    ("qp", "<i4"), ("reserved", "<i4", (2,))])
RDPCM_DESC = np.dtype([("resi_off", "<i8"), ("coeff_off", "<i8"), ("resi_stride", "<i4"), ("w", "<i2"), ("h", "<i2"), ("mode", "i1"), ("lossless", "i1"),
                       ("rotate", "i1"), ("intra_slice", "i1"), ("qp", "<i4"), ("reserved", "<i4"), ("pad", "<i4")])    # "pad": the C struct's tail padding
# vvcgpu_inter_resi_code_batch: one transform block of an inter CU (vvcgpu_inter_resi_item), its slot count, the transform-skip code and the flag
INTER_RESI_ITEM = np.dtype([("org_off", "<i8"), ("pred_off", "<i8"), ("pred_cand_pitch", "<i8"), ("cand_off", "<i8"), ("level_off", "<i8"),
                            ("org_stride", "<i4"), ("pred_stride", "<i4"), ("qp", "<i4"), ("list_row", "<i4"), ("w", "<i2"), ("h", "<i2"),
                            ("list_slot", "i1"), ("intra_slice", "i1"), ("sign_hiding", "i1"), ("reserved", "i1"), ("tr", "i1", (6,)),
                            ("reserved1", "i1", (2,)), ("reserved2", "<i4", (2,))])
INTER_RESI_SLOTS, INTER_RESI_TS, INTER_RESI_WRITE_REC = 6, 9, 1
# vvcgpu_inter_resi_code_dq_batch: the record beside an item (vvcgpu_inter_resi_dq) and the served value of `quantiser`
INTER_RESI_DQ = np.dtype([("lambda", "<f8"), ("rates_idx", "<i4"), ("luma", "i1"), ("reserved", "i1", (3,))])
INTER_RESI_Q_DEPQUANT = 1
INTER_RESI_DQ_TS = 8                                                        # its flag: an INTER_RESI_TS slot of a 4x4 item is served
# vvcgpu_resi_rate_batch: one level block (struct vvcgpu_resi_rate_item), the bytes of a context row and the offsets of its regions
RESI_RATE_ITEM = np.dtype([("level_off", "<i8"), ("ctx_idx", "<i4"), ("w", "<i2"), ("h", "<i2"), ("luma", "i1"), ("dep_quant", "i1"),
                           ("sign_hiding", "i1"), ("ts_flag", "i1"), ("emt_idx", "i1"), ("emt_inter", "i1"), ("emt_thr", "i1"), ("reserved", "i1", (9,))])
RESI_RATE_CTX_BYTES, RESI_RATE_CTX_USED = 192, 180
RESI_RATE_LAST_X, RESI_RATE_LAST_Y, RESI_RATE_SIG_GROUP, RESI_RATE_SIG, RESI_RATE_PAR = 0, 25, 50, 52, 112
RESI_RATE_GT2, RESI_RATE_GT1, RESI_RATE_TS, RESI_RATE_EMT = 133, 154, 175, 176
# vvcgpu_intra_luma_choose_batch / vvcgpu_intra_chroma_choose_batch: one PU and its result (struct vvcgpu_intra_choose_pu, _result, struct
# vvcgpu_intra_chroma_choose_pu, _result), the flags, and the 64 bits of a cost that was not formed
INTRA_CHOOSE_PU = np.dtype([("rec_dst_off", "<i8"), ("level_dst_off", "<i8"), ("mode_bits", "<u8", (4,)), ("cbf_bits", "<u8", (2,)), ("emt_cu_bits", "<u8"),
                            ("cand_first", "<i4"), ("rec_dst_stride", "<i4"), ("n_modes", "<i2"), ("n_tr", "<i2"), ("mpm", "i1", (3,)), ("flags", "i1"),
                            ("reserved", "<i4", (2,))])
INTRA_CHOOSE_RESULT = np.dtype([("best_cand", "<i4"), ("best_mode", "<i4"), ("best_tr", "<i4"), ("cbf", "<i4"), ("dist", "<u8"), ("bits", "<u8"),
                                ("cost", "<f8"), ("reserved", "<i8")])
INTRA_CHROMA_CHOOSE_PU = np.dtype([("mode_bits", "<u8", (6,)), ("cbf_cb_bits", "<u8", (2,)), ("cbf_cr_bits", "<u8", (4,)), ("dist_weight", "<f8", (2,)),
                                   ("rec_dst_off", "<i8", (2,)), ("level_dst_off", "<i8", (2,)), ("rec_dst_stride", "<i4"), ("reserved", "<i4", (3,))])
INTRA_CHROMA_CHOOSE_RESULT = np.dtype([("best_slot", "<i4"), ("best_mode", "<i4"), ("cbf", "<i4", (2,)), ("dist", "<u8"), ("bits", "<u8"), ("cost", "<f8"),
                                       ("reserved", "<i8")])
INTRA_CHOOSE_EMT_FLAG, INTRA_CHOOSE_TS_LAST, INTRA_CHOOSE_FAST_EMT = 1, 2, 4
INTRA_CHOOSE_PASSED = 0x7FF8000000564356

# ---- affine motion --------------------------------------------------------------------------------------------------------------
AFG_DESC = np.dtype([("pred_off", "<i8"), ("deriv_off", "<i8"), ("pred_stride", "<i4"), ("deriv_stride", "<i4"), ("w", "<i2"), ("h", "<i2"),
                     ("reserved", "<i4")])
AFE_DESC = np.dtype([("resi_off", "<i8"), ("deriv_off", "<i8"), ("deriv_stride", "<i4"), ("w", "<i2"), ("h", "<i2"), ("six_param", "<i4"),
                     ("reserved", "<i4")])
AFFINE_PU = np.dtype([("pos_x", "<i4"), ("pos_y", "<i4"), ("w", "<i2"), ("h", "<i2"), ("six_param", "<i2"), ("bi", "<i2"), ("mv", "<i4", (2, 3, 2)),
                      ("dst_off", "<i8"), ("dst_stride", "<i4"), ("first_desc", "<i4")])
AFFINE_ITER = np.dtype([("pu", AFFINE_PU), ("org_off", "<i8"), ("org_stride", "<i4"), ("reserved", "<i4")])
# vvcgpu_affine_me_batch: one (PU, reference picture) search, its result and one step of its trace
AFFINE_ME_MAX_STEPS = 8
AFFINE_ME_ITEM = np.dtype([("pu", AFFINE_PU), ("org_off", "<i8"), ("org_stride", "<i4"), ("half_weight", "<i4"), ("mvp", "<i4", (3, 2)), ("bits", "<u4"),
                           ("reserved", "<i4")])
AFFINE_ME_RESULT = np.dtype([("mv", "<i4", (3, 2)), ("bits", "<u4"), ("steps", "<u4"), ("cost", "<u8")])
AFFINE_ME_STEP = np.dtype([("mv", "<i4", (3, 2)), ("cost", "<u8")])


class AffineMeCfg(C.Structure):
    """vvcgpu_affine_me_cfg"""
    _fields_ = [("lambda_", C.c_double), ("pic_w", C.c_int32), ("pic_h", C.c_int32), ("max_cu_w", C.c_int32), ("max_cu_h", C.c_int32),
                ("ref_origin_x", C.c_int32), ("ref_origin_y", C.c_int32), ("ref_stride", C.c_int32), ("bit_depth", C.c_int32), ("clp_min", C.c_int32),
                ("clp_max", C.c_int32), ("affine_type", C.c_int32), ("reserved", C.c_int32 * 3)]


# vvcgpu_bipred_me_batch: one (list, reference index) record, one PU, its result and one step of its trace
BIPRED_ME_MAX_STEPS, BIPRED_ME_MAX_REFS, BIPRED_ME_MAX_PLANES = 16, 4, 16
BIPRED_ME_REF = np.dtype([("plane", "<i4"), ("mv", "<i4", (2,)), ("mv_cand", "<i4", (2, 2)), ("num_cand", "<i2"), ("mvp_idx", "<i2")])
BIPRED_ME_ITEM = np.dtype([("pos_x", "<i4"), ("pos_y", "<i4"), ("w", "<i2"), ("h", "<i2"), ("sub_shift", "<i2"), ("reserved0", "<i2"), ("org_off", "<i8"),
                           ("org_stride", "<i4"), ("n_ref", "<i4", (2,)), ("ref_idx", "<i4", (2,)), ("mv", "<i4", (2, 2)), ("reserved1", "<i4"),
                           ("cost", "<u8", (2,)), ("bits", "<u4", (2,)), ("mb_bits", "<u4", (3,)), ("reserved2", "<i4"),
                           ("ref", BIPRED_ME_REF, (2, BIPRED_ME_MAX_REFS))])
BIPRED_ME_RESULT = np.dtype([("mv", "<i4", (2, 2)), ("ref_idx", "<i4", (2,)), ("mvp_idx", "<i4", (2,)), ("mvp", "<i4", (2, 2)), ("bits", "<u4"),
                             ("mot_bits", "<u4", (2,)), ("me_calls", "<u4"), ("closing", "<u4"), ("reserved", "<u4"), ("cost", "<u8")])
BIPRED_ME_STEP = np.dtype([("list", "<i4"), ("ref", "<i4"), ("int_mv", "<i4", (2,)), ("mv", "<i4", (2,)), ("bits", "<u4"), ("mvp_idx", "<i4"),
                           ("accepted", "<i4"), ("reserved", "<i4"), ("cost", "<u8")])


class BipredMeCfg(C.Structure):
    """vvcgpu_bipred_me_cfg"""
    _fields_ = [("lambda_", C.c_double), ("ref_planes", C.c_void_p * BIPRED_ME_MAX_PLANES), ("n_planes", C.c_int32), ("ref_stride", C.c_int32),
                ("pic_w", C.c_int32), ("pic_h", C.c_int32), ("max_cu_w", C.c_int32), ("max_cu_h", C.c_int32), ("bit_depth", C.c_int32),
                ("clp_min", C.c_int32), ("clp_max", C.c_int32), ("num_iter", C.c_int32), ("pick_list_by_cost", C.c_int32), ("mvd_l1_zero", C.c_int32),
                ("bipred_search_range", C.c_int32), ("clip_for_bipred_me", C.c_int32), ("use_hadamard", C.c_int32), ("mvp_idx_cost", C.c_uint32 * 3),
                ("max_pu_w", C.c_int32), ("max_pu_h", C.c_int32), ("imv", C.c_int32), ("reserved", C.c_int32)]


# vvcgpu_unipred_me_batch: one (list, reference index) of an item, one PU, one (list, reference index) of a result, the result of a PU
UNIPRED_ME_MAX_REFS, UNIPRED_ME_MAX_PLANES = 4, 16
UNIPRED_PRED2, UNIPRED_CACHED = 1, 2              # UNIPRED_ME_REF.flags
UNIPRED_ME_REF = np.dtype([("mv_cand", "<i4", (2, 2)), ("pred2", "<i4", (2,)), ("cached_mv", "<i4", (2,)), ("num_cand", "<i2"), ("flags", "<i2"),
                           ("reserved", "<i4")])
UNIPRED_ME_ITEM = np.dtype([("pos_x", "<i4"), ("pos_y", "<i4"), ("w", "<i2"), ("h", "<i2"), ("sub_shift", "<i2"), ("tz_flags", "<i2"), ("org_off", "<i8"),
                            ("org_stride", "<i4"), ("mb_bits", "<u4", (3,)), ("ref", UNIPRED_ME_REF, (2, UNIPRED_ME_MAX_REFS))])
UNIPRED_ME_SEARCH = np.dtype([("mv", "<i4", (2,)), ("int_mv", "<i4", (2,)), ("mvp_idx", "<i4"), ("bits", "<u4"), ("cost", "<u8"), ("tmpl_cost", "<u8", (2,))])
UNIPRED_ME_RESULT = np.dtype([("s", UNIPRED_ME_SEARCH, (2, UNIPRED_ME_MAX_REFS)), ("ref_idx", "<i4", (2,)), ("mv", "<i4", (2, 2)), ("cost", "<u8", (2,)),
                              ("bits", "<u4", (2,)), ("best_bip_ref_idx_l1", "<i4"), ("best_bip_mvp_l1", "<i4"), ("best_bip_dist", "<u8"),
                              ("valid_l1_ref_idx", "<i4"), ("valid_l1_mv", "<i4", (2,)), ("valid_l1_bits", "<u4"), ("valid_l1_cost", "<u8")])


class UnipredMeCfg(C.Structure):
    """vvcgpu_unipred_me_cfg"""
    _fields_ = [("lambda_", C.c_double), ("ref_planes", C.c_void_p * UNIPRED_ME_MAX_PLANES), ("n_planes", C.c_int32), ("ref_stride", C.c_int32),
                ("pic_w", C.c_int32), ("pic_h", C.c_int32), ("max_cu_w", C.c_int32), ("max_cu_h", C.c_int32), ("bit_depth", C.c_int32),
                ("clp_min", C.c_int32), ("clp_max", C.c_int32), ("n_ref", C.c_int32 * 2), ("ref_plane", (C.c_int32 * UNIPRED_ME_MAX_REFS) * 2),
                ("search_range", (C.c_int32 * UNIPRED_ME_MAX_REFS) * 2), ("list1_to_list0", C.c_int32 * UNIPRED_ME_MAX_REFS),
                ("fast_me_gen_b_low_delay", C.c_int32), ("mvd_l1_zero", C.c_int32), ("first_search_stop", C.c_int32), ("use_hadamard", C.c_int32),
                ("mvp_idx_cost", C.c_uint32 * 3), ("max_pu_w", C.c_int32), ("max_pu_h", C.c_int32), ("imv", C.c_int32), ("reserved", C.c_int32)]


# vvcgpu_affine_bipred_me_batch: one (list, reference index) record, one PU, its result and one step of its trace
AFFINE_BIPRED_MAX_STEPS, AFFINE_BIPRED_MAX_REFS = 16, 4
AFFINE_BIPRED_REF = np.dtype([("plane", "<i4"), ("mv", "<i4", (3, 2)), ("mv_cand", "<i4", (2, 3, 2)), ("num_cand", "<i2"), ("mvp_idx", "<i2")])
AFFINE_BIPRED_ITEM = np.dtype([("pos_x", "<i4"), ("pos_y", "<i4"), ("w", "<i2"), ("h", "<i2"), ("six_param", "<i2"), ("reserved0", "<i2"), ("org_off", "<i8"),
                               ("org_stride", "<i4"), ("n_ref", "<i4", (2,)), ("ref_idx", "<i4", (2,)), ("mv", "<i4", (2, 3, 2)), ("reserved1", "<i4"),
                               ("cost", "<u8", (2,)), ("bits", "<u4", (2,)), ("mb_bits", "<u4", (3,)), ("only_ref", "<i4", (2,)), ("reserved2", "<i4"),
                               ("ref", AFFINE_BIPRED_REF, (2, AFFINE_BIPRED_MAX_REFS))])
AFFINE_BIPRED_RESULT = np.dtype([("mv", "<i4", (2, 3, 2)), ("ref_idx", "<i4", (2,)), ("mvp_idx", "<i4", (2,)), ("mvp", "<i4", (2, 3, 2)), ("bits", "<u4"),
                                 ("mot_bits", "<u4", (2,)), ("me_calls", "<u4"), ("closing", "<u4"), ("reserved", "<u4"), ("cost", "<u8")])
AFFINE_BIPRED_STEP = np.dtype([("list", "<i4"), ("ref", "<i4"), ("mv", "<i4", (3, 2)), ("steps", "<u4"), ("bits", "<u4"), ("mvp_idx", "<i4"),
                               ("accepted", "<i4"), ("cost", "<u8")])


class AffineBipredCfg(C.Structure):
    """vvcgpu_affine_bipred_cfg"""
    _fields_ = [("lambda_", C.c_double), ("ref_planes", C.c_void_p * 16), ("n_planes", C.c_int32), ("ref_stride", C.c_int32),
                ("pic_w", C.c_int32), ("pic_h", C.c_int32), ("max_cu_w", C.c_int32), ("max_cu_h", C.c_int32), ("bit_depth", C.c_int32),
                ("clp_min", C.c_int32), ("clp_max", C.c_int32), ("num_iter", C.c_int32), ("pick_list_by_cost", C.c_int32), ("mvd_l1_zero", C.c_int32),
                ("clip_for_bipred_me", C.c_int32), ("affine_type", C.c_int32), ("mvp_idx_cost", C.c_uint32 * 3),
                ("max_pu_w", C.c_int32), ("max_pu_h", C.c_int32), ("reserved", C.c_int32 * 3)]


# vvcgpu_affine_unipred_me_batch: one (list, reference index) of an item, one PU, one (list, reference index) of a result, the result of a PU
AFFINE_UNIPRED_MAX_REFS = 4
AFFINE_UNIPRED_REF = np.dtype([("mv_cand", "<i4", (2, 3, 2)), ("hevc_mv", "<i4", (2,)), ("mv4", "<i4", (2, 2)), ("num_cand", "<i2"), ("reserved0", "<i2"),
                               ("reserved1", "<i4")])
AFFINE_UNIPRED_ITEM = np.dtype([("pos_x", "<i4"), ("pos_y", "<i4"), ("w", "<i2"), ("h", "<i2"), ("six_param", "<i2"), ("reserved0", "<i2"), ("org_off", "<i8"),
                                ("org_stride", "<i4"), ("mb_bits", "<u4", (3,)), ("only_ref", "<i4", (2,)),
                                ("ref", AFFINE_UNIPRED_REF, (2, AFFINE_UNIPRED_MAX_REFS))])
AFFINE_UNIPRED_SEARCH = np.dtype([("mv", "<i4", (3, 2)), ("mvp_idx", "<i4"), ("bits", "<u4"), ("cost", "<u8"), ("tmpl_cost", "<u8", (2,)), ("start_cost", "<u8"),
                                  ("inherit_cost", "<u8"), ("start", "<i4"), ("steps", "<u4"), ("searched", "<i4"), ("reserved", "<i4")])
AFFINE_UNIPRED_RESULT = np.dtype([("s", AFFINE_UNIPRED_SEARCH, (2, AFFINE_UNIPRED_MAX_REFS)), ("ref_idx", "<i4", (2,)), ("mv", "<i4", (2, 3, 2)),
                                  ("cost", "<u8", (2,)), ("bits", "<u4", (2,)), ("best_bip_ref_idx_l1", "<i4"), ("best_bip_mvp_l1", "<i4"),
                                  ("best_bip_dist", "<u8"), ("valid_l1_ref_idx", "<i4"), ("valid_l1_mv", "<i4", (3, 2)), ("valid_l1_bits", "<u4"),
                                  ("valid_l1_cost", "<u8")])


class AffineUnipredCfg(C.Structure):
    """vvcgpu_affine_unipred_cfg"""
    _fields_ = [("lambda_", C.c_double), ("ref_planes", C.c_void_p * 16), ("n_planes", C.c_int32), ("ref_stride", C.c_int32),
                ("pic_w", C.c_int32), ("pic_h", C.c_int32), ("max_cu_w", C.c_int32), ("max_cu_h", C.c_int32), ("bit_depth", C.c_int32),
                ("clp_min", C.c_int32), ("clp_max", C.c_int32), ("n_ref", C.c_int32 * 2), ("ref_plane", (C.c_int32 * AFFINE_UNIPRED_MAX_REFS) * 2),
                ("list1_to_list0", C.c_int32 * AFFINE_UNIPRED_MAX_REFS), ("fast_me_gen_b_low_delay", C.c_int32), ("mvd_l1_zero", C.c_int32),
                ("affine_type", C.c_int32), ("mvp_idx_cost", C.c_uint32 * 3), ("max_pu_w", C.c_int32), ("max_pu_h", C.c_int32), ("reserved", C.c_int32)]


# ---- encoder picture analysis ---------------------------------------------------------------------------------------------------------------------
# vvcgpu_tile_stats: one tile of vvcgpu_tile_stats_picture; vvcgpu_wp_sad_cand: one candidate of vvcgpu_wp_sad_batch (flags: WP_SAD_*)
TILE_STATS = np.dtype([("sa_act", "<u8"), ("sum", "<u8"), ("ss_err", "<u8")])
WP_SAD_CAND = np.dtype([("log2_denom", "<i4"), ("weight", "<i4"), ("offset", "<i4"), ("flags", "<i4")])
WP_SAD_HIGH_PRECISION, WP_SAD_CLIPPED = 1, 2
