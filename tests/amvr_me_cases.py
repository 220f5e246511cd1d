"""The uni- and bi-predictive loops of InterSearch::predInterSearch (InterSearch.cpp:877-964, :1058-1164) with cu.imv (AMVR: 0 quarter-sample, 1
integer-sample, 2 four-sample vectors) restated for the tests of vvcgpu_unipred_me_batch / vvcgpu_bipred_me_batch with cfg.imv.  Written from the
reference's text over the CPU restatement's pixel steps: xTZSearch = orc_tz_search with imv_shift, xPatternSearch (:1887-1941) = orc_sad_search with
imv_shift in its vector cost, xPatternSearchIntRefine (:2408-2500) = orc_imv_refine with weight 1.0 / 0.5, the key as bipred_me_cases builds it.  What
imv changes (imvShift = imv << 1 in every vector cost, the integer refinement for the fractional one, xCheckBestMVP returning at once :1543-1546, the
vector bits of the list-1 shortcut :916) is written here; everything else is unipred_me_cases' and bipred_me_cases', whose Searchers these subclass.
With imv = 0 both give what those modules give (tests/test_amvr_me_cpu.py).  Also the builders of aligned inputs.  numpy only."""
import ctypes

import numpy as np

import bipred_me_cases as bc
import unipred_me_cases as uc
from oraclelib import p
from pu_search_kit import U64_MAX, clip_mv, ref_bits
from vvcsoftware_vtm_amd import abi

MARGIN, SIDES, MAX_REFS, MAX_STEPS = uc.MARGIN, uc.SIDES, uc.MAX_REFS, bc.MAX_STEPS
U32_MAX = 0xFFFFFFFF
TEST_POS = ((0, 0), (-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))      # :2432


def round_mv(v, sh):
    """roundMV of one component (Mv.cpp:44-52)"""
    return ((v + (1 << (sh - 1))) >> sh) << sh


class IntRefine:
    """xPatternSearchIntRefine for both Searchers (self.o, self.c, self.m, self.rs, self.planes, self.sh)"""

    def imv_bits(self, pred, scale, x, y):
        """getBitsOfVectorWithPredictor(x, y, imvShift) (RdCost.h:189)"""
        return self.o.orc_expgolomb_bits(((x << scale) - int(pred[0])) >> self.sh) + self.o.orc_expgolomb_bits(((y << scale) - int(pred[1])) >> self.sh)

    def int_refine(self, key, ks, kx, ky, it, plane, a, idx, bits, int_mv, weight, strict, facts):
        """-> (vector, predictor, predictor index, bits, cost); key: the plane the key block lies in (pitch ks) at (kx, ky)"""
        c, sh, w, h, px, py = self.c, self.sh, int(it["w"]), int(it["h"]), int(it["pos_x"]), int(it["pos_y"])
        cand = [[int(v) for v in a["mv_cand"][k]] for k in range(2)]
        nc = int(a["num_cand"])
        mv = [int_mv[0] << 2, int_mv[1] << 2]
        if strict and any((mv[k] - cand[i][k]) & 3 for i in range(2) for k in range(2)):     # the CHECKs of :2437-2438, on both candidates whatever numCand is
            raise bc.RefThrows()
        pu = np.zeros(1, abi.IMV_PU)
        pu[0]["org_x"], pu[0]["org_y"], pu[0]["ref_x"], pu[0]["ref_y"], pu[0]["mv_x"], pu[0]["mv_y"] = kx, ky, self.m + px, self.m + py, int_mv[0], int_mv[1]
        pu[0]["cand_x"], pu[0]["cand_y"] = [cand[0][0], cand[1][0]], [cand[0][1], cand[1][1]]
        pu[0]["pos_x"], pu[0]["pos_y"], pu[0]["idx_cost"], pu[0]["bits"] = px, py, c["mvp_idx_cost"][:2], bits & U32_MAX
        pu[0]["w"], pu[0]["h"], pu[0]["num_cand"], pu[0]["mvp_idx"] = w, h, nc, idx
        tc = np.zeros(1, abi.TZ_CFG)
        tc[0]["lambda"], tc[0]["imv_shift"], tc[0]["pic_w"], tc[0]["pic_h"], tc[0]["max_cu_w"], tc[0]["max_cu_h"] = c["lambda_"], sh, c["pic_w"], c["pic_h"], c["max_cu"], c["max_cu"]
        tc[0]["ref_x1"], tc[0]["ref_y1"] = self.rs, self.planes.shape[1]                       # the whole padded plane is readable: the clamp never binds
        out = np.zeros(1, abi.IMV_RESULT)
        self.o.orc_imv_refine(p(key), ks, p(self.planes[plane]), self.rs, p(pu), 1, p(tc), c["use_hadamard"], ctypes.c_double(weight), p(out))
        got = [int(out[0]["mv_x"]), int(out[0]["mv_y"])]
        nidx = int(out[0]["mvp_idx"])
        if facts is not None:
            base = [[round_mv(mv[k] - cand[i][k], sh) + cand[i][k] for k in range(2)] for i in range(nc)]
            if got != base[nidx]:
                facts.add("leaves_centre")
            if nidx != idx:
                facts.add("refine_switches_idx")
            if nc == 2:
                facts.add(("sets_equal" if base[0] == base[1] else "sets_differ", self.sh >> 1))
            lim = ((px, c["pic_w"]), (py, c["pic_h"]))
            for b in base:
                for d in TEST_POS:
                    if any(clip_mv(b[k] + (d[k] << sh), lim[k][0], lim[k][1], c["max_cu"]) != b[k] + (d[k] << sh) for k in range(2)):
                        facts.add("refine_clip_binds")
        return got, cand[nidx], nidx, int(out[0]["bits"]), int(out[0]["cost"])


class UniSearcher(uc.Searcher, IntRefine):
    """unipred_me_cases.Searcher with cu.imv: search(item) -> (result record, out-item record)"""

    def __init__(self, org, planes_pad, cfg, imv, margin=MARGIN):
        super().__init__(org, planes_pad, cfg, margin)
        self.imv, self.sh = imv, imv << 1

    def tz(self, it, lst, r, pred, facts):
        """xTZSearch of xMotionEstimation(bBi = false), the normal and the cached-start path, the vector cost with imvShift -> the integer vector"""
        c, w, h, px, py, m = self.c, int(it["w"]), int(it["h"]), int(it["pos_x"]), int(it["pos_y"]), self.m
        a = it["ref"][lst][r]
        oy, ox = divmod(int(it["org_off"]), int(it["org_stride"]))
        pu = np.zeros(1, abi.TZ_PU)
        pu[0]["org_x"], pu[0]["org_y"], pu[0]["ref_x"], pu[0]["ref_y"] = ox, oy, m + px, m + py
        if int(a["flags"]) & abi.UNIPRED_CACHED:
            pu[0]["start_x"], pu[0]["start_y"], pu[0]["flags"] = int(a["cached_mv"][0]) << 2, int(a["cached_mv"][1]) << 2, abi.TZ_FAST
        else:
            pu[0]["start_x"], pu[0]["start_y"] = pred
            pu[0]["flags"] = (int(it["tz_flags"]) & abi.TZ_EXTENDED) | (abi.TZ_PRED2 if int(a["flags"]) & abi.UNIPRED_PRED2 else 0)
        pu[0]["pred2_x"], pu[0]["pred2_y"] = a["pred2"]
        pu[0]["pos_x"], pu[0]["pos_y"], pu[0]["pred_hor"], pu[0]["pred_ver"] = px, py, pred[0], pred[1]
        pu[0]["w"], pu[0]["h"], pu[0]["sub_shift"] = w, h, int(it["sub_shift"])
        tc = np.zeros(1, abi.TZ_CFG)
        tc[0]["lambda"], tc[0]["cost_scale"], tc[0]["imv_shift"], tc[0]["search_range"] = c["lambda_"], 2, self.sh, c["search_range"][lst][r]
        tc[0]["first_search_stop"] = c["first_search_stop"]
        tc[0]["pic_w"], tc[0]["pic_h"], tc[0]["max_cu_w"], tc[0]["max_cu_h"] = c["pic_w"], c["pic_h"], c["max_cu"], c["max_cu"]
        e = c["max_cu"] + uc.CLAMP
        tc[0]["ref_x0"], tc[0]["ref_y0"], tc[0]["ref_x1"], tc[0]["ref_y1"] = m - e, m - e, m + c["pic_w"] + e, m + c["pic_h"] + e
        best = np.zeros(1, abi.SEARCH_BEST)
        self.o.orc_tz_search(p(self.org), int(it["org_stride"]), p(self.planes[c["ref_plane"][lst][r]]), self.rs, p(pu), 1, p(tc), p(best))
        if facts is not None:
            st = np.zeros(3, np.uint64)
            self.o.orc_tz_stats(p(st))
            facts.add("raster" if int(st[2]) else "no_raster")
        return [int(best[0]["x"]), int(best[0]["y"])]

    def search(self, it, facts=None, strict=False):
        """strict: raise bipred_me_cases.RefThrows where the reference's CHECKs of xPatternSearchIntRefine would"""
        c = self.c
        res, out = np.zeros(1, abi.UNIPRED_ME_RESULT), np.zeros(1, abi.BIPRED_ME_ITEM)
        if not uc.item_ok(it, c):
            res[0]["cost"] = U64_MAX
            return res[0], out[0]
        n_ref, mic, mb = c["n_ref"], c["mvp_idx_cost"], [int(v) for v in it["mb_bits"]]
        ui_cost, ui_bits, ref_idx, c_mv = [U64_MAX, U64_MAX], [0, 0], [0, 0], [[0, 0], [0, 0]]
        cost_l0, bits_l0 = [0] * MAX_REFS, [0] * MAX_REFS
        best_bip_dist, best_bip_mvp, best_bip_ref = U64_MAX, 0, 0
        cost_valid, bits_valid, mv_valid, ref_valid = U64_MAX, U32_MAX, [0, 0], 0
        mv_temp = [[[0, 0] for _ in range(MAX_REFS)] for _ in range(2)]
        mvp_idx = [[0] * MAX_REFS for _ in range(2)]
        oy, ox = divmod(int(it["org_off"]), int(it["org_stride"]))
        for lst in range(2):
            for r in range(n_ref[lst]):
                a = it["ref"][lst][r]
                cand = [[int(v) for v in a["mv_cand"][k]] for k in range(2)]
                bits = mb[lst] + ref_bits(n_ref[lst], r)
                best_cost, idx, tmpl = U64_MAX, 0, [0, 0]
                for i in range(int(a["num_cand"])):                        # xEstimateMvPredAMVP, bFilled
                    tmpl[i] = self.template_cost(it, c["ref_plane"][lst][r], cand[i], i)
                    if best_cost > tmpl[i]:
                        best_cost, idx = tmpl[i], i
                pred = cand[idx]
                if c["mvd_l1_zero"] and lst == 1 and best_cost < best_bip_dist:
                    best_bip_dist, best_bip_mvp, best_bip_ref = best_cost, idx, r
                bits += mic[idx]
                imv = [0, 0]
                if uc.shortcut(c, lst, r):                                 # :905-922, the vector bits with imvShift (:916)
                    k = c["list1_to_list0"][r]
                    mv = list(mv_temp[0][k])
                    cost = (cost_l0[k] - self.b.get_cost(bits_l0[k])) & U64_MAX
                    bits = (bits + self.imv_bits(pred, 0, mv[0], mv[1])) & U32_MAX
                    cost = (cost + self.b.get_cost(bits)) & U64_MAX
                    if facts is not None:
                        facts.add("shortcut")
                elif self.imv == 0:
                    imv, mv, bits, cost = self.motion_estimation(it, lst, r, pred, bits, facts)
                else:                                                      # :1668-1816 with imv: xTZSearch, then xPatternSearchIntRefine on the original
                    imv = self.tz(it, lst, r, pred, facts)
                    mv, pred, idx, bits, cost = self.int_refine(self.org, int(it["org_stride"]), ox, oy, it, c["ref_plane"][lst][r], a, idx, bits, imv, 1.0, strict, facts)
                    if facts is not None and lst == 1:
                        facts.add("searched_l1")
                mv_temp[lst][r] = mv
                if self.imv == 0:                                          # xCheckBestMVP returns at once otherwise (:1543-1546)
                    pred, idx, bits, cost = self.b.check_best_mvp(dict(mv_cand=cand, num_cand=int(a["num_cand"])), mv, pred, idx, bits, cost)
                mvp_idx[lst][r] = idx
                res[0]["s"][lst][r] = (mv, imv, idx, bits, cost, tmpl)
                if lst == 0:
                    cost_l0[r], bits_l0[r] = cost, bits
                if cost < ui_cost[lst]:
                    ui_cost[lst], ui_bits[lst], c_mv[lst], ref_idx[lst] = cost, bits, list(mv), r
                if lst == 1 and cost < cost_valid and c["list1_to_list0"][r] < 0:
                    cost_valid, bits_valid, mv_valid, ref_valid = cost, bits, list(mv), r
        res[0]["ref_idx"], res[0]["mv"], res[0]["cost"], res[0]["bits"] = ref_idx, c_mv, ui_cost, ui_bits
        res[0]["best_bip_ref_idx_l1"], res[0]["best_bip_mvp_l1"], res[0]["best_bip_dist"] = best_bip_ref, best_bip_mvp, best_bip_dist
        res[0]["valid_l1_ref_idx"], res[0]["valid_l1_mv"], res[0]["valid_l1_bits"], res[0]["valid_l1_cost"] = ref_valid, mv_valid, bits_valid, cost_valid
        o = out[0]
        for f in ("pos_x", "pos_y", "w", "h", "sub_shift", "org_off", "org_stride", "mb_bits"):
            o[f] = it[f]
        o["n_ref"], o["ref_idx"], o["mv"], o["cost"], o["bits"] = n_ref, ref_idx, c_mv, ui_cost, ui_bits
        for lst in range(2):
            for r in range(n_ref[lst]):
                a, q = it["ref"][lst][r], o["ref"][lst][r]
                q["plane"], q["mv"], q["mv_cand"], q["num_cand"], q["mvp_idx"] = c["ref_plane"][lst][r], mv_temp[lst][r], a["mv_cand"], a["num_cand"], mvp_idx[lst][r]
        if c["mvd_l1_zero"] and n_ref[1] > 0:                              # :1009-1023, :1038
            q = o["ref"][1][best_bip_ref]
            q["mvp_idx"] = best_bip_mvp
            q["mv"] = q["mv_cand"][best_bip_mvp]
            o["mv"][1], o["ref_idx"][1] = q["mv"], best_bip_ref
        return res[0], out[0]


class BiSearcher(bc.Searcher, IntRefine):
    """bipred_me_cases.Searcher with cu.imv: search(item) -> (result record, trace records)"""

    def __init__(self, org, planes_pad, cfg, imv, margin=MARGIN):
        super().__init__(org, planes_pad, cfg, margin)
        self.imv, self.sh = imv, imv << 1

    def int_search(self, it, plane, key, entry, pred):
        """xSetSearchRange (:1820-1854) around the entry vector and xPatternSearch with imvShift -> the integer vector"""
        c, w, h, px, py, R = self.c, int(it["w"]), int(it["h"]), int(it["pos_x"]), int(it["pos_y"]), self.c["search_range"]
        lim = ((px, c["pic_w"]), (py, c["pic_h"]))
        ctr = [clip_mv(entry[k], lim[k][0], lim[k][1], c["max_cu"]) for k in range(2)]
        tl = [(clip_mv(ctr[k] - (R << 2), lim[k][0], lim[k][1], c["max_cu"]) + 2) >> 2 for k in range(2)]
        br = [(clip_mv(ctr[k] + (R << 2), lim[k][0], lim[k][1], c["max_cu"]) + 2) >> 2 for k in range(2)]
        blk = np.array([(0, 0, self.m + px, self.m + py)], dtype=abi.SEARCH_BLK)
        mc = abi.MvCost(c["lambda_"], int(pred[0]), int(pred[1]), 2, self.sh)
        best = np.zeros(1, abi.SEARCH_BEST)
        self.o.orc_sad_search(p(key), w, p(self.planes[plane]), self.rs, p(blk), 1, w, h, int(it["sub_shift"]), tl[0], tl[1], br[0] - tl[0] + 1, br[1] - tl[1] + 1, 1, 1,
                              None, ctypes.byref(mc), p(best))
        return [int(best[0]["x"]), int(best[0]["y"])]

    def search(self, it, strict=False, facts=None):
        facts = set() if facts is None else facts
        c = self.c
        res, trace = np.zeros(1, abi.BIPRED_ME_RESULT), np.zeros(MAX_STEPS, abi.BIPRED_ME_STEP)
        if not bc.item_ok(it, c, len(self.planes)):
            res["cost"] = np.uint64(U64_MAX)
            return res[0], trace
        w = int(it["w"])
        n_ref = [int(v) for v in it["n_ref"]]
        rec = it["ref"]
        mv_temp = [[[int(v) for v in rec[l][r]["mv"]] for r in range(4)] for l in range(2)]
        mvp_idx = [[int(rec[l][r]["mvp_idx"]) & 1 for r in range(4)] for l in range(2)]
        mv_pred = [[[int(v) for v in rec[l][r]["mv_cand"][mvp_idx[l][r]]] for r in range(4)] for l in range(2)]
        mv_bi = [[int(v) for v in it["mv"][l]] for l in range(2)]
        ref_bi = [int(v) for v in it["ref_idx"]]
        uni_cost = [int(v) for v in it["cost"]]
        mb = [int(v) for v in it["mb_bits"]]
        mot = [(int(it["bits"][0]) - mb[0]) & U32_MAX, 0]
        if c["mvd_l1_zero"]:
            mot[1] = mb[1] + ref_bits(n_ref[1], ref_bi[1]) + c["mvp_idx_cost"][mvp_idx[1][ref_bi[1]]]
        else:
            mot[1] = (int(it["bits"][1]) - mb[1]) & U32_MAX
        bits2 = (mb[2] + mot[0] + mot[1]) & U32_MAX
        cost_bi, calls, closing = U64_MAX, 0, 0
        for it_no in range(c["num_iter"]):
            lst = it_no % 2
            if c["pick_list_by_cost"]:
                lst = 1 if uni_cost[0] <= uni_cost[1] else 0
            elif it_no == 0:
                lst = 0
            if c["mvd_l1_zero"]:
                lst = 0
            oth = 1 - lst
            key = self.key(it, self.predict(it, int(rec[oth][ref_bi[oth]]["plane"]), mv_bi[oth]))
            changed = False
            for r in range(n_ref[lst]):
                plane = int(rec[lst][r]["plane"])
                bits_t = (mb[2] + mot[oth] + ref_bits(n_ref[lst], r) + c["mvp_idx_cost"][mvp_idx[lst][r]]) & U32_MAX
                before = mvp_idx[lst][r]
                if self.imv == 0:
                    imv, mv, bits_t, cost_t = self.motion_estimation(it, plane, key, mv_temp[lst][r], mv_pred[lst][r], bits_t)
                    bits_t &= U32_MAX
                    mv_pred[lst][r], mvp_idx[lst][r], bits_t, cost_t = self.check_best_mvp(rec[lst][r], mv, mv_pred[lst][r], mvp_idx[lst][r], bits_t, cost_t, strict)
                else:                                                      # xPatternSearch, then xPatternSearchIntRefine with half weight on the key; no xCheckBestMVP
                    imv = self.int_search(it, plane, key, mv_temp[lst][r], mv_pred[lst][r])
                    mv, mv_pred[lst][r], mvp_idx[lst][r], bits_t, cost_t = self.int_refine(key, w, 0, 0, it, plane, rec[lst][r], mvp_idx[lst][r], bits_t, imv, 0.5,
                                                                                           strict, facts)
                mv_temp[lst][r] = mv
                if mvp_idx[lst][r] != before:
                    facts.add("mvp_switch")
                accepted = cost_t < cost_bi
                facts.add("accepted" if accepted else "rejected")
                trace[calls] = (lst, r, imv, mv, bits_t, mvp_idx[lst][r], int(accepted), 0, cost_t)
                calls += 1
                if accepted:
                    changed = True
                    if r > 0:
                        facts.add("nonzero_ref_accepted")
                    mv_bi[lst], ref_bi[lst], cost_bi = list(mv), r, cost_t
                    mot[lst] = (bits_t - mb[2] - mot[oth]) & U32_MAX
                    bits2 = bits_t
            if not changed:
                if cost_bi <= uni_cost[0] and cost_bi <= uni_cost[1]:
                    closing = 1                                            # the flag reports the condition of :1142-1163; with imv the two calls return at once
                    if self.imv == 0:
                        a = rec[0][ref_bi[0]] if lst == 0 else rec[1][n_ref[1] - 1]
                        r0 = ref_bi[0]
                        mv_pred[0][r0], mvp_idx[0][r0], bits2, cost_bi = self.check_best_mvp(a, mv_bi[0], mv_pred[0][r0], mvp_idx[0][r0], bits2, cost_bi, strict)
                        if not c["mvd_l1_zero"]:
                            a = rec[0][ref_bi[0]] if lst == 0 else rec[1][ref_bi[1]]
                            r1 = ref_bi[1]
                            mv_pred[1][r1], mvp_idx[1][r1], bits2, cost_bi = self.check_best_mvp(a, mv_bi[1], mv_pred[1][r1], mvp_idx[1][r1], bits2, cost_bi, strict)
                break
        res[0] = (mv_bi, ref_bi, [mvp_idx[l][ref_bi[l]] for l in range(2)], [mv_pred[l][ref_bi[l]] for l in range(2)], bits2 & U32_MAX, mot, calls, closing, 0, cost_bi)
        return res[0], trace


def uni_all(org, planes_pad, cfg, items, imv, facts=None, strict=False):
    s = UniSearcher(org, planes_pad, cfg, imv)
    res, out = np.zeros(len(items), abi.UNIPRED_ME_RESULT), np.zeros(len(items), abi.BIPRED_ME_ITEM)
    for i, it in enumerate(items):
        res[i], out[i] = s.search(it, facts, strict)
    return res, out


def bi_all(org, planes_pad, cfg, items, imv, facts=None, strict=False):
    s = BiSearcher(org, planes_pad, cfg, imv)
    res, trace = np.zeros(len(items), abi.BIPRED_ME_RESULT), np.zeros((len(items), MAX_STEPS), abi.BIPRED_ME_STEP)
    for i, it in enumerate(items):
        res[i], trace[i] = s.search(it, strict, facts)
    return res, trace


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def align_items(items, imv, align=None):
    """what PU::fillMvpCand does to the candidates of an AMVR pass: every candidate vector a multiple of 1 << (imv << 1) quarter units (rounded, in
    place).  align: another shift -- 2 with imv 2 leaves integer-sample candidates, which the reference's CHECKs (:2437-2438) accept and for which the
    two candidates' position sets differ"""
    if imv:
        sh = (imv << 1) if align is None else align
        c = items["ref"]["mv_cand"].astype(np.int64)
        items["ref"]["mv_cand"] = ((c + (1 << (sh - 1))) >> sh) << sh
    return items


def fresh_uni(seed, bd, shapes, imv, align=None, **kw):
    """unipred_me_cases.fresh_set with aligned candidates"""
    org, planes, cfg, items = uc.fresh_set(seed, bd, shapes, **kw)
    return org, planes, cfg, align_items(items, imv, align)


def bi_cfg_of(cfg, **kw):
    """the bi-predictive cfg that goes with a uni-predictive one (the same slice)"""
    return bc.cfg_dict(cfg["lambda_"], cfg["pic_w"], cfg["pic_h"], cfg["bit_depth"], mvd_l1_zero=cfg["mvd_l1_zero"], use_hadamard=cfg["use_hadamard"],
                       mvp_idx_cost=cfg["mvp_idx_cost"], max_cu=cfg["max_cu"], **kw)


# ---- the golden file ------------------------------------------------------------------------------------------------------------------------------
# facts the golden set holds per bit depth (the Searchers report them; "wave_owner" / "group_owner": a PU of at most / more than 1024 samples)
GOLDEN_NEED = {"leaves_centre", "refine_switches_idx", ("sets_differ", 2), ("sets_equal", 2), ("sets_equal", 1), "refine_clip_binds", "shortcut", "accepted", "rejected",
               "mvp_switch", "wave_owner", "group_owner", "raster", "no_raster"}


def golden_groups(g, bd, pic=(256, 128)):
    """tests/golden/amvr_me.npz -> [(imv, uni-predictive cfg dict, bi-predictive cfg dict or None (P slice), item indices)] of one bit depth: the items
    of a group share the pass and the slice-level settings"""
    k = "bd%d_" % bd
    lam, mic = float(g[k + "lambda"]), tuple(int(v) for v in g[k + "mvp_idx_cost"])
    out = []
    for gi in range(len(g[k + "g_imv"])):
        flags = {f: int(v) for f, v in zip(uc.GOLDEN_FLAGS, g[k + "g_flags"][gi])}
        cfg = uc.cfg_dict(lam, pic[0], pic[1], bd, n_ref=[int(v) for v in g[k + "g_n_ref"][gi]], ref_plane=g[k + "g_ref_plane"][gi].tolist(),
                          search_range=g[k + "g_search_range"][gi].tolist(), list1_to_list0=[int(v) for v in g[k + "g_list1_to_list0"][gi]], mvp_idx_cost=mic, **flags)
        n, pick, rng_, clip = (int(v) for v in g[k + "g_bi"][gi])
        bcfg = bc.cfg_dict(lam, pic[0], pic[1], bd, num_iter=n, pick_list_by_cost=pick, mvd_l1_zero=flags["mvd_l1_zero"], search_range=rng_, clip_key=clip,
                           use_hadamard=flags["use_hadamard"], mvp_idx_cost=mic) if cfg["n_ref"][1] else None
        out.append((int(g[k + "g_imv"][gi]), cfg, bcfg, np.nonzero(g[k + "group"] == gi)[0]))
    return out
