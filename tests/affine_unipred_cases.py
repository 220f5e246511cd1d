"""The uni-predictive part of InterSearch::xPredAffineInterSearch (InterSearch.cpp:2651-2814) restated for the tests of
vvcgpu_affine_unipred_me_batch: xGetAffineTemplateCost (:1645-1665) is the restated affine prediction (affine_me_cases.Searcher.predict) and a numpy
SAD, xAffineMotionEstimation(bBi = false) is affine_me_cases.Searcher.search, the vector bits and xCheckBestAffineMVP (:3181-3284) are those of
affine_bipred_cases; xEstimateAffineAMVP's choice (:3765-3784), the start vectors with the 4-to-6-parameter inheritance (:2681-2727), the list-1
shortcut (:2740-2774), the bookkeeping of :2730-2735 / :2788-2812 and the out-item for vvcgpu_affine_bipred_me_batch (:2840-2853) are written here
from the reference's text.  All vectors are in 1/16 sample units: the generator (tests/golden/gen_affine_unipred.py) fed the compiled reference Mv
objects with the precision flags they carry at :2683-2706 -- hevcMv quarter-sample, mvAffine4Para 1/16-sample as xAffineMotionEstimation returns it --
and found hevc_mv = hevcMv << 2 and mv4 = mvAffine4Para as it is to give the same costs, vectors and bits.  tests/golden/affine_unipred.npz pins this
file to the compiled reference (tests/test_affine_unipred_cpu.py).  Also item_ok and the builders of the test inputs that the generator, the tests
and tools/affine_unipred_time.py share.  numpy only."""
import numpy as np

import affine_bipred_cases as ac
import affine_me_cases as amc
from pu_search_kit import U64_MAX, pad, planes_and_first_org, ref_bits, round_signal, vec3
from vvcsoftware_vtm_amd import abi

MARGIN, SIDES = ac.MARGIN, ac.SIDES        # those of the affine bi-predictive entry, which takes the out-items
MAX_REFS = abi.AFFINE_UNIPRED_MAX_REFS
U32_MAX = 0xFFFFFFFF
WAVE_MAX = 1024             # samples a wavefront owns (afi_dev.h: AFI_WAVE_MAX)
SHAPES = [(16, 16), (32, 32), (64, 16), (32, 64), (16, 128), (128, 16), (128, 128)]


def cfg_dict(lambda_, pic_w, pic_h, bit_depth, n_ref=(2, 2), ref_plane=((0, 1, 2, 3), (1, 0, 3, 2)), list1_to_list0=(-1, -1, -1, -1),
             fast_me_gen_b_low_delay=0, mvd_l1_zero=0, affine_type=1, mvp_idx_cost=(1, 1, 0), max_cu=128, max_pu=(0, 0)):
    """the host cfg as plain values (the device tests turn it into ops.affine_unipred_cfg with the planes' addresses)"""
    return dict(lambda_=float(lambda_), pic_w=pic_w, pic_h=pic_h, max_cu=max_cu, bit_depth=bit_depth, clp_min=0, clp_max=(1 << bit_depth) - 1,
                n_ref=tuple(n_ref), ref_plane=tuple(tuple(v) for v in ref_plane), list1_to_list0=tuple(list1_to_list0),
                fast_me_gen_b_low_delay=int(fast_me_gen_b_low_delay), mvd_l1_zero=int(mvd_l1_zero), affine_type=int(affine_type),
                mvp_idx_cost=tuple(mvp_idx_cost), max_pu=tuple(max_pu))


def bipred_cfg(c, **kw):
    """the cfg of the bi-predictive stage that follows a uni-predictive stage run with `c`"""
    return ac.cfg_dict(c["lambda_"], c["pic_w"], c["pic_h"], c["bit_depth"], mvd_l1_zero=c["mvd_l1_zero"], affine_type=c["affine_type"],
                       mvp_idx_cost=c["mvp_idx_cost"], max_cu=c["max_cu"], **kw)


def skipped(it, lst, r):
    """:2673: a 6-parameter PU searches only the reference index its 4-parameter search chose"""
    return int(it["six_param"]) != 0 and int(it["only_ref"][lst]) != r


def shortcut(it, c, lst, r):
    """:2740-2746"""
    k = c["list1_to_list0"][r]
    return lst == 1 and bool(c["fast_me_gen_b_low_delay"]) and k >= 0 and (int(it["six_param"]) == 0 or k == int(it["only_ref"][0]))


def item_ok(it, c):
    w, h = int(it["w"]), int(it["h"])
    mw, mh = (c["max_pu"][0] or 128), (c["max_pu"][1] or 128)
    if w not in SIDES or h not in SIDES or w > c["max_cu"] or h > c["max_cu"] or w > mw or h > mh:
        return False
    if not (0 <= int(it["pos_x"]) <= c["pic_w"] - w and 0 <= int(it["pos_y"]) <= c["pic_h"] - h) or int(it["org_stride"]) <= 0:
        return False
    for l in range(2):
        if c["n_ref"][l] > 0 and not -1 <= int(it["only_ref"][l]) < c["n_ref"][l]:
            return False
        for r in range(c["n_ref"][l]):
            if not 1 <= int(it["ref"][l][r]["num_cand"]) <= 2:
                return False
    return True


def inherited(mv4, w, h):
    """mvFour of :2696-2706 from mvAffine4Para[..][0..1] (1/16 units)"""
    m0, m1 = [int(v) for v in mv4[0]], [int(v) for v in mv4[1]]
    sh = 7 + (h.bit_length() - 1) - (w.bit_length() - 1)
    vx2 = amc.wrap32((m0[0] << 7) - ((m1[1] - m0[1]) << sh)) >> 7
    vy2 = amc.wrap32((m0[1] << 7) + ((m1[0] - m0[0]) << sh)) >> 7
    return [m0, m1, [round_signal(vx2), round_signal(vy2)]]


class Searcher:
    """one (org plane, padded reference planes [n][H + 2 M][W + 2 M], cfg): search(item) -> (result record, out-item record)"""

    def __init__(self, org, planes_pad, cfg, margin=MARGIN):
        self.org, self.planes, self.c = np.ascontiguousarray(org), np.ascontiguousarray(planes_pad), cfg
        self.b = ac.Searcher(self.org, self.planes, bipred_cfg(cfg), margin)      # get_cost, vec_bits, check_best_mvp, predict, the per-plane searches

    def block(self, it):
        w, h, off, os_ = int(it["w"]), int(it["h"]), int(it["org_off"]), int(it["org_stride"])
        return np.lib.stride_tricks.as_strided(self.org.reshape(-1)[off:], (h, w), (os_ * 2, 2)).astype(np.int64)

    def template_cost(self, it, plane, mv, idx):
        """xGetAffineTemplateCost: xPredAffineBlk (bi = false) of the vectors as they are, full SAD, + getCost(m_auiMVPIdxCost[idx][AMVP_MAX_NUM_CANDS])"""
        w, h = int(it["w"]), int(it["h"])
        pred = self.b.predict(it, plane, mv).reshape(h, w).astype(np.int64)
        return int(np.abs(self.block(it) - pred).sum()) + self.b.get_cost(self.c["mvp_idx_cost"][idx])

    def motion_estimation(self, it, plane, start, pred, bits):
        """xAffineMotionEstimation(bBi = false) -> (vectors, bits, cost, steps)"""
        w, h = int(it["w"]), int(it["h"])
        me = amc.item(int(it["pos_x"]), int(it["pos_y"]), w, h, int(it["six_param"]) != 0, start, int(it["org_off"]), int(it["org_stride"]), 0, pred, bits)
        res, _ = self.b.me[plane].search(me)
        return vec3(res["mv"]), int(res["bits"]), int(res["cost"]), int(res["steps"])

    def search(self, it, facts=None):
        """facts (a set): receives ("start", 0..2), "six_skipped", "shortcut", "shortcut_refused_six", "searched_l1", "mvp_switch_search",
        "mvp_switch_shortcut", "best_ref_nonzero", "bip_ref_nonzero", "valid_l1", "no_valid_l1", "one_cand", "same_cands_first_wins", "zero_delta_stop",
        "full_limit" when they happen"""
        facts = set() if facts is None else facts
        c = self.c
        res, out = np.zeros(1, abi.AFFINE_UNIPRED_RESULT), np.zeros(1, abi.AFFINE_BIPRED_ITEM)
        if not item_ok(it, c):
            res[0]["cost"] = U64_MAX
            return res[0], out[0]
        six = int(it["six_param"]) != 0
        nmv = 3 if six else 2
        w, h = int(it["w"]), int(it["h"])
        limit = amc.iter_limit(six, False, c["affine_type"])
        n_ref, mic, mb = c["n_ref"], c["mvp_idx_cost"], [int(v) for v in it["mb_bits"]]
        ui_cost, ui_bits, ref_idx, aac_mv = [U64_MAX, U64_MAX], [0, 0], [0, 0], [[[0, 0]] * 3, [[0, 0]] * 3]
        cost_l0, bits_l0 = [U64_MAX] * MAX_REFS, [0] * MAX_REFS
        best_bip_dist, best_bip_mvp, best_bip_ref = U64_MAX, 0, 0
        cost_valid, bits_valid, mv_valid, ref_valid = U64_MAX, U32_MAX, [[0, 0]] * 3, 0
        mv_temp = [[[[0, 0]] * 3 for _ in range(MAX_REFS)] for _ in range(2)]
        mvp_idx = [[0] * MAX_REFS for _ in range(2)]
        for lst in range(2):
            for r in range(n_ref[lst]):
                a = it["ref"][lst][r]
                plane = c["ref_plane"][lst][r]
                cand = [vec3(a["mv_cand"][k]) for k in range(2)]
                bits = mb[lst] + ref_bits(n_ref[lst], r)
                # xEstimateAffineAMVP
                bip_dist, idx, tmpl = U64_MAX, 0, [0, 0]
                for i in range(int(a["num_cand"])):
                    tmpl[i] = self.template_cost(it, plane, cand[i], i)
                    if bip_dist > tmpl[i]:
                        bip_dist, idx = tmpl[i], i
                if int(a["num_cand"]) == 1:
                    facts.add("one_cand")
                elif cand[0] == cand[1] and idx == 0 and mic[0] == mic[1]:
                    facts.add("same_cands_first_wins")
                pred = cand[idx]
                mvp_idx[lst][r] = idx
                s = res[0]["s"][lst][r]
                s["mvp_idx"], s["tmpl_cost"] = idx, tmpl
                if skipped(it, lst, r):
                    facts.add("six_skipped")
                    continue
                is_shortcut = shortcut(it, c, lst, r)
                if lst == 1 and c["fast_me_gen_b_low_delay"] and c["list1_to_list0"][r] >= 0 and not is_shortcut:
                    facts.add("shortcut_refused_six")
                start_cost = inherit_cost = sel = steps = 0
                if not is_shortcut:                                   # the reference computes them for a shortcut too and then overwrites cMvTemp
                    hevc = [[int(a["hevc_mv"][0]), int(a["hevc_mv"][1])]] * 3
                    start, sel = hevc, 1
                    cand_cost = start_cost = self.template_cost(it, plane, hevc, idx)
                    if six:
                        four = inherited(a["mv4"], w, h)
                        inherit_cost = self.template_cost(it, plane, four, idx)
                        if inherit_cost < cand_cost:
                            cand_cost, start, sel = inherit_cost, four, 2
                    if not cand_cost < bip_dist:
                        start, sel = pred, 0
                    facts.add(("start", sel))
                if c["mvd_l1_zero"] and lst == 1 and bip_dist < best_bip_dist:
                    best_bip_dist, best_bip_mvp, best_bip_ref = bip_dist, idx, r
                bits += mic[idx]
                if is_shortcut:
                    k = c["list1_to_list0"][r]
                    mv = [list(v) for v in mv_temp[0][k]]
                    cost = (cost_l0[k] - self.b.get_cost(bits_l0[k])) & U64_MAX
                    bits = (bits + self.b.vec_bits(pred, nmv, mv)) & U32_MAX
                    cost = (cost + self.b.get_cost(bits)) & U64_MAX
                    facts.add("shortcut")
                else:
                    mv, bits, cost, steps = self.motion_estimation(it, plane, start, pred, bits)
                    facts.add("full_limit" if steps == limit + 1 else "zero_delta_stop")
                    if lst == 1:
                        facts.add("searched_l1")
                mv_temp[lst][r] = mv
                pred, idx2, bits, cost = self.b.check_best_mvp(a, nmv, mv, pred, idx, bits, cost)
                if idx2 != idx:
                    facts.add("mvp_switch_shortcut" if is_shortcut else "mvp_switch_search")
                mvp_idx[lst][r] = idx2
                res[0]["s"][lst][r] = (mv, idx2, bits, cost, tmpl, start_cost, inherit_cost, sel, steps, 2 if is_shortcut else 1, 0)
                if lst == 0:
                    cost_l0[r], bits_l0[r] = cost, bits
                if cost < ui_cost[lst]:
                    ui_cost[lst], ui_bits[lst], aac_mv[lst], ref_idx[lst] = cost, bits, [list(v) for v in mv], r
                    if r > 0:
                        facts.add("best_ref_nonzero")
                if lst == 1 and cost < cost_valid and c["list1_to_list0"][r] < 0:
                    cost_valid, bits_valid, mv_valid, ref_valid = cost, bits, [list(v) for v in mv], r
        if c["mvd_l1_zero"] and best_bip_ref > 0:
            facts.add("bip_ref_nonzero")
        if n_ref[1] > 0:
            facts.add("valid_l1" if cost_valid != U64_MAX else "no_valid_l1")
        res[0]["ref_idx"], res[0]["mv"], res[0]["cost"], res[0]["bits"] = ref_idx, aac_mv, ui_cost, ui_bits
        res[0]["best_bip_ref_idx_l1"], res[0]["best_bip_mvp_l1"], res[0]["best_bip_dist"] = best_bip_ref, best_bip_mvp, best_bip_dist
        res[0]["valid_l1_ref_idx"], res[0]["valid_l1_mv"], res[0]["valid_l1_bits"], res[0]["valid_l1_cost"] = ref_valid, mv_valid, bits_valid, cost_valid
        # what vvcgpu_affine_bipred_me_batch asks of its caller
        o = out[0]
        for f in ("pos_x", "pos_y", "w", "h", "six_param", "org_off", "org_stride", "mb_bits", "only_ref"):
            o[f] = it[f]
        o["n_ref"], o["ref_idx"], o["mv"], o["cost"], o["bits"] = n_ref, ref_idx, aac_mv, ui_cost, ui_bits
        for lst in range(2):
            for r in range(n_ref[lst]):
                a, q = it["ref"][lst][r], o["ref"][lst][r]
                q["plane"], q["mv"], q["mv_cand"], q["num_cand"], q["mvp_idx"] = c["ref_plane"][lst][r], mv_temp[lst][r], a["mv_cand"], a["num_cand"], mvp_idx[lst][r]
        if c["mvd_l1_zero"] and n_ref[1] > 0:                     # :2840-2853
            q = o["ref"][1][best_bip_ref]
            q["mvp_idx"] = best_bip_mvp
            q["mv"] = q["mv_cand"][best_bip_mvp]
            o["mv"][1], o["ref_idx"][1] = q["mv"], best_bip_ref
        return res[0], out[0]


def search_all(org, planes_pad, cfg, items, facts=None):
    s = Searcher(org, planes_pad, cfg)
    res, out = np.zeros(len(items), abi.AFFINE_UNIPRED_RESULT), np.zeros(len(items), abi.AFFINE_BIPRED_ITEM)
    for i, it in enumerate(items):
        res[i], out[i] = s.search(it, facts)
    return res, out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def item(px, py, w, h, six, org_off, org_stride, refs, only_ref=(-1, -1), mb_bits=(2, 2, 4)):
    """refs = ([records of list 0], [records of list 1]), each (candidates [1 or 2][3][2], hevc_mv [2], mv4 [2][2])"""
    it = np.zeros(1, abi.AFFINE_UNIPRED_ITEM)
    it[0]["pos_x"], it[0]["pos_y"], it[0]["w"], it[0]["h"], it[0]["six_param"] = px, py, w, h, 1 if six else 0
    it[0]["org_off"], it[0]["org_stride"], it[0]["mb_bits"], it[0]["only_ref"] = org_off, org_stride, mb_bits, only_ref
    for l in range(2):
        for r, (cands, hevc, mv4) in enumerate(refs[l][:MAX_REFS]):
            a = it[0]["ref"][l][r]
            cands = [np.asarray(v, np.int32).reshape(3, 2) for v in cands]
            a["mv_cand"], a["num_cand"], a["hevc_mv"], a["mv4"] = (cands + cands)[:2], len(cands), hevc, mv4
    return it[0]


def random_item(rng, W, H, w, h, six, n_ref, px=None, py=None, far=0, cands=None, truth=None):
    """one PU around a true warp `truth` (default: a seeded gentle one): per (list, reference) candidates, the translational vector and the 4-parameter
    vectors are the truth displaced by seeded amounts of seeded scale, so that each of the three starts wins somewhere; far: every vector is displaced
    by +-far samples as well (the sub-block clip binds at the picture's corners); cands: 1 one candidate, 2 two identical ones, None seeded"""
    if px is None:
        px, py = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
    if truth is None:
        truth = amc.random_true_mv(rng, w, h, six, spread=10)
    refs = []
    for l in range(2):
        recs = []
        for _ in range(MAX_REFS):
            off = rng.integers(-1, 2, 2) * far * 16
            s = [int(v) for v in rng.choice([0, 1, 3, 8], 3)]             # how far the candidates, the translational and the 4-parameter vectors are off

            def near(v, k):
                return np.asarray(v) + off + rng.integers(-s[k], s[k] + 1, np.asarray(v).shape) * 4
            kind = int(rng.integers(0, 6)) if cands is None else {1: 0, 2: 1}[cands]
            cs = [near(truth, 0)] if kind == 0 else [near(truth, 0)] * 2 if kind == 1 else [near(truth, 0), near(truth, 0)]
            recs.append((cs, near(truth[0], 1), near(truth[:2], 2)))
        refs.append(recs)
    only = (int(rng.integers(0, n_ref[0])), int(rng.integers(-1, n_ref[1])) if n_ref[1] else -1) if six else (-1, -1)
    return item(px, py, w, h, six, py * W + px, W, refs, only, [int(v) for v in rng.integers(1, 6, 3)]), truth


def paint(org, searcher, it, plane, truth, rng, noise=2):
    """the item's block of the original := the affine prediction of `truth` from `plane` plus noise (restated prediction; painting only makes inputs)"""
    w, h, px, py = int(it["w"]), int(it["h"]), int(it["pos_x"]), int(it["pos_y"])
    pr = searcher.b.predict(it, plane, vec3(truth)).reshape(h, w).astype(np.int32)
    org[py:py + h, px:px + w] = np.clip(pr + rng.integers(-noise, noise + 1, (h, w)), 0, searcher.c["clp_max"]).astype(np.int16)


def fresh_set(seed, bd, shapes, pic=(256, 128), n_planes=4, painted=0.7, far=0, corners=False, **cfgkw):
    """seeded inputs for the device tests: -> (org plane, padded planes, cfg dict, items); one PU per entry of `shapes` = (w, h, six).  A share `painted`
    of the PUs sits on a warped patch of one of its reference planes, so that its searches do real work (later PUs may paint over earlier ones: still
    valid searches); corners: the PUs sit in the picture's corners"""
    rng = np.random.default_rng(seed)
    W, H = pic
    planes, org = planes_and_first_org(rng, n_planes, W, H, bd)
    cfg = cfg_dict(4.0 + (seed % 5) * 9.25, W, H, bd, **cfgkw)
    planes = pad(planes)
    s = Searcher(org, planes, cfg)
    items = np.zeros(len(shapes), abi.AFFINE_UNIPRED_ITEM)
    for i, (w, h, six) in enumerate(shapes):
        pos = ((0, W - w)[i & 1], (0, H - h)[(i >> 1) & 1]) if corners else (None, None)
        items[i], truth = random_item(rng, W, H, w, h, six, cfg["n_ref"], pos[0], pos[1], far)
        if rng.random() < painted:
            l = int(rng.integers(0, 2)) if cfg["n_ref"][1] else 0
            paint(org, s, items[i], cfg["ref_plane"][l][int(rng.integers(0, cfg["n_ref"][l]))], truth, rng)
    return np.ascontiguousarray(org), planes, cfg, items


def alternating_shapes(n):
    """n shapes (w, h, six) in which wavefront-owned (<= WAVE_MAX samples) and workgroup-owned PUs alternate, 4- and 6-parameter items alternate within
    each kind, and every side pair occurs (n >= 32)"""
    pairs = [(w, h) for w in SIDES for h in SIDES]
    small = [s for s in pairs if s[0] * s[1] <= WAVE_MAX]
    large = [s for s in pairs if s[0] * s[1] > WAVE_MAX]
    out = []
    for i in range(n):
        pool = small if i % 2 == 0 else large
        out.append(pool[(i // 2) % len(pool)] + ((i // 2) % 2,))
    return out


# ---- the golden file ------------------------------------------------------------------------------------------------------------------------------
GOLDEN_FLAGS = ("fast_me_gen_b_low_delay", "mvd_l1_zero", "affine_type")
GOLDEN_NEED = {("start", 0), ("start", 1), ("start", 2), "six_skipped", "shortcut", "shortcut_refused_six", "mvp_switch_search", "mvp_switch_shortcut",
               "best_ref_nonzero", "bip_ref_nonzero", "valid_l1", "no_valid_l1", "one_cand", "same_cands_first_wins", "flat", "corner_far", "p_slice",
               "shortcut_mixed", ("six", 0), ("six", 1), ("affine_type", 0), ("affine_type", 1)} | {("shape",) + s for s in SHAPES}


def golden_groups(g, bd, pic=(256, 128)):
    """tests/golden/affine_unipred.npz -> [(cfg dict, item indices)] of one bit depth: the items of a group share the slice-level settings"""
    k = "bd%d_" % bd
    out = []
    for gi in range(len(g[k + "g_n_ref"])):
        cfg = cfg_dict(float(g[k + "lambda"]), pic[0], pic[1], bd, n_ref=[int(v) for v in g[k + "g_n_ref"][gi]], ref_plane=g[k + "g_ref_plane"][gi].tolist(),
                       list1_to_list0=[int(v) for v in g[k + "g_list1_to_list0"][gi]], mvp_idx_cost=tuple(int(v) for v in g[k + "mvp_idx_cost"]),
                       **{f: int(v) for f, v in zip(GOLDEN_FLAGS, g[k + "g_flags"][gi])})
        out.append((cfg, np.nonzero(g[k + "group"] == gi)[0]))
    return out


def golden_facts(org, cfg, it, res, facts):
    """what an item of the golden set covers, beyond the facts its search reported"""
    w, h, px, py = int(it["w"]), int(it["h"]), int(it["pos_x"]), int(it["pos_y"])
    out = {("shape", w, h), ("six", int(it["six_param"])), ("affine_type", cfg["affine_type"])}
    if not cfg["n_ref"][1]:
        out.add("p_slice")
    if {"shortcut", "searched_l1"} <= facts:
        out.add("shortcut_mixed")
    blk = org[py:py + h, px:px + w]
    if blk.min() == blk.max() and (res["s"]["steps"][res["s"]["searched"] == 1] == 1).all():
        out.add("flat")                                           # a singular system: every search stops on the zero deltas of its first solve
    if px in (0, cfg["pic_w"] - w) and py in (0, cfg["pic_h"] - h):
        for l in range(2):
            for r in range(cfg["n_ref"][l]):
                v = it["ref"][l][r]["mv_cand"][0][0]
                if abs(int(v[0])) > (cfg["max_cu"] + 8) * 16 or abs(int(v[1])) > (cfg["max_cu"] + 8) * 16:
                    out.add("corner_far")
    return out
