"""The merge candidate pass (EncCu::xCheckRDCostMerge2Nx2N, first pass, EncCu.cpp:1537-1612) restated for the tests of vvcgpu_merge_cand_batch: the pixel
steps go through the CPU restatement (orc_mc_batch for motionCompensation / xSubPuMC, orc_satd / orc_sad for the distFunc, orc_sse for the DF_SSE of the
no-residual leg); updateCandList (UnitTools.h:190-223), the candidate bits, the cost and the MRG_FAST_RATIO cut are written here from the reference's text.
Also the case builders: a 4:2:0 frame of four reference pictures whose three planes each sit in ONE allocation, and the helper that turns a PU's
candidates -- per list (picture, vector in quarter or 1/16 units), or a sub-block motion field -- into descriptor runs (it does clipMv and
xCheckIdenticalMotion, which are the caller's in the entry's contract).  numpy only: the generator and the CPU tests load this file without torch."""
import os

import numpy as np

import pu_search_kit as kit
from oraclelib import oracle, p
from vvcsoftware_vtm_amd import abi

W, H = 256, 128
N_PICS = 4
MAX_CU = 128
MRG_MAX_NUM_CANDS, NUM_MRG_SATD_CAND, MRG_FAST_RATIO = 7, 4, 1.25
GUARD = -5                          # what the tests paint pred_base with
GAP = 8                             # samples between two blocks of pred_base
FLAT = (192, 64, 64, 64)            # x, y, w, h of the flat patch of the original (luma)
SIDES = (4, 8, 16, 32, 64, 128)
U64_MAX = kit.U64_MAX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_cand.npz")


def all_shapes():
    return [(w, h) for w in SIDES for h in SIDES]


# ---- the frame -----------------------------------------------------------------------------------------------------------------------------------
class Frame:
    """luma [pictures][h][w], chroma [pictures][2][h/2][w/2], the original's three planes -> refs: one int16 allocation of the padded planes
    (plane_off[pic][comp], stride[comp], margin[comp]); org: one allocation of the original's planes (org_off[comp], org_stride[comp])"""
    def __init__(self, luma, chroma, org_y, org_c, bd):
        self.bd, self.luma, self.chroma, self.org_y, self.org_c = bd, luma, chroma, org_y, org_c
        self.h, self.w = h, w = luma.shape[1], luma.shape[2]
        self.margin = (kit.MARGIN, kit.MARGIN // 2, kit.MARGIN // 2)
        parts, self.plane_off, pos = [], [], 0
        for k in range(len(luma)):
            offs = []
            for comp in range(3):
                pl = kit.pad(luma[k] if comp == 0 else chroma[k][comp - 1], self.margin[comp])
                offs.append(pos)
                parts.append(pl.reshape(-1))
                pos += pl.size
            self.plane_off.append(offs)
        self.stride = (w + 2 * self.margin[0], w // 2 + 2 * self.margin[1], w // 2 + 2 * self.margin[2])
        self.refs = np.ascontiguousarray(np.concatenate(parts))
        self.org = np.ascontiguousarray(np.concatenate([org_y.reshape(-1), org_c[0].reshape(-1), org_c[1].reshape(-1)]))
        self.org_off = (0, w * h, w * h + (w // 2) * (h // 2))
        self.org_stride = (w, w // 2, w // 2)


def derived_frame(l0, l1, org_y, bd):
    """the frame of two luma planes and a luma original: pictures 2, 3 are shifted copies of 0, 1, every chroma plane is a sub-sampling of its luma
    plane (so that a golden file stores three planes only)"""
    luma = np.stack([l0, l1, np.roll(l0, (5, -7), axis=(0, 1)), np.roll(l1, (-3, 11), axis=(0, 1))])
    chroma = np.stack([np.stack([y[0::2, 0::2], y[1::2, 1::2]]) for y in luma])
    return Frame(luma, chroma, org_y, np.stack([org_y[0::2, 0::2], org_y[1::2, 1::2]]), bd)


def fresh_planes(rng, bd):
    """-> (l0, l1, org_y) for derived_frame: two textures and an original that is a shifted copy of the first plus noise, flat inside FLAT"""
    mx = (1 << bd) - 1
    l0, l1 = kit.texture(rng, H, W, bd, 0.0), kit.texture(rng, H, W, bd, 1.5)
    org = np.clip(np.roll(l0, (2, -3), axis=(0, 1)).astype(np.int32) + rng.integers(-5, 6, (H, W)), 0, mx).astype(np.int16)
    fx, fy, fw, fh = FLAT
    org[fy:fy + fh, fx:fx + fw] = mx // 3 + 7
    return l0, l1, np.ascontiguousarray(org)


# ---- candidates -> descriptor runs ---------------------------------------------------------------------------------------------------------------
def default_cand(l0, l1, prec=2):
    """a MRG_TYPE_DEFAULT_N candidate: l0 / l1 = (picture, mv_x, mv_y) or None; prec 2: quarter-sample vectors, 4: 1/16 (high precision)"""
    return ("default", l0, l1, prec)


def atmvp_cand(sub, field, prec=2):
    """a MRG_TYPE_SUBPU_ATMVP candidate: sub = 1 << getSubPuMvpSubblkLog2Size() (4 or 8), field[j][i] = (l0, l1) of the sub-block at (i, j)"""
    return ("atmvp", sub, field, prec)


def _block_desc(fr, comp, bx, by, bw, bh, l0, l1, prec, cu_pos, dst_off, dst_stride):
    """xPredInterUni / xPredInterBi of one block: clipMv against the CU's position (Mv.cpp:64-80), then xPredInterBlk's split of the vector (:497-526)"""
    s = 1 if comp else 0
    if l0 is not None and l1 is not None and tuple(l0) == tuple(l1):       # xCheckIdenticalMotion: uni-prediction from list 0
        l1 = None
    refs = [v for v in (l0, l1) if v is not None]
    e = np.zeros((), abi.MC_DESC)
    for r, (pic, mx, my) in enumerate(refs):
        mx, my = kit.clip_mv(int(mx), cu_pos[0], fr.w, MAX_CU, prec), kit.clip_mv(int(my), cu_pos[1], fr.h, MAX_CU, prec)
        sh = prec + s
        m = fr.margin[comp]
        e["ref%d_off" % r] = fr.plane_off[pic][comp] + (m + (by >> s) + (my >> sh)) * fr.stride[comp] + m + (bx >> s) + (mx >> sh)
        e["ref%d_stride" % r] = fr.stride[comp]
        e["frac_x%d" % r], e["frac_y%d" % r] = (mx & ((1 << sh) - 1)) << (4 - prec), (my & ((1 << sh) - 1)) << (4 - prec)
    e["dst_off"], e["dst_stride"], e["w"], e["h"] = dst_off, dst_stride, bw >> s, bh >> s
    e["is_luma"], e["bi"], e["reserved"] = 0 if comp else 1, 1 if len(refs) == 2 else 0, comp
    return e


def cand_descs(fr, px, py, w, h, cand, cur_off, cur_stride, n_comp):
    """the descriptor run of one candidate of the PU (px, py, w, h); cur_off / cur_stride [comp]: its blocks in pred_base"""
    out = []
    if cand[0] == "default":
        _, l0, l1, prec = cand
        for comp in range(n_comp):
            out.append(_block_desc(fr, comp, px, py, w, h, l0, l1, prec, (px, py), cur_off[comp], cur_stride[comp]))
        return out
    _, sub, field, prec = cand
    sw, sh = min(sub, w), min(sub, h)                                      # (xSubPuMC :283-286: a side below the sub-block size is one part)
    for j in range(max(h // sub, 1)):
        for i in range(max(w // sub, 1)):
            l0, l1 = field[j][i]
            for comp in range(n_comp):
                s = 1 if comp else 0
                off = cur_off[comp] + ((j * sh) >> s) * cur_stride[comp] + ((i * sw) >> s)
                out.append(_block_desc(fr, comp, px + i * sw, py + j * sh, sw, sh, l0, l1, prec, (px, py), off, cur_stride[comp]))
    return out


def layout(fr, pus, n_comp=3, pad_of=lambda c: (0, 2, 6)[c % 3]):
    """pus: [(px, py, w, h, [candidates])] -> the entry's arrays.  pred_base holds, candidate after candidate, the blocks of its components with
    GAP samples between two blocks and a row pitch of the block's width + pad_of(candidate)"""
    mc, cand_mc_first, cand_dist, pu_cand_first, pos = [], [0], [], [0], GAP
    for (px, py, w, h, cands) in pus:
        for cand in cands:
            c = len(cand_mc_first) - 1
            cur_off, cur_stride = [], []
            for comp in range(n_comp):
                s = 1 if comp else 0
                cs = (w >> s) + pad_of(c)
                cur_off.append(pos)
                cur_stride.append(cs)
                pos += (h >> s) * cs + GAP
                d = np.zeros((), abi.DIST_DESC)
                d["org_off"] = fr.org_off[comp] + (py >> s) * fr.org_stride[comp] + (px >> s)
                d["cur_off"], d["org_stride"], d["cur_stride"], d["w"], d["h"] = cur_off[comp], fr.org_stride[comp], cs, w >> s, h >> s
                cand_dist.append(d)
            mc += cand_descs(fr, px, py, w, h, cand, cur_off, cur_stride, n_comp)
            cand_mc_first.append(len(mc))
        pu_cand_first.append(len(cand_mc_first) - 1)
    return dict(mc=np.array(mc, dtype=abi.MC_DESC), cand_mc_first=np.array(cand_mc_first, np.int32), cand_dist=np.array(cand_dist, dtype=abi.DIST_DESC),
                pu_cand_first=np.array(pu_cand_first, np.int32), pred_size=pos, n_comp=n_comp)


def gather_blocks(pred, L):
    """the samples of every block of pred_base (candidate after candidate, component after component, rows without their pitch padding)"""
    out = []
    for d in L["cand_dist"]:
        rows = int(d["cur_off"]) + np.arange(int(d["h"]))[:, None] * int(d["cur_stride"]) + np.arange(int(d["w"]))[None, :]
        out.append(pred[rows].reshape(-1))
    return np.concatenate(out)


def _ref_ints(v):
    return [0, 0, 0, 0] if v is None else [1, int(v[0]), int(v[1]), int(v[2])]


def pus_to_arrays(pus):
    """a PU list as three int32 arrays (what a golden file stores): pu [n][5] = px, py, w, h, candidates; cand [n][11] = type (0 default, 1 ATMVP),
    prec, sub, then l0 and l1 as (present, picture, mv_x, mv_y) -- for ATMVP: the first row of its field in `field` [m][8], row-major"""
    pu, cand, field = [], [], []
    for (px, py, w, h, cands) in pus:
        pu.append([px, py, w, h, len(cands)])
        for c in cands:
            if c[0] == "default":
                cand.append([0, c[3], 0] + _ref_ints(c[1]) + _ref_ints(c[2]))
            else:
                cand.append([1, c[3], c[1], len(field)] + [0] * 7)
                field += [_ref_ints(e[0]) + _ref_ints(e[1]) for row in c[2] for e in row]
    return np.array(pu, np.int32), np.array(cand, np.int32), np.array(field, np.int32).reshape(-1, 8)


def pus_from_arrays(pu, cand, field):
    ref = lambda a: (int(a[1]), int(a[2]), int(a[3])) if a[0] else None
    pus, k = [], 0
    for (px, py, w, h, n) in pu.tolist():
        cands = []
        for c in cand[k:k + n]:
            if c[0] == 0:
                cands.append(default_cand(ref(c[3:7]), ref(c[7:11]), int(c[1])))
            else:
                sub, nx, ny, f = int(c[2]), max(w // int(c[2]), 1), max(h // int(c[2]), 1), int(c[3])
                cands.append(atmvp_cand(sub, [[(ref(field[f + j * nx + i][0:4]), ref(field[f + j * nx + i][4:8])) for i in range(nx)] for j in range(ny)], int(c[1])))
        k += n
        pus.append((px, py, w, h, cands))
    return pus


def golden_case(g, bd):
    """-> (frame, pus, layout, settings dict) of one bit depth of the loaded golden file"""
    k = "bd%d_" % bd
    fr = derived_frame(g[k + "l0"], g[k + "l1"], g[k + "org"], bd)
    pus = pus_from_arrays(g[k + "pu"], g[k + "cand"], g[k + "field"])
    return fr, pus, layout(fr, pus), dict(max_num=int(g[k + "max_num"]), had=int(g[k + "had"]), lam=float(g[k + "sqrt_lambda"]))


# ---- the list logic, from the reference's text ----------------------------------------------------------------------------------------------------
def update_cand_list(mode, cost, mode_list, cost_list, fast_num=NUM_MRG_SATD_CAND):
    """updateCandList (UnitTools.h:190-223)"""
    shift = 0
    cur = min(fast_num, len(cost_list))
    while shift < fast_num and shift < cur and cost < cost_list[cur - 1 - shift]:
        shift += 1
    if len(mode_list) >= fast_num and shift != 0:
        for i in range(1, shift):
            mode_list[cur - i] = mode_list[cur - 1 - i]
            cost_list[cur - i] = cost_list[cur - 1 - i]
        mode_list[cur - shift] = mode
        cost_list[cur - shift] = cost
        return 1
    if cur < fast_num:
        mode_list.insert(len(mode_list) - shift, mode)
        cost_list.insert(len(cost_list) - shift, cost)
        return 1
    return 0


def cand_bits(k, max_num_merge_cand):
    """uiBitsCand (:1594-1598)"""
    return k + 1 - (1 if k == max_num_merge_cand - 1 else 0)


def rd_list(dist, max_num_merge_cand, sqrt_lambda):
    """:1594-1612 of one PU's distortions -> (costs, the row of rd_list_out).  Below four candidates the reference's cut indexes candCostList
    beyond its size: it stops at the list's size here, as the entry does"""
    modes, costs, out = [], [], []
    for k, d in enumerate(dist):
        cost = float(int(d)) + float(cand_bits(k, max_num_merge_cand)) * sqrt_lambda
        out.append(cost)
        update_cand_list(k, cost, modes, costs)
    num = min(NUM_MRG_SATD_CAND, len(modes))
    for i in range(1, num):
        if costs[i] > MRG_FAST_RATIO * costs[0]:
            num = i
            break
    return out, [num] + modes + [-1] * (7 - len(modes))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def restate(fr, L, max_num_merge_cand, use_hadamard, sqrt_lambda, clp=None):
    """the pass over the entry's arrays -> dict(pred, dist [n_cand] u64, sse [n_cand][n_comp] u64, cost [n_cand] f64, rd_list [n_pu][8] i32)"""
    O = oracle()
    for f in ("orc_sad", "orc_satd", "orc_sse"):
        getattr(O, f).restype = np.ctypeslib.ctypes.c_uint64
    clp = clp or (0, (1 << fr.bd) - 1)
    n_comp, n_cand, n_pu = L["n_comp"], len(L["cand_mc_first"]) - 1, len(L["pu_cand_first"]) - 1
    pred = np.full(L["pred_size"], GUARD, np.int16)
    O.orc_mc_batch(p(fr.refs), p(fr.refs), p(pred), p(L["mc"]), len(L["mc"]), fr.bd, clp[0], clp[1])
    at = lambda a, off: np.ctypeslib.ctypes.c_void_p(a.ctypes.data + 2 * int(off))
    dist, sse = np.zeros(n_cand, np.uint64), np.zeros((n_cand, n_comp), np.uint64)
    for c in range(n_cand):
        for comp in range(n_comp):
            d = L["cand_dist"][n_comp * c + comp]
            a = (at(fr.org, d["org_off"]), int(d["org_stride"]), at(pred, d["cur_off"]), int(d["cur_stride"]), int(d["w"]), int(d["h"]))
            sse[c, comp] = O.orc_sse(*a)
            if comp == 0:
                dist[c] = O.orc_satd(*a) if use_hadamard else O.orc_sad(*a, 0)
    cost, rows = np.zeros(n_cand, np.float64), np.zeros((n_pu, 8), np.int32)
    for q in range(n_pu):
        c0, c1 = int(L["pu_cand_first"][q]), int(L["pu_cand_first"][q + 1])
        cost[c0:c1], rows[q] = rd_list(dist[c0:c1], max_num_merge_cand, sqrt_lambda)
    return dict(pred=pred, dist=dist, sse=sse, cost=cost, rd_list=rows)


# ---- seeded PU lists ------------------------------------------------------------------------------------------------------------------------------
def random_ref(rng, prec, far=0):
    """(picture, vector): mostly small vectors with any phase, some full-sample ones; far: +- that many samples, so that clipMv binds"""
    one = 1 << prec
    v = rng.integers(-12 * one, 12 * one + 1, 2)
    if rng.integers(0, 4) == 0:
        v = (v >> prec) << prec
    if far:
        v = v + far * one * rng.choice([-1, 1], 2)
    return (int(rng.integers(0, N_PICS)), int(v[0]), int(v[1]))


def random_lists(rng, prec, far=0):
    kind = int(rng.integers(0, 3))                                        # list 0 only, list 1 only, both
    l0 = random_ref(rng, prec, far) if kind != 1 else None
    l1 = random_ref(rng, prec, far) if kind != 0 else None
    return l0, l1


def random_cand(rng, w, h, far=0, atmvp=None):
    prec = int(rng.choice([2, 4]))
    if atmvp:
        nx, ny = max(w // atmvp, 1), max(h // atmvp, 1)
        base = random_lists(rng, prec)
        field = [[(base if rng.integers(0, 3) else random_lists(rng, prec)) for _ in range(nx)] for _ in range(ny)]
        return atmvp_cand(atmvp, field, prec)
    return default_cand(*random_lists(rng, prec, far), prec)


def place(rng, w, h):
    return int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4


def fresh_pus(rng, n_pu):
    """about n_pu PUs: every one of the 36 side pairs, candidates from either list and both, all phases, ATMVP candidates with sub-blocks of 4 and 8
    on PUs from 8x8 to 64x64 (one side equal to the sub-block size included), PUs at the picture's corners whose vectors clip at each edge"""
    pus = []
    shapes = all_shapes()
    for i in range(n_pu):
        w, h = shapes[i % len(shapes)]
        px, py = place(rng, w, h)
        n = int(rng.integers(1, 8))
        cands = [random_cand(rng, w, h) for _ in range(n)]
        if 8 <= w <= 64 and 8 <= h <= 64 and i % 2 == 0:
            cands[int(rng.integers(0, n))] = random_cand(rng, w, h, atmvp=(4, 8)[(i // 2) % 2])
        pus.append((px, py, w, h, cands))
    for (px, py, w, h) in [(0, 0, 32, 32), (W - 16, H - 16, 16, 16), (0, H - 8, 8, 8), (W - 64, 0, 64, 16), (W - 8, 0, 8, 64), (0, H - 128, 128, 128)]:
        pus.append((px, py, w, h, [random_cand(rng, w, h, far=int(rng.integers(300, 600))) for _ in range(int(rng.integers(4, 8)))]))
    pus.append((64, 32, 8, 8, [random_cand(rng, 8, 8, atmvp=8), random_cand(rng, 8, 8, atmvp=4)]))
    pus.append((96, 32, 8, 16, [random_cand(rng, 8, 16, atmvp=8), random_cand(rng, 8, 16)]))
    return pus
