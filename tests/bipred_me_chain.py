"""The bi-predictive refinement loop as a caller had to build it before vvcgpu_bipred_me_batch existed: per iteration vvcgpu_mc_batch (other
prediction) -> vvcgpu_pelop_batch op 4 (search key) -> per reference index vvcgpu_sad_search (the +-range SAD surface) -> download, vector costs and
arg-min on the host -> vvcgpu_frac_refine -> download, cost and keep-if-better on the host.  Used by the consistency test of
tests/test_gpu_bipred_me.py and by tools/bipred_me_time.py.  The public entries take ONE vector predictor per call, so the chain serves lists whose
items all have a single candidate, the same for every (list, reference) of the list (xCheckBestMVP is then a no-op), the same n_ref, no
pick_list_by_cost and no mvd_l1_zero; calls are grouped by (shape, plane).  Host decisions are vectorised numpy."""
import numpy as np
import torch

import pu_search_kit as kit
from pu_search_kit import U64_MAX, eg_bits
from vvcsoftware_vtm_amd import abi, ops


def get_cost(lam, bits):
    return kit.get_cost(lam, bits).astype(np.int64)                          # this chain keeps its costs signed



class Chain:
    def __init__(self, org_dev, planes_dev, cfg, items, margin):
        self.org, self.planes, self.c, self.items, self.m = org_dev, planes_dev, cfg, items, margin
        n = len(items)
        assert not cfg["pick_list_by_cost"] and not cfg["mvd_l1_zero"]
        self.n_ref = [int(items["n_ref"][0, l]) for l in range(2)]
        assert (items["n_ref"] == items["n_ref"][0]).all() and (items["ref"]["num_cand"][:, :, 0] == 1).all()
        self.pred = [int(v) for v in items["ref"]["mv_cand"][0, 0, 0, 0]]
        for l in range(2):
            assert (items["ref"]["mv_cand"][:, l, :self.n_ref[l], 0] == self.pred).all()
        self.shape_key = items["w"].astype(np.int64) * 1000 + items["h"]
        # one flat work buffer: per item a w x h block for the prediction and one for the key
        sz = items["w"].astype(np.int64) * items["h"]
        order = np.argsort(self.shape_key, kind="stable")                     # the blocks of one shape lie side by side, in item order
        self.off = np.zeros(n, np.int64)
        self.off[order] = np.concatenate([[0], np.cumsum(sz[order])[:-1]])
        self.pred_buf = torch.empty(int(sz.sum()), dtype=torch.int16, device=org_dev.device)
        self.key_buf = torch.empty(int(sz.sum()), dtype=torch.int16, device=org_dev.device)
        self.launches = 0
        self.rs = planes_dev.shape[2]
        self.plane_sz = planes_dev.shape[1] * planes_dev.shape[2]
        self.n = n

    def clip(self, v, pos, pic):
        c = self.c
        return np.minimum((pic + 8 - pos - 1) << 2, np.maximum((-c["max_cu"] - 8 - pos + 1) << 2, v))

    def make_key(self, idx, plane, mv):
        """other prediction and key of the items idx"""
        it, c, m = self.items[idx], self.c, self.m
        px, py = it["pos_x"].astype(np.int64), it["pos_y"].astype(np.int64)
        mx, my = self.clip(mv[:, 0], px, c["pic_w"]), self.clip(mv[:, 1], py, c["pic_h"])
        d = np.zeros(len(idx), abi.MC_DESC)
        d["ref0_off"] = plane * self.plane_sz + (m + py + (my >> 2)) * self.rs + m + px + (mx >> 2)
        d["ref0_stride"], d["dst_off"], d["dst_stride"], d["w"], d["h"] = self.rs, self.off[idx], it["w"], it["w"], it["h"]
        d["frac_x0"], d["frac_y0"], d["is_luma"] = (mx & 3) << 2, (my & 3) << 2, 1
        ops.mc_batch(self.planes, self.planes, self.pred_buf, ops.struct_to_device(d), len(idx), c["bit_depth"], (c["clp_min"], c["clp_max"]))
        e = np.zeros(len(idx), abi.PELOP_DESC)
        e["src0_off"], e["src0_stride"], e["src1_off"], e["src1_stride"] = it["org_off"], it["org_stride"], self.off[idx], it["w"]
        e["dst_off"], e["dst_stride"], e["w"], e["h"] = self.off[idx], it["w"], it["w"], it["h"]
        ops.pelop_batch(4, self.org, self.pred_buf, self.key_buf, ops.struct_to_device(e), len(idx), abi.PelopCfg(0, 0, 0, c["clip_key"], c["clp_min"], c["clp_max"]))
        self.launches += 2

    def motion_estimation(self, idx, plane, entry, bits):
        """xMotionEstimation(bBi) of the items idx (their keys are current) -> (mv, bits, cost)"""
        it, c, m, R = self.items[idx], self.c, self.m, self.c["search_range"]
        px, py = it["pos_x"].astype(np.int64), it["pos_y"].astype(np.int64)
        pos, pic = (px, py), (c["pic_w"], c["pic_h"])
        ctr = [self.clip(entry[:, k], pos[k], pic[k]) for k in range(2)]
        tl = [(self.clip(ctr[k] - (R << 2), pos[k], pic[k]) + 2) >> 2 for k in range(2)]
        br = [(self.clip(ctr[k] + (R << 2), pos[k], pic[k]) + 2) >> 2 for k in range(2)]
        N = 2 * R + 1
        imv = np.zeros((len(idx), 2), np.int64)
        fr = np.zeros(len(idx), abi.FRAC_RESULT)
        mc = abi.MvCost(c["lambda_"], self.pred[0], self.pred[1], 0, 0)
        groups = {}
        for k in np.unique(self.shape_key[idx] * 100 + plane):
            groups[int(k)] = np.nonzero(self.shape_key[idx] * 100 + plane == k)[0]
        pending = []
        for k, g in groups.items():                                           # integer search: the SAD surfaces
            w, h, pl = k // 100000, (k // 100) % 1000, k % 100
            gi = idx[g]
            assert (np.diff(gi) > 0).all()
            lo = int(self.off[gi[0]])
            rows = (self.off[gi] - lo) // w
            key2d = self.key_buf[lo:lo + int(rows[-1] + h) * w].view(-1, w)
            blk = np.zeros(len(g), abi.SEARCH_BLK)
            blk["org_y"], blk["ref_x"], blk["ref_y"] = rows, m + px[g] + tl[0][g], m + py[g] + tl[1][g]
            sad, _ = ops.sad_search(key2d, self.planes[pl], ops.struct_to_device(blk), len(g), w, h, int(it["sub_shift"][g[0]]), 0, 0, N, N, 1, 1)
            self.launches += 1
            pending.append((g, w, h, pl, key2d, rows, sad))
        for g, w, h, pl, key2d, rows, sad in pending:                         # download, vector cost, arg-min in scan order; fractional refinement
            s = sad.cpu().numpy().astype(np.int64)
            x = tl[0][g][:, None, None] + np.arange(N)[None, None, :]
            y = tl[1][g][:, None, None] + np.arange(N)[None, :, None]
            cost = s + get_cost(c["lambda_"], eg_bits((x << 2) - self.pred[0]) + eg_bits((y << 2) - self.pred[1]))
            cost = np.where((x <= br[0][g][:, None, None]) & (y <= br[1][g][:, None, None]), cost, np.int64(1) << 62)
            best = cost.reshape(len(g), -1).argmin(axis=1)
            imv[g, 0], imv[g, 1] = tl[0][g] + best % N, tl[1][g] + best // N
            fb = np.zeros(len(g), abi.FRAC_BLK)
            fb["org_y"], fb["ref_x"], fb["ref_y"], fb["mv_x"], fb["mv_y"] = rows, m + px[g] + imv[g, 0], m + py[g] + imv[g, 1], imv[g, 0], imv[g, 1]
            pending_fr = ops.frac_refine(key2d, self.planes[pl], ops.struct_to_device(fb), len(g), w, h, c["bit_depth"], mc, bool(c["use_hadamard"]), (c["clp_min"], c["clp_max"]))
            self.launches += 1
            fr[g] = pending_fr.cpu().numpy().view(abi.FRAC_RESULT)
        mv = np.stack([(imv[:, 0] << 2) + (fr["half_x"].astype(np.int64) << 1) + fr["qter_x"], (imv[:, 1] << 2) + (fr["half_y"].astype(np.int64) << 1) + fr["qter_y"]], axis=1)
        mv_bits = eg_bits(mv[:, 0] - self.pred[0]) + eg_bits(mv[:, 1] - self.pred[1])
        bits = bits + mv_bits
        cost = np.floor(0.5 * (fr["cost"].astype(np.float64) - get_cost(c["lambda_"], mv_bits).astype(np.float64))) + get_cost(c["lambda_"], bits).astype(np.float64)
        return mv, bits, cost.astype(np.uint64).astype(np.int64)

    def run(self):
        it, c, n = self.items, self.c, self.n
        mv_temp = it["ref"]["mv"].astype(np.int64)                             # [n][2][4][2]
        planes = it["ref"]["plane"].astype(np.int64)
        mv_bi, ref_bi = it["mv"].astype(np.int64), it["ref_idx"].astype(np.int64)
        uni = it["cost"].astype(np.float64)
        mb = it["mb_bits"].astype(np.int64)
        mot = it["bits"].astype(np.int64) - mb[:, :2]
        bits2 = mb[:, 2] + mot[:, 0] + mot[:, 1]
        cost_bi = np.full(n, float(U64_MAX))
        calls, closing = np.zeros(n, np.int64), np.zeros(n, np.int64)
        active = np.arange(n)
        for it_no in range(c["num_iter"]):
            lst = it_no % 2
            oth = 1 - lst
            self.make_key(active, planes[active, oth, ref_bi[active, oth]], mv_bi[active, oth])
            changed = np.zeros(n, bool)
            for r in range(self.n_ref[lst]):
                rb = (r + 1 - (1 if r == self.n_ref[lst] - 1 else 0)) if self.n_ref[lst] > 1 else 0
                bits_t = mb[active, 2] + mot[active, oth] + rb + c["mvp_idx_cost"][0]
                mv, bits_t, cost_t = self.motion_estimation(active, planes[active, lst, r], mv_temp[active, lst, r], bits_t)
                mv_temp[active, lst, r] = mv
                calls[active] += 1
                acc = cost_t.astype(np.float64) < cost_bi[active]
                a = active[acc]
                changed[a] = True
                mv_bi[a, lst], ref_bi[a, lst], cost_bi[a] = mv[acc], r, cost_t[acc].astype(np.float64)
                mot[a, lst] = bits_t[acc] - mb[a, 2] - mot[a, oth]
                bits2[a] = bits_t[acc]
            stop = active[~changed[active]]
            closing[stop] = (cost_bi[stop] <= uni[stop, 0]) & (cost_bi[stop] <= uni[stop, 1])
            active = active[changed[active]]
            if len(active) == 0:
                break
        res = np.zeros(n, abi.BIPRED_ME_RESULT)
        res["mv"], res["ref_idx"], res["bits"], res["mot_bits"], res["me_calls"], res["closing"] = mv_bi, ref_bi, bits2, mot, calls, closing
        res["mvp"][:] = self.pred
        res["cost"] = cost_bi.astype(np.uint64)
        return res


def chained(org_dev, planes_dev, cfg, items, margin):
    """-> (BIPRED_ME_RESULT records, launches made)"""
    ch = Chain(org_dev, planes_dev, cfg, items, margin)
    res = ch.run()
    torch.cuda.synchronize()
    return res, ch.launches
