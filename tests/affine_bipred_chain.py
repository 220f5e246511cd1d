"""The affine bi-predictive search as a caller had to build it before vvcgpu_affine_bipred_me_batch existed: per iteration vvcgpu_affine_pred_batch
(the other list's prediction, one call per reference plane) -> vvcgpu_pelop_batch op 4 (search key) -> per reference index vvcgpu_affine_me_batch with
half_weight (one call per reference plane) -> synchronise, download -> xCheckBestAffineMVP and keep-if-better on the host -> upload.  Used by the
consistency test of tests/test_gpu_affine_bipred.py and by tools/affine_bipred_time.py.  Serves lists whose items share n_ref, without
pick_list_by_cost and mvd_l1_zero.  Host decisions are vectorised numpy."""
import numpy as np
import torch

from pu_search_kit import U64_MAX, get_cost, vec_bits
from vvcsoftware_vtm_amd import abi, ops

U32 = 0xFFFFFFFF


class Chain:
    def __init__(self, org_dev, planes_dev, cfg, items, margin):
        self.org, self.planes, self.c, self.items, self.m = org_dev, planes_dev, cfg, items, margin
        n = len(items)
        assert not cfg["pick_list_by_cost"] and not cfg["mvd_l1_zero"]
        self.n_ref = [int(items["n_ref"][0, l]) for l in range(2)]
        assert (items["n_ref"] == items["n_ref"][0]).all()
        sz = items["w"].astype(np.int64) * items["h"]
        self.off = np.concatenate([[0], np.cumsum(sz)[:-1]])                 # per item a w x h block for the prediction and one for the key
        self.first = np.concatenate([[0], np.cumsum(sz >> 4)[:-1]])
        self.pred_buf = torch.empty(int(sz.sum()), dtype=torch.int16, device=org_dev.device)
        self.key_buf = torch.empty(int(sz.sum()), dtype=torch.int16, device=org_dev.device)
        self.rs = planes_dev.shape[2]
        self.mecfg = ops.affine_me_cfg(cfg["lambda_"], cfg["pic_w"], cfg["pic_h"], (margin, margin), self.rs, cfg["bit_depth"], (cfg["clp_min"], cfg["clp_max"]),
                                       cfg["affine_type"], cfg["max_cu"])
        self.nmv = np.where(items["six_param"] != 0, 3, 2)
        self.launches = 0
        self.n = n

    def pus(self, idx, mv):
        it = self.items[idx]
        pu = np.zeros(len(idx), abi.AFFINE_PU)
        pu["pos_x"], pu["pos_y"], pu["w"], pu["h"], pu["six_param"] = it["pos_x"], it["pos_y"], it["w"], it["h"], it["six_param"]
        pu["mv"][:, 0] = mv
        return pu

    def make_key(self, idx, plane, mv):
        """other prediction and key of the items idx"""
        it, c, m = self.items[idx], self.c, self.m
        for pl in np.unique(plane):
            g = np.nonzero(plane == pl)[0]
            pu = self.pus(idx[g], mv[g])
            nsb = (it["w"][g].astype(np.int64) * it["h"][g]) >> 4
            pu["dst_off"], pu["dst_stride"], pu["first_desc"] = self.off[idx[g]], it["w"][g], np.concatenate([[0], np.cumsum(nsb)[:-1]])
            ops.affine_pred_batch(self.planes[int(pl)], None, self.pred_buf, ops.struct_to_device(pu), len(g), int(nsb.sum()), 0, c["pic_w"], c["pic_h"], (m, m),
                                  self.rs, self.rs, c["bit_depth"], (c["clp_min"], c["clp_max"]), c["max_cu"])
            self.launches += 1
        e = np.zeros(len(idx), abi.PELOP_DESC)
        e["src0_off"], e["src0_stride"], e["src1_off"], e["src1_stride"] = it["org_off"], it["org_stride"], self.off[idx], it["w"]
        e["dst_off"], e["dst_stride"], e["w"], e["h"] = self.off[idx], it["w"], it["w"], it["h"]
        ops.pelop_batch(4, self.org, self.pred_buf, self.key_buf, ops.struct_to_device(e), len(idx), abi.PelopCfg(0, 0, 0, c["clip_key"], c["clp_min"], c["clp_max"]))
        self.launches += 1

    def motion_estimation(self, idx, plane, start, pred, bits):
        """xAffineMotionEstimation(bBi) of the items idx (their keys are current) -> (mv, bits, cost)"""
        out = np.zeros(len(idx), abi.AFFINE_ME_RESULT)
        pending = []
        for pl in np.unique(plane):
            g = np.nonzero(plane == pl)[0]
            me = np.zeros(len(g), abi.AFFINE_ME_ITEM)
            me["pu"] = self.pus(idx[g], start[g])
            me["org_off"], me["org_stride"], me["half_weight"], me["mvp"], me["bits"] = self.off[idx[g]], self.items["w"][idx[g]], 1, pred[g], bits[g]
            r, _ = ops.affine_me_batch(self.key_buf, self.planes[int(pl)], ops.struct_to_device(me), len(g), self.mecfg, want_trace=False)
            self.launches += 1
            pending.append((g, r))
        for g, r in pending:                                                 # synchronise and download
            out[g] = r.cpu().numpy().view(abi.AFFINE_ME_RESULT)
        return out["mv"].astype(np.int64), out["bits"].astype(np.int64), out["cost"].copy()

    def check_best_mvp(self, idx, cands, num_cand, mv, pred, mvp_idx, bits, cost):
        """xCheckBestAffineMVP, vectorised: -> (pred, mvp_idx, bits, cost)"""
        c = self.c
        mic = np.asarray(c["mvp_idx_cost"], np.int64)
        nmv = self.nmv[idx]
        ar = np.arange(len(idx))
        org_bits = vec_bits(pred, nmv, mv) + mic[mvp_idx]
        oth = 1 - mvp_idx
        oth_bits = vec_bits(cands[ar, oth], nmv, mv) + mic[oth]
        sw = (num_cand >= 2) & (oth_bits < org_bits)
        nb = (bits - org_bits + oth_bits) & U32
        ncost = (cost - get_cost(c["lambda_"], bits)) + get_cost(c["lambda_"], nb)
        return (np.where(sw[:, None, None], cands[ar, oth], pred), np.where(sw, oth, mvp_idx), np.where(sw, nb, bits), np.where(sw, ncost, cost))

    def run(self):
        it, c, n = self.items, self.c, self.n
        rec = it["ref"]
        mv_temp = rec["mv"].astype(np.int64)                                   # [n][2][4][3][2]
        cands = rec["mv_cand"].astype(np.int64)                                # [n][2][4][2][3][2]
        num_cand = rec["num_cand"].astype(np.int64)
        mvp_idx = rec["mvp_idx"].astype(np.int64) & 1
        ar = np.arange(n)
        mv_pred = np.stack([np.stack([cands[ar, l, r, mvp_idx[:, l, r]] for r in range(4)], axis=1) for l in range(2)], axis=1)
        planes = rec["plane"].astype(np.int64)
        mv_bi, ref_bi = it["mv"].astype(np.int64), it["ref_idx"].astype(np.int64)
        only = np.where((it["six_param"] != 0)[:, None], it["only_ref"], -1).astype(np.int64)
        uni = it["cost"]
        mb = it["mb_bits"].astype(np.int64)
        mot = (it["bits"].astype(np.int64) - mb[:, :2]) & U32
        bits2 = (mb[:, 2] + mot[:, 0] + mot[:, 1]) & U32
        cost_bi = np.full(n, U64_MAX, np.uint64)
        calls, closing = np.zeros(n, np.int64), np.zeros(n, np.int64)
        active = ar
        for it_no in range(c["num_iter"]):
            lst = it_no % 2
            oth = 1 - lst
            self.make_key(active, planes[active, oth, ref_bi[active, oth]], mv_bi[active, oth, :])
            changed = np.zeros(n, bool)
            for r in range(self.n_ref[lst]):
                a = active[(only[active, lst] < 0) | (only[active, lst] == r)]
                if len(a) == 0:
                    continue
                rb = (r + 1 - (1 if r == self.n_ref[lst] - 1 else 0)) if self.n_ref[lst] > 1 else 0
                bits_t = (mb[a, 2] + mot[a, oth] + rb + np.asarray(c["mvp_idx_cost"], np.int64)[mvp_idx[a, lst, r]]) & U32
                mv, bits_t, cost_t = self.motion_estimation(a, planes[a, lst, r], mv_temp[a, lst, r], mv_pred[a, lst, r], bits_t)
                mv_temp[a, lst, r] = mv
                mv_pred[a, lst, r], mvp_idx[a, lst, r], bits_t, cost_t = self.check_best_mvp(a, cands[a, lst, r], num_cand[a, lst, r], mv, mv_pred[a, lst, r],
                                                                                             mvp_idx[a, lst, r], bits_t, cost_t)
                calls[a] += 1
                acc = cost_t < cost_bi[a]
                b = a[acc]
                changed[b] = True
                mv_bi[b, lst], ref_bi[b, lst], cost_bi[b] = mv[acc], r, cost_t[acc]
                mot[b, lst] = (bits_t[acc] - mb[b, 2] - mot[b, oth]) & U32
                bits2[b] = bits_t[acc]
            stop = active[~changed[active]]
            s = stop[(cost_bi[stop] <= uni[stop, 0]) & (cost_bi[stop] <= uni[stop, 1])]
            closing[s] = 1
            for l in range(2):
                r = ref_bi[s, l]
                mv_pred[s, l, r], mvp_idx[s, l, r], bits2[s], cost_bi[s] = self.check_best_mvp(s, cands[s, l, r], num_cand[s, l, r], mv_bi[s, l], mv_pred[s, l, r],
                                                                                               mvp_idx[s, l, r], bits2[s], cost_bi[s])
            active = active[changed[active]]
            if len(active) == 0:
                break
        res = np.zeros(n, abi.AFFINE_BIPRED_RESULT)
        res["mv"], res["ref_idx"], res["bits"], res["mot_bits"], res["me_calls"], res["closing"], res["cost"] = mv_bi, ref_bi, bits2, mot, calls, closing, cost_bi
        for l in range(2):
            res["mvp_idx"][:, l], res["mvp"][:, l] = mvp_idx[ar, l, ref_bi[:, l]], mv_pred[ar, l, ref_bi[:, l]]
        return res


def chained(org_dev, planes_dev, cfg, items, margin):
    """-> (AFFINE_BIPRED_RESULT records, launches made)"""
    ch = Chain(org_dev, planes_dev, cfg, items, margin)
    res = ch.run()
    torch.cuda.synchronize()
    return res, ch.launches
