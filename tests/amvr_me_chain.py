"""The uni-predictive stage of an AMVR pass (cu.imv = 1, 2) as a caller has to build it without cfg.imv of vvcgpu_unipred_me_batch: one
vvcgpu_mc_dist_batch for the template costs of every candidate -> download, predictor choice on the host -> per (list, reference index) and owner
kind (a wavefront or a workgroup per PU) one vvcgpu_tz_search_batch with imv_shift -> download -> per (list, reference index) one
vvcgpu_imv_refine_batch -> download, the list-1 shortcut and keep-if-better on the host.  Used by the consistency test of
tests/test_gpu_amvr_me.py and by tools/amvr_me_time.py.  Host decisions are vectorised numpy."""
import time

import numpy as np
import torch

import unipred_me_chain
from pu_search_kit import eg_bits
from vvcsoftware_vtm_amd import abi, ops

U64 = np.uint64
MAXU = U64(0xFFFFFFFFFFFFFFFF)


class Chain(unipred_me_chain.Chain):
    def __init__(self, org_dev, planes_dev, cfg, items, margin, imv):
        super().__init__(org_dev, planes_dev, cfg, items, margin)
        self.sh = imv << 1

    def run(self):
        """-> UNIPRED_ME_RESULT records"""
        it, c, m, n, sh = self.items, self.c, self.m, self.n, self.sh
        ar = np.arange(n)
        mic = np.array(c["mvp_idx_cost"], np.int64)
        sad = self.template_costs()
        t0 = time.perf_counter()
        res = np.zeros(n, abi.UNIPRED_ME_RESULT)
        st = {}
        for s, (l, r) in enumerate(self.searches):
            nc = it["ref"]["num_cand"][:, l, r].astype(np.int64)
            tmpl = sad[:, s] + self.get_cost(mic[:2])[None, :]
            tmpl[nc < 2, 1] = 0
            idx = ((nc > 1) & (tmpl[:, 0] > tmpl[:, 1])).astype(np.int64)
            pred = it["ref"]["mv_cand"][ar, l, r, idx].astype(np.int64)
            bits = it["mb_bits"][:, l].astype(np.int64) + (r + 1 - (1 if r == c["n_ref"][l] - 1 else 0) if c["n_ref"][l] > 1 else 0) + mic[idx]
            st[(l, r)] = dict(tmpl=tmpl, amvp=idx.copy(), idx=idx, pred=pred, bits=bits, imv=np.zeros((n, 2), np.int64), mv=np.zeros((n, 2), np.int64),
                              cost=np.zeros(n, U64))
        self.host_s += time.perf_counter() - t0
        e = c["max_cu"] + unipred_me_chain.CLAMP
        oy, ox = np.divmod(it["org_off"].astype(np.int64), it["org_stride"].astype(np.int64))
        tc = np.zeros(1, abi.TZ_CFG)
        tc[0]["lambda"], tc[0]["cost_scale"], tc[0]["imv_shift"], tc[0]["first_search_stop"] = c["lambda_"], 2, sh, c["first_search_stop"]
        tc[0]["pic_w"], tc[0]["pic_h"], tc[0]["max_cu_w"], tc[0]["max_cu_h"] = c["pic_w"], c["pic_h"], c["max_cu"], c["max_cu"]
        tc[0]["ref_x0"], tc[0]["ref_y0"], tc[0]["ref_x1"], tc[0]["ref_y1"] = m - e, m - e, m + c["pic_w"] + e, m + c["pic_h"] + e
        pending = []
        for (l, r) in self.searches:                                  # the searches are independent: all issued before the one download
            if self.shortcut(l, r):
                continue
            a, q = it["ref"][:, l, r], st[(l, r)]
            cached = (a["flags"] & abi.UNIPRED_CACHED) != 0
            pu = np.zeros(n, abi.TZ_PU)
            pu["org_x"], pu["org_y"], pu["ref_x"], pu["ref_y"] = ox, oy, m + it["pos_x"], m + it["pos_y"]
            pu["start_x"] = np.where(cached, a["cached_mv"][:, 0].astype(np.int64) << 2, q["pred"][:, 0])
            pu["start_y"] = np.where(cached, a["cached_mv"][:, 1].astype(np.int64) << 2, q["pred"][:, 1])
            pu["pred2_x"], pu["pred2_y"], pu["pos_x"], pu["pos_y"] = a["pred2"][:, 0], a["pred2"][:, 1], it["pos_x"], it["pos_y"]
            pu["pred_hor"], pu["pred_ver"], pu["w"], pu["h"], pu["sub_shift"] = q["pred"][:, 0], q["pred"][:, 1], it["w"], it["h"], it["sub_shift"]
            pu["flags"] = np.where(cached, abi.TZ_FAST, (it["tz_flags"] & abi.TZ_EXTENDED) | np.where(a["flags"] & abi.UNIPRED_PRED2, abi.TZ_PRED2, 0))
            tcs = tc.copy()
            tcs[0]["search_range"] = c["search_range"][l][r]
            for big in (False, True):                                 # one wavefront per PU up to 1024 samples, one workgroup above
                sel = np.nonzero((it["w"].astype(np.int64) * it["h"] > 1024) == big)[0]
                if len(sel) == 0:
                    continue
                tcs[0]["wg_per_pu"] = int(big)
                d_pu = ops.struct_to_device(pu[sel])
                t0 = time.perf_counter()
                best = ops.tz_search_batch(self.org, self.planes[c["ref_plane"][l][r]], d_pu, len(sel), tcs)
                self.device_s += time.perf_counter() - t0
                self.launches += 1
                pending.append((l, r, sel, best))
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        got = {}
        for l, r, sel, best in pending:
            got.setdefault((l, r), np.zeros(n, abi.SEARCH_BEST))[sel] = best.cpu().numpy().view(abi.SEARCH_BEST)
        self.device_s += time.perf_counter() - t0
        pending = []
        for (l, r), best in got.items():                              # xPatternSearchIntRefine around the integer vectors
            a, q = it["ref"][:, l, r], st[(l, r)]
            q["imv"][:, 0], q["imv"][:, 1] = best["x"], best["y"]
            pu = np.zeros(n, abi.IMV_PU)
            pu["org_x"], pu["org_y"], pu["ref_x"], pu["ref_y"], pu["mv_x"], pu["mv_y"] = ox, oy, m + it["pos_x"], m + it["pos_y"], best["x"], best["y"]
            pu["cand_x"], pu["cand_y"] = a["mv_cand"][:, :, 0], a["mv_cand"][:, :, 1]
            pu["pos_x"], pu["pos_y"], pu["idx_cost"], pu["bits"] = it["pos_x"], it["pos_y"], mic[:2][None, :], q["bits"]
            pu["w"], pu["h"], pu["num_cand"], pu["mvp_idx"] = it["w"], it["h"], a["num_cand"], q["idx"]
            tcs = tc.copy()
            tcs[0]["ref_x0"], tcs[0]["ref_y0"], tcs[0]["ref_x1"], tcs[0]["ref_y1"] = 0, 0, self.rs, self.planes.shape[1]
            d_pu = ops.struct_to_device(pu)
            t0 = time.perf_counter()
            out = ops.imv_refine_batch(self.org, self.planes[c["ref_plane"][l][r]], d_pu, n, tcs, bool(c["use_hadamard"]), 1.0)
            self.device_s += time.perf_counter() - t0
            self.launches += 1
            pending.append((l, r, out))
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        got = [(l, r, out.cpu().numpy().view(abi.IMV_RESULT)) for l, r, out in pending]
        self.device_s += time.perf_counter() - t0
        t0 = time.perf_counter()
        for l, r, out in got:
            q = st[(l, r)]
            q["mv"][:, 0], q["mv"][:, 1], q["idx"], q["bits"], q["cost"] = out["mv_x"], out["mv_y"], out["mvp_idx"].astype(np.int64), out["bits"].astype(np.int64), out["cost"]
        ui_cost, ui_bits = np.full((n, 2), MAXU), np.zeros((n, 2), np.int64)
        ref_idx, c_mv = np.zeros((n, 2), np.int64), np.zeros((n, 2, 2), np.int64)
        bip_dist, bip_mvp, bip_ref = np.full(n, MAXU), np.zeros(n, np.int64), np.zeros(n, np.int64)
        v_cost, v_bits, v_mv, v_ref = np.full(n, MAXU), np.full(n, 0xFFFFFFFF, np.int64), np.zeros((n, 2), np.int64), np.zeros(n, np.int64)
        for (l, r) in self.searches:
            q = st[(l, r)]
            if c["mvd_l1_zero"] and l == 1:
                d = q["tmpl"][ar, q["amvp"]]
                better = d < bip_dist
                bip_dist, bip_mvp, bip_ref = np.where(better, d, bip_dist), np.where(better, q["amvp"], bip_mvp), np.where(better, r, bip_ref)
            if self.shortcut(l, r):                                   # :905-922 with imvShift; xCheckBestMVP returns at once
                z = st[(0, c["list1_to_list0"][r])]
                q["mv"] = z["mv"].copy()
                cost = z["cost"] - self.get_cost(z["bits"])
                q["bits"] = q["bits"] + eg_bits((q["mv"][:, 0] - q["pred"][:, 0]) >> sh) + eg_bits((q["mv"][:, 1] - q["pred"][:, 1]) >> sh)
                q["cost"] = cost + self.get_cost(q["bits"])
            rs = res["s"][:, l, r]
            rs["mv"], rs["int_mv"], rs["mvp_idx"], rs["bits"], rs["cost"], rs["tmpl_cost"] = q["mv"], q["imv"], q["idx"], q["bits"], q["cost"], q["tmpl"]
            better = q["cost"] < ui_cost[:, l]
            ui_cost[:, l], ui_bits[:, l], ref_idx[:, l] = np.where(better, q["cost"], ui_cost[:, l]), np.where(better, q["bits"], ui_bits[:, l]), np.where(better, r, ref_idx[:, l])
            c_mv[:, l] = np.where(better[:, None], q["mv"], c_mv[:, l])
            if l == 1 and c["list1_to_list0"][r] < 0:
                better = q["cost"] < v_cost
                v_cost, v_bits, v_ref = np.where(better, q["cost"], v_cost), np.where(better, q["bits"], v_bits), np.where(better, r, v_ref)
                v_mv = np.where(better[:, None], q["mv"], v_mv)
        res["ref_idx"], res["mv"], res["cost"], res["bits"] = ref_idx, c_mv, ui_cost, ui_bits
        res["best_bip_ref_idx_l1"], res["best_bip_mvp_l1"], res["best_bip_dist"] = bip_ref, bip_mvp, bip_dist
        res["valid_l1_ref_idx"], res["valid_l1_mv"], res["valid_l1_bits"], res["valid_l1_cost"] = v_ref, v_mv, v_bits, v_cost
        self.host_s += time.perf_counter() - t0
        return res


def chained(org_dev, planes_dev, cfg, items, margin, imv):
    """-> (UNIPRED_ME_RESULT records, entry calls made)"""
    ch = Chain(org_dev, planes_dev, cfg, items, margin, imv)
    res = ch.run()
    return res, ch.launches
