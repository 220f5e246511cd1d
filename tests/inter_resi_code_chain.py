"""The inter residual pixel pass as a caller had to build it before vvcgpu_inter_resi_code_batch existed, from entries whose code the new entry does not
alter: vvcgpu_pelop_batch (subtract) -> vvcgpu_tr_fwd_batch -> vvcgpu_quant_batch -> vvcgpu_dequant_tr_inv_batch -> vvcgpu_dist_batch kind 2 twice
(orgResi against resi', orgResi against a zero block) -> vvcgpu_pelop_batch (reconstruct) -> vvcgpu_dist_batch kind 2 (org against rec): eight launches, the
residual, the coefficients and the de-quantised residual through device memory between them.  Served for items with a given prediction (no list items) and
slots the entry serves.  Used by the consistency test of tests/test_gpu_inter_resi_code.py and by tools/inter_resi_code_time.py; Device.run_entry is the one
call of the entry both use.  Device also carries what the tests of the entry and of its DepQuant sibling (tests/inter_resi_dq_chain.py subclasses it) do
alike: run / collect, the hand-over from vvcgpu_merge_cand_batch and the stored-zeros check."""
import numpy as np
import torch

import inter_resi_code_cases as irc
import merge_cand_chain
import rd_pass_kit as kit
from rd_pass_kit import dev
from vvcsoftware_vtm_amd import abi, ops

KEYS = ("abs_sum", "zero_dist", "dist_resi", "dist_rec", "level", "resi", "rec")          # of kit.same: whole buffers, the canaries are part of the comparison
FILLS = (irc.RESI_CANARY, irc.REC_CANARY, irc.LEVEL_CANARY)


class Device:
    """the buffers and item records of a case (org, pred: flat int16 arrays; items: abi.INTER_RESI_ITEM) on the device, uploaded once"""
    def __init__(self, bd, org, pred, items, cand_size, level_size, fills=(0, 0, 0)):
        self.bd, self.items, self.n = bd, items, len(items)
        self.org, self.pred, self.items_dev = dev(org), dev(pred), ops.struct_to_device(items)
        self.cand_size, self.level_size, self.fills = int(cand_size), int(level_size), fills

    @staticmethod
    def collect(resi, rec, level, outs):
        """the three buffers and the entry's four outputs -> the dict the restatement returns"""
        return kit.download((resi, rec, level) + tuple(outs), ("resi", "rec", "level", "abs_sum", "dist_resi", "dist_rec", "zero_dist"))

    def run(self, flags=0, rd_list=None, with_rec=None):
        """the entry on fresh buffers -> the dict the restatement returns (rec_base is NULL without WRITE_REC unless with_rec)"""
        resi, rec, level = self.fresh()
        give_rec = bool(flags & irc.WRITE_REC) if with_rec is None else with_rec
        return self.collect(resi, rec, level, self.run_entry(resi, rec if give_rec else None, level, flags, rd_list))

    def handover(self, M, pred_len):
        """vvcgpu_merge_cand_batch (M: its merge_cand_chain.Device), then the entry under WRITE_REC with list items on the same stream, no download in
        between; self holds the frame's original, the merge buffer of pred_len samples (with the room make() left behind it) becomes its prediction
        -> (the dict the restatement returns, rd_list, the merge buffer) on the host"""
        self.pred = torch.full((pred_len,), irc.PRED_GUARD, dtype=torch.int16, device="cuda")
        resi, rec, level = self.fresh()
        _, _, _, rd = merge_cand_chain.run_entry(M, self.pred, irc.HANDOVER_MAX_NUM, 1, irc.HANDOVER_LAM)
        got = self.collect(resi, rec, level, self.run_entry(resi, rec, level, irc.WRITE_REC, rd))
        return got, rd.cpu().numpy(), self.pred.cpu().numpy()

    def fresh(self):
        """-> (resi, rec, level) buffers painted with self.fills"""
        return (torch.full((self.cand_size,), self.fills[0], dtype=torch.int16, device="cuda"), torch.full((self.cand_size,), self.fills[1], dtype=torch.int16, device="cuda"),
                torch.full((self.level_size,), self.fills[2], dtype=torch.int32, device="cuda"))

    def run_entry(self, resi, rec, level, flags=0, rd_list=None, clp=None):
        clp = clp or (0, (1 << self.bd) - 1)
        return ops.inter_resi_code_batch(self.org, self.pred, self.items_dev, self.n, resi, level, rec, rd_list, flags, self.bd, clp)


def check_all_zero_slots(items, got):
    """every served slot of `got` is an all-zero one: abs_sum 0, dist_resi == zero_dist, and resi' stored as zeros"""
    served = got["abs_sum"] != irc.U32_MAX
    assert (got["abs_sum"][served] == 0).all() and (got["dist_resi"] == got["zero_dist"][:, None])[served].all()
    for i, it in enumerate(items):
        for k in np.flatnonzero(served[i]):
            sz = int(it["w"]) * int(it["h"])
            co = int(it["cand_off"]) + int(k) * sz
            assert not got["resi"][co:co + sz].any()


class Chain:
    """the descriptor arrays of the eight launches for the served slots of D's items (uploaded once) and the intermediate buffers"""
    def __init__(self, D):
        it = D.items
        assert (it["list_row"] < 0).all()
        n = len(it)
        w, h = it["w"].astype(np.int64), it["h"].astype(np.int64)
        area = w * h
        roff = np.concatenate([[0], np.cumsum(area)[:-1]])                   # orgResi of item i: contiguous, at roff[i]
        pi, pk = np.nonzero((it["tr"] >= 0) & (it["tr"] < 9))                  # the served (item, slot) pairs (no transform skip here, no invalid codes)
        self.pairs, self.m, self.n, self.D = (pi, pk), len(pi), n, D
        code = it["tr"][pi, pk].astype(np.int64)
        sw, sh, sa = w[pi], h[pi], area[pi]
        cand, lev = it["cand_off"][pi] + pk * sa, it["level_off"][pi] + pk * sa
        sub = np.zeros(n, abi.PELOP_DESC)
        sub["src0_off"], sub["src1_off"], sub["dst_off"], sub["src0_stride"], sub["src1_stride"], sub["dst_stride"], sub["w"], sub["h"] = (
            it["org_off"], it["pred_off"], roff, it["org_stride"], it["pred_stride"], w, w, h)
        tr = np.zeros(self.m, abi.TR_DESC)
        tr["resi_off"], tr["coeff_off"], tr["resi_stride"], tr["w"], tr["h"], tr["tr_hor"], tr["tr_ver"] = roff[pi], lev, sw, sw, sh, code % 3, code // 3
        qd = np.zeros(self.m, abi.QUANT_DESC)
        qd["coeff_off"], qd["level_off"], qd["w"], qd["h"], qd["intra_slice"], qd["sign_hiding"], qd["qp"] = lev, lev, sw, sh, it["intra_slice"][pi], it["sign_hiding"][pi], it["qp"][pi]
        dq = np.zeros(self.m, abi.DQTR_DESC)
        dq["resi_off"], dq["level_off"], dq["resi_stride"], dq["w"], dq["h"], dq["tr_hor"], dq["tr_ver"], dq["qp"] = cand, lev, sw, sw, sh, code % 3, code // 3, it["qp"][pi]
        d1 = np.zeros(self.m, abi.DIST_DESC)
        d1["org_off"], d1["cur_off"], d1["org_stride"], d1["cur_stride"], d1["w"], d1["h"] = roff[pi], cand, sw, sw, sw, sh
        d0 = np.zeros(n, abi.DIST_DESC)
        d0["org_off"], d0["cur_off"], d0["org_stride"], d0["cur_stride"], d0["w"], d0["h"] = roff, 0, w, w, w, h
        rc = np.zeros(self.m, abi.PELOP_DESC)
        rc["src0_off"], rc["src1_off"], rc["dst_off"], rc["src0_stride"], rc["src1_stride"], rc["dst_stride"], rc["w"], rc["h"] = (
            it["pred_off"][pi], cand, cand, it["pred_stride"][pi], sw, sw, sw, sh)
        d2 = np.zeros(self.m, abi.DIST_DESC)
        d2["org_off"], d2["cur_off"], d2["org_stride"], d2["cur_stride"], d2["w"], d2["h"] = it["org_off"][pi], cand, it["org_stride"][pi], sw, sw, sh
        up = ops.struct_to_device
        self.sub, self.tr, self.qd, self.dq, self.d1, self.d0, self.rc, self.d2 = up(sub), up(tr), up(qd), up(dq), up(d1), up(d0), up(rc), up(d2)
        self.org_resi = torch.zeros(int(area.sum()), dtype=torch.int16, device="cuda")
        self.coeff = torch.zeros(D.level_size, dtype=torch.int32, device="cuda")
        self.zeros = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
        mx = (1 << D.bd) - 1
        self.cfg_sub, self.cfg_rec = abi.PelopCfg(0, 0, 0, 0, 0, mx), abi.PelopCfg(0, 0, 0, 1, 0, mx)

    def run(self, resi, rec, level):
        """the eight launches; resi' into resi, the reconstruction into rec, the levels into level -> (abs_sum [m], dist_resi [m], dist_rec [m], zero_dist [n])"""
        D, bd = self.D, self.D.bd
        ops.pelop_batch(3, D.org, D.pred, self.org_resi, self.sub, self.n, self.cfg_sub)
        ops.tr_fwd_batch(self.org_resi, self.coeff, self.tr, self.m, bd)
        abs_sum = ops.quant_batch(self.coeff, level, self.qd, self.m, bd)
        ops.dequant_tr_inv_batch(level, resi, self.dq, self.m, bd)
        dist_resi = ops.dist_batch(2, self.org_resi, resi, self.d1, self.m, bd)
        zero_dist = ops.dist_batch(2, self.org_resi, self.zeros, self.d0, self.n, bd)
        ops.pelop_batch(1, D.pred, resi, rec, self.rc, self.m, self.cfg_rec)
        dist_rec = ops.dist_batch(2, D.org, rec, self.d2, self.m, bd)
        return abs_sum, dist_resi, dist_rec, zero_dist

    def same(self, chain_out, entry_out):
        """the chain's results == the entry's, on the device"""
        (a, dr, dc, zd), (ea, edr, edc, ezd) = chain_out, entry_out
        pi, pk = dev(self.pairs[0]), dev(self.pairs[1])
        return bool(torch.equal(a, ea[pi, pk]) and torch.equal(dr, edr[pi, pk]) and torch.equal(dc, edc[pi, pk]) and torch.equal(zd, ezd))
