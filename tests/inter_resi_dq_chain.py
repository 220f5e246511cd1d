"""The inter residual pixel pass under DepQuant 1 as a caller has to build it without vvcgpu_inter_resi_code_dq_batch, from entries whose results the new
entry does not alter: vvcgpu_pelop_batch (subtract) -> vvcgpu_tr_fwd_batch -> vvcgpu_depquant_batch -> vvcgpu_dequant_tr_inv_batch (dep_quant = 1) ->
vvcgpu_dist_batch kind 2 twice (orgResi against resi', orgResi against a zero block) -> vvcgpu_pelop_batch (reconstruct) -> vvcgpu_dist_batch kind 2 (org
against rec): eight launches.  Served for items with a given prediction (no list items) and slots the entry serves.  Used by the consistency test of
tests/test_gpu_inter_resi_dq.py and by tools/inter_resi_dq_time.py; Device.run_entry is the one call of the entry both use."""
import numpy as np
import torch

import inter_resi_code_chain as base
from vvcsoftware_vtm_amd import abi, ops

dev, KEYS, FILLS, check_all_zero_slots = base.dev, base.KEYS, base.FILLS, base.check_all_zero_slots


class Device(base.Device):
    """the sibling's device copy of a case + the dq records, the rate tables and a workspace for the level extent"""
    def __init__(self, bd, org, pred, items, dq, rates, cand_size, level_size, fills=(0, 0, 0), ws_fill=None):
        base.Device.__init__(self, bd, org, pred, items, cand_size, level_size, fills)
        self.dq, self.dq_dev, self.rates, self.rates_dev = dq, ops.struct_to_device(dq), rates, ops.struct_to_device(rates)
        self.ws = ops.inter_resi_code_dq_workspace(self.level_size, self.n)
        if ws_fill is not None:
            self.ws.fill_(ws_fill)

    def run_entry(self, resi, rec, level, flags=0, rd_list=None, clp=None, ws=None):
        clp = clp or (0, (1 << self.bd) - 1)
        return ops.inter_resi_code_dq_batch(self.org, self.pred, self.items_dev, self.dq_dev, self.n, self.rates_dev, len(self.rates), resi, level, rec, rd_list,
                                            flags, self.bd, clp, self.ws if ws is None else ws)


class Chain(base.Chain):
    """the descriptor arrays of the eight launches: the sibling's, with the trellis' descriptors in place of the scalar quantiser's and dep_quant = 1"""
    def __init__(self, D):
        base.Chain.__init__(self, D)
        it = D.items
        pi, pk = self.pairs
        area = it["w"].astype(np.int64) * it["h"]
        lev = it["level_off"][pi] + pk * area[pi]
        dd = np.zeros(self.m, abi.DEPQUANT_DESC)
        dd["coeff_off"], dd["level_off"], dd["lambda"], dd["qp"], dd["rates_idx"], dd["w"], dd["h"], dd["luma"] = (
            lev, lev, D.dq["lambda"][pi], it["qp"][pi], D.dq["rates_idx"][pi], it["w"][pi], it["h"][pi], D.dq["luma"][pi])
        dq = np.zeros(self.m, abi.DQTR_DESC)
        code = it["tr"][pi, pk].astype(np.int64)
        dq["resi_off"], dq["level_off"], dq["resi_stride"], dq["w"], dq["h"], dq["tr_hor"], dq["tr_ver"], dq["dep_quant"], dq["qp"] = (
            it["cand_off"][pi] + pk * area[pi], lev, it["w"][pi], it["w"][pi], it["h"][pi], code % 3, code // 3, 1, it["qp"][pi])
        self.dd, self.dq = ops.struct_to_device(dd), ops.struct_to_device(dq)

    def run(self, resi, rec, level):
        D, bd = self.D, self.D.bd
        ops.pelop_batch(3, D.org, D.pred, self.org_resi, self.sub, self.n, self.cfg_sub)
        ops.tr_fwd_batch(self.org_resi, self.coeff, self.tr, self.m, bd)
        abs_sum = ops.depquant_batch(self.coeff, level, self.dd, self.m, D.rates_dev, D.level_size, bd)
        ops.dequant_tr_inv_batch(level, resi, self.dq, self.m, bd)
        dist_resi = ops.dist_batch(2, self.org_resi, resi, self.d1, self.m, bd)
        zero_dist = ops.dist_batch(2, self.org_resi, self.zeros, self.d0, self.n, bd)
        ops.pelop_batch(1, D.pred, resi, rec, self.rc, self.m, self.cfg_rec)
        dist_rec = ops.dist_batch(2, D.org, rec, self.d2, self.m, bd)
        return abs_sum, dist_resi, dist_rec, zero_dist
