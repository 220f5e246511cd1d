"""The intra RD loop's pixel pass under DepQuant 1 as a caller has to build it without vvcgpu_intra_tu_code_dq_batch, from entries whose results the new entry
does not alter: vvcgpu_intra_pred_batch -> vvcgpu_pelop_batch (subtract) -> vvcgpu_tr_fwd_batch -> vvcgpu_depquant_batch -> vvcgpu_dequant_tr_inv_batch
(dep_quant = 1) -> vvcgpu_pelop_batch (reconstruct) -> vvcgpu_dist_batch kind 2: seven launches, the prediction, the residual, the coefficients and the
de-quantised residual through device memory between them.  Served for valid items with an explicit mode or a given prediction (no list items).  Used by the
consistency test of tests/test_gpu_intra_tu_dq.py and by tools/intra_tu_dq_time.py; Device is the harness of that test file, run_entry the one call of the
entry both use."""
import numpy as np
import torch

import rd_pass_kit as kit
from rd_pass_kit import dev
from vvcsoftware_vtm_amd import abi, ops

KEYS = ("pred", "rec", "level", "abs_sum", "num_sig", "dist", "mode_out")     # of kit.same: whole buffers, the canaries are part of the comparison


def run_entry(refs, preds, org, pred, rec, level, tus, dq, n, rates, n_rates, mode_list=None, flags=0, bd=10, clp=None, ws=None):
    """one call of the entry -> the device tensors (abs_sum, num_sig, dist, mode_out); no synchronisation"""
    return ops.intra_tu_code_dq_batch(refs, preds, org, pred, rec, level, tus, dq, n, rates, n_rates, mode_list, flags, bd, clp or (0, (1 << bd) - 1), ws)


class Device:
    """the planes, references, descriptors, records and rate tables of a case (tests/intra_tu_dq_cases.py) on the device, uploaded once, and a workspace for
    its level extent (ws_fill: painted with that byte)"""
    def __init__(self, case, ws_fill=None, refs=None, org=None):
        tc = case.tc
        self.case, self.bd, self.n = case, case.bd, len(tc.items)
        self.d_host, self.t_host = tc.descs()
        up = ops.struct_to_device
        self.preds, self.tus, self.dq, self.rates = up(self.d_host), up(self.t_host), up(case.dq), up(case.rates)
        self.refs = dev(tc.refs()) if refs is None else refs
        self.org = dev(tc.base.org.reshape(-1)) if org is None else org
        self.ws = ops.intra_tu_code_dq_workspace(tc.level_size, self.n)
        if ws_fill is not None:
            self.ws.fill_(ws_fill)

    def fresh(self):
        """-> (pred, rec, level) as they are before a call"""
        return tuple(dev(b) for b in self.case.tc.initial())

    def launch(self, pred, rec, level, flags=0, mode_list=None, clp=None, ws=None, n=None):
        return run_entry(self.refs, self.preds, self.org, pred, rec, level, self.tus, self.dq, self.n if n is None else n, self.rates, len(self.case.rates),
                         mode_list, flags, self.bd, clp, self.ws if ws is None else ws)

    def run(self, flags=0, mode_list=None, clp=None, use_pred=True, ws=None, n=None):
        """the entry on fresh buffers -> the dict the restatement returns"""
        pred, rec, level = self.fresh()
        return kit.download((pred, rec, level) + self.launch(pred if use_pred else None, rec, level, flags, mode_list, clp, ws, n), KEYS)


class Chain:
    """the descriptor arrays of the seven launches (uploaded once) and the intermediate buffers, from the host arrays of the items: d (INTRA_DESC), t (RC_DESC),
    dq (INTER_RESI_DQ); every item valid, no FROM_LIST item; an item with mode -1 has its prediction in the prediction buffer already"""
    def __init__(self, d, t, dq, rates_dev, level_size, bd, refs, org):
        n = len(t)
        assert (d["mode"] >= -1).all() and (t["level_off"] % 16 == 0).all()
        w, h = t["w"].astype(np.int64), t["h"].astype(np.int64)
        area = w * h
        roff = np.concatenate([[0], np.cumsum(area)[:-1]])                    # the residual and resi' of item i: contiguous, at roff[i]
        self.n, self.bd, self.refs, self.org, self.rates, self.level_size = n, bd, refs, org, rates_dev, int(level_size)
        ip = d[d["mode"] >= 0].copy()
        ip["dst_off"], ip["dst_stride"] = t["pred_off"][d["mode"] >= 0], t["pred_stride"][d["mode"] >= 0]
        sub = np.zeros(n, abi.PELOP_DESC)
        sub["src0_off"], sub["src1_off"], sub["dst_off"], sub["src0_stride"], sub["src1_stride"], sub["dst_stride"], sub["w"], sub["h"] = (
            t["org_off"], t["pred_off"], roff, t["org_stride"], t["pred_stride"], w, w, h)
        tr = np.zeros(n, abi.TR_DESC)
        tr["resi_off"], tr["coeff_off"], tr["resi_stride"], tr["w"], tr["h"], tr["tr_hor"], tr["tr_ver"] = roff, t["level_off"], w, w, h, t["tr_hor"], t["tr_ver"]
        dd = np.zeros(n, abi.DEPQUANT_DESC)
        dd["coeff_off"], dd["level_off"], dd["lambda"], dd["qp"], dd["rates_idx"], dd["w"], dd["h"], dd["luma"] = (
            t["level_off"], t["level_off"], dq["lambda"], t["qp"], dq["rates_idx"], w, h, dq["luma"])
        iq = np.zeros(n, abi.DQTR_DESC)
        iq["resi_off"], iq["level_off"], iq["resi_stride"], iq["w"], iq["h"], iq["tr_hor"], iq["tr_ver"], iq["dep_quant"], iq["qp"] = (
            roff, t["level_off"], w, w, h, t["tr_hor"], t["tr_ver"], 1, t["qp"])
        rc = np.zeros(n, abi.PELOP_DESC)
        rc["src0_off"], rc["src1_off"], rc["dst_off"], rc["src0_stride"], rc["src1_stride"], rc["dst_stride"], rc["w"], rc["h"] = (
            t["pred_off"], roff, t["rec_off"], t["pred_stride"], w, t["rec_stride"], w, h)
        d2 = np.zeros(n, abi.DIST_DESC)
        d2["org_off"], d2["cur_off"], d2["org_stride"], d2["cur_stride"], d2["w"], d2["h"] = t["org_off"], t["rec_off"], t["org_stride"], t["rec_stride"], w, h
        up = ops.struct_to_device
        self.n_pred = len(ip)
        self.ip, self.sub, self.tr, self.dd, self.iq, self.rc, self.d2 = (up(ip) if len(ip) else None), up(sub), up(tr), up(dd), up(iq), up(rc), up(d2)
        self.resi = torch.zeros(int(area.sum()), dtype=torch.int16, device="cuda")
        self.resi2 = torch.zeros_like(self.resi)
        self.coeff = torch.zeros(self.level_size, dtype=torch.int32, device="cuda")
        mx = (1 << bd) - 1
        self.cfg_sub, self.cfg_rec = abi.PelopCfg(0, 0, 0, 0, 0, mx), abi.PelopCfg(0, 0, 0, 1, 0, mx)

    def run(self, pred, rec, level):
        """the seven launches; the prediction into pred, the reconstruction into rec, the levels into level -> (abs_sum [n], dist [n])"""
        bd, clp = self.bd, (0, (1 << self.bd) - 1)
        if self.n_pred:
            ops.intra_pred_batch(self.refs, pred, self.ip, self.n_pred, clp)
        ops.pelop_batch(3, self.org, pred, self.resi, self.sub, self.n, self.cfg_sub)
        ops.tr_fwd_batch(self.resi, self.coeff, self.tr, self.n, bd)
        abs_sum = ops.depquant_batch(self.coeff, level, self.dd, self.n, self.rates, self.level_size, bd)
        ops.dequant_tr_inv_batch(level, self.resi2, self.iq, self.n, bd)
        ops.pelop_batch(1, pred, self.resi2, rec, self.rc, self.n, self.cfg_rec)
        return abs_sum, ops.dist_batch(2, self.org, rec, self.d2, self.n, bd)
