"""The intra chroma mode pass under DepQuant 1 as a chain of the entries that existed before vvcgpu_intra_chroma_code_dq_batch, for its GPU tests and for
tools/intra_chroma_dq_time.py: the prediction part of tests/intra_chroma_code_chain.py (vvcgpu_intra_fill_refs_batch x 2, vvcgpu_intra_pred_batch,
vvcgpu_cclm_pred_batch), then vvcgpu_intra_tu_code_dq_batch with PRED_GIVEN items for the Cb blocks, the DOWNLOAD of their abs_sum, the choice of every
Cr block's record on the host (dq[3 p + 1] behind abs_sum == 0, dq[3 p + 2] behind abs_sum > 0), its upload, and vvcgpu_intra_tu_code_dq_batch for the Cr
blocks.  The host synchronisation between Cb and Cr is what the new entry removes."""
import numpy as np
import torch

from intra_chroma_code_chain import Chain
from vvcsoftware_vtm_amd import abi, ops


class DqChain(Chain):
    """pus, fill as Chain's; dq: three abi.INTER_RESI_DQ records per PU; rates: the abi.DQ_RATES array"""
    def __init__(self, pus, fill, dq, rates, bd, clp, rec, flags, luma, org, refs, pred, cand_rec, level):
        Chain.__init__(self, pus, fill, bd, clp, rec, flags, luma, org, refs, pred, cand_rec, level)
        t, g = self.t.cpu().numpy().view(abi.RC_DESC).reshape(-1), self.g.cpu().numpy().view(abi.INTRA_DESC).reshape(-1)
        comp = self.item % 2                                                    # the items run (PU, slot, component): Cb and Cr of a slot alternate
        assert (comp[0::2] == 0).all() and (comp[1::2] == 1).all()
        self.P, self.dq = self.item[0::2] // 12, dq
        self.half = len(self.P)
        self.t_c = [ops.struct_to_device(np.ascontiguousarray(t[c::2])) for c in range(2)]
        self.g_c = [ops.struct_to_device(np.ascontiguousarray(g[c::2])) for c in range(2)]
        self.dq_cb = ops.struct_to_device(np.ascontiguousarray(dq[3 * self.P]))
        self.rates, self.n_rates = ops.struct_to_device(rates), len(rates)
        self.ws = ops.intra_tu_code_dq_workspace(int(level.numel()), self.half)

    def code(self, c, dq_dev):
        a, _, d, _ = ops.intra_tu_code_dq_batch(self.refs, self.g_c[c], self.org, self.pred, self.cand_rec, self.level, self.t_c[c], dq_dev, self.half, self.rates,
                                                self.n_rates, None, 0, self.bd, self.clp, self.ws)
        return a, d

    def run(self):
        """the chain on the current stream (repack() once, after a gather()) -> (abs_sum, dist) of the items in list order"""
        self.gather()
        if self.n_ang:
            ops.intra_pred_batch(self.refs, self.pred, self.d, self.n_ang, self.clp)
        if self.n_lm:
            ops.cclm_pred_batch(self.luma, self.nb, self.pred, self.cd, self.n_lm, self.bd, self.bd, self.clp)
        a_cb, d_cb = self.code(0, self.dq_cb)
        coded = a_cb.cpu().numpy() != 0                                         # the download: the stream drains here
        a_cr, d_cr = self.code(1, ops.struct_to_device(np.ascontiguousarray(self.dq[3 * self.P + np.where(coded, 2, 1)])))
        return torch.stack([a_cb, a_cr], 1).reshape(-1), torch.stack([d_cb, d_cr], 1).reshape(-1)
