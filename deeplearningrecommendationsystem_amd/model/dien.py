"""DIEN -- counterpart of the reference's model/dien.py:8-81."""
from __future__ import annotations

import os

import torch
import torch.nn as nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_NONE, ACT_SIGMOID
from ._base import Params
from ._grid import HistoryGridScorer
from .din import SequenceModel, folded_attention, mlp_layers, unfold_attention_grad

# the GRU kernels form the input projection themselves (ctr_gru_fused_fwd / _bwd); CTR_DIEN_FUSED_GRU=0 keeps the
# gi GEMM + recurrence + three gradient GEMMs for A/B
FUSED_GRU = os.environ.get("CTR_DIEN_FUSED_GRU", "1") != "0"


class DIN(nn.Module):
    """parameter container of DIEN's attention unit (reference model/dien.py:8-39:
    attention MLP 3E -> 64 -> 32 -> 1, returns the un-summed weighted history)"""

    def __init__(self, num_items, embed_size, table=None):
        super().__init__()
        if table is None:
            table = nn.Embedding(num_items, embed_size)
            xavier_normal_(table.weight.data)
        self.item_embedding = table
        self.attention = nn.Sequential(nn.Linear(embed_size * 3, 64), nn.ReLU(), nn.Linear(64, 32), nn.ReLU(),
                                       nn.Linear(32, 1))


class DIEN(SequenceModel):
    """``DIEN(num_items, embed_size)``; ``forward(hist, target_item) -> (B,1)``.

    attention (as DIN, un-summed) -> gi = seq W_ih^T + b_ih as ONE GEMM over all
    B*L rows -> sequential GRU kernel (h0 = 0) -> hidden[-1] lands in the left half
    of the fc input next to t -> fc MLP + sigmoid."""

    def __init__(self, num_items, embed_size, *, sharded=False, group=None):
        super().__init__()
        self.sharded = bool(sharded)
        self.din = DIN(num_items, embed_size, self._make_table(num_items, embed_size, sharded, group))
        self.interest_evolution = nn.GRU(embed_size, embed_size, batch_first=True)
        self.fc = nn.Sequential(nn.Linear(embed_size * 2, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU(),
                                nn.Linear(64, 1), nn.Sigmoid())

    def _params(self):
        g = self.interest_evolution
        return Params(table=self.din.item_embedding.weight, att=mlp_layers(self.din.attention, ACT_NONE),
                      fc=mlp_layers(self.fc, ACT_SIGMOID), w_ih=g.weight_ih_l0, w_hh=g.weight_hh_l0, b_ih=g.bias_ih_l0,
                      b_hh=g.bias_hh_l0)

    def forward(self, hist, target_item):
        return self._run_sequence(self.din.item_embedding, hist, target_item, self._params())

    def run_forward(self, inputs, p):
        hist, target = inputs
        table = p.table
        batch, length = hist.shape
        dim = table.shape[1]
        dev = table.device
        att, w1f, _ = folded_attention(p.att, dim)  # [h, t] operand instead of [h, h-t, t]
        c = torch.empty((batch * length, 2 * dim), dtype=torch.float32, device=dev)
        fcin = torch.empty((batch, 2 * dim), dtype=torch.float32, device=dev)
        ops.din_concat_fwd(table, hist, target, c, fcin[:, dim:], self._flag, pair=True)
        att_acts = ops.mlp_fwd(c, att)
        attn = torch.empty((batch, length), dtype=torch.float32, device=dev)
        seq = torch.empty((batch * length, dim), dtype=torch.float32, device=dev)
        ops.din_pool_fwd(att_acts[-1], c, batch, length, dim, attn, seq, summed=False)
        hbuf = torch.empty((batch * (length + 1), dim), dtype=torch.float32, device=dev)
        # the recurrence kernel forms the input projection itself where it can (E = 16): no (B*L, 3E) gi
        gi = None
        if not (FUSED_GRU and ops.gru_fused_fwd(seq, p.w_ih, p.b_ih, p.w_hh, p.b_hh, batch, length, dim, hbuf,
                                                fcin[:, :dim])):
            gi = ops.linear_fwd(seq, p.w_ih, p.b_ih)
            ops.gru_fwd(gi, p.w_hh, p.b_hh, batch, length, dim, hbuf, fcin[:, :dim])
        fc_acts = ops.mlp_fwd(fcin, p.fc)
        return fc_acts[-1], (att_acts, attn, seq, gi, hbuf, fc_acts, w1f)

    def run_backward(self, state, inputs, p, gprob, zeros):
        hist, target = inputs
        att_acts, attn, seq, gi, hbuf, fc_acts, w1f = state
        table = p.table
        batch, length = hist.shape
        dim = table.shape[1]
        dev = table.device
        c = att_acts[0]
        att, _, w1 = folded_attention(p.att, dim, w1f)
        zeros[id(w1f)] = torch.zeros_like(w1f)
        _, gfcin = ops.mlp_bwd(fc_acts, p.fc, gprob, None, zeros=zeros)
        g_w_ih, g_w_hh, g_b_ih, g_b_hh = (zeros[id(t)] for t in (p.w_ih, p.w_hh, p.b_ih, p.b_hh))
        gseq = torch.empty_like(seq)
        if gi is None:
            # input gradient and the four parameter gradients straight out of the recurrence's backward
            ops.gru_fused_bwd(seq, p.w_ih, p.b_ih, p.w_hh, p.b_hh, hbuf, batch, length, dim, gfcin[:, :dim], gseq,
                              g_w_ih, g_b_ih, g_w_hh, g_b_hh)
        else:
            dgi = torch.empty((batch * length, 3 * dim), dtype=torch.float32, device=dev)
            dgh = torch.empty((batch * (length + 1), 3 * dim), dtype=torch.float32, device=dev)
            ops.gru_bwd(gi, p.w_hh, p.b_hh, hbuf, batch, length, dim, gfcin[:, :dim], dgi, dgh)
            ops.linear_bwd(seq, p.w_ih, None, dgi, ACT_NONE, gseq, g_w_ih, g_b_ih)
            # dW_hh = sum_{b,t} dgh_t (x) h_{t-1}: rows r+1 of dgh against rows r of hbuf; the
            # zero row at the head of every sample makes the pairs that straddle samples vanish
            rows = batch * (length + 1) - 1
            if rows > 0:
                ops.linear_bwd(hbuf[:rows], p.w_hh, None, dgh[1:], ACT_NONE, None, g_w_hh, g_b_hh)
        gscore = torch.empty((batch * length, 1), dtype=torch.float32, device=dev)
        ops.din_pool_bwd(attn, c, batch, length, dim, gseq, False, gscore)
        _, gc = ops.mlp_bwd(att_acts, att, gscore, None, zeros=zeros)
        ops.din_concat_bwd(hist, target, table.shape[0], dim, gc, attn, gseq, False, gfcin[:, dim:], zeros[id(table)],
                           pair=True)
        unfold_attention_grad(zeros[id(w1f)], zeros[id(w1)], dim)

    def recommendation(self, num_users, num_items, hist_list, k):
        return self._rank_histories(num_users, num_items, hist_list, k)

    def _grid_scorer(self):
        return _HistoryScorer(self)


def grid_path(embed_size, attention_dims=ops.DIEN_GRID_ATTENTION) -> str:
    """how ``score_histories`` / ``recommend`` score a DIEN of this embedding width: "grid" -- the split first attention
    layer and the GRU's input projection on the table rows, then ``ctr_dien_grid_hidden`` and the fc stack -- where the
    library has that kernel, else "forward": the per-sample forward over ids generated chunk by chunk"""
    return "grid" if ops.dien_grid_supported(embed_size, attention_dims) else "forward"


class _HistoryScorer(HistoryGridScorer):
    """DIEN on the history x item grid: the history part HP is the table under the stacked weight ``wh`` =
    [Wa + Wb ; W_ih] (attention and the GRU's input projection in one product), the kernel runs attention and GRU"""

    def _grid_path(self, embed_size, attention_dims):
        return grid_path(embed_size, attention_dims)

    def _operands(self, p, w1):
        dim, n1 = self.table.shape[1], w1.shape[0]
        self.wh = torch.empty((n1 + 3 * dim, dim), dtype=torch.float32, device=self.table.device)
        torch.add(w1[:, :dim], w1[:, dim:2 * dim], out=self.wh[:n1])     # Wa + Wb: the history part, over
        self.wh[n1:] = p.w_ih.detach()                                   # W_ih: the GRU's input projection
        self.b_ih, self.w_hh, self.b_hh = p.b_ih.detach(), p.w_hh.detach().contiguous(), p.b_hh.detach()
        return self.wh, torch.sub(w1[:, 2 * dim:], w1[:, dim:2 * dim])   # Wc - Wb: the item part

    def _fill(self, hist, hp, by_position, out):
        ops.dien_grid_hidden(self.at, hp, self.w2, self.b2, self.w3, self.b_ih, self.w_hh, self.b_hh, hist, out=out,
                             hp_by_position=by_position, err_flag=self.flag)
