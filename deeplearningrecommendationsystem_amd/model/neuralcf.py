"""NeuralCF -- counterpart of the reference's model/neuralcf.py:7-72."""
from __future__ import annotations

import os
from typing import List, NamedTuple, Tuple

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import loss as _loss
from .. import ops, topn
from ..ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, FieldSpec, Layer
from .._lib import FIELD_ID_I64, FIELD_PROD_I64, CtrHipError
from ._base import CtrModule, Params
from ._grid import UserGridScorer

# Vocabularies much smaller than the batch (BASELINE configs[1]: 943 + 1682 rows, batch 65536): the first tower layer
# and its backward on the TABLE ROWS instead of the samples (csrc/ncf_proj.hip, ops.NcfProj).  CTR_NCF_PROJ=0 keeps the
# per-sample kernels for A/B; they are also what every other shape runs (and the cross-check of this path in the tests).
PROJECT_TABLES = os.environ.get("CTR_NCF_PROJ", "1") != "0"


class _Params(NamedTuple):
    """the model's parameters by name; ``flat`` is the order autograd sees them in:
    GMF_U, GMF_I, MLP_U, MLP_I, (W,b) x n_hidden, linear W,b, linear2 W,b"""
    tables: Tuple[torch.Tensor, ...]    # (gmf_u, gmf_i, mlp_u, mlp_i)
    hidden: List[Layer]
    proj: Tuple[torch.Tensor, torch.Tensor]     # ``linear``
    head: Tuple[torch.Tensor, torch.Tensor]     # ``linear2``
    flat: Tuple[torch.Tensor, ...]


def _unpack(flat, n_hidden) -> _Params:
    dense = flat[4:]
    return _Params(tuple(flat[:4]), [Layer(dense[2 * k], dense[2 * k + 1], ACT_RELU) for k in range(n_hidden)],
                   (dense[2 * n_hidden], dense[2 * n_hidden + 1]), (dense[2 * n_hidden + 2], dense[2 * n_hidden + 3]),
                   tuple(flat))


def _grads(zeros, p: _Params):
    """the gradient of every parameter, in autograd order, out of a ``zeros`` dict of ``ops.zero_grads``"""
    return tuple(zeros[id(t)] for t in p.flat)


def _specs(user_idx, item_idx, gmf_u, gmf_i, mlp_u, mlp_i):
    mf, half = gmf_u.shape[1], mlp_u.shape[1]
    l0 = 2 * half
    return [
        FieldSpec(FIELD_ID_I64, half, 0, table=mlp_u, idx=user_idx),
        FieldSpec(FIELD_ID_I64, half, half, table=mlp_i, idx=item_idx),
        FieldSpec(FIELD_PROD_I64, mf, l0, table=gmf_u, idx=user_idx, table2=gmf_i, idx2=item_idx),
    ]


def _head_tower_bwd(buf, gbuf, x0, mf, wfold, prob, gprob, gwfold, gcfold, acts, layers, zeros):
    """the head as a single-unit layer on [gmf | h] (the columns of ``buf`` from ``x0`` on), then the tower ``layers``
    down to the first ``x0`` columns of ``gbuf``"""
    ops.linear_bwd(buf[:, x0:], wfold, prob, gprob.contiguous(), ACT_SIGMOID, gbuf[:, x0:], gwfold, gcfold)
    ops.mlp_bwd(acts, layers, gbuf[:, x0 + mf:], gbuf[:, :x0], zeros=zeros)


# The three ways through the model.  Each has the same two entry points:
#   forward(p, user_idx, item_idx, err_flag, wants_grad, training, counts) -> prob, tensors to save, other state
#   backward(p, user_idx, item_idx, saved, state, gprob) -> the ``zeros`` dict holding every parameter's gradient
class _ProjPath:
    """one ``ctr_ncf_proj_fwd`` forward, one ``ctr_ncf_proj_bwd`` backward"""

    @staticmethod
    def forward(p, user_idx, item_idx, err_flag, wants_grad, training, counts):
        run = ops.NcfProj(user_idx, item_idx, p.tables, p.hidden, p.proj, p.head, err_flag, training, counts)
        prob = run.forward()
        if prob is None:
            raise CtrHipError("ctr_ncf_proj_fwd refused a shape NcfProj.supported() accepted")
        if training:
            _loss.offer_deferral(run, prob)      # (inside a captured step alone: this backward can form the BCE loss)
        return prob, (), {"run": run if training else None}

    @staticmethod
    def backward(p, user_idx, item_idx, saved, state, gprob):
        run = state["run"]
        if run is None:
            raise RuntimeError("NeuralCF backward without a training forward")
        state["run"] = None
        zeros = ops.zero_grads(list(p.flat), lazy=True)   # cleared by the backward's first launch
        flat = zeros.pop("flat")
        deferred = getattr(run, "deferred", None)
        if deferred is None:
            run.backward(gprob.contiguous(), zeros, flat)
        else:
            # a deferred BCELoss sits on prob: its gradient is a placeholder nobody wrote.  Anything but that very tensor
            # (a sum with another consumer's gradient, a copy) cannot be honoured -- and is never computed from
            target, loss, placeholder = deferred
            if gprob.data_ptr() != placeholder.data_ptr() or gprob.numel() != placeholder.numel():
                raise RuntimeError("NeuralCF backward: prob of a step with a deferred BCELoss may feed that loss alone")
            run.backward(None, zeros, flat, target=target, loss=loss)
        return zeros


class _RowsPath:
    """The same move for ANY tower (the reference script's NeuralCF(943, 1682, 256, [512, 256, 128, 64, 32]),
    scripts/neuralcf.py:60): the first layer on the table rows, composed from library calls --
        P_U = MLP_U W0[:, :h]^T, P_I = MLP_I W0[:, h:]^T + b0           two ctr_linear_fwd over U + I rows
        a0  = relu(P_U[u] + P_I[i])                                      ctr_rows_sum_act_fwd
        tower layers 1.., folded head, GMF product                       as in _SamplesPath
    backward: the gradient of a0, masked (ctr_act_mask_bwd), is the gradient of BOTH projected rows: ctr_embed_bwd sums
    it by user and by item (S_U, S_I), and two ctr_linear_bwd over the table rows give dMLP = S W0half,
    dW0half = S^T MLP, db0 = column sums.  Three quarters of the tower's matrix work leave the batch."""

    @staticmethod
    def admits(tables, hidden, batch) -> bool:
        """a tower of at least two layers whose first layer takes cat(MLP_U[u], MLP_I[i]), row counts far below the
        batch, widths the library's row kernels take"""
        gmf_u, gmf_i, mlp_u, mlp_i = tables
        if len(hidden) < 2 or hidden[0].bias is None:
            return False
        n0, k0 = hidden[0].weight.shape
        half = mlp_u.shape[1]
        return (k0 == 2 * half and half % 4 == 0 and n0 % 4 == 0 and n0 <= 256 and gmf_u.shape[1] % 4 == 0 and
                ops.few_table_rows(gmf_u.shape[0] + gmf_i.shape[0], batch))

    @staticmethod
    def forward(p, user_idx, item_idx, err_flag, wants_grad, training, counts):
        gmf_u, gmf_i, mlp_u, mlp_i = p.tables
        batch = user_idx.numel()
        mf, half = gmf_u.shape[1], mlp_u.shape[1]
        w0, b0 = p.hidden[0].weight, p.hidden[0].bias
        n0, kh = w0.shape[0], p.proj[0].shape[1]
        p_u = ops.linear_fwd(mlp_u, w0[:, :half], None)
        p_i = ops.linear_fwd(mlp_i, w0[:, half:], b0)
        buf = torch.empty((batch, n0 + mf + kh), dtype=torch.float32, device=gmf_u.device)   # [a0 | gmf | h]
        ops.rows_sum_act_fwd(p_u, user_idx, p_i, item_idx, ACT_RELU, buf[:, :n0], err_flag)
        ops.embed_fwd([FieldSpec(FIELD_PROD_I64, mf, n0, table=gmf_u, idx=user_idx, table2=gmf_i, idx2=item_idx)], None,
                      batch, buf, err_flag)
        wfold, cfold = ops.fold_head_fwd(p.head[0], mf, *p.proj, p.head[1])
        head = ops.Head(buf[:, n0:n0 + mf], wfold, cfold, ACT_SIGMOID)
        acts = ops.mlp_fwd(buf[:, :n0], p.hidden[1:], last_out=buf[:, n0 + mf:], head=head)
        return head.out, (buf, head.out, wfold, p_u, p_i, *acts[1:-1]), {}

    @staticmethod
    def backward(p, user_idx, item_idx, saved, state, gprob):
        buf, prob, wfold, p_u, p_i, *mids = saved
        gmf_u, gmf_i, mlp_u, mlp_i = p.tables
        (proj_w, proj_b), (head_w, head_b) = p.proj, p.head
        batch = user_idx.numel()
        mf, half = gmf_u.shape[1], mlp_u.shape[1]
        w0, b0 = p.hidden[0].weight, p.hidden[0].bias
        n0 = w0.shape[0]
        zeros = ops.zero_grads(list(p.flat) + [wfold, head_b.new_empty(4), p_u, p_i])
        gwfold, gcfold = zeros[id(wfold)], zeros[id(wfold)].new_zeros(1)
        s_u, s_i = zeros[id(p_u)], zeros[id(p_i)]                 # the row sums of the first layer's gradient
        gbuf = torch.empty_like(buf)
        acts = [buf[:, :n0]] + mids + [buf[:, n0 + mf:]]
        _head_tower_bwd(buf, gbuf, n0, mf, wfold, prob, gprob, gwfold, gcfold, acts, p.hidden[1:], zeros)   # down to a0
        ops.act_mask_bwd(gbuf[:, :n0], buf[:, :n0], ACT_RELU)
        ops.fold_head_bwd(head_w, mf, proj_w, proj_b, gwfold, gcfold, zeros[id(head_w)], zeros[id(proj_w)],
                          zeros[id(proj_b)], zeros[id(head_b)])
        specs = [FieldSpec(FIELD_ID_I64, n0, 0, table=p_u, idx=user_idx),
                 FieldSpec(FIELD_ID_I64, n0, 0, table=p_i, idx=item_idx),
                 FieldSpec(FIELD_PROD_I64, mf, n0, table=gmf_u, idx=user_idx, table2=gmf_i, idx2=item_idx)]
        ops.embed_bwd(specs, None, batch, gbuf, zeros)
        g_w0 = zeros[id(w0)]
        ops.linear_bwd(mlp_u, w0[:, :half], None, s_u, ACT_NONE, zeros[id(mlp_u)], g_w0[:, :half], None, accumulate_gx=True)
        ops.linear_bwd(mlp_i, w0[:, half:], None, s_i, ACT_NONE, zeros[id(mlp_i)], g_w0[:, half:], zeros[id(b0)],
                       accumulate_gx=True)
        return zeros


class _SamplesPath:
    """Every layer on the samples.

    ``linear`` (h -> mf_dim, no activation) feeds only ``linear2`` (reference model/neuralcf.py:50-56), so
    the pair is one k-wide dot product per sample: ``[gmf | linear(h)] . w2 + b2 == [gmf | h] . wfold + c``
    with ``wfold = [w2[:mf] | W_l^T w2[mf:]]``, ``c = b_l . w2[mf:] + b2`` (ops.fold_head_fwd, O(mf*k) per
    step).  The (B, mf_dim) output of ``linear`` and its gradient never exist; the gradients of
    ``linear`` / ``linear2`` come back through the chain rule (ops.fold_head_bwd) from the k + mf sums the
    head's backward produces anyway.  Same values up to fp32 rounding (parity tests unchanged).

    Buffer layout (one (B, L0 + mf + k) matrix, no torch.cat anywhere):
        [ MLP_U[u] | MLP_I[i] |  GMF_U[u]*GMF_I[i] | h = tower(x0) ]
          `-- MLP input x0 --'   `--- input of the folded head ---'

    Where the library has the kernels (the BASELINE shape) the four embedding rows are gathered inside the tower's
    forward kernel (ctr_embed_mlp_head_fwd) and, when a gradient is wanted, AGAIN by the tower's backward kernel
    (ctr_embed_mlp_head_bwd): the forward then never writes the (B, 128) tower input and the backward never reads it
    (the tables of the BASELINE shape sit in L2).
    """

    @staticmethod
    def forward(p, user_idx, item_idx, err_flag, wants_grad, training, counts):
        (proj_w, proj_b), (head_w, head_b) = p.proj, p.head
        batch = user_idx.numel()
        mf, l0 = p.tables[0].shape[1], 2 * p.tables[2].shape[1]
        kh = proj_w.shape[1]  # width of h
        buf = torch.empty((batch, l0 + mf + (kh if p.hidden else 0)), dtype=torch.float32, device=p.tables[0].device)
        specs = _specs(user_idx, item_idx, *p.tables)
        acts = fold_out = None
        if p.hidden:
            # gather + head fold + tower + folded head in one launch; None: the library has no such kernel for this shape
            fold_out = (torch.empty((1, mf + kh), dtype=torch.float32, device=buf.device),
                        torch.empty(1, dtype=torch.float32, device=buf.device))
            head = ops.Head(buf[:, l0:l0 + mf], *fold_out, ACT_SIGMOID)
            acts = ops.embed_mlp_head_fwd(specs, batch, buf, l0, p.hidden, head, buf[:, l0 + mf:], err_flag,
                                          write_x=not wants_grad, fold=(head_w, proj_w, proj_b, head_b))
        regather = wants_grad and acts is not None
        if acts is not None:
            wfold = head.w
        else:
            wfold, cfold = ops.fold_head_fwd(head_w, mf, proj_w, proj_b, head_b, out=fold_out)
            ops.embed_fwd(specs, None, batch, buf, err_flag)
            if p.hidden:
                # tower + folded head in one launch: the head's dot product runs on the tile's last
                # activations while they are still in LDS
                head = ops.Head(buf[:, l0:l0 + mf], wfold, cfold, ACT_SIGMOID)
                acts = ops.mlp_fwd(buf[:, :l0], p.hidden, last_out=buf[:, l0 + mf:], head=head)
        if p.hidden:
            prob = head.out
        else:
            # no tower: h is x0 itself, which sits in FRONT of the GMF columns
            acts = [buf[:, :l0]]
            wf = torch.cat([wfold[:, mf:], wfold[:, :mf]], dim=1)
            prob = ops.linear_fwd(buf, wf, cfold, ACT_SIGMOID)
        return prob, (buf, prob, wfold, *acts[1:-1]), {"regather": regather}

    @staticmethod
    def backward(p, user_idx, item_idx, saved, state, gprob):
        buf, prob, wfold, *mids = saved
        (proj_w, proj_b), (head_w, head_b) = p.proj, p.head
        regather = state["regather"]
        batch = user_idx.numel()
        mf, l0 = p.tables[0].shape[1], 2 * p.tables[2].shape[1]
        specs = _specs(user_idx, item_idx, *p.tables)
        gcpad = head_b.new_empty(4)     # the folded bias's gradient is the first float of a 16-byte piece
        # (with the gathering backward the flat gradient buffer is cleared by that call's first launch, not by a fill)
        zeros = ops.zero_grads(list(p.flat) + [wfold, gcpad], lazy=regather)
        flat = zeros.pop("flat", None)
        gwfold, gcfold = zeros[id(wfold)], zeros[id(gcpad)][:1]
        gbuf = torch.empty_like(buf)
        g_proj_w, g_proj_b = zeros[id(proj_w)], zeros[id(proj_b)]
        g_head_w, g_head_b = zeros[id(head_w)], zeros[id(head_b)]
        if p.hidden:
            acts = [buf[:, :l0]] + mids + [buf[:, l0 + mf:]]
            # head backward + tower backward in one launch where the library has it (the BASELINE tower) ...
            head = ops.Head(buf[:, l0:l0 + mf], wfold, None, ACT_SIGMOID)
            fused = ops.mlp_head_bwd(acts, p.hidden, head, prob, gprob.contiguous(), gbuf[:, l0:l0 + mf], gwfold,
                                     gcfold, gbuf[:, :l0], zeros, gather_specs=specs if regather else None,
                                     # ... and fold_head_bwd in that call's reduction launch
                                     fold_grad=(head_w, proj_w, proj_b, g_head_w, g_proj_w, g_proj_b, g_head_b)
                                     if regather else None, zero=flat)
            if fused is None:
                # ... else the head as a single-unit layer on [gmf | h], then the tower
                _head_tower_bwd(buf, gbuf, l0, mf, wfold, prob, gprob, gwfold, gcfold, acts, p.hidden, zeros)
        else:
            wf = torch.cat([wfold[:, mf:], wfold[:, :mf]], dim=1)
            gwf = torch.zeros_like(wf)
            ops.linear_bwd(buf, wf, prob, gprob.contiguous(), ACT_SIGMOID, gbuf, gwf, gcfold)
            gwfold.copy_(torch.cat([gwf[:, l0:], gwf[:, :l0]], dim=1))
        if not regather:
            ops.fold_head_bwd(head_w, mf, proj_w, proj_b, gwfold, gcfold, g_head_w, g_proj_w, g_proj_b, g_head_b)
        ops.embed_bwd(specs, None, batch, gbuf, zeros)
        return zeros


_PATHS = {"proj": _ProjPath, "rows": _RowsPath, "samples": _SamplesPath}


def choose_path(tables, hidden, proj, batch, ids_1d) -> str:
    """which of ``_PATHS`` a forward over ``batch`` samples takes: a function of shapes alone (CPU tensors will do).
    The two table-row paths want the switch on, one-dimensional ids and no table in sparse mode; the pinned kernel
    where the library has it, else the composed path where its row kernels take the widths."""
    if PROJECT_TABLES and ids_1d and not any(getattr(t, "_ctr_sparse", None) is not None for t in tables):
        if ops.NcfProj.supported(tables, hidden, proj, batch):
            return "proj"
        if _RowsPath.admits(tables, hidden, batch):
            return "rows"
    return "samples"


_N_ARGS = 7      # of _NeuralCFFunction, in front of the parameters


class _NeuralCFFunction(torch.autograd.Function):
    """inputs: user_idx, item_idx, err_flag, path (a key of ``_PATHS``), n_hidden, grad_mode (the caller's: it is off in
    here), counts (the model's ``ops.NcfCounts`` for the ``proj`` path), then the parameters in ``_Params.flat`` order"""

    @staticmethod
    def forward(ctx, user_idx, item_idx, err_flag, path, n_hidden, grad_mode, counts, *flat):
        p = _unpack(flat, n_hidden)
        wants_grad = any(ctx.needs_input_grad[_N_ARGS:])
        # needs_input_grad is True for parameters under torch.no_grad() too; without a graph there will be no backward, and
        # the proj forward then takes no ranks (the backward's bucketing needs them; they are returning atomics:
        # profiles/r03_rank_atomics.txt)
        training = grad_mode and wants_grad
        prob, saved, ctx.state = _PATHS[path].forward(p, user_idx, item_idx, err_flag, wants_grad, training, counts)
        ctx.path, ctx.n_hidden, ctx.n_saved = path, n_hidden, len(saved)
        ctx.save_for_backward(user_idx, item_idx, *saved, *flat)
        return prob

    @staticmethod
    def backward(ctx, gprob):
        user_idx, item_idx, *rest = ctx.saved_tensors
        p = _unpack(rest[ctx.n_saved:], ctx.n_hidden)
        zeros = _PATHS[ctx.path].backward(p, user_idx, item_idx, rest[:ctx.n_saved], ctx.state, gprob)
        return (None,) * _N_ARGS + _grads(zeros, p)


class NeuralCF(CtrModule):
    """``NeuralCF(num_user, num_item, mf_dim, layers)``;
    ``forward(user_indices, item_indices) -> (B,1)`` (reference
    model/neuralcf.py:8-59)."""

    def __init__(self, num_user, num_item, mf_dim, layers):
        super().__init__()
        self.GMF_Embedding_User = nn.Embedding(num_user, mf_dim)
        self.GMF_Embedding_Item = nn.Embedding(num_item, mf_dim)
        self.MLP_Embedding_User = nn.Embedding(num_user, int(layers[0] / 2))
        self.MLP_Embedding_Item = nn.Embedding(num_item, int(layers[0] / 2))
        for emb in (self.GMF_Embedding_User, self.GMF_Embedding_Item, self.MLP_Embedding_User,
                    self.MLP_Embedding_Item):
            xavier_normal_(emb.weight.data)
        self.dnn_network = nn.ModuleList([nn.Linear(a, b) for a, b in zip(layers[:-1], layers[1:])])
        self.relu = nn.ReLU()
        self.linear = nn.Linear(layers[-1], mf_dim)
        self.linear2 = nn.Linear(2 * mf_dim, 1)
        self.sigmoid = nn.Sigmoid()

    def _params(self) -> _Params:
        flat = [self.GMF_Embedding_User.weight, self.GMF_Embedding_Item.weight, self.MLP_Embedding_User.weight,
                self.MLP_Embedding_Item.weight]
        for lin in list(self.dnn_network) + [self.linear, self.linear2]:
            flat += [lin.weight, lin.bias]
        return _unpack(flat, len(self.dnn_network))

    def forward(self, user_indices, item_indices):
        p = self._params()
        self._need_device(p.tables[0], user_indices, item_indices)
        path = choose_path(p.tables, p.hidden, p.proj, user_indices.numel(), user_indices.dim() == 1)
        if path == "proj" and getattr(self, "_ncf_counts", None) is None:
            object.__setattr__(self, "_ncf_counts", ops.NcfCounts())
        out = _NeuralCFFunction.apply(user_indices.contiguous(), item_indices.contiguous(),
                                      self._err_flag(p.tables[0].device), path, len(p.hidden), torch.is_grad_enabled(),
                                      getattr(self, "_ncf_counts", None), *p.flat)
        self._raise_if_bad_index()
        return out

    def recommendation(self, num_users, num_items, chunk: int = 1 << 20):
        """score every (user, item) pair and rank: the result of the reference's per-user loop
        (model/neuralcf.py:61-72; 943 forward calls of 1682 samples) from a few forward calls over
        the whole user x item grid, ``chunk`` pairs at a time, ranked on the device"""
        dev = self.GMF_Embedding_User.weight.device
        scores = torch.empty((num_users, num_items), dtype=torch.float32, device=dev)
        with torch.no_grad():
            topn.forward_grid(scores, chunk, self.forward)
        return ops.topk_rows(scores, num_items).cpu().numpy()

    # ---- the user x item grid: row scorers and a bounded-workspace ranker (no gradients, training paths untouched)
    def _table_sizes(self):
        return self.GMF_Embedding_User.weight.shape[0], self.GMF_Embedding_Item.weight.shape[0]

    def score_rows(self, start: int, stop: int) -> torch.Tensor:
        """(stop - start, num_items) float32 device tensor, fresh and row-major: the probabilities of users
        [start, stop) against every item -- the ``scores(start, stop)`` callable ``ranking_metrics`` takes.  Not
        chunked: the caller chose the rows."""
        return _GridScorer(self).score_rows(start, stop)

    def score_grid(self, users=None) -> torch.Tensor:
        """(len(users), num_items) float32 probabilities for any 1-D list of user ids (repeats and any order allowed;
        an id outside the table raises IndexError); ``None``: every user.  Not chunked: the caller chose the rows."""
        return _GridScorer(self).score_grid(users)

    def recommend(self, users=None, n: int = 20, exclude=None) -> torch.Tensor:
        """(len(users), n) int64: the items with the highest probability, best first, ties by ascending item id.
        ``exclude``: an ``ObservedPairs`` whose pairs are left out (``ops.rank_mask``), or None; rows with fewer than
        ``n`` items left end in -1.  Users are scored in chunks, so the workspace stays bounded."""
        return _GridScorer(self).recommend(users, n, exclude)


def grid_path(tables, hidden, proj) -> str:
    """how ``score_rows`` / ``score_grid`` / ``recommend`` score a model of these shapes (CPU tensors will do):
    "grid" -- projected tables, folded head, then ``ctr_ncf_grid_scores`` -- where the library has that kernel,
    else "forward": the per-sample forward over ids generated chunk by chunk"""
    return "grid" if ops.ncf_grid_supported(tables, hidden, proj) else "forward"


_FORWARD_CHUNK = 1 << 20     # pairs per forward call of the "forward" path


class _GridScorer(UserGridScorer):
    """score rows of the user x item grid of one model: what does not depend on the rows -- the projected tables and the
    folded head of the "grid" path -- is made once per public call (``_shared``), and not once per chunk"""

    def __init__(self, model: NeuralCF):
        p = model._params()
        super().__init__(*model._table_sizes(), p.tables[0].device)
        self.model = model
        self.path = grid_path(p.tables, p.hidden, p.proj)

    def _shared(self):
        """the operands of ``ops.ncf_grid_scores`` by name (the tables alone on the "forward" path)"""
        p = self.model._params()
        sh = Params(tables=tuple(t.detach() for t in p.tables))
        self.model._need_device(sh.tables[0])
        if self.path == "grid":
            gmf_u, gmf_i, mlp_u, mlp_i = sh.tables
            half = mlp_u.shape[1]
            w0, b0 = p.hidden[0].weight.detach(), p.hidden[0].bias.detach()
            sh.p_u = ops.linear_fwd(mlp_u, w0[:, :half], None)
            sh.p_i = ops.linear_fwd(mlp_i, w0[:, half:], b0)
            sh.layers = [Layer(layer.weight.detach(), layer.bias.detach(), layer.act) for layer in p.hidden[1:]]
            sh.wfold, sh.cfold = ops.fold_head_fwd(p.head[0].detach(), gmf_u.shape[1], p.proj[0].detach(),
                                                   p.proj[1].detach(), p.head[1].detach())
        return sh

    def _scores(self, users, start, stop, sh) -> torch.Tensor:
        gmf_u, gmf_i = sh.tables[:2]
        rows = users.numel() if users is not None else stop - start
        if self.path == "grid":
            return ops.ncf_grid_scores(sh.p_u, sh.p_i, gmf_u, gmf_i, sh.layers, sh.wfold, sh.cfold,
                                       users=users, user0=start, rows=rows, act=ACT_SIGMOID)
        out = torch.empty((rows, self.num_items), dtype=torch.float32, device=self.device)
        topn.forward_grid(out, _FORWARD_CHUNK,
                          lambda r, i: self.model.forward(users[r] if users is not None else r + start, i))
        return out
