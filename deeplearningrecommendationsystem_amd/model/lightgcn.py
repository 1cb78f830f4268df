"""LightGCN (He et al. 2020): embeddings propagated over the user-item graph, MF's head on the propagated tables.

With R the (U, I) 0/1 matrix of the TRAIN pairs, ``S_U = diag(d_u^-1/2)`` and ``S_I = diag(d_i^-1/2)`` (0 for a row
without a pair)::

    E_U^(0) = user_embeddings.weight            E_I^(0) = item_embeddings.weight
    E_U^(l+1) = S_U R S_I E_I^(l)               E_I^(l+1) = S_I R^T S_U E_U^(l)
    F = mean_{l = 0..L} E^(l)                   prob(u, i) = sigmoid(<F_U[u], F_I[i]>)

Every product is one ``ops.graph_propagate`` call (csrc/graph_prop.hip) over the user CSR or its transpose.  The
propagation is linear and the normalised adjacency ``A = [[0, S_U R S_I], [S_I R^T S_U, 0]]`` is symmetric, so the
gradient of ``F = 1/(L+1) sum_l A^l E^(0)`` is ``1/(L+1) sum_l A^l gF``: the Horner recursion ``g <- gF/(L+1) + A g``,
L times -- the same 2L kernel calls, nothing saved but the graph, no atomics, bitwise reproducible gradients.

Not here: edge or message dropout, layer weights other than the mean, NGCF's transforms, the L2 term on the batch's ego
embeddings (the optimizer's ``weight_decay`` stands in), valued edges, several devices.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops, topn
from ..data import ObservedPairs
from ._base import CtrModule
from ._grid import UserGridScorer
from .mf import _FORWARD_CHUNK, _MFFunction
from .mf import grid_path as _mf_grid_path


class _Graph:
    """the two CSRs of one set of pairs with their degree scales and launch plans, built once"""

    def __init__(self, observed: ObservedPairs):
        dev = observed.indptr.device
        users = torch.repeat_interleave(torch.arange(observed.num_users, device=dev), observed.indptr.diff())
        items = observed.indices.to(torch.int64)
        self.users = observed
        self.items = ObservedPairs(items, users, observed.num_items, observed.num_users)      # the transposed CSR
        self.scale_u = _inv_sqrt_degree(self.users.indptr)
        self.scale_i = _inv_sqrt_degree(self.items.indptr)
        self.plan_u = ops.graph_plan(self.users.indptr)
        self.plan_i = ops.graph_plan(self.items.indptr)

    def step(self, e_u, e_i, flag):
        """(S_U R S_I e_i, S_I R^T S_U e_u): one layer, and -- the operator being symmetric -- one step of its adjoint"""
        new_u = ops.graph_propagate(e_i, self.users.indptr, self.users.indices, self.scale_i, self.scale_u,
                                    plan=self.plan_u, err_flag=flag)
        new_i = ops.graph_propagate(e_u, self.items.indptr, self.items.indices, self.scale_u, self.scale_i,
                                    plan=self.plan_i, err_flag=flag)
        return new_u, new_i


def _inv_sqrt_degree(indptr):
    degree = indptr.diff().to(torch.float32)
    return torch.where(degree > 0, degree.rsqrt(), torch.zeros_like(degree)).contiguous()


class _PropagateFunction(torch.autograd.Function):
    """(W_U, W_I) -> (F_U, F_I): one node over the two tables; nothing is saved between forward and backward"""

    @staticmethod
    def forward(ctx, w_u, w_i, graph, layers, flag):
        ctx.graph, ctx.layers, ctx.flag = graph, layers, flag
        e_u, e_i = w_u.contiguous(), w_i.contiguous()
        sum_u, sum_i = e_u.clone(), e_i.clone()
        for _ in range(layers):
            e_u, e_i = graph.step(e_u, e_i, flag)
            sum_u += e_u
            sum_i += e_i
        scale = 1.0 / (layers + 1)
        return sum_u.mul_(scale), sum_i.mul_(scale)

    @staticmethod
    def backward(ctx, gf_u, gf_i):
        scale = 1.0 / (ctx.layers + 1)
        g0_u, g0_i = gf_u.contiguous() * scale, gf_i.contiguous() * scale
        g_u, g_i = g0_u, g0_i
        for _ in range(ctx.layers):      # Horner: g <- gF / (L + 1) + A g, both sides carried whoever needs a gradient
            a_u, a_i = ctx.graph.step(g_u, g_i, ctx.flag)
            g_u, g_i = a_u.add_(g0_u), a_i.add_(g0_i)
        return (g_u if ctx.needs_input_grad[0] else None, g_i if ctx.needs_input_grad[1] else None, None, None, None)


class LightGCN(CtrModule):
    """``LightGCN(num_users, num_items, embedding_size=64, num_layers=3)``; ``set_graph(observed)`` once, then
    ``forward(user_indices, item_indices) -> (B,)`` probabilities: MF's forward signature, so the losses, ``Trainer``,
    ``rank_epoch`` and ``score_epoch`` take it as they take ``MatrixFactorization``.  ``num_layers = 0`` is MF."""

    def __init__(self, num_users: int, num_items: int, embedding_size: int = 64, num_layers: int = 3):
        super().__init__()
        if isinstance(num_layers, bool) or not isinstance(num_layers, int) or num_layers < 0:
            raise ValueError(f"num_layers = {num_layers!r} must be an integer and not negative")
        if num_layers > 0 and not ops.graph_supported(embedding_size):
            raise ValueError(f"embedding_size = {embedding_size!r} is not a multiple of 16 in [16, {ops.GRAPH_MAX_DIM}]: "
                             "the propagation kernel takes no other width")
        self.num_layers = num_layers
        self.user_embeddings = nn.Embedding(num_users, embedding_size)
        self.item_embeddings = nn.Embedding(num_items, embedding_size)
        xavier_normal_(self.user_embeddings.weight.data)
        xavier_normal_(self.item_embeddings.weight.data)
        object.__setattr__(self, "_graph", None)
        object.__setattr__(self, "_cache", None)      # (key, F_U, F_I) of the last propagation under no_grad

    # ---- the graph
    def set_graph(self, observed: ObservedPairs) -> "LightGCN":
        """the graph to propagate over: an ``ObservedPairs`` of the TRAIN pairs on the model's device.  Builds the
        transposed CSR, the degree scales ``d^-1/2`` (0 for a row without a pair) and both launch plans, once."""
        if not isinstance(observed, ObservedPairs):
            raise TypeError("LightGCN.set_graph: the graph must be an ObservedPairs")
        if (observed.num_users, observed.num_items) != self._table_sizes():
            raise ValueError(f"observed was built for {observed.num_users} x {observed.num_items}, the model is "
                             "{} x {}".format(*self._table_sizes()))
        self._need_device(self.user_embeddings.weight, observed.indptr)
        object.__setattr__(self, "_graph", _Graph(observed))
        object.__setattr__(self, "_cache", None)
        return self

    def _need_graph(self) -> _Graph:
        if self._graph is None:
            raise RuntimeError("the graph is needed: call set_graph(observed) first")
        return self._graph

    def propagate(self):
        """(F_U, F_I), differentiable in both weights.  Under ``no_grad`` the pair is cached until a weight changes (its
        ``_version``) or the graph does; with gradients enabled the cache is neither read nor written."""
        graph = self._need_graph()
        w_u, w_i = self.user_embeddings.weight, self.item_embeddings.weight
        if self.num_layers == 0:
            return w_u, w_i
        self._need_device(w_u, w_i)
        flag = self._err_flag(w_u.device)
        if torch.is_grad_enabled():
            return _PropagateFunction.apply(w_u, w_i, graph, self.num_layers, flag)
        key = (w_u._version, w_i._version, w_u.data_ptr(), w_i.data_ptr(), id(graph))
        if self._cache is None or self._cache[0] != key:
            pair = _PropagateFunction.apply(w_u.detach(), w_i.detach(), graph, self.num_layers, flag)
            object.__setattr__(self, "_cache", (key,) + tuple(pair))
        return self._cache[1], self._cache[2]

    def forward(self, user_indices: torch.Tensor, item_indices: torch.Tensor) -> torch.Tensor:
        f_u, f_i = self.propagate()
        self._need_device(f_u, user_indices, item_indices)
        out = _MFFunction.apply(f_u, f_i, user_indices.contiguous(), item_indices.contiguous(),
                                self._err_flag(f_u.device))
        self._raise_if_bad_index()
        return out

    # ---- the user x item grid: row scorers and a bounded-workspace ranker (no gradients)
    def _table_sizes(self):
        return self.user_embeddings.weight.shape[0], self.item_embeddings.weight.shape[0]

    def score_rows(self, start: int, stop: int) -> torch.Tensor:
        """(stop - start, num_items) float32 device tensor, fresh and row-major: the probabilities of users
        [start, stop) against every item -- the ``scores(start, stop)`` callable ``ranking_metrics`` takes"""
        return _GridScorer(self).score_rows(start, stop)

    def score_grid(self, users=None) -> torch.Tensor:
        """(len(users), num_items) float32 probabilities for any 1-D list of user ids; ``None``: every user"""
        return _GridScorer(self).score_grid(users)

    def recommend(self, users=None, n: int = 20, exclude=None) -> torch.Tensor:
        """(len(users), n) int64: the items with the highest probability, best first, ties by ascending item id.
        ``exclude``: an ``ObservedPairs`` whose pairs are left out, or None; rows with fewer than ``n`` items left end
        in -1.  Users are scored in chunks, so the workspace stays bounded."""
        return _GridScorer(self).recommend(users, n, exclude)


def grid_path(embedding_size) -> str:
    """how ``score_rows`` / ``score_grid`` / ``recommend`` score a model of this embedding size: "grid" --
    ``ctr_lowrank_grid_scores`` over the propagated tables -- where the library has that kernel, else "forward"""
    return _mf_grid_path(embedding_size)


class _GridScorer(UserGridScorer):
    """score rows of the user x item grid; the operands are the propagated tables, made (or found in the cache) once
    per public call"""

    row_blocks = 0

    def __init__(self, model: LightGCN):
        super().__init__(*model._table_sizes(), model.user_embeddings.weight.device)
        self.model = model
        self.path = grid_path(model.user_embeddings.weight.shape[1])

    def _shared(self):
        tables = tuple(t.detach() for t in self.model.propagate())
        self.model._need_device(*tables)
        return tables

    def _scores(self, users, start, stop, shared) -> torch.Tensor:
        rows = users.numel() if users is not None else stop - start
        if self.path == "grid":
            return ops.lowrank_grid_scores(*shared, None, None, users=users, user0=start, rows=rows,
                                           row_blocks=self.row_blocks)
        out = torch.empty((rows, self.num_items), dtype=torch.float32, device=self.device)
        topn.forward_grid(out, _FORWARD_CHUNK,
                          lambda r, i: self.model.forward(users[r] if users is not None else r + start, i))
        return out
