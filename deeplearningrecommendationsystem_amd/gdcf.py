"""GDCF: the reference's GDCF_Final.py, matrix factorisation trained on the full implicit matrix, as a library.

The reference forms ``pre = P @ Q`` over all users x items, takes ``BCEWithLogitsLoss`` (mean) against the 0/1 matrix,
so every unobserved pair is a negative, and steps ``torch.optim.Adam([P, Q], lr)``.  Here the loss and both gradients
come from two fused fp32 matrix-core passes (csrc/gdcf.hip) that never write an m x n tensor:

* ``model(matrix)`` returns the loss; with grad enabled the forward (row pass) also forms dP, the backward runs the
  column pass for dQ.  A frozen ``P`` or ``Q`` skips its product;
* ``recommend(n=50)`` ranks all items by ``P Q^T`` (ties by ascending item id).  Like the reference's evaluation it
  does not exclude training items unless ``exclude_rated=True``.

Deliberate deviations: float32 rather than float64 arithmetic; matrix columns are item ids (the reference's ``pivot``
drops items that never occur in training).  ``Q`` is (num_items, k), item-major like the package's embedding tables,
where the reference keeps ``Q.T``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops, topn
from .cf import ImplicitMatrix

__all__ = ["GDCF"]


class _GDCFLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, Q, matrix):
        loss, gp = ops.gdcf_rows(P, Q, matrix.data, grad=ctx.needs_input_grad[0])
        ctx.matrix = matrix
        ctx.save_for_backward(P, Q, gp)
        return loss

    @staticmethod
    def backward(ctx, gout):
        P, Q, gp = ctx.saved_tensors
        gout = gout.to(torch.float32)
        dp = gp * gout if ctx.needs_input_grad[0] else None
        dq = ops.gdcf_cols(P, Q, ctx.matrix.transposed(), gout) if ctx.needs_input_grad[1] else None
        return dp, dq, None


class GDCF(torch.nn.Module):
    """P (num_users, k) and Q (num_items, k), initialised U[0, 1) as ``np.random.rand`` (the reference's lines 32-33;
    ``seed`` seeds a ``np.random.RandomState``, which then draws P before Q)."""

    def __init__(self, num_users: int, num_items: int, k: int = 100, seed: Optional[int] = None, device="cuda"):
        super().__init__()
        if num_users < 1 or num_items < 1:
            raise ValueError("num_users and num_items must be positive")
        if not 1 <= k <= ops.GDCF_MAX_DIM:
            raise ValueError(f"k = {k} outside [1, {ops.GDCF_MAX_DIM}] (CTR_GDCF_MAX_DIM)")
        rs = np.random.RandomState(seed)
        p = rs.rand(num_users, k)
        q = rs.rand(num_items, k)
        self.P = torch.nn.Parameter(torch.from_numpy(p).to(device=device, dtype=torch.float32))
        self.Q = torch.nn.Parameter(torch.from_numpy(q).to(device=device, dtype=torch.float32))
        self.matrix: Optional[ImplicitMatrix] = None

    def forward(self, matrix: ImplicitMatrix) -> torch.Tensor:
        """BCEWithLogitsLoss (mean) of ``P Q^T`` against the whole 0/1 matrix, a 0-dim float32 tensor"""
        if (matrix.num_users, matrix.num_items) != (self.P.shape[0], self.Q.shape[0]):
            raise ValueError(f"matrix is {matrix.num_users} x {matrix.num_items}, the model "
                             f"{self.P.shape[0]} x {self.Q.shape[0]}")
        self.matrix = matrix
        if torch.is_grad_enabled() and (self.P.requires_grad or self.Q.requires_grad):
            return _GDCFLoss.apply(self.P, self.Q, matrix)
        return ops.gdcf_rows(self.P.detach(), self.Q.detach(), matrix.data, grad=False)[0]

    @torch.no_grad()
    def recommend(self, users=None, n: int = 50, exclude_rated: bool = False) -> torch.Tensor:
        """(len(users), n) int64: items by ``P[u] . Q[i]`` descending, ties by ascending item id.  With
        ``exclude_rated`` the items rated in the last matrix passed to ``forward`` are left out and short rows end
        in -1.  Users are scored in chunks, so the workspace stays bounded."""
        if n < 1:
            raise ValueError("n must be at least 1")
        P, Q = self.P.detach(), self.Q.detach()
        num_items = Q.shape[0]
        if exclude_rated and self.matrix is None:
            raise RuntimeError("exclude_rated needs the interaction matrix: call the model on it first")
        u = topn.users_tensor(users, P.shape[0], P.device)

        def chunk_scores(s, e):
            scores = ops.linear_fwd(P.index_select(0, u[s:e]), Q, None)
            if not exclude_rated:
                return scores, None
            scores.masked_fill_(self.matrix.data.index_select(0, u[s:e])[:, :num_items] != 0, float("-inf"))
            return scores, num_items - torch.isneginf(scores).sum(1)
        return topn.top_n(u.numel(), num_items, n, chunk_scores, P.device)
