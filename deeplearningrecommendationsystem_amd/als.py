"""ALS: matrix factorisation by alternating least squares, in closed form, for three objectives.

``objective="implicit"`` (Hu, Koren & Volinsky 2008, "iALS") over ALL U x I cells, ``reg > 0``::

    L(P, Q) = sum_{u,i} c_ui (y_ui - <p_u, q_i>)^2 + reg (|P|_F^2 + |Q|_F^2)

  * ``fit(ObservedPairs)``: 0/1 preferences ``y_ui`` with one confidence ``c_ui = 1 + alpha y_ui``.  A user half-sweep
    fixes Q, forms ``G = Q^T Q`` once and solves, for every user,
    ``(G + alpha sum_{i in N(u)} q_i q_i^T + reg I) p_u = (1 + alpha) sum_{i in N(u)} q_i`` exactly.
  * ``fit(Interactions)``: a value ``v_ui >= 0`` per stored pair (a count, a dwell time), ``y_ui = 1`` for every stored
    pair and ``c_ui = 1 + alpha v_ui`` (a stored pair with ``v = 0`` is an observation of confidence 1):
    ``(G + alpha sum v_ui q_i q_i^T + reg I) p_u = sum (1 + alpha v_ui) q_i``.

``objective="explicit"`` (Zhou et al. 2008, "ALS-WR"): least squares over the observed cells only, ratings of any sign
from an ``Interactions``, the regulariser weighted by the list lengths ``n_u`` / ``n_i``::

    L(P, Q) = sum_obs (v_ui - <p_u, q_i>)^2 + reg (sum_u n_u |p_u|^2 + sum_i n_i |q_i|^2)
    (sum_{i in N(u)} q_i q_i^T + reg n_u I) p_u = sum_{i in N(u)} v_ui q_i          -- no Gram, ``alpha`` is not read

An item half-sweep is the same with the roles swapped, over the transposed CSR.  No sampler, no learning rate, no
optimizer state.  The systems are assembled on the fp32 matrix cores and factorised in LDS (csrc/als.hip), one workgroup
per row: no (rows, k, k) tensor exists.  A row with an empty list gets exact zeros.

Not here: biases, a conjugate-gradient solver, k above 128 or not a multiple of 16, rows split over workgroups, several
devices.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib, ops, topn
from .data import Interactions, ObservedPairs
from .model._grid import UserGridScorer

__all__ = ["ALS"]

_LOSS_PAIRS = 1 << 20     # observed pairs per chunk of loss()


class _Side:
    """one CSR with the plan of its half-sweep: the rows by descending list length (stable), so that the tail of a
    launch is one long row and not a late-starting one.  Built once per CSR; results do not depend on it."""

    def __init__(self, observed):
        weighted = isinstance(observed, Interactions)
        self.pairs: ObservedPairs = observed.pairs if weighted else observed
        self.values = observed.values if weighted else None      # aligned with pairs.indices; None: a set
        self.plan = torch.argsort(self.pairs.indptr.diff(), descending=True, stable=True).contiguous()


def _pairs_of(observed: ObservedPairs):
    rows = torch.repeat_interleave(torch.arange(observed.num_users, device=observed.indptr.device),
                                   observed.indptr.diff())
    return rows, observed.indices.to(torch.int64)


class _Scorer(UserGridScorer):
    """raw dots ``P[rows] Q^T`` (no sigmoid: it would tie large scores)"""

    def __init__(self, model: "ALS"):
        super().__init__(model.num_users, model.num_items, model.P.device)
        self.model = model

    def _scores(self, users, start, stop, shared):
        P, Q = self.model.P, self.model.Q
        rows = P[start:stop] if users is None else P.index_select(0, users)
        return ops.linear_fwd(rows.contiguous(), Q, None)


class ALS:
    """``ALS(num_users, num_items, k=64, reg=0.1, alpha=40.0, seed=0, objective="implicit")``: ``P`` (num_users, k)
    and ``Q`` (num_items, k) are plain float32 device tensors (nothing is differentiated), initialised N(0, 0.01) from
    a ``np.random.RandomState(seed)`` that draws P before Q.  ``objective``: ``"implicit"`` or ``"explicit"`` (module
    docstring)."""

    def __init__(self, num_users: int, num_items: int, k: int = 64, reg: float = 0.1, alpha: float = 40.0,
                 seed: Optional[int] = 0, device="cuda", objective: str = "implicit"):
        if objective not in ("implicit", "explicit"):
            raise ValueError(f"objective must be 'implicit' or 'explicit', got {objective!r}")
        self.objective = objective
        if num_users < 1 or num_items < 1:
            raise ValueError("num_users and num_items must be positive")
        if not ops.als_supported(k):
            raise ValueError(f"k = {k} is not a multiple of 16 in [16, {ops.ALS_MAX_DIM}] (CTR_ALS_MAX_DIM)")
        if not float(reg) > 0.0 or not np.isfinite(reg):
            raise ValueError(f"reg = {reg} must be positive: it keeps every system positive definite")
        if not float(alpha) >= 0.0 or not np.isfinite(alpha):
            raise ValueError(f"alpha = {alpha} must not be negative")
        self.num_users, self.num_items, self.k = int(num_users), int(num_items), int(k)
        self.reg, self.alpha = float(reg), float(alpha)
        rs = np.random.RandomState(seed)
        p = rs.normal(0.0, 0.01, (self.num_users, self.k))
        q = rs.normal(0.0, 0.01, (self.num_items, self.k))
        self.P = torch.from_numpy(p).to(device=device, dtype=torch.float32)
        self.Q = torch.from_numpy(q).to(device=device, dtype=torch.float32)
        self._users: Optional[_Side] = None     # CSR over users, lists of items
        self._items: Optional[_Side] = None     # the transposed CSR
        self._flag = None

    # ------------------------------------------------------------------ training
    def fit(self, observed, sweeps: int = 10) -> "ALS":
        """``sweeps`` sweeps over ``observed`` -- an ``ObservedPairs`` (implicit: one confidence) or an ``Interactions``
        (implicit: values >= 0 as confidences; explicit: ratings); builds the transposed CSR and both plans once"""
        if (observed.num_users, observed.num_items) != (self.num_users, self.num_items):
            raise ValueError(f"observed was built for {observed.num_users} x {observed.num_items}, the model is "
                             f"{self.num_users} x {self.num_items}")
        if int(sweeps) < 0:
            raise ValueError("sweeps must not be negative")
        self._check(observed)
        if isinstance(observed, Interactions):
            _lib.require_device(self.P, observed.values)
            self._users = _Side(observed)
            self._items = _Side(observed.transpose())
        else:
            _lib.require_device(self.P, observed.indptr)
            users, items = _pairs_of(observed)
            self._users = _Side(observed)
            self._items = _Side(ObservedPairs(items, users, self.num_items, self.num_users))
        for _ in range(int(sweeps)):
            self.sweep()
        return self

    def sweep(self) -> None:
        """one user half-sweep, then one item half-sweep"""
        self.solve_users()
        self.solve_items()

    def solve_users(self, users=None) -> Optional[torch.Tensor]:
        """solve the rows ``users`` of P (any 1-D id list; ``None``: all) against the current Q and store them in P.
        Returns a fresh (len(users), k) tensor of the solved rows in the order of ``users``; with ``None`` nothing is
        copied and the return is None: the rows are ``model.P``."""
        return self._half(self._need(self._users), self.Q, self.P, users, self.num_users)

    def solve_items(self, items=None) -> Optional[torch.Tensor]:
        """the same for the rows ``items`` of Q against the current P (``None``: all, stored in ``model.Q``)"""
        return self._half(self._need(self._items), self.P, self.Q, items, self.num_items)

    def fold_in(self, new_observed) -> torch.Tensor:
        """(new_users, k): the factors of NEW users from their item lists (an ``ObservedPairs`` or an ``Interactions``
        over the same items as ``fit`` takes them, any number of users), solved against the current Q.  P and Q are
        untouched."""
        if new_observed.num_items != self.num_items:
            raise ValueError(f"new_observed has {new_observed.num_items} items, the model {self.num_items}")
        self._check(new_observed)
        return self._solve(_Side(new_observed), self.Q, None)

    def _check(self, observed) -> None:
        """what the objective takes: explicit needs values; confidences must not be negative"""
        if not isinstance(observed, (ObservedPairs, Interactions)):
            raise TypeError("ALS: the observations must be an ObservedPairs or an Interactions")
        if self.objective == "explicit":
            if not isinstance(observed, Interactions):
                raise ValueError("ALS(objective='explicit') needs an Interactions: ratings that are all ones are "
                                 "degenerate")
        elif isinstance(observed, Interactions) and len(observed) and bool((observed.values < 0).any()):
            raise ValueError("ALS(objective='implicit'): a negative value would be a confidence below 1 + alpha * 0; "
                             "values must not be negative")

    def _need(self, side):
        if side is None:
            raise RuntimeError("the observed pairs are needed: call fit(observed) first")
        return side

    def _half(self, side: _Side, fixed, solved, ids, num_rows):
        if ids is None:
            out = self._solve(side, fixed, side.plan)
            solved.index_copy_(0, side.plan, out)
            return None
        rows = topn.users_tensor(ids, num_rows, solved.device)      # IndexError for an id outside the table
        out = self._solve(side, fixed, rows)
        solved.index_copy_(0, rows, out)      # a repeated id carries the same row every time
        return out

    def _solve(self, side: _Side, fixed, rows):
        if self._flag is None:
            _lib.require_device(fixed)
            self._flag = torch.zeros(1, dtype=torch.int32, device=fixed.device)
        pairs = side.pairs
        if self.objective == "explicit":      # observed cells only: no Gram launch, reg times the list length
            out = ops.als_solve_rows_weighted(fixed, None, pairs.indptr, pairs.indices, side.values, (1.0, 0.0),
                                              (0.0, 1.0), 0.0, self.reg, rows=rows, err_flag=self._flag)
        elif side.values is not None:         # c = 1 + alpha v, preference 1
            out = ops.als_solve_rows_weighted(fixed, ops.als_gram(fixed), pairs.indptr, pairs.indices, side.values,
                                              (0.0, self.alpha), (1.0, self.alpha), self.reg, rows=rows,
                                              err_flag=self._flag)
        else:
            gram = ops.als_gram(fixed)
            out = ops.als_solve_rows(fixed, gram, pairs.indptr, pairs.indices, self.reg, self.alpha, rows=rows,
                                     err_flag=self._flag)
        bits = int(self._flag.item())      # read once per half-sweep
        if bits:
            self._flag.zero_()
            if bits & ops.ALS_ERR_INDEX:
                raise IndexError("ALS: an id of the observed pairs is outside the table it indexes")
            raise FloatingPointError("ALS: a pivot was not a positive finite number (a NaN or Inf in a table?)")
        return out

    # ------------------------------------------------------------------ the objective
    @torch.no_grad()
    def loss(self) -> float:
        """L(P, Q) in float64 without a U x I tensor, with ``s`` the dot of an observed pair and ``v`` its value (1 for
        an ``ObservedPairs``).  Implicit: ``<P^T P, Q^T Q> + sum_obs((1 + alpha v)(1 - s)^2 - s^2) + reg (|P|^2 +
        |Q|^2)``; explicit: ``sum_obs (v - s)^2 + reg (sum_u n_u |p_u|^2 + sum_i n_i |q_i|^2)``"""
        side = self._need(self._users)
        P, Q = self.P.double(), self.Q.double()
        if self.objective == "explicit":
            n_u = side.pairs.indptr.diff().double()
            n_i = self._need(self._items).pairs.indptr.diff().double()
            total = self.reg * ((n_u * P.square().sum(1)).sum() + (n_i * Q.square().sum(1)).sum())
        else:
            total = (P.T @ P).mul_(Q.T @ Q).sum() + self.reg * (P.square().sum() + Q.square().sum())
        users, items = _pairs_of(side.pairs)
        for s in range(0, users.numel(), _LOSS_PAIRS):
            dots = (P[users[s:s + _LOSS_PAIRS]] * Q[items[s:s + _LOSS_PAIRS]]).sum(1)
            v = None if side.values is None else side.values[s:s + _LOSS_PAIRS].double()
            if self.objective == "explicit":
                total = total + (v - dots).square().sum()
            else:
                conf = 1.0 + self.alpha if v is None else 1.0 + self.alpha * v
                total = total + (conf * (1.0 - dots).square() - dots.square()).sum()
        return float(total.item())

    # ------------------------------------------------------------------ scoring
    @torch.no_grad()
    def predict(self, users, items) -> torch.Tensor:
        """(N,) float32: the raw dots ``<p_u, q_i>`` of N (user, item) pairs -- the predicted rating of the explicit
        objective, the predicted preference of the implicit one.  IndexError for an id outside the tables."""
        u = topn.users_tensor(users, self.num_users, self.P.device)
        i = topn.users_tensor(items, self.num_items, self.Q.device)
        if u.shape != i.shape:
            raise ValueError("predict(): users and items must have one length")
        return (self.P[u] * self.Q[i]).sum(1)

    def score_rows(self, start: int, stop: int) -> torch.Tensor:
        """(stop - start, num_items) float32 device tensor, fresh and row-major: ``<p_u, q_i>`` of users [start, stop)
        against every item -- the ``scores(start, stop)`` callable ``ranking_metrics`` takes"""
        return _Scorer(self).score_rows(start, stop)

    def score_grid(self, users=None) -> torch.Tensor:
        """(len(users), num_items) float32 scores for any 1-D list of user ids; ``None``: every user"""
        return _Scorer(self).score_grid(users)

    def recommend(self, users=None, n: int = 20, exclude=None) -> torch.Tensor:
        """(len(users), n) int64: the items with the highest score, best first, ties by ascending item id.
        ``exclude``: an ``ObservedPairs`` whose pairs are left out, or None; rows with fewer than ``n`` items left end
        in -1."""
        return _Scorer(self).recommend(users, n, exclude)
