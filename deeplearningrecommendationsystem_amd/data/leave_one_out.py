"""Candidates of the sampled leave-one-out evaluation: every held-out positive with ``negatives`` DISTINCT items the
user has not observed, drawn once on the device (``ctr_eval_candidates``, csrc/group_eval.hip) and the same for every
epoch -- the "1 positive + 99 negatives" protocol of the NeuralCF paper.  The loader's own negatives
(``DeviceLoader(..., negatives=k)``) are drawn per slot and may repeat within a group; these cannot, because they are
the first k eligible values of a per-group permutation of the items (the definition stands in the kernel file's header
comment), and the draw with k' < k is a prefix of the draw with k.

The flattened candidates -- group g at positions g (1 + k) .. g (1 + k) + k, the positive first -- feed an ordinary
unshuffled ``DeviceLoader``, so the three model families get their joins from the existing loader, and
``Trainer.rank_epoch`` turns the gathered predictions into HR@c / NDCG@c / MRR (``evaluator.sampled``).

Memory: 8 B of candidate, 8 B of repeated user id and 4 B of rating per candidate, 20 B; at ml-20m shape (138 493
users, one positive each, k = 99) that is 277 MB.  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from .. import _lib
from .loader import DeviceLoader, ObservedPairs


class LeaveOneOut:
    """``LeaveOneOut(users, items, observed, negatives=99, seed=0)``: ``users`` / ``items`` the N held-out positives
    (1-D int64 device tensors), ``observed`` the ``ObservedPairs`` no negative may come from (train | valid | test).

    ``candidates`` (N, 1 + k) int64, column 0 the positive; ``users`` / ``items`` (N (1 + k),) and ``ratings``
    (N (1 + k), 1), 1 at every group's first slot and 0 elsewhere, are the flattened samples.  The constructor raises
    ValueError when the longest observed row could leave fewer than ``negatives`` eligible items (one sync);
    ``check()`` surfaces what the draw itself flagged."""

    def __init__(self, users, items, observed: ObservedPairs, negatives: int = 99, seed: int = 0):
        from .. import ops
        _lib.require_device(users, items, observed.indptr, observed.indices)
        if users.dtype != torch.int64 or items.dtype != torch.int64 or users.dim() != 1 or users.shape != items.shape:
            raise ValueError("LeaveOneOut: users and items must be 1-D int64 tensors of one length")
        if users.shape[0] < 1:
            raise ValueError("LeaveOneOut: no held-out positive")
        self.negatives, self.seed = int(negatives), int(seed)
        if not 1 <= self.negatives <= ops.GROUP_MAX_K:
            raise ValueError(f"LeaveOneOut: negatives must be in [1, {ops.GROUP_MAX_K}]")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError("LeaveOneOut: seed must fit an unsigned 64-bit integer")
        longest = int(observed.indptr.diff().max()) if len(observed) else 0
        if observed.num_items - 1 - longest < self.negatives:
            raise ValueError(f"LeaveOneOut: {self.negatives} negatives asked for, but a user has observed {longest} of "
                             f"{observed.num_items} items")
        self.observed, self.device = observed, users.device
        self.num_groups = users.shape[0]
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        per = 1 + self.negatives
        self.candidates = ops.eval_candidates(users.contiguous(), items.contiguous(), observed.indptr, observed.indices,
                                              observed.num_users, observed.num_items, self.negatives, self.seed,
                                              self._err, self._fail)
        self.users = users.repeat_interleave(per)
        self.items = self.candidates.view(-1)
        self.ratings = torch.zeros((self.num_groups, per), dtype=torch.float32, device=self.device)
        self.ratings[:, 0] = 1.0
        self.ratings = self.ratings.view(-1, 1)

    @property
    def num_samples(self):
        return self.num_groups * (1 + self.negatives)

    def check(self):
        """raise the IndexError of a user id outside the observed set's rows (or of an inconsistent CSR row), or the
        RuntimeError of a group that found fewer than ``negatives`` eligible items"""
        if int(self._err.item()):
            raise IndexError("index out of range in self")
        if int(self._fail.item()):
            raise RuntimeError("LeaveOneOut: a user has fewer unobserved items than negatives were asked for")

    # -- loaders: unshuffled, no drawn negatives, the groups contiguous -----------------------------------------
    def pairs(self, batch_size) -> DeviceLoader:
        """MF / NeuralCF: batches ``(user_idx, item_idx), rating``"""
        return DeviceLoader.pairs(self.users, self.items, self.ratings, batch_size, shuffle=False)

    def features(self, assembler, batch_size) -> DeviceLoader:
        """feature models: batches ``(x (B, assembler.width),), rating``"""
        return DeviceLoader.features(assembler, self.users, self.items, self.ratings, batch_size, shuffle=False)

    def sequences(self, history, batch_size) -> DeviceLoader:
        """DIN / DIEN: batches ``(hist (B, L), target (B,)), rating``, ``history`` one row per user"""
        return DeviceLoader.sequences(history, self.users, self.items, self.ratings, batch_size, shuffle=False)
