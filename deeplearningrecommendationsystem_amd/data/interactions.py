"""Observed (user, item) pairs WITH a value each -- a play count, a dwell time, a rating -- as the CSR of
``ObservedPairs`` and a float32 array beside it: what ``ALS`` takes for per-pair confidences and for explicit ratings.
"""
from __future__ import annotations

import torch

from .loader import ObservedPairs

_DUPLICATES = ("sum", "mean", "error")


def _segment_sums(values, segment, counts):
    """(segments,) float32 sums of the runs of ``values`` (run of position p: ``segment[p]``, ascending; ``counts``
    their lengths) by ONE fixed binary tree per run: in pass s = 1, 2, 4, ... the element of rank r, r a multiple of 2s,
    takes in the element of rank r + s.  Every pass is an elementwise add onto distinct targets, so the result depends
    on the run's values and their order alone -- the same bits on every call and on every device."""
    values = values.clone()
    start = torch.cumsum(counts, 0) - counts
    rank = torch.arange(values.numel(), device=values.device) - start[segment]
    length = counts[segment]
    stride, longest = 1, int(counts.max())
    while stride < longest:
        at = torch.nonzero((rank % (2 * stride) == 0) & (rank + stride < length)).flatten()
        values[at] += values[at + stride]
        stride *= 2
    return values[start]


class Interactions:
    """``Interactions(users, items, values, num_users, num_items, duplicates="sum")``

    ``pairs``   an ``ObservedPairs``: the SAME ``indptr`` / ``indices`` that ``ObservedPairs(users, items, num_users,
                num_items)`` builds, so it serves wherever one is taken (``exclude=``)
    ``values``  (nnz,) float32, ``values[p]`` belongs to ``pairs.indices[p]``

    ``users`` / ``items`` are 1-D int64 tensors, or sequences of them to concatenate; ``values`` float32 of the same
    length (or a sequence likewise).  Several values of one pair are reduced as ``duplicates`` says: ``"sum"`` (counts
    add), ``"mean"`` (a rating given twice) or ``"error"`` (ValueError).  The reduction is a stable sort and a segmented
    sum by a fixed tree over each pair's values in the order they were given -- no float atomics, no library reduction
    whose order is its own -- so two calls give the same bits, on the host and on the device alike.  A non-finite
    value is ValueError, an id outside the tables IndexError; the size limits are those of ``ObservedPairs``.  Built
    once with torch ops on the device the ids live on."""

    def __init__(self, users, items, values, num_users, num_items, duplicates: str = "sum"):
        if duplicates not in _DUPLICATES:
            raise ValueError(f"Interactions: duplicates must be one of {_DUPLICATES}, got {duplicates!r}")
        users = torch.cat([t.reshape(-1) for t in users]) if isinstance(users, (list, tuple)) else users
        items = torch.cat([t.reshape(-1) for t in items]) if isinstance(items, (list, tuple)) else items
        values = torch.cat([t.reshape(-1) for t in values]) if isinstance(values, (list, tuple)) else values
        self.pairs = ObservedPairs(users, items, num_users, num_items)      # checks the ids and the sizes
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.shape != users.shape:
            raise ValueError("Interactions: values must be a 1-D float32 tensor of the length of users and items")
        if values.device != users.device:
            raise ValueError("Interactions: values must live on the device of the ids")
        if values.numel() and not bool(torch.isfinite(values).all()):
            raise ValueError("Interactions: values must be finite")
        keys = users * self.pairs.num_items + items
        order = torch.argsort(keys, stable=True)      # by user, then item, duplicates in the order they were given
        values = values[order]
        if len(self.pairs) != keys.numel():
            if duplicates == "error":
                raise ValueError(f"Interactions: {keys.numel() - len(self.pairs)} repeated (user, item) pairs")
            _, segment, counts = torch.unique_consecutive(keys[order], return_inverse=True, return_counts=True)
            values = _segment_sums(values, segment, counts)
            if duplicates == "mean":
                values = values / counts.to(torch.float32)
        self.values = values.contiguous()

    num_users = property(lambda self: self.pairs.num_users)
    num_items = property(lambda self: self.pairs.num_items)

    def __len__(self):
        return len(self.pairs)

    def transpose(self) -> "Interactions":
        """the Interactions of (items, users): the transposed CSR with the values carried along"""
        p = self.pairs
        users = torch.repeat_interleave(torch.arange(p.num_users, device=p.indptr.device), p.indptr.diff())
        return Interactions(p.indices.to(torch.int64), users, self.values, p.num_items, p.num_users, "error")
