"""The chunked top-n ranker behind every ``recommend()`` and what its callers share: a model scores a chunk of rows
against every item, ``top_n`` ranks it with ``ctr_topk_rows``, pads with -1 and stitches.  Depends on no model."""
from __future__ import annotations

import torch

from . import ops

SCORE_CHUNK_FLOATS = 1 << 27    # float32 scores per chunk (512 MB)
MAX_ROWS = 65535                # rows per chunk: the y extent of a launch grid


def chunk_rows(num_items: int) -> int:
    return max(1, min(MAX_ROWS, SCORE_CHUNK_FLOATS // num_items))


def users_tensor(users, num_users: int, device) -> torch.Tensor:
    """``users`` (None: every user) as a validated 1-D int64 tensor on ``device``"""
    if users is None:
        return torch.arange(num_users, device=device)
    u = torch.as_tensor(users, dtype=torch.int64).reshape(-1).to(device)
    if u.numel() and (int(u.min()) < 0 or int(u.max()) >= num_users):
        raise IndexError("a user id is outside [0, num_users)")
    return u


def excluded_rows(observed, users):
    """the rows ``users`` of an ``ObservedPairs`` as the CSR ``ops.rank_mask`` takes: (offsets (len + 1), ids) int64"""
    lo = observed.indptr[users]
    lens = observed.indptr[users + 1] - lo
    off = torch.zeros(users.numel() + 1, dtype=torch.int64, device=users.device)
    torch.cumsum(lens, 0, out=off[1:])
    row = torch.repeat_interleave(torch.arange(users.numel(), device=users.device), lens)
    at = torch.arange(row.numel(), device=users.device) - off[row] + lo[row]
    return off, observed.indices[at].to(torch.int64)


def top_n(rows: int, num_items: int, n: int, chunk_scores, device) -> torch.Tensor:
    """(rows, n) int64: every row's ``n`` best items, best first, ties by ascending item id, -1 where a row has fewer
    than ``n`` items left in.  ``chunk_scores(s, e)`` is called for consecutive ranges that cover [0, rows) once, in
    order, and returns ``(scores, kept)``: a fresh row-major (e - s, num_items) float32 device tensor in which every
    left-out item already ranks last, and an (e - s,) int64 tensor of how many items of each row are left in (None:
    all of them)."""
    if n < 1:
        raise ValueError("n must be at least 1")
    out = torch.full((rows, n), -1, dtype=torch.int64, device=device)
    take = min(n, num_items)
    place = torch.arange(take, device=device)
    chunk = chunk_rows(num_items)
    for s in range(0, rows, chunk):
        e = min(rows, s + chunk)
        scores, kept = chunk_scores(s, e)
        idx = ops.topk_rows(scores, take)
        if kept is not None:        # the left-out items rank last: what lies past a row's survivors is padding
            idx = idx.masked_fill(place[None, :] >= kept[:, None], -1)
        out[s:e, :take] = idx
    return out


def forward_grid(out: torch.Tensor, pairs_per_call: int, forward) -> None:
    """fill the row-major (rows, num_items) ``out`` from a per-sample forward: ``forward(row_index, item_index)``, two
    1-D int64 tensors, scores the pairs of one flat range of the grid, ``pairs_per_call`` pairs a call"""
    rows, num_items = out.shape
    flat = out.view(-1)
    for lo in range(0, rows * num_items, pairs_per_call):
        k = torch.arange(lo, min(lo + pairs_per_call, rows * num_items), device=out.device)
        r = torch.div(k, num_items, rounding_mode="floor")
        flat[lo:lo + k.numel()] = forward(r, k - r * num_items).view(-1)
