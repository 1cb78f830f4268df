"""Evaluation on the device: top-k ranking metrics (csrc/rank_eval.hip), sampled leave-one-out (csrc/group_eval.hip)
and score-level metrics (csrc/score_eval.hip)."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ._call import _call, _flat_f32, _flat_int, _i64


# ---------------------------------------------------------------------------
# top-k ranking evaluation (csrc/rank_eval.hip); the CSRs are (offsets (rows + 1), ids) int64 device tensors, the
# offsets already sliced to the rows of the call (they index ``ids`` absolutely)
# ---------------------------------------------------------------------------


RANK_MASK_BITS = _lib.CTR_RANK_MASK_BITS
RANK_ERR_OFFSETS, RANK_ERR_LENGTH, RANK_ERR_SURVIVOR, RANK_ERR_COUNT = (
    _lib.CTR_RANK_ERR_OFFSETS, _lib.CTR_RANK_ERR_LENGTH, _lib.CTR_RANK_ERR_SURVIVOR, _lib.CTR_RANK_ERR_COUNT)
RANK_MAX_ROWS = _lib.CTR_RANK_MAX_ROWS


_RANK_TABLE_SLOTS = 1 << 25   # hash-set workspace of rank_metrics_lists: at most 256 MB (or one user's table)


def rank_filter(rec: torch.Tensor, ex_off: torch.Tensor, ex_ids: torch.Tensor, err: torch.Tensor):
    """remove_itemid's compaction: (out (rows, len), out_len (rows,)); out[u, out_len[u]:] is unwritten (zeros)"""
    _i64(rec, ex_off, ex_ids)
    rows, length = rec.shape
    out = torch.zeros((rows, length), dtype=torch.int64, device=rec.device)
    out_len = torch.empty(rows, dtype=torch.int64, device=rec.device)
    _call("rank_filter", "ctr_rank_filter", lambda: (16 * rows * length, 0), _lib.ptr(rec) if rec.numel() else None, length,
          rows, length, ex_off.data_ptr(), _lib.ptr(ex_ids) if ex_ids.numel() else None, ex_ids.numel(),
          _lib.ptr(out) if out.numel() else None, length, out_len.data_ptr(), err.data_ptr(), _lib.stream_ptr())
    return out, out_len


def rank_metrics_lists(pred: torch.Tensor, pred_len: torch.Tensor, act_off: torch.Tensor, act_ids: torch.Tensor,
                       alen: torch.Tensor, k: int, err: torch.Tensor) -> torch.Tensor:
    """(rows, 7) float64 partials (same, rec, real, ap, dcg, idcg, rr) of explicit predicted rows"""
    _i64(pred, pred_len, act_off, act_ids, alen)
    rows, length = pred.shape
    slots = C.c_int64()
    _lib.check(_lib.load().ctr_rank_table_slots(k, length, C.byref(slots)), "ctr_rank_table_slots")
    cap = slots.value
    table = torch.empty(max(cap, min(rows, max(1, _RANK_TABLE_SLOTS // cap)) * cap), dtype=torch.int64,
                        device=pred.device)
    parts = torch.empty((rows, 7), dtype=torch.float64, device=pred.device)
    _call("rank_metrics_lists", "ctr_rank_metrics_lists", lambda: (8 * rows * length + 8 * act_ids.numel(), 0),
          _lib.ptr(pred) if pred.numel() else None, length, pred_len.data_ptr(), rows, length, act_off.data_ptr(),
          _lib.ptr(act_ids) if act_ids.numel() else None, act_ids.numel(), alen.data_ptr(), k, table.data_ptr(),
          table.numel(), parts.data_ptr(), err.data_ptr(), _lib.stream_ptr())
    return parts


def rank_mask(scores: torch.Tensor, ex_off: torch.Tensor, ex_ids: torch.Tensor, err: torch.Tensor) -> None:
    """write RANK_MASK_BITS over every excluded item of the (rows, n) float32 chunk, in place"""
    _lib.require_device(scores)
    _i64(ex_off, ex_ids)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError("rank_mask expects a row-major 2-D float32 tensor")
    rows, n = scores.shape
    _call("rank_mask", "ctr_rank_mask", lambda: (8 * ex_ids.numel() + 4 * ex_ids.numel(), 0), scores.data_ptr(),
          scores.stride(0), rows, n, ex_off.data_ptr(), _lib.ptr(ex_ids) if ex_ids.numel() else None, ex_ids.numel(),
          err.data_ptr(), _lib.stream_ptr())


def rank_metrics_scores(scores: torch.Tensor, top: torch.Tensor, k: int, act_off: torch.Tensor, act_ids: torch.Tensor,
                        alen: torch.Tensor, n_real: torch.Tensor, pad: torch.Tensor, parts: torch.Tensor,
                        err: torch.Tensor) -> None:
    """partials of masked score rows from their top-min(k, n) into ``parts`` (rows, 7) float64"""
    _lib.require_device(scores, parts)
    _i64(top, act_off, act_ids, alen, n_real, pad)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError("rank_metrics_scores expects a row-major 2-D float32 tensor")
    rows, n = scores.shape
    if parts.dtype != torch.float64 or parts.shape != (rows, 7) or not parts.is_contiguous():
        raise ValueError("partials: contiguous (rows, 7) float64")
    _call("rank_metrics_scores", "ctr_rank_metrics_scores", lambda: (4 * rows * n + 8 * top.numel() + 56 * rows, 0),
          scores.data_ptr(), scores.stride(0), rows, n, top.data_ptr(), top.shape[1], k, act_off.data_ptr(),
          _lib.ptr(act_ids) if act_ids.numel() else None, act_ids.numel(), alen.data_ptr(), n_real.data_ptr(),
          pad.data_ptr(), parts.data_ptr(), err.data_ptr(), _lib.stream_ptr())


# ---------------------------------------------------------------------------
# sampled leave-one-out evaluation (csrc/group_eval.hip)
# ---------------------------------------------------------------------------
GROUP_MAX_K = _lib.CTR_GROUP_MAX_K


def eval_candidates(users: torch.Tensor, items: torch.Tensor, indptr: torch.Tensor, indices: torch.Tensor,
                    num_users: int, num_items: int, k: int, seed: int, err: torch.Tensor, fail: torch.Tensor,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(N, 1 + k) int64 candidates: column 0 the held-out item, then k distinct items that are neither it nor observed
    for the user (``ctr_eval_candidates``).  ``out``: an (N, >= 1 + k) int64 tensor with unit inner stride to write
    into (columns past 1 + k are left alone); ``err`` / ``fail``: device int32 flags, raised and never cleared."""
    _i64(users, items, indptr)
    _lib.require_device(indices, err, fail, out)
    if users.dim() != 1 or users.shape != items.shape:
        raise ValueError("eval_candidates: users and items must be 1-D tensors of one length")
    if indices.dtype != torch.int32 or not indices.is_contiguous() or indptr.numel() != num_users + 1:
        raise ValueError("eval_candidates: indptr (num_users + 1) int64, indices contiguous int32")
    if not 1 <= int(k) <= GROUP_MAX_K:
        raise ValueError(f"eval_candidates: negatives = {k} outside [1, {GROUP_MAX_K}]")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("eval_candidates: seed must fit an unsigned 64-bit integer")
    n = users.shape[0]
    if out is None:
        out = torch.empty((n, 1 + k), dtype=torch.int64, device=users.device)
    elif out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != n or out.shape[1] < 1 + k or \
            (n > 0 and out.stride(1) != 1) or (n > 1 and out.stride(0) < 1 + k):
        raise ValueError("eval_candidates: out must be an (N, >= 1 + k) int64 tensor with unit inner stride")
    ld = out.stride(0) if n > 1 else max(out.shape[1], 1 + k)
    _call("eval_candidates", "ctr_eval_candidates", lambda: (16 * n + 8 * n * (1 + k), 0), _lib.ptr(users) if n else None,
          _lib.ptr(items) if n else None, n, indptr.data_ptr(), _lib.ptr(indices) if indices.numel() else None,
          indices.numel(), int(num_users), int(num_items), int(k), int(seed), _lib.ptr(out) if n else None, ld,
          err.data_ptr(), fail.data_ptr(), _lib.stream_ptr())
    return out


def group_rank(scores: torch.Tensor, k: int, hist: torch.Tensor, ranks: Optional[torch.Tensor] = None) -> None:
    """``ctr_group_rank``: scores (N, >= 1 + k) float32 with unit inner stride, slot 0 of a row the positive;
    ``hist`` (k + 1,) int64 is added to, ``ranks`` (N,) int32 (optional) receives every group's rank"""
    _lib.require_device(scores, hist, ranks)
    if not 1 <= int(k) <= GROUP_MAX_K:
        raise ValueError(f"group_rank: negatives = {k} outside [1, {GROUP_MAX_K}]")
    n = scores.shape[0] if scores.dim() == 2 else -1
    if scores.dtype != torch.float32 or n < 0 or scores.shape[1] < 1 + k or (n > 0 and scores.stride(1) != 1) or \
            (n > 1 and scores.stride(0) < 1 + k):
        raise ValueError("group_rank: scores must be an (N, >= 1 + k) float32 tensor with unit inner stride")
    if hist.dtype != torch.int64 or hist.shape != (k + 1,) or not hist.is_contiguous():
        raise ValueError("group_rank: hist must be a contiguous (k + 1,) int64 tensor")
    if ranks is not None and (ranks.dtype != torch.int32 or ranks.shape != (n,) or not ranks.is_contiguous()):
        raise ValueError("group_rank: ranks must be a contiguous (N,) int32 tensor")
    ld = scores.stride(0) if n > 1 else max(scores.shape[1], 1 + k)
    _call("group_rank", "ctr_group_rank", lambda: (4 * n * (1 + k) + (4 * n if ranks is not None else 0), 0),
          _lib.ptr(scores) if n else None, ld, n, int(k), _lib.ptr(ranks), hist.data_ptr(), _lib.stream_ptr())


# ---------------------------------------------------------------------------
# score-level evaluation (csrc/score_eval.hip)
# ---------------------------------------------------------------------------
SCORE_CHUNK = _lib.CTR_SCORE_CHUNK
GAUC_SMALL, GAUC_SLAB = _lib.CTR_GAUC_SMALL, _lib.CTR_GAUC_SLAB


def score_counts(prob: torch.Tensor, target: torch.Tensor, counts: torch.Tensor, sums: torch.Tensor) -> None:
    """``ctr_score_counts``: prob / target contiguous (N,) float32; ``counts`` (8,) int64 is added to
    ({positives, negatives, tp, fp, fn, tn, bad, 0}), ``sums`` (ceil(N / SCORE_CHUNK), 4) float64 receives one row
    {sum BCE term, sum p, sum (p - y)^2, sum y} per chunk of SCORE_CHUNK samples"""
    _lib.require_device(prob, target, counts, sums)
    _flat_f32("score_counts", "prob", prob)
    n = prob.shape[0]
    _flat_f32("score_counts", "target", target, n)
    _flat_int("score_counts", "counts", counts, torch.int64, 8)
    chunks = -(-n // SCORE_CHUNK)
    if sums.dtype != torch.float64 or sums.shape != (chunks, 4) or not sums.is_contiguous():
        raise ValueError(f"score_counts: sums must be a contiguous ({chunks}, 4) float64 tensor")
    _call("score_counts", "ctr_score_counts", lambda: (8 * n + 32 * chunks, 0), _lib.ptr(prob) if n else None,
          _lib.ptr(target) if n else None, n, counts.data_ptr(), _lib.ptr(sums) if n else None, _lib.stream_ptr())


def gauc_groups(prob: torch.Tensor, target: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor,
                small_groups: torch.Tensor, slab_group: torch.Tensor, slab_first: torch.Tensor, pos: torch.Tensor,
                neg: torch.Tensor, u2: torch.Tensor, err: torch.Tensor) -> None:
    """``ctr_gauc_groups``: prob / target contiguous (N,) float32, group g = the samples order[offsets[g] ..
    offsets[g + 1]) (order (N,) int32, offsets (G + 1,) int64), ``small_groups`` / ``slab_group`` / ``slab_first`` the
    int32 work lists of ``evaluator.score.UserGroups``.  ``pos`` / ``neg`` (G,) int32 receive the class counts,
    ``u2`` (G,) int64 is added to; ``err``: device int32 flag, raised and never cleared."""
    _lib.require_device(prob, target, order, offsets, small_groups, slab_group, slab_first, pos, neg, u2, err)
    _flat_f32("gauc_groups", "prob", prob)
    n = prob.shape[0]
    _flat_f32("gauc_groups", "target", target, n)
    _flat_int("gauc_groups", "order", order, torch.int32, n)
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1 or not offsets.is_contiguous():
        raise ValueError("gauc_groups: offsets must be a contiguous (G + 1,) int64 tensor")
    groups = offsets.shape[0] - 1
    if n >= 1 << 31 or groups >= 1 << 31:
        raise ValueError("gauc_groups: N and G must be below 2^31")
    _flat_int("gauc_groups", "small_groups", small_groups, torch.int32, small_groups.numel())
    _flat_int("gauc_groups", "slab_group", slab_group, torch.int32, slab_group.numel())
    _flat_int("gauc_groups", "slab_first", slab_first, torch.int32, slab_group.numel())
    _flat_int("gauc_groups", "pos", pos, torch.int32, groups)
    _flat_int("gauc_groups", "neg", neg, torch.int32, groups)
    _flat_int("gauc_groups", "u2", u2, torch.int64, groups)
    _flat_int("gauc_groups", "err", err, torch.int32, 1)
    nz = lambda t: _lib.ptr(t) if t.numel() else None                                     # noqa: E731
    _call("gauc_groups", "ctr_gauc_groups", lambda: (12 * n + 24 * groups, 0), nz(prob), nz(target), n, nz(order),
          offsets.data_ptr(), groups, nz(small_groups), small_groups.numel(), nz(slab_group), nz(slab_first),
          slab_group.numel(), nz(pos), nz(neg), nz(u2), err.data_ptr(), _lib.stream_ptr())
