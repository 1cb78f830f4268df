"""Collaborative filtering on dense matrices: row-wise top-k (csrc/topk.hip), UserCF / ItemCF (csrc/knn_cf.hip),
GDCF (csrc/gdcf.hip) and the full softmax over the catalogue (csrc/softmax_full.hip)."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ._call import _call


TOPK_MAX_K = _lib.CTR_TOPK_MAX_K


def topk_rows(scores: torch.Tensor, k: int, dim: int = -1) -> torch.Tensor:
    """indices of the k best scores along ``dim`` of a 2-D float32 tensor, best first, ties by ascending index
    (csrc/topk.hip) -- the ranking step of every ``recommendation()`` (reference: ``torch.topk(...)[1]``,
    model/mf.py:28-35, neuralcf.py:61-72, pnn.py:133-143, din.py:55-66).  ``dim=0`` ranks columns (AutoRec's
    item-based variant) and returns (k, cols) like torch.  k up to TOPK_MAX_K runs the kernel; a larger k (a
    catalogue of more than 4096 items ranked whole, as MF / NeuralCF do) is a stable descending device sort of the
    kernel's own 32-bit keys, which gives the same order: NaN first, ties by ascending index."""
    _lib.require_device(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("topk_rows expects a 2-D float32 tensor")
    along = dim % 2
    rows, n = scores.shape[1 - along], scores.shape[along]
    if not 1 <= k <= n:
        raise RuntimeError(f"selected index k out of range: k = {k}, {n} candidates")
    if k > TOPK_MAX_K:
        # ordered_key() of csrc/topk.hip: sign bit set -> ~bits, else bits | 2^31 (int64, so no unsigned compare needed)
        bits = scores.view(torch.int32).to(torch.int64)
        key = torch.where(bits < 0, ~bits, bits + (1 << 31))
        return torch.sort(key, dim=along, descending=True, stable=True).indices.narrow(along, 0, k)
    out = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    _call("topk_rows", "ctr_topk_rows", lambda: (4 * rows * n + 8 * rows * k, 0), _lib.ptr(scores) if rows else None,
          scores.stride(1 - along), scores.stride(along), rows, n, k, _lib.ptr(out) if rows else None, None,
          _lib.stream_ptr())
    return out if along == 1 else out.t()


CF_KNN_MAX_K = _lib.CTR_CF_KNN_MAX_K   # the longest list (k + 1 entries) ctr_cf_knn keeps per row


def _cf_operand(x: torch.Tensor, counts: torch.Tensor):
    _lib.require_device(x, counts)
    if x.dim() != 2 or x.dtype != torch.int8 or not x.is_contiguous() or x.shape[1] % 64:
        raise ValueError("expected a contiguous (rows, cols_pad) int8 matrix with cols_pad a multiple of 64")
    if counts.dtype != torch.int32 or counts.shape != (x.shape[0],) or not counts.is_contiguous():
        raise ValueError("expected int32 row counts, one per row")


def cf_knn(x: torch.Tensor, counts: torch.Tensor, kk: int, q_begin: int = 0, q_count: Optional[int] = None):
    """per query row of the int8 0/1 matrix ``x`` the ``kk`` best rows by cosine similarity (csrc/knn_cf.hip),
    descending, ties by ascending index, the row itself included -> (idx int64, sim float32), (q_count, kk); a list
    shorter than kk ends in -1 / 0.  Query rows are ``[q_begin, q_begin + q_count)``, base rows all of ``x``."""
    _cf_operand(x, counts)
    rows = x.shape[0]
    q_count = rows - q_begin if q_count is None else q_count
    if not 1 <= kk <= CF_KNN_MAX_K:
        raise ValueError(f"k + 1 = {kk} neighbours requested: the kernel keeps at most {CF_KNN_MAX_K} (k <= "
                         f"{CF_KNN_MAX_K - 1})")
    idx = torch.empty((q_count, kk), dtype=torch.int64, device=x.device)
    sim = torch.empty((q_count, kk), dtype=torch.float32, device=x.device)
    rc = _lib.load().ctr_cf_knn(x.data_ptr(), rows, x.shape[1], counts.data_ptr(), q_begin, q_count, kk,
                                idx.data_ptr(), sim.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_cf_knn")
    return idx, sim


def _cf_scores(fn_name: str, x: torch.Tensor, num_items: int, nbr: torch.Tensor, nsim: torch.Tensor,
               users: torch.Tensor, table_rows: int) -> torch.Tensor:
    _lib.require_device(x, nbr, nsim, users)
    if x.dim() != 2 or x.dtype != torch.int8 or not x.is_contiguous() or x.shape[1] % 64 or x.shape[1] < num_items:
        raise ValueError("expected the contiguous (num_users, cols_pad) int8 interaction matrix")
    if nbr.dtype != torch.int64 or nsim.dtype != torch.float32 or nbr.shape != nsim.shape or nbr.dim() != 2 \
            or not (nbr.is_contiguous() and nsim.is_contiguous()):
        raise ValueError("neighbours: contiguous int64 indices and float32 similarities of one (n, k) shape")
    if nbr.shape[0] != table_rows:
        raise ValueError(f"neighbour table has {nbr.shape[0]} rows, expected {table_rows}")
    users = users.to(torch.int64).contiguous()
    out = torch.empty((users.numel(), num_items), dtype=torch.float32, device=x.device)
    rc = getattr(_lib.load(), fn_name)(x.data_ptr(), x.shape[0], x.shape[1], num_items, nbr.data_ptr(),
                                       nsim.data_ptr(), nbr.shape[1], users.data_ptr(), users.numel(),
                                       out.data_ptr(), num_items, _lib.stream_ptr())
    _lib.check(rc, fn_name)
    return out


def usercf_scores(x, num_items, nbr, nsim, users):
    """prediction_dating (UserCF_Final.py:26-39) of every item for each user in ``users``; rated items -inf"""
    return _cf_scores("ctr_usercf_scores", x, num_items, nbr, nsim, users, x.shape[0])


def itemcf_scores(x, num_items, nbr, nsim, users):
    """prediction_item_based (ItemCF_Final.py:27-38) of every item for each user in ``users``; rated items -inf"""
    return _cf_scores("ctr_itemcf_scores", x, num_items, nbr, nsim, users, num_items)


# ---------------------------------------------------------------------------
# GDCF: BCEWithLogits over the full implicit matrix (csrc/gdcf.hip); the m x n scores are never written
# ---------------------------------------------------------------------------
GDCF_MAX_DIM = _lib.CTR_GDCF_MAX_DIM


def _gdcf_operands(p: torch.Tensor, q: torch.Tensor, y: torch.Tensor, y_rows: int, y_cols: int, what: str):
    _lib.require_device(p, q, y)
    for t, name in ((p, "P"), (q, "Q")):
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"gdcf: {name} must be a contiguous 2-D float32 tensor, got {tuple(t.shape)} {t.dtype}")
    if p.shape[1] != q.shape[1]:
        raise ValueError(f"gdcf: P has {p.shape[1]} columns, Q {q.shape[1]}")
    k = p.shape[1]
    if not 1 <= k <= GDCF_MAX_DIM:
        raise ValueError(f"gdcf: k = {k} outside [1, {GDCF_MAX_DIM}] (CTR_GDCF_MAX_DIM)")
    if p.shape[0] < 1 or q.shape[0] < 1:
        raise ValueError("gdcf: P and Q need at least one row")
    if y.dim() != 2 or y.dtype != torch.int8 or not y.is_contiguous() or y.shape[0] != y_rows \
            or y.shape[1] % 64 or y.shape[1] < y_cols:
        raise ValueError(f"gdcf: {what} must be the contiguous ({y_rows}, pad64({y_cols})) int8 matrix, got "
                         f"{tuple(y.shape)} {y.dtype}")
    return k


def gdcf_rows(p: torch.Tensor, q: torch.Tensor, y: torch.Tensor, grad: bool = True):
    """row pass: (loss, dP) with loss a 0-dim float32 device tensor, the mean of softplus(s) - y s over the m x n
    matrix, and dP = (sigmoid(S) - Y) Q / (m n); ``grad=False`` forms the scores only and returns (loss, None).
    ``y`` is ImplicitMatrix.data, (m, cols_pad) int8, columns >= n ignored."""
    m, n = p.shape[0], q.shape[0]
    k = _gdcf_operands(p, q, y, m, n, "the interaction matrix")
    ws = C.c_int64()
    _lib.check(_lib.load().ctr_gdcf_workspace_bytes(m, n, k, C.byref(ws)), "ctr_gdcf_workspace_bytes")
    parts = torch.empty(ws.value // 8, dtype=torch.float64, device=p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    gp = torch.empty_like(p) if grad else None
    _call("gdcf_rows" if grad else "gdcf_rows_loss", "ctr_gdcf_rows",
          lambda: (4 * (m * k + n * k) + m * y.shape[1] + (4 * m * k if grad else 0),
                   (4 if grad else 2) * m * n * k),
          p.data_ptr(), q.data_ptr(), m, n, k, y.data_ptr(), y.shape[1], loss.data_ptr(), _lib.ptr(gp), parts.data_ptr(),
          ws.value, _lib.stream_ptr())
    return loss, gp


def gdcf_cols(p: torch.Tensor, q: torch.Tensor, yt: torch.Tensor, gout: torch.Tensor) -> torch.Tensor:
    """column pass: dQ = gout * (sigmoid(S) - Y)^T P / (m n), ``gout`` the loss's upstream gradient (one float32 on
    the device, read there: no host synchronisation).  ``yt`` is ImplicitMatrix.transposed(), (n, pad64(m)) int8."""
    m, n = p.shape[0], q.shape[0]
    k = _gdcf_operands(p, q, yt, n, m, "the transposed interaction matrix")
    _lib.require_device(gout)
    if gout.numel() != 1 or gout.dtype != torch.float32:
        raise ValueError("gdcf: the upstream gradient must be one float32")
    gout = gout.reshape(1).contiguous()
    gq = torch.empty_like(q)
    _call("gdcf_cols", "ctr_gdcf_cols", lambda: (4 * (m * k + 2 * n * k) + n * yt.shape[1], 4 * m * n * k), p.data_ptr(),
          q.data_ptr(), m, n, k, yt.data_ptr(), yt.shape[1], gout.data_ptr(), gq.data_ptr(), _lib.stream_ptr())
    return gq


# ---------------------------------------------------------------------------
# full softmax over the catalogue (csrc/softmax_full.hip): nll of a target item against every item; the B x I logits
# are never written
# ---------------------------------------------------------------------------
SOFTMAX_FULL_MAX_DIM = _lib.CTR_SOFTMAX_FULL_MAX_DIM
SOFTMAX_FULL_MAX_SPLITS = 64


def _softmax_full_operands(x: torch.Tensor, q: torch.Tensor, target: torch.Tensor, splits: int):
    _lib.require_device(x, q, target)
    for t, name in ((x, "X"), (q, "Q")):
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"softmax_full: {name} must be a contiguous 2-D float32 tensor, got {tuple(t.shape)} "
                             f"{t.dtype}")
    if x.shape[1] != q.shape[1]:
        raise ValueError(f"softmax_full: X has {x.shape[1]} columns, Q {q.shape[1]}")
    k = x.shape[1]
    if not 1 <= k <= SOFTMAX_FULL_MAX_DIM:
        raise ValueError(f"softmax_full: k = {k} outside [1, {SOFTMAX_FULL_MAX_DIM}] (CTR_SOFTMAX_FULL_MAX_DIM)")
    if q.shape[0] < 1:
        raise ValueError("softmax_full: Q needs at least one row")
    if target.dim() != 1 or target.dtype != torch.int64 or not target.is_contiguous() or target.numel() != x.shape[0]:
        raise ValueError(f"softmax_full: the targets must be a contiguous ({x.shape[0]},) int64 tensor, got "
                         f"{tuple(target.shape)} {target.dtype}")
    if not 0 <= int(splits) <= SOFTMAX_FULL_MAX_SPLITS:
        raise ValueError(f"softmax_full: splits = {splits} outside [0, {SOFTMAX_FULL_MAX_SPLITS}]")
    return k


def _softmax_full_row_vector(t: torch.Tensor, batch: int, what: str) -> None:
    _lib.require_device(t)
    if t.dim() != 1 or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != batch:
        raise ValueError(f"softmax_full: {what} must be a contiguous ({batch},) float32 tensor, got {tuple(t.shape)} "
                         f"{t.dtype}")


def _softmax_full_workspace(batch, num_items, k, splits_rows, splits_cols, device):
    ws = C.c_int64()
    _lib.check(_lib.load().ctr_softmax_full_workspace_bytes(batch, num_items, k, splits_rows, splits_cols,
                                                             C.byref(ws)), "ctr_softmax_full_workspace_bytes")
    return torch.empty(ws.value // 4, dtype=torch.float32, device=device) if ws.value else None, ws.value


def softmax_full_rows(x: torch.Tensor, q: torch.Tensor, target: torch.Tensor, grad: bool = True, splits: int = 0,
                      err_flag: Optional[torch.Tensor] = None):
    """row pass: (nll, lse, gx_unit) for query rows ``x`` (B, k), the item table ``q`` (I, k) and ``target`` (B,)
    int64: lse[b] = log sum_i exp(<x[b], q[i]>), nll = lse - <x[b], q[t_b]>, and gx_unit = softmax(z[b]) q - q[t_b],
    the gradient of nll[b] by x[b] (``grad=False``: None).  A target outside [0, I) is never read: nll = lse for that
    row and ``err_flag`` (device int32) is set.  ``splits``: parts the item range is cut into (0: automatic)."""
    k = _softmax_full_operands(x, q, target, splits)
    b, n = x.shape[0], q.shape[0]
    nll = torch.empty(b, dtype=torch.float32, device=x.device)
    lse = torch.empty(b, dtype=torch.float32, device=x.device)
    gx = torch.empty_like(x) if grad else None
    if b == 0:
        return nll, lse, gx
    ws, nbytes = _softmax_full_workspace(b, n, k, int(splits), 1, x.device)
    _call("softmax_full_rows" if grad else "softmax_full_rows_loss", "ctr_softmax_full_rows",
          lambda: (4 * (b * k + n * k) + 8 * b + 8 * b + (4 * b * k if grad else 0) + 2 * nbytes,
                   (4 if grad else 2) * b * n * k),
          x.data_ptr(), q.data_ptr(), b, n, k, target.data_ptr(), nll.data_ptr(), lse.data_ptr(), _lib.ptr(gx), int(splits),
          _lib.ptr(ws), nbytes, _lib.ptr(err_flag), _lib.stream_ptr())
    return nll, lse, gx


def softmax_full_cols(x: torch.Tensor, q: torch.Tensor, target: torch.Tensor, lse: torch.Tensor, gout: torch.Tensor,
                      splits: int = 0, nll: Optional[torch.Tensor] = None) -> torch.Tensor:
    """column pass: dQ (I, k) = G^T x with G[b, i] = gout[b] (exp(<x[b], q[i]> - lse[b]) - [i == t_b]); ``lse`` from
    the row pass, ``gout`` (B,) float32 the upstream gradient of nll, read on the device.  ``splits``: parts the batch
    is cut into (0: automatic).  ``nll``: the row pass's, when at hand: a target's entry is then gout expm1(-nll),
    which keeps its digits where the target's probability nears 1 (a float32 lse alone cannot)."""
    k = _softmax_full_operands(x, q, target, splits)
    b, n = x.shape[0], q.shape[0]
    _softmax_full_row_vector(lse, b, "lse")
    _softmax_full_row_vector(gout, b, "the upstream gradient")
    if nll is not None:
        _softmax_full_row_vector(nll, b, "nll")
    if b == 0:
        return torch.zeros_like(q)
    gq = torch.empty_like(q)
    ws, nbytes = _softmax_full_workspace(b, n, k, 1, int(splits), x.device)
    _call("softmax_full_cols", "ctr_softmax_full_cols",
          lambda: (4 * (b * k + 2 * n * k) + 20 * b + 2 * nbytes, 4 * b * n * k), x.data_ptr(), q.data_ptr(), b, n, k,
          target.data_ptr(), lse.data_ptr(), _lib.ptr(nll), gout.data_ptr(), gq.data_ptr(), int(splits), _lib.ptr(ws),
          nbytes, _lib.stream_ptr())
    return gq
