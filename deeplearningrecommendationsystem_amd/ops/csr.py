"""The CSR-row calls: ALS's row solves (csrc/als.hip) and LightGCN's graph propagation (csrc/graph_prop.hip).  What
they check and count alike on ``indptr``, ``indices``, ``rows``, ``err_flag`` and ``out`` is ``_CsrRows``."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ._call import _call


# ---------------------------------------------------------------------------
# the frame of a CSR-row call
# ---------------------------------------------------------------------------
_ROW_COUNT_NAME = {"als": "csr_rows", "graph": "num_rows"}     # what each family's messages call the CSR's row count


def _csr_indptr(who: str, indptr) -> int:
    if not isinstance(indptr, torch.Tensor) or indptr.dim() != 1 or indptr.dtype != torch.int64 or \
            not indptr.is_contiguous() or indptr.numel() < 2:
        raise ValueError(f"{who}: indptr must be a contiguous ({_ROW_COUNT_NAME[who]} + 1,) int64 tensor")
    if indptr.numel() - 1 >= 1 << 31:
        raise ValueError(f"{who}: a CSR must have fewer than 2^31 rows")
    return indptr.numel() - 1


class _CsrRows:
    """the CSR, the rows and the flag of one call under its ``als`` / ``graph`` prefix, checked by value; ``output``
    then settles ``out`` and asks for the device, after everything that needs none to tell"""

    def __init__(self, who: str, indptr, indices, rows, err_flag):
        self.who, self.indptr, self.indices, self.rows, self.err_flag = who, indptr, indices, rows, err_flag
        self.num_rows = _csr_indptr(who, indptr)
        if not isinstance(indices, torch.Tensor) or indices.dim() != 1 or indices.dtype != torch.int32 or \
                not indices.is_contiguous():
            raise ValueError(f"{who}: indices must be a contiguous 1-D int32 tensor")
        self.nnz = indices.numel()
        if self.nnz >= 1 << 31:
            raise ValueError(f"{who}: a CSR must have fewer than 2^31 entries")
        if rows is not None and (not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.dtype != torch.int64 or
                                 not rows.is_contiguous()):
            raise ValueError(f"{who}: rows must be a contiguous 1-D int64 tensor")
        self.count = self.num_rows if rows is None else rows.numel()
        if self.count >= 1 << 31:
            raise ValueError(f"{who}: at most 2^31 - 1 rows a call")
        if err_flag is not None and (err_flag.dtype != torch.int32 or err_flag.numel() != 1):
            raise ValueError(f"{who}: err_flag must be one int32")

    def output(self, out, k: int, operands, layout=None):
        """(out, ldo): ``out`` checked, or a fresh one next to ``operands[0]``.  ``layout(out, count, "out")`` gives
        the row stride or raises; without one the rule is a unit inner stride and a row stride of at least k."""
        who, count = self.who, self.count
        what = f"{who}: out must be a ({count}, {k}) float32 tensor" + ("" if layout else " with unit inner stride")
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2 or
                                out.shape != (count, k)):
            raise ValueError(what)
        if out is None or count == 0:
            ldo = k
        elif layout is not None:
            ldo = layout(out, count, "out")
        else:
            if out.stride(1) != 1 or (count > 1 and out.stride(0) < k):
                raise ValueError(what)
            ldo = out.stride(0) if count > 1 else k
        _lib.require_device(*operands, self.indptr, self.indices, self.rows, out, self.err_flag)
        if out is None:
            out = torch.empty((count, k), dtype=torch.float32, device=operands[0].device)
        return out, ldo

    def entries(self) -> int:
        """list entries of the rows of the call, for ``meta()``: a sync where ``rows`` is given, so only a profiler asks"""
        if self.rows is None:
            return self.nnz
        at = self.rows.clamp(0, self.num_rows - 1)
        return int((self.indptr[at + 1] - self.indptr[at]).sum())


# ---------------------------------------------------------------------------
# ALS (csrc/als.hip): the row solves of implicit-feedback alternating least squares; no (rows, k, k) tensor exists
# ---------------------------------------------------------------------------
ALS_MAX_DIM = _lib.CTR_ALS_MAX_DIM
ALS_ERR_INDEX, ALS_ERR_PIVOT = 1, 2


def als_supported(k) -> bool:
    """does ``als_gram`` / ``als_solve_rows`` take tables of ``k`` columns: a multiple of 16 in [16, ALS_MAX_DIM]"""
    return isinstance(k, int) and not isinstance(k, bool) and 16 <= k <= ALS_MAX_DIM and k % 16 == 0


def _als_table(y: torch.Tensor, what: str) -> int:
    if y.dim() != 2 or y.dtype != torch.float32 or not y.is_contiguous() or y.shape[0] < 1:
        raise ValueError(f"als: {what} must be a contiguous 2-D float32 tensor with at least one row, got "
                         f"{tuple(y.shape)} {y.dtype}")
    k = int(y.shape[1])
    if not als_supported(k):
        raise ValueError(f"als: k = {k} is not a multiple of 16 in [16, {ALS_MAX_DIM}] (CTR_ALS_MAX_DIM)")
    if y.shape[0] >= 1 << 31:
        raise ValueError("als: a table must have fewer than 2^31 rows")
    return k


def als_gram_workspace_bytes(rows: int, k: int) -> int:
    ws = C.c_int64()
    _lib.check(_lib.load().ctr_als_gram_workspace_bytes(int(rows), int(k), C.byref(ws)), "ctr_als_gram_workspace_bytes")
    return ws.value


def als_gram(y: torch.Tensor) -> torch.Tensor:
    """(k, k) float32 ``y^T y`` of a (rows, k) table: partials over fixed slabs of rows, added in ascending order, so
    the result is bitwise reproducible"""
    k = _als_table(y, "the table")
    _lib.require_device(y)
    rows = y.shape[0]
    nbytes = als_gram_workspace_bytes(rows, k)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=y.device)
    gram = torch.empty((k, k), dtype=torch.float32, device=y.device)
    _call("als_gram", "ctr_als_gram", lambda: (4 * rows * k + 2 * nbytes + 4 * k * k, rows * k * (k + 16)),
          y.data_ptr(), rows, k, gram.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr())
    return gram


def als_solve_rows(y: torch.Tensor, gram: torch.Tensor, indptr: torch.Tensor, indices: torch.Tensor, reg: float,
                   alpha: float, rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(count, k) float32: for every CSR row ``rows[j]`` (``None``: all rows, in order) the solution x of
    ``(gram + alpha sum_{i in list} y_i y_i^T + reg I) x = (1 + alpha) sum_{i in list} y_i`` over the (y_rows, k) table
    ``y``; ``indptr`` (csr_rows + 1) int64 and ``indices`` int32 as ``ObservedPairs`` keeps them.  A row is a bitwise
    function of its list, ``y``, ``gram``, ``reg`` and ``alpha`` alone.  ``out``: a (count, k) float32 tensor with unit
    inner stride to write into.  ``err_flag`` (device int32, OR-ed into): ALS_ERR_INDEX for an index outside ``y`` (never
    read), ALS_ERR_PIVOT for a pivot that is not positive and finite; such rows are zeros."""
    k = _als_table(y, "the table")
    if gram.shape != (k, k) or gram.dtype != torch.float32 or not gram.is_contiguous():
        raise ValueError(f"als: gram must be a contiguous ({k}, {k}) float32 tensor, got {tuple(gram.shape)} {gram.dtype}")
    reg, alpha = float(reg), float(alpha)
    if reg != reg or alpha != alpha:
        raise ValueError("als: reg and alpha must be numbers")
    csr = _CsrRows("als", indptr, indices, rows, err_flag)
    out, ldo = csr.output(out, k, (y, gram))
    count, nnz = csr.count, csr.nnz
    if count == 0:
        return out

    def meta():      # 2 k^2 per list entry of the rows solved plus k^3 / 3 per row; read only under a profiler
        entries = csr.entries()
        return (4 * entries * (k + 1) + 16 * count + 4 * count * k + 4 * k * k,
                2 * k * k * entries + count * (k ** 3) // 3)
    _call("als_solve_rows", "ctr_als_solve_rows", meta,
          y.data_ptr(), y.shape[0], k, gram.data_ptr(), indptr.data_ptr(), _lib.ptr(indices) if nnz else None,
          csr.num_rows, _lib.ptr(rows), count, reg, alpha, out.data_ptr(), ldo, _lib.ptr(err_flag), _lib.stream_ptr())
    return out


def als_solve_rows_weighted(y: torch.Tensor, gram: Optional[torch.Tensor], indptr: torch.Tensor, indices: torch.Tensor,
                            values: torch.Tensor, w, t, reg: float, reg_per_entry: float = 0.0,
                            rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                            err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``als_solve_rows`` with a weight per list entry: ``values`` (nnz,) float32 is aligned with ``indices`` and, with
    ``w = (w0, w1)``, ``t = (t0, t1)``, ``w_e = fma(w1, v_e, w0)``, ``t_e = fma(t1, v_e, t0)`` and n the row's list
    length, a row solves ``(gram + sum_e w_e y_e y_e^T + (reg + reg_per_entry n) I) x = sum_e t_e y_e``; ``gram=None``:
    no dense part.  Confidences ``1 + alpha v``: ``w = (0, alpha)``, ``t = (1, alpha)``; explicit ratings with the
    regulariser weighted by the list length: ``gram=None``, ``w = (1, 0)``, ``t = (0, 1)``, ``reg=0``,
    ``reg_per_entry``.  A row is a bitwise function of its list, its values, ``y``, ``gram`` and the six scalars alone.
    ``rows``, ``out`` and ``err_flag`` as in ``als_solve_rows``; a non-finite value gives a zero row and ALS_ERR_PIVOT."""
    k = _als_table(y, "the table")
    if gram is not None and (gram.shape != (k, k) or gram.dtype != torch.float32 or not gram.is_contiguous()):
        raise ValueError(f"als: gram must be None or a contiguous ({k}, {k}) float32 tensor, got {tuple(gram.shape)} "
                         f"{gram.dtype}")
    csr = _CsrRows("als", indptr, indices, rows, err_flag)
    if values.dim() != 1 or values.dtype != torch.float32 or not values.is_contiguous() or \
            values.numel() != indices.numel():
        raise ValueError("als: values must be a contiguous 1-D float32 tensor of the length of indices")
    try:
        (w0, w1), (t0, t1) = (float(v) for v in w), (float(v) for v in t)
    except (TypeError, ValueError):
        raise ValueError("als: w and t must be pairs of numbers (w0, w1), (t0, t1)") from None
    reg, reg_per_entry = float(reg), float(reg_per_entry)
    if any(v != v for v in (w0, w1, t0, t1, reg, reg_per_entry)):
        raise ValueError("als: w, t, reg and reg_per_entry must be numbers")
    out, ldo = csr.output(out, k, (y, gram, values))
    count, nnz = csr.count, csr.nnz
    if count == 0:
        return out

    def meta():      # als_solve_rows' with 4 B more read per entry; the dense part only where there is one
        entries = csr.entries()
        return (4 * entries * (k + 2) + 16 * count + 4 * count * k + (4 * k * k if gram is not None else 0),
                2 * k * k * entries + count * (k ** 3) // 3)
    _call("als_solve_rows_weighted", "ctr_als_solve_rows_weighted", meta,
          y.data_ptr(), y.shape[0], k, _lib.ptr(gram), indptr.data_ptr(), _lib.ptr(indices) if nnz else None,
          _lib.ptr(values) if nnz else None, csr.num_rows, _lib.ptr(rows), count, w0, w1, t0, t1, reg, reg_per_entry,
          out.data_ptr(), ldo, _lib.ptr(err_flag), _lib.stream_ptr())
    return out


# ---------------------------------------------------------------------------
# graph propagation (csrc/graph_prop.hip): the CSR row sum of LightGCN; its backward is itself over the transposed CSR
# ---------------------------------------------------------------------------
GRAPH_MAX_DIM = _lib.CTR_GRAPH_MAX_DIM
GRAPH_SEGMENT = _lib.CTR_GRAPH_SEGMENT     # a list is cut every GRAPH_SEGMENT entries from its own start
GRAPH_ERR_INDEX, GRAPH_ERR_PLAN = 1, 2


def graph_supported(k) -> bool:
    """does ``graph_propagate`` take tables of ``k`` columns: a multiple of 16 in [16, GRAPH_MAX_DIM], the ranks
    ``lowrank_grid_scores`` takes"""
    return isinstance(k, int) and not isinstance(k, bool) and 16 <= k <= GRAPH_MAX_DIM and k % 16 == 0


class GraphPlan:
    """what an all-rows ``graph_propagate`` over one CSR needs from the host, built once (``graph_plan``): the work
    items by descending list length, the segments of rows longer than GRAPH_SEGMENT as items of their own, the rows to
    merge and the number of workspace slots.  Results do not depend on it."""

    __slots__ = ("indptr", "num_rows", "work", "merge", "slots")

    def __init__(self, indptr, num_rows, work, merge, slots):
        self.indptr, self.num_rows, self.work, self.merge, self.slots = indptr, num_rows, work, merge, slots


def graph_plan(indptr: torch.Tensor) -> GraphPlan:
    """the plan of ``graph_propagate(..., rows=None)`` over the CSR with these offsets: one device-to-host sync here,
    none in the calls that use it"""
    num_rows = _csr_indptr("graph", indptr)
    _lib.require_device(indptr)
    dev = indptr.device
    length = indptr.diff()
    order = torch.argsort(length, descending=True, stable=True)
    nseg = ((length[order] + (GRAPH_SEGMENT - 1)) // GRAPH_SEGMENT).clamp_(min=1)
    split = nseg > 1
    slot_count = nseg * split
    slot0 = slot_count.cumsum(0) - slot_count                    # first slot of a split row
    first = nseg.cumsum(0) - nseg                                # first item of a row
    nwork, slots, nsplit = torch.stack((nseg.sum(), slot_count.sum(), split.sum())).tolist()      # the sync
    if nwork >= 1 << 31:
        raise ValueError("graph: the CSR has 2^31 or more work items")
    seg = torch.arange(nwork, device=dev) - torch.repeat_interleave(first, nseg, output_size=nwork)
    slot = torch.where(torch.repeat_interleave(split, nseg, output_size=nwork),
                       torch.repeat_interleave(slot0, nseg, output_size=nwork) + seg, -1)
    work = torch.stack((torch.repeat_interleave(order, nseg, output_size=nwork), seg, slot, torch.zeros_like(seg)),
                       dim=1).to(torch.int32).contiguous()
    # the split rows are the longest: the first nsplit of the order
    merge = torch.stack((order[:nsplit], slot0[:nsplit]), dim=1).to(torch.int32).contiguous() if nsplit else None
    return GraphPlan(indptr, num_rows, work, merge, slots)


def graph_workspace_bytes(slots: int, k: int) -> int:
    ws = C.c_int64()
    _lib.check(_lib.load().ctr_graph_propagate_workspace_bytes(int(slots), int(k), C.byref(ws)),
               "ctr_graph_propagate_workspace_bytes")
    return ws.value


def _graph_scale(t, n, what):
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != (n,) or
                          not t.is_contiguous()):
        raise ValueError(f"graph: {what} must be a contiguous ({n},) float32 tensor or None")


def graph_propagate(x: torch.Tensor, indptr: torch.Tensor, indices: torch.Tensor,
                    scale_in: Optional[torch.Tensor] = None, scale_out: Optional[torch.Tensor] = None,
                    rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    plan: Optional[GraphPlan] = None, err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(count, k) float32: for every CSR row ``r = rows[j]`` (``None``: all rows, in order)
    ``out[j] = scale_out[r] * sum_{e in list(r)} scale_in[indices[e]] * x[indices[e]]`` over the (x_rows, k) table
    ``x`` (unit inner stride, a row stride that is a multiple of 4, 16-byte aligned); ``indptr`` (num_rows + 1) int64
    and ``indices`` int32 as ``ObservedPairs`` keeps them; a scale that is ``None`` is ones.  A row is a bitwise
    function of its list, the rows of ``x`` it names and the two scales alone: not of ``rows``, of ``plan`` or of the
    run.  ``plan`` (``graph_plan(indptr)``, all-rows calls only) orders the work by list length and splits long lists
    over waves.  ``out``: a (count, k) float32 tensor to write into, same layout rules as ``x``.  ``err_flag`` (device
    int32, OR-ed into): GRAPH_ERR_INDEX for an index outside ``x`` (never read, it adds nothing); without an
    ``err_flag`` the call reads a flag of its own (one sync) and raises ``IndexError``."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 1:
        raise ValueError("graph: x must be a 2-D float32 tensor with at least one row")
    x_rows, k = int(x.shape[0]), int(x.shape[1])
    if not graph_supported(k):
        raise ValueError(f"graph: k = {k} is not a multiple of 16 in [16, {GRAPH_MAX_DIM}] (CTR_GRAPH_MAX_DIM)")
    if x_rows >= 1 << 31:
        raise ValueError("graph: a table must have fewer than 2^31 rows")

    def layout(t, n, what):
        if t.stride(1) != 1 or (n > 1 and (t.stride(0) < k or t.stride(0) % 4)) or t.data_ptr() % 16:
            raise ValueError(f"graph: {what} needs unit inner stride, a row stride that is a multiple of 4 and at "
                             f"least {k}, and 16-byte alignment")
        return t.stride(0) if n > 1 else k
    ldx = layout(x, x_rows, "x")
    csr = _CsrRows("graph", indptr, indices, rows, err_flag)
    num_rows, nnz, count = csr.num_rows, csr.nnz, csr.count
    _graph_scale(scale_in, x_rows, "scale_in")
    _graph_scale(scale_out, num_rows, "scale_out")
    if plan is not None:
        if not isinstance(plan, GraphPlan):
            raise ValueError("graph: plan must come from graph_plan()")
        if rows is not None:
            raise ValueError("graph: a plan covers all rows in order; pass rows or a plan, not both")
        if plan.num_rows != num_rows or plan.indptr.data_ptr() != indptr.data_ptr():
            raise ValueError("graph: the plan was built for another CSR")
    out, ldo = csr.output(out, k, (x, scale_in, scale_out), layout)
    if count == 0:
        return out
    flag = err_flag if err_flag is not None else torch.zeros(1, dtype=torch.int32, device=x.device)
    work = merge = ws = None
    nbytes = 0
    if plan is not None:
        work, merge = plan.work, plan.merge
        if plan.slots:
            nbytes = graph_workspace_bytes(plan.slots, k)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)

    def meta():      # a gathered row and an index per entry, the out rows, the partials written and read back
        entries = csr.entries()
        return 4 * entries * (k + 1) + 4 * count * (k + 4) + 2 * nbytes, 2 * entries * k
    _call("graph_propagate", "ctr_graph_propagate", meta,
          x.data_ptr(), x_rows, ldx, k, indptr.data_ptr(), _lib.ptr(indices) if nnz else None, num_rows, nnz,
          _lib.ptr(scale_in), _lib.ptr(scale_out), _lib.ptr(rows), count, _lib.ptr(work),
          0 if work is None else work.shape[0], _lib.ptr(merge), 0 if merge is None else merge.shape[0], out.data_ptr(),
          ldo, _lib.ptr(ws), nbytes, flag.data_ptr(), _lib.stream_ptr())
    if err_flag is None:
        bits = int(flag.item())
        if bits & GRAPH_ERR_INDEX:
            raise IndexError("graph: an index of the CSR is outside the table it indexes (or a row is outside the CSR)")
        if bits:
            raise RuntimeError(f"graph: the plan does not fit the call (error bits {bits:#x})")
    return out
