"""Host-side wrappers over the C ABI (include/ctrhip.h).

PyTorch is plumbing here: it owns device memory and the stream; every function
passes raw pointers + leading dimensions to libctrhip and enqueues on torch's
current stream.  2-D operands may be column slices of a wider buffer (stride(1)
must be 1), which is how the reference's ``torch.cat`` calls disappear: producers
write straight into the consumer's operand.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (ACT_NONE, ACT_RELU, ACT_SIGMOID, FIELD_BAG, FIELD_DENSE, FIELD_ID_F32, FIELD_ID_I64,
                   FIELD_PROD_I64, Field)

__all__ = ["FieldSpec", "embed_fwd", "embed_bwd", "linear_fwd", "linear_bwd", "mf_fwd", "mf_bwd",
           "ACT_NONE", "ACT_RELU", "ACT_SIGMOID"]


# ---------------------------------------------------------------------------
# optional per-launch timing (bench.py): a HIP event pair on the stream the
# kernel is enqueued on, plus the launch's algorithmic bytes / flops
# ---------------------------------------------------------------------------
class KernelProfiler:
    """HIP-event timing of every C-ABI call of the steps run while it is installed.

    ``spacer_us`` > 0 keeps the GPU busy for about that long (``torch.cuda._sleep``) before each
    bracketed call: start event, launch and end event are then all queued before the GPU reaches
    them, so the pair measures the kernel(s) of the call and not the host's launch latency (without
    it a 70 us kernel reads ~85 us; with it the numbers agree with rocprofv3 to a few per cent)."""

    def __init__(self, spacer_us: float = 0.0):
        self.records = []
        self.spacer_cycles = 0
        if spacer_us > 0:
            # calibrate _sleep: cycles per microsecond of whatever clock it spins on
            probe = 200_000
            torch.cuda._sleep(probe)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(probe)
            b.record()
            torch.cuda.synchronize()
            us = max(a.elapsed_time(b) * 1e3, 1e-3)
            self.spacer_cycles = max(1, int(probe / us * spacer_us))

    def add(self, label, nbytes, flops, start, end):
        self.records.append((label, nbytes, flops, start, end))

    def summary(self):
        """{label: dict(calls, total_us, avg_us, bytes, flops)} -- call after a sync.  ``bytes`` / ``flops`` are the
        AVERAGE per call of what the calls under that label declared, ``avg_us`` the average duration: a label that
        covers launches of different shapes (two stacks through ``mlp_fused_fwd``) then still gives a physically
        possible rate, total work over total time (round 2 divided the first call's work by the average time of
        all calls and printed a fraction above 1).  ``shapes`` counts the distinct (bytes, flops) pairs seen."""
        torch.cuda.synchronize()
        return self.fold([(label, nbytes, flops, start.elapsed_time(end) * 1e3)
                          for label, nbytes, flops, start, end in self.records])

    @staticmethod
    def fold(timed):
        """``summary`` over (label, bytes, flops, microseconds) records"""
        out = {}
        for label, nbytes, flops, us in timed:
            d = out.setdefault(label, dict(calls=0, total_us=0.0, total_bytes=0, total_flops=0, _shapes=set()))
            d["calls"] += 1
            d["total_us"] += us
            d["total_bytes"] += nbytes
            d["total_flops"] += flops
            d["_shapes"].add((nbytes, flops))
        for d in out.values():
            d["avg_us"] = d["total_us"] / d["calls"]
            d["bytes"] = d["total_bytes"] / d["calls"]
            d["flops"] = d["total_flops"] / d["calls"]
            d["shapes"] = len(d.pop("_shapes"))
        return out


_profiler: Optional[KernelProfiler] = None


def set_profiler(p: Optional[KernelProfiler]) -> None:
    global _profiler
    _profiler = p


def _timed(label, meta, fn, *args):
    """run one C call; when a profiler is installed bracket it with events"""
    p = _profiler
    if p is None:
        return fn(*args)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if p.spacer_cycles:
        torch.cuda._sleep(p.spacer_cycles)
    start.record()
    rc = fn(*args)
    end.record()
    nbytes, flops = meta()
    p.add(label, nbytes, flops, start, end)
    return rc


def _embed_bytes(specs, batch, backward):
    """algorithmic HBM bytes of one embedding-stage launch"""
    rows = idx = xcols = out = small = 0
    seen = set()
    for s in specs:
        out += s.width * 4
        for t in (s.idx, s.idx2):
            if t is not None and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                idx += 8
        if s.kind in (FIELD_ID_I64, FIELD_ID_F32):
            rows += s.width * 4
            xcols += 4 if s.kind == FIELD_ID_F32 else 0
        elif s.kind == FIELD_PROD_I64:
            rows += 2 * s.width * 4
        elif s.kind == FIELD_BAG:
            xcols += 4 * s.bag_size
            small += s.bag_size * s.width * 4
        else:
            xcols += 4 * s.width
    if not backward:
        return batch * (rows + idx + xcols + out) + small
    # backward: read gout, idx, (PROD: both rows), read-modify-write each touched grad row
    prod_rows = sum(2 * s.width * 4 for s in specs if s.kind == FIELD_PROD_I64)
    return batch * (out + idx + xcols + prod_rows + 2 * rows) + 2 * small


SCRATCH_FLOATS = 16 * 1024 * 1024  # 64 MiB: per-workgroup partials of the weight-gradient reductions


def _scratch(device) -> torch.Tensor:
    """device scratch for one backward launch.  Taken from torch's caching allocator per
    call (a few microseconds, no hipMalloc in steady state), so it follows the usual
    stream-ordered lifetime rules instead of being shared global state."""
    return torch.empty(SCRATCH_FLOATS, dtype=torch.float32, device=device)


def _mat(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: expected a 2-D float32 tensor with unit inner stride, got "
                         f"{tuple(t.shape)} {t.dtype} strides {t.stride()}")
    _lib.require_device(t)
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


@dataclass
class FieldSpec:
    """one output slice of the embedding stage (mirror of ``ctr_field_t``)"""
    kind: int
    width: int
    out_col: int
    table: Optional[torch.Tensor] = None      # (vocab, width) parameter
    src_col: int = 0
    bag_size: int = 0
    idx: Optional[torch.Tensor] = None        # int64, (B,) or a column of (B,L)
    idx_stride: int = 1
    table2: Optional[torch.Tensor] = None
    idx2: Optional[torch.Tensor] = None


def _field_array(specs: Sequence[FieldSpec], grads=None):
    if len(specs) > _lib.CTR_MAX_FIELDS:
        raise ValueError(f"at most {_lib.CTR_MAX_FIELDS} fields per launch")
    arr = (Field * len(specs))()
    for k, s in enumerate(specs):
        f = arr[k]
        f.kind, f.width, f.out_col, f.src_col, f.bag_size = s.kind, s.width, s.out_col, s.src_col, s.bag_size
        f.idx_stride = s.idx_stride
        if s.table is not None:
            _lib.require_device(s.table)
            if s.table.dtype != torch.float32 or not s.table.is_contiguous() or s.table.shape[1] != s.width:
                raise ValueError("embedding table must be contiguous float32 (vocab, width)")
            f.vocab = s.table.shape[0]
            f.table = s.table.data_ptr()
        if s.idx is not None:
            _lib.require_device(s.idx)
            if s.idx.dtype != torch.int64:
                raise ValueError("indices must be int64")
            f.idx = s.idx.data_ptr()
        if s.table2 is not None:
            f.vocab2 = s.table2.shape[0]
            f.table2 = s.table2.data_ptr()
            f.idx2 = s.idx2.data_ptr()
        if grads is not None:
            g = grads.get(id(s.table)) if s.table is not None else None
            f.grad = None if g is None else g.data_ptr()
            g2 = grads.get(id(s.table2)) if s.table2 is not None else None
            f.grad2 = None if g2 is None else g2.data_ptr()
    return arr


def embed_fwd(specs: Sequence[FieldSpec], x: Optional[torch.Tensor], batch: int, out: torch.Tensor,
              err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fused gather + bag pooling + concat into ``out`` (B, >= sum widths)"""
    out = _mat(out, "out")
    if x is not None:
        x = _mat(x, "x")
    arr = _field_array(specs)
    rc = _timed("embed_fwd", lambda: (_embed_bytes(specs, batch, False), 0),
                _lib.load().ctr_embed_fwd, arr, len(specs), _lib.ptr(x), _ld(x) if x is not None else 0, batch,
                out.data_ptr(), _ld(out), _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_embed_fwd")
    return out


def embed_bwd(specs: Sequence[FieldSpec], x: Optional[torch.Tensor], batch: int, gout: torch.Tensor,
              grads: dict) -> None:
    """accumulate into ``grads[id(table)]`` (dense, same shape as the table)"""
    gout = _mat(gout, "gout")
    if x is not None:
        x = _mat(x, "x")
    arr = _field_array(specs, grads)
    ws = _scratch(gout.device)  # bag partials + the small-table sort buffers
    rc = _timed("embed_bwd", lambda: (_embed_bytes(specs, batch, True), 0),
                _lib.load().ctr_embed_bwd, arr, len(specs), _lib.ptr(x), _ld(x) if x is not None else 0, batch,
                gout.data_ptr(), _ld(gout), _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr())
    _lib.check(rc, "ctr_embed_bwd")


def linear_fwd(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], act: int = ACT_NONE,
               out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act(x @ w.T + b (+ residual)); ``w`` is nn.Linear's (out, in) weight"""
    x, w = _mat(x, "x"), _mat(w, "w")
    m, k = x.shape
    n = w.shape[0]
    if w.shape[1] != k:
        raise ValueError(f"linear: x has {k} columns, weight expects {w.shape[1]}")
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    out = _mat(out, "out")
    if residual is not None:
        residual = _mat(residual, "residual")
    rc = _timed(f"linear_fwd[{m}x{n}x{k}]",
                lambda: (4 * (m * k + n * k + n + m * n * (2 if residual is not None else 1)), 2 * m * n * k),
                _lib.load().ctr_linear_fwd, x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), _lib.ptr(b),
                _lib.ptr(residual), _ld(residual) if residual is not None else 0, out.data_ptr(), _ld(out),
                m, n, k, act, _lib.stream_ptr())
    _lib.check(rc, "ctr_linear_fwd")
    return out


def linear_bwd(x: torch.Tensor, w: torch.Tensor, y: Optional[torch.Tensor], gy: torch.Tensor, act: int,
               gx: Optional[torch.Tensor], gw: Optional[torch.Tensor], gb: Optional[torch.Tensor],
               accumulate_gx: bool = False) -> None:
    """gz = gy*act'(y); gx (=|+=) gz @ w; gw += gz.T @ x; gb += gz.sum(0)"""
    x, w, gy = _mat(x, "x"), _mat(w, "w"), _mat(gy, "gy")
    m, k = x.shape
    n = w.shape[0]
    if y is not None:
        y = _mat(y, "y")
    if gx is not None:
        gx = _mat(gx, "gx")
    fn = _lib.load().ctr_linear_bwd
    ygy = 4 * m * n * (2 if (y is not None and act != ACT_NONE) else 1)
    ws = _scratch(x.device) if gw is not None else None

    def call(gx_, gw_, gb_):
        return (x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), _lib.ptr(y), _ld(y) if y is not None else 0,
                gy.data_ptr(), _ld(gy), _lib.ptr(gx_), _ld(gx_) if gx_ is not None else 0, int(accumulate_gx),
                _lib.ptr(gw_), _ld(gw_) if gw_ is not None else 0, _lib.ptr(gb_), m, n, k, act,
                _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr())

    if _profiler is None:
        _lib.check(fn(*call(gx, gw, gb)), "ctr_linear_bwd")
        return
    # profiling: one C call per kernel so each gets its own event pair
    if gx is not None:
        _lib.check(_timed(f"linear_bwd_dx[{m}x{n}x{k}]", lambda: (ygy + 4 * (n * k + m * k), 2 * m * n * k),
                          fn, *call(gx, None, None)), "ctr_linear_bwd")
    if gw is not None:
        _lib.check(_timed(f"linear_bwd_dw[{m}x{n}x{k}]", lambda: (ygy + 4 * (m * k + 2 * n * k), 2 * m * n * k),
                          fn, *call(None, gw, gb)), "ctr_linear_bwd")


def mf_fwd(user_table, item_table, user_idx, item_idx, err_flag=None) -> torch.Tensor:
    _lib.require_device(user_table, item_table, user_idx, item_idx)
    batch = user_idx.numel()
    prob = torch.empty(batch, dtype=torch.float32, device=user_table.device)
    dim = user_table.shape[1]
    rc = _timed("mf_fwd", lambda: (batch * (8 * dim + 16 + 4), 2 * batch * dim),
                _lib.load().ctr_mf_fwd, user_table.data_ptr(), user_table.shape[0], item_table.data_ptr(),
                item_table.shape[0], dim, user_idx.data_ptr(), item_idx.data_ptr(), batch, prob.data_ptr(),
                _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_mf_fwd")
    return prob


def mf_bwd(user_table, item_table, user_idx, item_idx, prob, gprob, guser, gitem) -> None:
    dim, batch = user_table.shape[1], user_idx.numel()
    rc = _timed("mf_bwd", lambda: (batch * (8 * dim + 16 + 8 + 16 * dim), 4 * batch * dim),
                _lib.load().ctr_mf_bwd, user_table.data_ptr(), user_table.shape[0], item_table.data_ptr(),
                item_table.shape[0], dim, user_idx.data_ptr(), item_idx.data_ptr(), batch, prob.data_ptr(),
                gprob.data_ptr(), _lib.ptr(guser), _lib.ptr(gitem), _lib.stream_ptr())
    _lib.check(rc, "ctr_mf_bwd")


# ---------------------------------------------------------------------------
# a stack of nn.Linear(+activation) layers, forward and hand-written backward
# ---------------------------------------------------------------------------
@dataclass
class Layer:
    weight: torch.Tensor
    bias: Optional[torch.Tensor]
    act: int


def zero_grads(tensors: Sequence[torch.Tensor], lazy: bool = False) -> dict:
    """{id(t): zero tensor shaped like t} for every parameter of a backward pass, carved
    out of ONE flat buffer so a step issues a single memset instead of one per
    parameter (each piece starts 16-byte aligned).  ``lazy=True``: the flat buffer is NOT filled; it is returned
    under the key ``"flat"`` and whoever launches first has to clear it (``mlp_head_bwd(zero=...)``) or call
    ``.zero_()`` on it."""
    out = {}
    dense = []
    for t in tensors:
        st = getattr(t, "_ctr_sparse", None)
        if st is None:
            dense.append(t)
            continue
        # sparse mode (sparse.py): the table's persistent accumulation buffer, clean outside pending rows --
        # the scatter kernels add into it as they would into a fresh zero buffer, nothing is zero-filled
        if st.grad.device != t.device or st.grad.shape != t.shape:
            raise RuntimeError("sparse-mode state does not match its table (enable sparse_grads after .to(device))")
        out[id(t)] = st.grad
    if not dense:
        return out
    sizes = [(t.numel() + 3) // 4 * 4 for t in dense]
    flat = (torch.empty if lazy else torch.zeros)(sum(sizes), dtype=torch.float32, device=dense[0].device)
    if lazy:
        out["flat"] = flat
    off = 0
    for t, n in zip(dense, sizes):
        out[id(t)] = flat[off:off + t.numel()].view(t.shape)
        off += n
    return out


def fold_head_fwd(u_full: torch.Tensor, p: int, w: torch.Tensor, b: Optional[torch.Tensor],
                  b2: Optional[torch.Tensor], out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wfold (1, p+k), cfold (1,)) of the layer ``w, b`` (n x k) composed with the single-unit layer
    ``u_full`` (1, p+n) whose first p columns pass through (ctr_fold_head_fwd)"""
    n, k = w.shape
    if out is not None:
        wfold, cfold = out
    else:
        wfold = torch.empty((1, p + k), dtype=torch.float32, device=w.device)
        cfold = torch.empty(1, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().ctr_fold_head_fwd(u_full.data_ptr(), p, w.data_ptr(), _ld(w), _lib.ptr(b), _lib.ptr(b2), n, k,
                                             wfold.data_ptr(), cfold.data_ptr(), _lib.stream_ptr()), "ctr_fold_head_fwd")
    return wfold, cfold


def fold_head_bwd(u_full: torch.Tensor, p: int, w: torch.Tensor, b: Optional[torch.Tensor], gwfold: torch.Tensor,
                  gc: torch.Tensor, gu_full: Optional[torch.Tensor], gw: Optional[torch.Tensor],
                  gb: Optional[torch.Tensor], gb2: Optional[torch.Tensor]) -> None:
    """chain rule through ``fold_head_fwd``; every gradient is accumulated (ctr_fold_head_bwd)"""
    n, k = w.shape
    _lib.check(_lib.load().ctr_fold_head_bwd(u_full.data_ptr(), p, w.data_ptr(), _ld(w), _lib.ptr(b), n, k,
                                             gwfold.data_ptr(), gc.data_ptr(), _lib.ptr(gu_full), _lib.ptr(gw),
                                             _ld(gw) if gw is not None else 0, _lib.ptr(gb), _lib.ptr(gb2),
                                             _lib.stream_ptr()), "ctr_fold_head_bwd")


FUSED_MLP = True  # narrow stacks run as one launch (ctr_mlp_fwd/bwd) when their shape allows
_REFUSED = (-2, -4)  # CTR_ELIMIT / CTR_EALIGN: nothing was enqueued, take the per-layer path


def _refused(rc, label) -> bool:
    """whether the library refused the ``_timed`` call that returned ``rc``; nothing ran then, so the profiler's record
    of it goes and what the caller issues instead is what gets timed"""
    if rc not in _REFUSED:
        return False
    if _profiler is not None and _profiler.records and _profiler.records[-1][0] == label:
        _profiler.records.pop()
    return True


def _mlp_layer_array(layers, ys, grads=None):
    arr = (_lib.MlpLayer * len(layers))()
    for k, (layer, y) in enumerate(zip(layers, ys)):
        e = arr[k]
        e.w, e.b = layer.weight.data_ptr(), _lib.ptr(layer.bias)
        e.y, e.ldy = y.data_ptr(), _ld(y)
        e.n, e.k, e.act = layer.weight.shape[0], layer.weight.shape[1], layer.act
        if grads is not None:
            e.gw, e.gb = grads[k][0].data_ptr(), _lib.ptr(grads[k][1])
    return arr


def _fusable(x, layers) -> bool:
    if not FUSED_MLP or len(layers) < 2 or len(layers) > 8:
        return False
    for layer in layers:
        n, k = layer.weight.shape
        if n > 128 or k > 128 or k % 8 or layer.bias is None or not layer.weight.is_contiguous():
            return False
    return x.shape[0] >= 1024


class Head:
    """single-unit layer on [x_extra | last activations] formed in the fused stack's epilogue
    (``ctr_mlp_head_t``): ``out = act(x_extra . w[:p] + y_last . w[p:] + c)``"""

    def __init__(self, x_extra: Optional[torch.Tensor], w: torch.Tensor, c: torch.Tensor, act: int):
        self.x_extra, self.w, self.c, self.act = x_extra, w, c, act
        self.out: Optional[torch.Tensor] = None  # (m, 1), set by mlp_fwd


def mlp_fwd(x: torch.Tensor, layers: Sequence[Layer], last_out: Optional[torch.Tensor] = None,
            head: Optional[Head] = None) -> List[torch.Tensor]:
    """returns [x, y_1, ..., y_n]; the last layer may write into ``last_out``.  With ``head`` the
    single-unit layer on top is computed too and left in ``head.out`` (in the same launch when the
    stack runs fused, else by ``linear_fwd`` on the concatenation-free operand, which then must be
    the columns right in front of ``last_out``)."""
    x = _mat(x, "x")
    m = x.shape[0]
    if _fusable(x, layers):
        ys = [torch.empty((m, layer.weight.shape[0]), dtype=torch.float32, device=x.device) for layer in layers[:-1]]
        ys.append(last_out if last_out is not None else
                  torch.empty((m, layers[-1].weight.shape[0]), dtype=torch.float32, device=x.device))
        arr = _mlp_layer_array(layers, ys)
        dims = [(layer.weight.shape[0], layer.weight.shape[1]) for layer in layers]
        lib = _lib.load()
        if head is not None:
            p = 0 if head.x_extra is None else head.x_extra.shape[1]
            out = torch.empty((m, 1), dtype=torch.float32, device=x.device)
            hd = _lib.MlpHead(_lib.ptr(head.x_extra), _ld(head.x_extra) if p else 0, head.w.data_ptr(),
                              head.c.data_ptr(), out.data_ptr(), 1, p, head.act)
            rc = _timed("mlp_fused_fwd", lambda: (4 * m * (dims[0][1] + p + 1 + sum(n for n, _ in dims)),
                                                  2 * m * (sum(n * k for n, k in dims) + p + dims[-1][0])),
                        lib.ctr_mlp_head_fwd, x.data_ptr(), _ld(x), m, arr, len(layers), C.byref(hd), _lib.stream_ptr())
            if not _refused(rc, "mlp_fused_fwd"):
                _lib.check(rc, "ctr_mlp_head_fwd")
                head.out = out
                return [x] + ys
        rc = _timed("mlp_fused_fwd", lambda: (4 * m * (dims[0][1] + sum(n for n, _ in dims)),
                                              2 * m * sum(n * k for n, k in dims)),
                    lib.ctr_mlp_fwd, x.data_ptr(), _ld(x), m, arr, len(layers), _lib.stream_ptr())
        if not _refused(rc, "mlp_fused_fwd"):
            _lib.check(rc, "ctr_mlp_fwd")
            _head_unfused(head, ys[-1])
            return [x] + ys
    acts = [x]
    for k, layer in enumerate(layers):
        out = last_out if (k == len(layers) - 1) else None
        acts.append(linear_fwd(acts[-1], layer.weight, layer.bias, layer.act, out=out))
    _head_unfused(head, acts[-1])
    return acts


def embed_mlp_head_fwd(specs: Sequence[FieldSpec], batch: int, buf: torch.Tensor, k0: int, layers: Sequence[Layer],
                       head: Head, last_out: torch.Tensor, err_flag: Optional[torch.Tensor] = None, write_x: bool = True,
                       fold: Optional[tuple] = None):
    """``embed_fwd(specs -> buf)`` and ``mlp_fwd(buf[:, :k0], layers, last_out, head)`` in ONE launch
    (ctr_embed_mlp_head_fwd) where the library has a kernel for the pattern (NeuralCF at BASELINE configs[1]); returns
    the activation list of ``mlp_fwd`` or None when it refused (nothing was enqueued: issue the two calls).
    ``write_x=False``: ``buf[:, :k0]`` is left untouched and the backward has to be ``embed_mlp_head_bwd``.
    ``fold=(u_full, w, b, b2)``: ``fold_head_fwd`` done by the same launch -- ``head.w`` / ``head.c`` are then OUTPUTS
    (uninitialised buffers of the folded shape) that the kernel fills for the backward."""
    buf = _mat(buf, "buf")
    x = buf[:, :k0]
    if not _fusable(x, layers) or head.x_extra is None:
        return None
    m = batch
    ys = [torch.empty((m, layer.weight.shape[0]), dtype=torch.float32, device=buf.device) for layer in layers[:-1]]
    ys.append(last_out)
    arr = _mlp_layer_array(layers, ys)
    farr = _field_array(specs)
    dims = [(layer.weight.shape[0], layer.weight.shape[1]) for layer in layers]
    p = head.x_extra.shape[1]
    out = torch.empty((m, 1), dtype=torch.float32, device=buf.device)
    hd = _lib.MlpHead(_lib.ptr(head.x_extra), _ld(head.x_extra), head.w.data_ptr(), head.c.data_ptr(), out.data_ptr(), 1, p,
                      head.act)
    fd = None
    if fold is not None:
        u_full, fw, fb, fb2 = fold
        fd = _lib.HeadFold(u_full.data_ptr(), fw.data_ptr(), _ld(fw), _lib.ptr(fb), _lib.ptr(fb2), head.w.data_ptr(),
                           head.c.data_ptr(), p, fw.shape[0], fw.shape[1], 0)
    rc = _timed("embed_mlp_fused_fwd",
                lambda: (_embed_bytes(specs, batch, False) + 4 * m * (1 + sum(n for n, _ in dims)),
                         2 * m * (sum(n * k for n, k in dims) + p + dims[-1][0])),
                _lib.load().ctr_embed_mlp_head_fwd, farr, len(specs), batch, buf.data_ptr(), _ld(buf), _lib.ptr(err_flag),
                1 if write_x else 0, arr, len(layers), C.byref(hd), C.byref(fd) if fd is not None else None,
                _lib.stream_ptr())
    if _refused(rc, "embed_mlp_fused_fwd"):
        return None
    _lib.check(rc, "ctr_embed_mlp_head_fwd")
    head.out = out
    return [x] + ys


def _head_unfused(head: Optional[Head], y_last: torch.Tensor) -> None:
    if head is None:
        return
    if head.x_extra is None:
        operand = y_last
    else:
        # [x_extra | y_last] must already be adjacent columns of one buffer (no torch.cat on the hot path)
        p, n = head.x_extra.shape[1], y_last.shape[1]
        adjacent = (head.x_extra.stride(0) == y_last.stride(0) and
                    head.x_extra.data_ptr() + 4 * p == y_last.data_ptr())
        operand = (torch.as_strided(head.x_extra, (head.x_extra.shape[0], p + n), (head.x_extra.stride(0), 1))
                   if adjacent else torch.cat([head.x_extra, y_last], dim=1))
    head.out = linear_fwd(operand, head.w, head.c, head.act)


def mlp_head_bwd(acts: Sequence[torch.Tensor], layers: Sequence[Layer], head: Head, prob: torch.Tensor,
                 gprob: torch.Tensor, g_extra: torch.Tensor, gw_head: torch.Tensor, gc_head: torch.Tensor,
                 gx_first: torch.Tensor, zeros: dict, gather_specs: Optional[Sequence[FieldSpec]] = None,
                 fold_grad: Optional[tuple] = None, zero: Optional[torch.Tensor] = None):
    """backward of ``mlp_fwd(..., head=head)`` in one launch (ctr_mlp_head_bwd): the head's gz, the stack's
    backward, ``g_extra = gz * w[:p]`` and the head's weight / bias sums.  Returns the per-layer
    ``[(gw, gb)]`` or None when the library has no fused path for this stack (nothing was enqueued)."""
    if not _fusable(acts[0], layers) or head.x_extra is None:
        return None
    grads = [(zeros[id(layer.weight)], zeros[id(layer.bias)]) for layer in layers]
    x0 = _mat(acts[0], "x")
    m = x0.shape[0]
    arr = _mlp_layer_array(layers, acts[1:], grads)
    ws = _scratch(x0.device)
    dims = [(layer.weight.shape[0], layer.weight.shape[1]) for layer in layers]
    p = head.x_extra.shape[1]
    prob, gprob = prob.reshape(-1), gprob.reshape(-1)
    hg = _lib.MlpHeadGrad(prob.data_ptr(), prob.stride(0), gprob.data_ptr(), gprob.stride(0), head.x_extra.data_ptr(),
                          _ld(head.x_extra), head.w.data_ptr(), g_extra.data_ptr(), _ld(g_extra), gw_head.data_ptr(),
                          gc_head.data_ptr(), p, head.act)
    meta = lambda: (4 * m * (2 * dims[0][1] + sum(n for n, _ in dims) + 2 * p + 2),  # noqa: E731
                    4 * m * (sum(n * k for n, k in dims) + p + dims[-1][0]))
    # read: stack input, every saved activation, the extra columns, prob, gprob; written: gX, g_extra.
    # flops: dW + dX of every layer, the head's products and sums
    if gather_specs is not None:
        # the forward ran embed_mlp_head_fwd(write_x=False): the stack input is gathered again from the tables
        farr = _field_array(gather_specs)
        fg = None
        if fold_grad is not None:
            # fold_head_bwd in the reduction launch of the same call: (u_full, w, b, gu_full, gw, gb, gb2)
            fu, fw, fb, gu, gw_, gb_, gb2_ = fold_grad
            fg = _lib.HeadFoldGrad(fu.data_ptr(), fw.data_ptr(), _ld(fw), _lib.ptr(fb), _lib.ptr(gu), _lib.ptr(gw_),
                                   _ld(gw_) if gw_ is not None else 0, _lib.ptr(gb_), _lib.ptr(gb2_), p, fw.shape[0],
                                   fw.shape[1], 0)
        rc = _timed("mlp_fused_bwd", meta, _lib.load().ctr_embed_mlp_head_bwd, farr, len(gather_specs), m, arr, len(layers),
                    C.byref(hg), C.byref(fg) if fg is not None else None, gx_first.data_ptr(), _ld(gx_first), ws.data_ptr(),
                    ws.numel(), _lib.ptr(zero), zero.numel() if zero is not None else 0, _lib.stream_ptr())
        _lib.check(rc, "ctr_embed_mlp_head_bwd")  # a refusal is an error here: the input columns were never written
        return grads
    rc = _timed("mlp_fused_bwd", meta, _lib.load().ctr_mlp_head_bwd, x0.data_ptr(), _ld(x0), m, arr, len(layers),
                C.byref(hg), gx_first.data_ptr(), _ld(gx_first), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    if _refused(rc, "mlp_fused_bwd"):
        return None
    _lib.check(rc, "ctr_mlp_head_bwd")
    return grads


def mlp_bwd(acts: Sequence[torch.Tensor], layers: Sequence[Layer], gy: torch.Tensor,
            gx_first: Optional[torch.Tensor], want_gx_first: bool = True, zeros: Optional[dict] = None):
    """backward through ``mlp_fwd``; returns ([(gw, gb) per layer], gx of the
    first layer input or None)"""
    grads = [None] * len(layers)
    if _fusable(acts[0], layers):
        # whole stack in one launch: dX chain in LDS, dW tiles in registers
        for k, layer in enumerate(layers):
            if zeros is not None:
                grads[k] = (zeros[id(layer.weight)], zeros[id(layer.bias)])
            else:
                grads[k] = (torch.zeros_like(layer.weight), torch.zeros_like(layer.bias))
        x0 = _mat(acts[0], "x")
        m = x0.shape[0]
        gx = gx_first if want_gx_first else None
        if want_gx_first and gx is None:
            gx = torch.empty((m, x0.shape[1]), dtype=torch.float32, device=x0.device)
        gy = _mat(gy, "gy")
        arr = _mlp_layer_array(layers, acts[1:], grads)
        ws = _scratch(x0.device)
        dims = [(layer.weight.shape[0], layer.weight.shape[1]) for layer in layers]
        # algorithmic bytes: x and every intermediate Y read once (as the next layer's input; the
        # activation mask is folded into the dX write-back), gY read, the last Y only when it has an
        # activation to mask, gX written
        last_mask = dims[-1][0] if layers[-1].act != ACT_NONE else 0
        rc = _timed("mlp_fused_bwd", lambda: (4 * m * (dims[0][1] + sum(n for n, _ in dims[:-1]) + dims[-1][0] +
                                                       last_mask + (dims[0][1] if gx is not None else 0)),
                                              4 * m * sum(n * k for n, k in dims)),
                    _lib.load().ctr_mlp_bwd, x0.data_ptr(), _ld(x0), m, arr, len(layers), gy.data_ptr(), _ld(gy),
                    _lib.ptr(gx), _ld(gx) if gx is not None else 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        if not _refused(rc, "mlp_fused_bwd"):
            _lib.check(rc, "ctr_mlp_bwd")
            return grads, gx
    g = gy
    for k in range(len(layers) - 1, -1, -1):
        layer = layers[k]
        xin, yout = acts[k], acts[k + 1]
        if zeros is not None:
            gw = zeros[id(layer.weight)]
            gb = zeros[id(layer.bias)] if layer.bias is not None else None
        else:
            gw = torch.zeros_like(layer.weight)
            gb = torch.zeros_like(layer.bias) if layer.bias is not None else None
        if k > 0:
            gx = torch.empty((xin.shape[0], xin.shape[1]), dtype=torch.float32, device=xin.device)
        else:
            gx = gx_first if want_gx_first else None
            if want_gx_first and gx is None:
                gx = torch.empty((xin.shape[0], xin.shape[1]), dtype=torch.float32, device=xin.device)
        linear_bwd(xin, layer.weight, yout, g, layer.act, gx, gw, gb)
        grads[k] = (gw, gb)
        g = gx
    return grads, g


def rows_sum_act_fwd(table_a, idx_a, table_b, idx_b, act: int, out, err_flag=None) -> torch.Tensor:
    """out[b] = act(table_a[idx_a[b]] + table_b[idx_b[b]]) (ctr_rows_sum_act_fwd)"""
    out = _mat(out, "out")
    _lib.require_device(table_a, table_b, idx_a, idx_b)
    batch, width = idx_a.numel(), table_a.shape[1]
    rc = _timed("rows_sum_act_fwd", lambda: (batch * (16 + 12 * width), batch * width),
                _lib.load().ctr_rows_sum_act_fwd, table_a.data_ptr(), idx_a.data_ptr(), idx_a.stride(0) if batch > 1 else 1,
                table_a.shape[0], table_b.data_ptr(), idx_b.data_ptr(), idx_b.stride(0) if batch > 1 else 1, table_b.shape[0],
                batch, width, act, out.data_ptr(), _ld(out), _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_rows_sum_act_fwd")
    return out


def act_mask_bwd(g, y, act: int) -> None:
    """g *= act'(y) in place (ctr_act_mask_bwd)"""
    g, y = _mat(g, "g"), _mat(y, "y")
    m, n = g.shape
    rc = _timed("act_mask_bwd", lambda: (12 * m * n, m * n), _lib.load().ctr_act_mask_bwd, g.data_ptr(), _ld(g),
                y.data_ptr(), _ld(y), m, n, act, _lib.stream_ptr())
    _lib.check(rc, "ctr_act_mask_bwd")


# ---------------------------------------------------------------------------
# NeuralCF with the first tower layer on the table rows (csrc/ncf_proj.hip)
# ---------------------------------------------------------------------------
def few_table_rows(rows: int, batch: int) -> bool:
    """the admission both of NeuralCF's table-row paths share: a batch worth a launch over the tables' ``rows`` (both
    tables together), with every row met by four samples on average"""
    return batch >= 4096 and batch >= 4 * rows


class NcfCounts:
    """the bucket plan of ``ctr_ncf_proj_fwd`` (one holder per model): per-row sample counts of the batch's chunks,
    row totals, bucket offsets and block totals, built by every training forward and read by its backward.  The
    kernels write every entry they read later and never touch the buffer's first word (it stays the zero written
    here), so in the usual forward -> backward rhythm the buffer is filled once, here.  ``take`` hands it out when no
    forward owns it; while a forward's plan still waits for its
    backward (two graphs alive at once) a later forward gets a freshly zeroed buffer of its own instead, and after a
    training forward that never got its backward the buffer is cleared before it is handed out again."""

    def __init__(self):
        self.buf, self.state = None, "clean"

    def take(self, rows: int, device):
        n = rows * _lib.CTR_NCF_PROJ_COUNT_STRIDE      # chunk counts, total and offset per row (ctrhip.h)
        if self.buf is None or self.buf.numel() < n or self.buf.device != device:
            self.buf, self.state = torch.zeros(n, dtype=torch.int32, device=device), "clean"
        if self.state == "dirty":            # a training forward whose graph was dropped without a backward
            self.buf.zero_()
            self.state = "clean"
        if self.state == "clean":
            self.state = "busy"
            return self.buf, True
        return torch.zeros(n, dtype=torch.int32, device=device), False


class NcfProj:
    """one forward of ``ctr_ncf_proj_fwd`` and what its backward needs.  ``tables`` = (gmf_u, gmf_i, mlp_u, mlp_i),
    ``hidden`` = the four tower layers, ``proj`` = (w, b) of ``linear``, ``head`` = (w, b) of ``linear2``."""

    def __init__(self, user_idx, item_idx, tables, hidden, proj, head, err_flag, training, counts: "NcfCounts" = None):
        self.user_idx, self.item_idx = user_idx, item_idx
        self.tables, self.hidden, self.proj, self.head = tables, hidden, proj, head
        gmf_u, gmf_i, mlp_u, mlp_i = tables
        dev = gmf_u.device
        self.batch, self.nu, self.ni = user_idx.numel(), gmf_u.shape[0], gmf_i.shape[0]
        m, rows = self.batch, self.nu + self.ni
        self.ptab = torch.empty((rows, hidden[0].weight.shape[0]), dtype=torch.float32, device=dev)
        self.wfold = torch.empty(76, dtype=torch.float32, device=dev)
        # every per-sample buffer has a spare row m: lanes without a sample store there (unconditional, countable stores)
        self.ys = [torch.empty((m + 1, layer.weight.shape[0]), dtype=torch.float32, device=dev) for layer in hidden[1:]]
        self.prob_buf = torch.empty((m + 1, 1), dtype=torch.float32, device=dev)
        self.prob = self.prob_buf[:m]
        self._holder, self._owns = None, False
        self.plan = self.ranks = None
        if training:
            self._holder = counts if counts is not None else NcfCounts()
            self.plan, self._owns = self._holder.take(rows, dev)
            self.ranks = torch.empty(2 * (m + 1), dtype=torch.int32, device=dev)
        self.err_flag, self.training = err_flag, training

    def __del__(self):
        # a training forward that never saw its backward: the holder clears the plan before it hands it out again
        if getattr(self, "_owns", False) and self._holder.state == "busy":
            self._holder.state = "dirty"

    def _desc(self):
        gmf_u, gmf_i, mlp_u, mlp_i = self.tables
        d = _lib.NcfProj()
        d.user_idx, d.user_stride = self.user_idx.data_ptr(), self.user_idx.stride(0) if self.user_idx.numel() > 1 else 1
        d.item_idx, d.item_stride = self.item_idx.data_ptr(), self.item_idx.stride(0) if self.item_idx.numel() > 1 else 1
        d.batch, d.num_users, d.num_items = self.batch, self.nu, self.ni
        d.mlp_user, d.mlp_item, d.gmf_user, d.gmf_item = (t.data_ptr() for t in (mlp_u, mlp_i, gmf_u, gmf_i))
        d.mlp_dim, d.mf_dim = mlp_u.shape[1], gmf_u.shape[1]
        for k, layer in enumerate(self.hidden):
            e = d.layers[k]
            e.w, e.b, e.n, e.k, e.act = layer.weight.data_ptr(), _lib.ptr(layer.bias), layer.weight.shape[0], layer.weight.shape[1], layer.act
            if k:
                e.y, e.ldy = self.ys[k - 1].data_ptr(), _ld(self.ys[k - 1])
        pw, pb = self.proj
        hw, hb = self.head
        d.proj_w, d.ld_proj_w, d.proj_b, d.proj_n, d.proj_k = pw.data_ptr(), _ld(pw), _lib.ptr(pb), pw.shape[0], pw.shape[1]
        d.head_w, d.head_b, d.head_act = hw.data_ptr(), _lib.ptr(hb), ACT_SIGMOID
        d.prob, d.ldprob, d.err_flag = self.prob.data_ptr(), 1, _lib.ptr(self.err_flag)
        d.ptab, d.wfold, d.plan, d.ranks = self.ptab.data_ptr(), self.wfold.data_ptr(), _lib.ptr(self.plan), _lib.ptr(self.ranks)
        d.training = 1 if self.training else 0
        return d

    def bucket_offsets(self) -> torch.Tensor:
        """(rows + 1) int32 of the training forward's plan: row v's bucket is the slots [o[v], o[v + 1]), user rows first
        (the plan's layout, csrc/ncf_proj.hip: 4 int32 of head, 64 chunks x rows bases, rows totals, the offsets, then
        the block totals)"""
        rows = self.nu + self.ni
        return self.plan[4 + 65 * rows: 4 + 66 * rows + 1]

    @staticmethod
    def supported(tables, hidden, proj, batch) -> bool:
        gmf_u, gmf_i, mlp_u, mlp_i = tables
        rows = gmf_u.shape[0] + gmf_i.shape[0]
        dims = [tuple(layer.weight.shape) for layer in hidden]
        return (dims == [(64, 128), (32, 64), (16, 32), (8, 16)] and gmf_u.shape[1] == 64 and mlp_u.shape[1] == 64 and
                tuple(proj[0].shape) == (64, 8) and all(layer.bias is not None for layer in hidden) and
                rows <= _lib.CTR_NCF_PROJ_MAX_ROWS and few_table_rows(rows, batch) and 2 * batch < 2 ** 31)

    # algorithmic bytes / flops of the launches: per sample unless said otherwise
    def _meta(self, which):
        m, rows = self.batch, self.nu + self.ni
        tower = 64 * 32 + 32 * 16 + 16 * 8
        shift = 8                            # the plan's chunks of the batch (csrc/ncf_proj.hip, plan_of)
        while (64 << shift) < m:
            shift += 1
        chunks = -(-m // (1 << shift))
        blocks = -(-rows // 256)             # the rows of one plan workgroup; block totals only for more than one
        blk = chunks * blocks * 4 if blocks > 1 else 0
        return {
            # (rows, 64) tables read, (rows, 64) projected rows written; one 64 x 64 product per row
            # (+ in training, by the rank workgroups of the same launch: ids, an 8-byte rank record per sample, a
            # histogram of the rows per chunk and its sums over the blocks)
            "ncfp_prep": lambda: (rows * 512 + ((m * (16 + 8) + chunks * rows * 4 + blk) if self.training else 0),
                                  2 * rows * 64 * 64),
            # ids, four 256-byte rows (cache-resident tables), saved activations + prob written; tower + head
            # (+ in training, by the plan workgroups of the same launch: the histograms read and written back as
            # absolute bases, row totals and bucket offsets written, and plan workgroup k reads the block totals of
            # the k blocks in front of it)
            "ncfp_fwd": lambda: (m * (16 + 4 * 256 + 4 * (32 + 16 + 8) + 4) +
                                 ((2 * chunks * rows * 4 + 2 * rows * 4 + blk * (blocks - 1) // 2) if self.training else 0),
                                 2 * m * (tower + 72 + 64)),
            # ids, prob, gprob, ranks, two absolute bases (slot = base + rank: no copy of the offsets), two projected
            # rows, saved activations read; gz0 row stored once + two records
            "ncfp_bwd": lambda: (m * (16 + 16 + 8 + 2 * 256 + 4 * (32 + 16 + 8) + 256 + 32), 4 * m * tower + 2 * m * 8),
            # per slot: its record, the gz0 row and the partner row the record names read; (rows, 128) sums added
            # (the slab reduction and the head fold left this launch: they ride with ncfp_finish, phase 4)
            "ncfp_segsum": lambda: (2 * m * (256 + 16 + 256) + rows * 512, 2 * 2 * m * 64 * 2),
            # sums + tables read, table gradients read-modify-written; three 64 x 64 products per row
            # (+ on workgroups of their own: ncfp_bwd's slabs summed into the tower gradients, the head fold's chain
            # rule and the fused loss -- a few hundred KB, not counted)
            "ncfp_finish": lambda: (rows * (512 + 512 + 4 * 256), 3 * 2 * rows * 64 * 64),
        }[which]

    def forward(self) -> torch.Tensor:
        d = self._desc()
        fn = _lib.load().ctr_ncf_proj_fwd
        if _profiler is None:
            rc = fn(C.byref(d), _lib.stream_ptr())
        else:   # one call per launch, so that each gets its own event pair
            rc = 0
            for phase, label in ((1, "ncfp_prep"), (2, "ncfp_fwd")):
                d.phases = phase
                rc = rc or _timed(label, self._meta(label), fn, C.byref(d), _lib.stream_ptr())
        if rc in _REFUSED:
            return None
        _lib.check(rc, "ctr_ncf_proj_fwd")
        return self.prob

    def backward(self, gprob: Optional[torch.Tensor], grads: dict, zero: Optional[torch.Tensor],
                 target: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None) -> None:
        """``grads[id(param)]``: where each parameter's gradient accumulates; ``zero``: the flat buffer behind them,
        cleared by the call's first launch.  With ``target`` (float32, one element per sample, any stride) ``gprob`` is
        not read: the gradient is the binary cross entropy's for an upstream of exactly 1, formed inside the per-sample
        launch, and ``loss`` (a float32 scalar, optional) receives the mean loss from the call's last launch."""
        if getattr(self, "_spent", False):
            # the first backward hands the plan buffer back to its holder: the next forward may have rebuilt it for
            # other ids by the time a second backward over this forward would read it
            raise RuntimeError("NeuralCF backward consumes what its forward saved: run the forward again before a second "
                               "backward (retain_graph is not supported)")
        self._spent = True
        gmf_u, gmf_i, mlp_u, mlp_i = self.tables
        d = self._desc()
        g = _lib.NcfProjGrad()
        if gprob is not None:
            gprob = gprob.reshape(-1)
            g.gprob, g.ldgprob = gprob.data_ptr(), gprob.stride(0) if gprob.numel() > 1 else 1
        if target is not None:
            _lib.require_device(target)
            if target.dtype != torch.float32 or target.dim() != 1 or target.numel() != self.batch:
                raise ValueError("NcfProj.backward: target must be float32 with one element per sample, flattened")
            g.target, g.ldtarget = target.data_ptr(), target.stride(0) if target.numel() > 1 else 1
        if loss is not None:
            _lib.require_device(loss)
            if loss.dtype != torch.float32 or loss.numel() != 1:
                raise ValueError("NcfProj.backward: loss must be one float32")
            g.loss = loss.data_ptr()
        for k, layer in enumerate(self.hidden):
            g.layers[k].gw, g.layers[k].gb = grads[id(layer.weight)].data_ptr(), grads[id(layer.bias)].data_ptr()
        g.g_mlp_user, g.g_mlp_item, g.g_gmf_user, g.g_gmf_item = (grads[id(t)].data_ptr() for t in (mlp_u, mlp_i, gmf_u, gmf_i))
        pw, pb = self.proj
        hw, hb = self.head
        g.g_proj_w, g.ld_g_proj_w, g.g_proj_b = grads[id(pw)].data_ptr(), _ld(grads[id(pw)]), _lib.ptr(grads.get(id(pb)))
        g.g_head_w, g.g_head_b = grads[id(hw)].data_ptr(), _lib.ptr(grads.get(id(hb)))
        need = C.c_int64(0)
        _lib.check(_lib.load().ctr_ncf_proj_workspace_floats(self.batch, self.nu, self.ni, C.byref(need)), "workspace")
        ws = _scratch(gmf_u.device) if need.value <= SCRATCH_FLOATS else torch.empty(need.value, dtype=torch.float32,
                                                                                      device=gmf_u.device)
        g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
        g.zero_buf, g.zero_floats = _lib.ptr(zero), zero.numel() if zero is not None else 0
        fn = _lib.load().ctr_ncf_proj_bwd
        if _profiler is None:
            rc = fn(C.byref(d), C.byref(g), _lib.stream_ptr())
        else:
            rc = 0
            for phase, label in ((1, "ncfp_bwd"), (2, "ncfp_segsum"), (4, "ncfp_finish")):
                g.phases = phase
                rc = rc or _timed(label, self._meta(label), fn, C.byref(d), C.byref(g), _lib.stream_ptr())
        _lib.check(rc, "ctr_ncf_proj_bwd")
        if self._owns:
            self._holder.state = "clean"     # (the plan has been read; the next forward rewrites what it reads)
        self._owns = False


# ---------------------------------------------------------------------------
# the grid scorers' wrappers (csrc/*_grid.hip): what they check alike, under the calling wrapper's ``name``
# ---------------------------------------------------------------------------
def _grid_rows(name, users, user0, rows, nu, ni, out, device):
    """(user0, rows, out) of a user-grid call: the rows are ``users`` (1-D int64), else the users ``user0 .. user0 +
    rows`` (``rows`` None: up to the table's end); ``out`` is (rows, ni), checked or fresh"""
    if users is not None:
        _i64(users)
        if users.dim() != 1:
            raise ValueError(f"{name}: users must be 1-D")
        rows, user0 = users.numel(), 0
    elif rows is None:
        rows = nu - user0
    if out is None:
        out = torch.empty((rows, ni), dtype=torch.float32, device=device)
    out = _mat(out, "out")
    if out.shape != (rows, ni):
        raise ValueError(f"{name}: out must be ({rows}, {ni})")
    return user0, rows, out


def _history_rows(name, hist):
    """(R, L) of the history matrix of a history-grid call"""
    _i64(hist)
    if hist.dim() != 2 or hist.shape[1] < 1:
        raise ValueError(f"{name}: hist must be (R, L) with L >= 1, got {tuple(hist.shape)}")
    return hist.shape


def _history_out(name, out, pairs, dim, device):
    """the (pairs, >= dim) left half of the fc operand: ``out`` checked, or a fresh one"""
    if out is None:
        out = torch.empty((pairs, dim), dtype=torch.float32, device=device)
    out = _mat(out, "out")
    if out.shape[0] != pairs or out.shape[1] < dim:
        raise ValueError(f"{name}: out must be ({pairs}, >= {dim})")
    return out


def _f32_vectors(name, what, *tensors):
    """``tensors`` flattened and contiguous on the device, float32 or ``name: what must be float32``"""
    vecs = [t.detach().reshape(-1).contiguous() for t in tensors]
    _lib.require_device(*vecs)
    if any(t.dtype != torch.float32 for t in vecs):
        raise ValueError(f"{name}: {what} must be float32")
    return vecs


def _attention_shapes_match(embed_size, attention_dims, want_embed, want_dims) -> bool:
    return int(embed_size) == want_embed and tuple(tuple(int(v) for v in d) for d in attention_dims) == want_dims


# ---------------------------------------------------------------------------
# NeuralCF over the user x item grid (csrc/ncf_grid.hip)
# ---------------------------------------------------------------------------
def ncf_grid_supported(tables, hidden, proj) -> bool:
    """whether ``ctr_ncf_grid_scores`` takes the model: the shape test of ``NcfProj.supported`` without the batch and
    without the row cap (both belong to the training plan).  A function of shapes alone: CPU or meta tensors will do."""
    gmf_u, gmf_i, mlp_u, mlp_i = tables
    dims = [tuple(layer.weight.shape) for layer in hidden]
    return (dims == [(64, 128), (32, 64), (16, 32), (8, 16)] and gmf_u.shape[1] == 64 and mlp_u.shape[1] == 64 and
            tuple(proj[0].shape) == (64, 8) and all(layer.bias is not None for layer in hidden) and
            1 <= gmf_u.shape[0] < 2 ** 31 and 1 <= gmf_i.shape[0] < 2 ** 31)


def ncf_grid_scores(p_u: torch.Tensor, p_i: torch.Tensor, gmf_u: torch.Tensor, gmf_i: torch.Tensor,
                    layers: Sequence[Layer], wfold: torch.Tensor, cfold: torch.Tensor,
                    users: Optional[torch.Tensor] = None, user0: int = 0, rows: Optional[int] = None,
                    act: int = ACT_SIGMOID, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows, num_items) float32: ``act([gmf_u[u] * gmf_i[i] | tower(relu(p_u[u] + p_i[i]))] . wfold + cfold)`` for the
    users ``users`` (1-D int64, validated by the caller) or ``user0 .. user0 + rows`` against every item
    (ctr_ncf_grid_scores).  ``p_u`` / ``p_i``: the first tower layer applied to the table rows, ``layers`` the remaining
    ones, ``wfold`` / ``cfold`` from ``fold_head_fwd``.  A shape the kernel is not built for raises: there is no
    other path behind this call (``ncf_grid_supported`` says beforehand)."""
    p_u, p_i, gmf_u, gmf_i = (_mat(t, w).contiguous() for t, w in ((p_u, "p_u"), (p_i, "p_i"), (gmf_u, "gmf_u"),
                                                                    (gmf_i, "gmf_i")))
    _lib.require_device(wfold, cfold)
    nu, ni = gmf_u.shape[0], gmf_i.shape[0]
    if p_u.shape[0] != nu or p_i.shape[0] != ni:
        raise ValueError("ncf_grid_scores: the projected tables and the GMF tables differ in rows")
    user0, rows, out = _grid_rows("ncf_grid_scores", users, user0, rows, nu, ni, out, gmf_u.device)
    arr = (_lib.MlpLayer * len(layers))()
    for k, layer in enumerate(layers):
        w = layer.weight
        if not w.is_contiguous():
            raise ValueError("ncf_grid_scores: tower weights must be contiguous")
        arr[k].w, arr[k].b, arr[k].n, arr[k].k, arr[k].act = w.data_ptr(), _lib.ptr(layer.bias), w.shape[0], w.shape[1], layer.act
    tower = sum(layer.weight.numel() for layer in layers)
    mf, width = gmf_u.shape[1], p_u.shape[1]
    fold_k = wfold.numel() - mf
    # algorithmic: every table row of the call read once (the user tiles re-read item rows from cache), the scores
    # written; per pair the tower, the relu'd sum of the projected rows and the mf + fold_k term dot
    rc = _timed("ncf_grid_scores",
                lambda: (4 * ((rows + ni) * (width + mf) + rows * ni) + (8 * rows if users is not None else 0),
                         rows * ni * (2 * tower + 2 * (mf + fold_k) + width)),
                _lib.load().ctr_ncf_grid_scores, p_u.data_ptr(), p_i.data_ptr(), gmf_u.data_ptr(), gmf_i.data_ptr(),
                nu, ni, mf, width, arr, len(layers), wfold.data_ptr(), cfold.data_ptr(), fold_k,
                _lib.ptr(users) if users is not None and rows else None, user0, rows, act,
                _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, _lib.stream_ptr())
    _lib.check(rc, "ctr_ncf_grid_scores")
    return out


# ---------------------------------------------------------------------------
# DIN over the history x item grid (csrc/din_grid.hip)
# ---------------------------------------------------------------------------
DIN_GRID_EMBED = 64
DIN_GRID_ATTENTION = ((128, 3 * DIN_GRID_EMBED), (64, 128), (1, 64))


def din_grid_supported(embed_size: int, attention_dims) -> bool:
    """whether ``ctr_din_grid_pool`` takes a DIN of this embedding width whose attention ``Linear`` weights have the
    shapes ``attention_dims`` ((out, in) per layer).  A function of shapes alone: CPU or meta tensors will do."""
    return _attention_shapes_match(embed_size, attention_dims, DIN_GRID_EMBED, DIN_GRID_ATTENTION)


def din_grid_pool(table: torch.Tensor, at: torch.Tensor, ah: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                  w3: torch.Tensor, hist: torch.Tensor, out: Optional[torch.Tensor] = None,
                  ah_by_position: bool = False, err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[r * I + i, :E] = sum_l softmax_l(w3 . relu(w2 relu(AH[r, l] + at[i]) + b2))[l] * table[hist[r, l]]`` for every
    history row r of ``hist`` (R, L) and EVERY item i (ctr_din_grid_pool).  ``at`` (I, 128) is the item part of the first
    attention layer, ``ah`` its history part: (I, 128) read by history id, or -- ``ah_by_position`` -- (R * L, 128) read
    by position.  ``out``: (R * I, >= E) with a row stride that is a multiple of 4 floats (a view of the fc operand);
    columns past E are left alone.  A shape the kernel is not built for raises: there is no other path behind this call
    (``din_grid_supported`` says beforehand)."""
    table, at, ah, w2 = (_mat(t, w) for t, w in ((table, "table"), (at, "at"), (ah, "ah"), (w2, "w2")))
    _lib.require_device(b2, w3, err_flag)
    rows, length = _history_rows("din_grid_pool", hist)
    ni, dim = table.shape
    if not (table.is_contiguous() and at.is_contiguous() and ah.is_contiguous() and w2.is_contiguous()
            and b2.is_contiguous() and w3.is_contiguous()):
        raise ValueError("din_grid_pool: table, at, ah and the weights must be contiguous")
    n2, n1 = w2.shape
    if at.shape != (ni, n1) or ah.shape != ((rows * length) if ah_by_position else ni, n1):
        raise ValueError(f"din_grid_pool: at {tuple(at.shape)} / ah {tuple(ah.shape)} do not fit {ni} items, "
                         f"{rows} x {length} positions")
    if b2.numel() != n2 or w3.numel() != n2:
        raise ValueError("din_grid_pool: b2 and w3 must have one element per unit of w2")
    out = _history_out("din_grid_pool", out, rows * ni, dim, table.device)
    if rows * ni == 0:
        return out
    # algorithmic: the table-side rows of the call read once (the row tiles re-read them from cache), the pooled rows
    # written; per pair and position the 128 -> 64 layer, the relu'd sum, the score dot and the weighted sum
    rc = _timed("din_grid_pool",
                lambda: (4 * (ni * (dim + n1) + rows * length * (2 + n1 + dim) + rows * ni * dim),
                         rows * ni * length * (2 * n1 * n2 + n1 + 2 * n2 + 2 * dim)),
                _lib.load().ctr_din_grid_pool, table.data_ptr(), ni, dim, at.data_ptr(), ah.data_ptr(),
                int(ah_by_position), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), n1, n2,
                hist.data_ptr() if hist.numel() else None, rows, length, _lib.ptr(out) if out.numel() else None,
                max(_ld(out), dim) if out.shape[0] else dim, _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_din_grid_pool")
    return out


# ---------------------------------------------------------------------------
# DIEN over the history x item grid (csrc/dien_grid.hip)
# ---------------------------------------------------------------------------
DIEN_GRID_EMBED = 16
DIEN_GRID_ATTENTION = ((64, 3 * DIEN_GRID_EMBED), (32, 64), (1, 32))
DIEN_GRID_KEEP = _lib.CTR_DIEN_GRID_KEEP     # history positions whose score waits in LDS; later ones are recomputed


def dien_grid_supported(embed_size: int, attention_dims) -> bool:
    """whether ``ctr_dien_grid_hidden`` takes a DIEN of this embedding (= GRU) width whose attention ``Linear`` weights
    have the shapes ``attention_dims`` ((out, in) per layer).  A function of shapes alone: CPU or meta tensors will do."""
    return _attention_shapes_match(embed_size, attention_dims, DIEN_GRID_EMBED, DIEN_GRID_ATTENTION)


def dien_grid_hidden(at: torch.Tensor, hp: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor,
                     b_ih: torch.Tensor, w_hh: torch.Tensor, b_hh: torch.Tensor, hist: torch.Tensor,
                     out: Optional[torch.Tensor] = None, hp_by_position: bool = False,
                     err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[r * I + i, :E]`` = the last state of DIEN's GRU (h_0 = 0) over the attention-weighted history row r of
    ``hist`` (R, L) against EVERY item i (ctr_dien_grid_hidden).  ``at`` (I, 64) is the item part of the first attention
    layer; ``hp`` = [AH | GX] (112 wide) its history part next to the GRU's input projection without bias: (I, 112)
    read by history id, or -- ``hp_by_position`` -- (R * L, 112) read by position.  ``out``: (R * I, >= E) with a row
    stride that is a multiple of 4 floats (a view of the fc operand); columns past E are left alone.  A shape the
    kernel is not built for raises: there is no other path behind this call (``dien_grid_supported`` says beforehand)."""
    at, hp, w2, w_hh = (_mat(t, w) for t, w in ((at, "at"), (hp, "hp"), (w2, "w2"), (w_hh, "w_hh")))
    _lib.require_device(b2, w3, b_ih, b_hh, err_flag)
    if any(t.dtype != torch.float32 for t in (b2, w3, b_ih, b_hh)):
        raise ValueError("dien_grid_hidden: b2, w3, b_ih and b_hh must be float32")
    rows, length = _history_rows("dien_grid_hidden", hist)
    if not all(t.is_contiguous() for t in (at, hp, w2, b2, w3, b_ih, w_hh, b_hh)):
        raise ValueError("dien_grid_hidden: at, hp and the weights must be contiguous")
    ni, (n2, n1) = at.shape[0], w2.shape
    gates, dim = w_hh.shape
    if gates != 3 * dim or at.shape[1] != n1 or hp.shape != ((rows * length) if hp_by_position else ni, n1 + gates):
        raise ValueError(f"dien_grid_hidden: at {tuple(at.shape)} / hp {tuple(hp.shape)} / w_hh {tuple(w_hh.shape)} do "
                         f"not fit {ni} items, {rows} x {length} positions")
    if b2.numel() != n2 or w3.numel() != n2 or b_ih.numel() != gates or b_hh.numel() != gates:
        raise ValueError("dien_grid_hidden: b2 and w3 must have one element per unit of w2, b_ih and b_hh one per row "
                         "of w_hh")
    out = _history_out("dien_grid_hidden", out, rows * ni, dim, at.device)
    if rows * ni == 0:
        return out
    # algorithmic: the table-side rows of the call read once (the row tiles re-read them from cache), the states
    # written; per pair and position the 64 -> 32 layer, the relu'd sum, the score dot, the recurrent product and gates
    rc = _timed("dien_grid_hidden",
                lambda: (4 * (ni * n1 + rows * length * (2 + n1 + gates) + rows * ni * dim),
                         rows * ni * length * (2 * n1 * n2 + n1 + 2 * n2 + 2 * dim * gates + 4 * gates)),
                _lib.load().ctr_dien_grid_hidden, at.data_ptr(), hp.data_ptr(), int(hp_by_position), ni, dim,
                w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), n1, n2, b_ih.data_ptr(), w_hh.data_ptr(), b_hh.data_ptr(),
                hist.data_ptr(), rows, length, _lib.ptr(out), max(_ld(out), dim), _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_dien_grid_hidden")
    return out


# ---------------------------------------------------------------------------
# DeepFM over the user x item grid (csrc/deepfm_grid.hip)
# ---------------------------------------------------------------------------
DEEPFM_GRID_HIDDEN = (256, 128, 1)          # hidden_units[1:]; hidden_units[0] is free (it is folded into the table rows)
DEEPFM_GRID_ITEM_TILE = _lib.CTR_DEEPFM_GRID_ITEM_TILE     # items of a workgroup
DEEPFM_GRID_USER_TILE = _lib.CTR_DEEPFM_GRID_USER_TILE     # users staged at a time


def deepfm_grid_supported(hidden_units, embedding_dim) -> bool:
    """whether ``ctr_deepfm_grid_scores`` takes a six-field DeepFM of these ``hidden_units`` and this embedding width.
    A function of the two shapes alone."""
    hidden = tuple(int(h) for h in hidden_units)
    dim = int(embedding_dim)
    return len(hidden) == 4 and hidden[0] >= 1 and hidden[1:] == DEEPFM_GRID_HIDDEN and 16 <= dim <= 128 and dim % 16 == 0


def deepfm_grid_scores(zu: torch.Tensor, zi: torch.Tensor, su: torch.Tensor, si: torch.Tensor, a: torch.Tensor,
                       b: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor,
                       out_w: torch.Tensor, out_b: torch.Tensor, users: Optional[torch.Tensor] = None, user0: int = 0,
                       rows: Optional[int] = None, out: Optional[torch.Tensor] = None, row_blocks: int = 0) -> torch.Tensor:
    """(rows, num_items) float32: ``sigmoid(out_w[0] (a[u] + b[i] + <su[u], si[i]>) + out_w[1] relu(w3 . relu(w2
    relu(zu[u] + zi[i]) + b2) + b3) + out_b)`` for the users ``users`` (1-D int64, validated by the caller) or ``user0 ..
    user0 + rows`` against every item (ctr_deepfm_grid_scores).  ``row_blocks``: workgroups that share an item tile's
    user tiles, 0 for the launch's own choice; the scores do not depend on it.  A shape the kernel is not built for
    raises: there is no other path behind this call (``deepfm_grid_supported`` says beforehand)."""
    zu, zi, su, si, w2 = (_mat(t, w).contiguous() for t, w in ((zu, "zu"), (zi, "zi"), (su, "su"), (si, "si"), (w2, "w2")))
    a, b, b2, w3, b3, out_w, out_b = _f32_vectors("deepfm_grid_scores", "a, b and the weights", a, b, b2, w3, b3, out_w,
                                                  out_b)
    nu, ni, dim = zu.shape[0], zi.shape[0], su.shape[1]
    n2, n1 = w2.shape
    if su.shape[0] != nu or a.numel() != nu or si.shape != (ni, dim) or b.numel() != ni:
        raise ValueError("deepfm_grid_scores: the rows of a side differ in number, or su and si in width")
    if zu.shape[1] != n1 or zi.shape[1] != n1 or b2.numel() != n2 or w3.numel() != n2:
        raise ValueError("deepfm_grid_scores: zu / zi must be as wide as a row of w2, b2 and w3 one element per unit of w2")
    if b3.numel() != 1 or out_w.numel() != 2 or out_b.numel() != 1:
        raise ValueError("deepfm_grid_scores: b3 and out_b hold one element, out_w two")
    user0, rows, out = _grid_rows("deepfm_grid_scores", users, user0, rows, nu, ni, out, zu.device)
    # algorithmic: every table row of the call read once (the user tiles re-read item rows from cache), the scores
    # written; per pair the 256 -> 128 layer, the relu'd sum of the rows, the w3 dot and the FM dot
    rc = _timed("deepfm_grid_scores",
                lambda: (4 * ((rows + ni) * (n1 + dim + 1) + rows * ni) + (8 * rows if users is not None else 0),
                         rows * ni * (2 * n1 * n2 + n1 + 2 * n2 + 2 * dim)),
                _lib.load().ctr_deepfm_grid_scores, zu.data_ptr(), zi.data_ptr(), su.data_ptr(), si.data_ptr(),
                a.data_ptr(), b.data_ptr(), nu, ni, dim, n1, n2, w2.data_ptr(), b2.data_ptr(), w3.data_ptr(),
                b3.data_ptr(), out_w.data_ptr(), out_b.data_ptr(),
                _lib.ptr(users) if users is not None and rows else None, user0, rows,
                _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
    _lib.check(rc, "ctr_deepfm_grid_scores")
    return out


# ---------------------------------------------------------------------------
# PNN over the user x item grid (csrc/pnn_grid.hip)
# ---------------------------------------------------------------------------
PNN_GRID_HIDDEN = (256, 128, 64, 32)       # hidden_units: the product layer's width, then the three DNN layers
PNN_GRID_MAX_EMBED = 256
PNN_GRID_CROSS = 8                          # inner products of a user-side with an item-side field vector
PNN_GRID_ITEM_TILE = _lib.CTR_PNN_GRID_ITEM_TILE     # items of a workgroup
PNN_GRID_USER_TILE = _lib.CTR_PNN_GRID_USER_TILE     # users staged at a time


def pnn_grid_supported(hidden_units, embed_dim, model: str = "in") -> bool:
    """whether ``ctr_pnn_grid_scores`` takes a six-field PNN of these ``hidden_units``, this embedding width and this
    product mode.  A function of the shapes alone."""
    hidden = tuple(int(h) for h in hidden_units)
    dim = int(embed_dim)
    return model == "in" and hidden == PNN_GRID_HIDDEN and 16 <= dim <= PNN_GRID_MAX_EMBED and dim % 16 == 0


def pnn_grid_scores(zu: torch.Tensor, zi: torch.Tensor, fu: torch.Tensor, fi: torch.Tensor, g: torch.Tensor,
                    d2_w: torch.Tensor, d2_b: torch.Tensor, d3_w: torch.Tensor, d3_b: torch.Tensor,
                    out_w: torch.Tensor, out_b: torch.Tensor, users: Optional[torch.Tensor] = None, user0: int = 0,
                    rows: Optional[int] = None, out: Optional[torch.Tensor] = None, row_blocks: int = 0) -> torch.Tensor:
    """(rows, num_items) float32: ``sigmoid(out_w . relu(d3 relu(d2 relu(zu[u] + zi[i] + g d(u, i)))) + out_b)`` with
    ``d`` the eight inner products of a user-side vector of ``fu[u]`` (U, 4E) with an item-side vector of ``fi[i]``
    (I, 2E), for the users ``users`` (1-D int64, validated by the caller) or ``user0 .. user0 + rows`` against every
    item (ctr_pnn_grid_scores).  ``row_blocks``: workgroups that share an item tile's user tiles, 0 for the launch's
    own choice; the scores do not depend on it.  A shape the kernel is not built for raises: there is no other path
    behind this call (``pnn_grid_supported`` says beforehand)."""
    zu, zi, fu, fi, g, d2_w, d3_w = (_mat(t.detach(), w).contiguous() for t, w in (
        (zu, "zu"), (zi, "zi"), (fu, "fu"), (fi, "fi"), (g, "g"), (d2_w, "d2_w"), (d3_w, "d3_w")))
    d2_b, d3_b, out_w, out_b = _f32_vectors("pnn_grid_scores", "the biases and out_w", d2_b, d3_b, out_w, out_b)
    nu, ni = zu.shape[0], zi.shape[0]
    (n2, n1), n3 = d2_w.shape, d3_w.shape[0]
    if fu.shape[0] != nu or fi.shape[0] != ni or fu.shape[1] % 4 or fi.shape[1] * 2 != fu.shape[1]:
        raise ValueError("pnn_grid_scores: fu must be (num_users, 4E) and fi (num_items, 2E)")
    dim = fu.shape[1] // 4
    if zu.shape[1] != n1 or zi.shape[1] != n1 or g.shape != (n1, PNN_GRID_CROSS):
        raise ValueError(f"pnn_grid_scores: zu / zi must be as wide as a row of d2_w and g ({n1}, {PNN_GRID_CROSS})")
    if d3_w.shape[1] != n2 or d2_b.numel() != n2 or d3_b.numel() != n3 or out_w.numel() != n3 or out_b.numel() != 1:
        raise ValueError("pnn_grid_scores: d3_w must take d2_w's units, a bias holds one element per unit, out_w one per "
                         "unit of d3_w and out_b one")
    user0, rows, out = _grid_rows("pnn_grid_scores", users, user0, rows, nu, ni, out, zu.device)
    # algorithmic: every table row of the call read once (the user tiles re-read item rows from cache), the scores
    # written; per pair the eight dots, the 128 x 8 product on the sum of the rows, the two layers and the output dot
    rc = _timed("pnn_grid_scores",
                lambda: (4 * (rows * (n1 + 4 * dim) + ni * (n1 + 2 * dim) + rows * ni) + (8 * rows if users is not None else 0),
                         rows * ni * 2 * (PNN_GRID_CROSS * dim + n1 * PNN_GRID_CROSS + n1 + n1 * n2 + n2 * n3 + n3)),
                _lib.load().ctr_pnn_grid_scores, zu.data_ptr(), zi.data_ptr(), fu.data_ptr(), fi.data_ptr(),
                g.data_ptr(), nu, ni, dim, n1, n2, n3, d2_w.data_ptr(), d2_b.data_ptr(), d3_w.data_ptr(),
                d3_b.data_ptr(), out_w.data_ptr(), out_b.data_ptr(),
                _lib.ptr(users) if users is not None and rows else None, user0, rows,
                _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
    _lib.check(rc, "ctr_pnn_grid_scores")
    return out


# ---------------------------------------------------------------------------
# AFM over the user x item grid (csrc/afm_grid.hip)
# ---------------------------------------------------------------------------
AFM_GRID_ATTENTION = 64                     # attention_dim: four sixteen-unit blocks of the matrix cores
AFM_GRID_MAX_EMBED = 128
AFM_GRID_CROSS = 8                          # products of a user-side with an item-side field vector
AFM_GRID_ITEM_TILE = _lib.CTR_AFM_GRID_ITEM_TILE     # items of a workgroup
AFM_GRID_USER_TILE = _lib.CTR_AFM_GRID_USER_TILE     # users staged at a time


def afm_grid_supported(embedding_dim, attention_dim) -> bool:
    """whether ``ctr_afm_grid_scores`` takes a six-field AFM of this embedding width and this attention width.  A
    function of the two shapes alone."""
    dim = int(embedding_dim)
    return int(attention_dim) == AFM_GRID_ATTENTION and 16 <= dim <= AFM_GRID_MAX_EMBED and dim % 16 == 0


def afm_grid_scores(su: torch.Tensor, si: torch.Tensor, fu: torch.Tensor, fi: torch.Tensor, att_w: torch.Tensor,
                    att_b: torch.Tensor, att_h: torch.Tensor, out_w: torch.Tensor, users: Optional[torch.Tensor] = None,
                    user0: int = 0, rows: Optional[int] = None, out: Optional[torch.Tensor] = None,
                    row_blocks: int = 0) -> torch.Tensor:
    """(rows, num_items) float32: ``sigmoid(a[u] + b[i] + sum_k w_k t_k)`` with ``w`` the softmax over the logits
    ``s = att_h . relu(att_w^T p + att_b)`` of AFM's 15 pair products and ``t = out_w . p``: the user's six come as
    ``su[u]`` = (a, max s, sum exp(s - max), sum exp(s - max) t), the item's one as ``si[i]`` = (b, s, t), and the eight
    products of a vector of ``fu[u]`` (U, 4E) with a vector of ``fi[i]`` (I, 2E) are formed in the kernel
    (ctr_afm_grid_scores), for the users ``users`` (1-D int64, validated by the caller) or ``user0 .. user0 + rows``
    against every item.  ``att_w`` is (E, A) as the model stores it.  ``row_blocks``: workgroups that share an item
    tile's user tiles, 0 for the launch's own choice; the scores do not depend on it.  A shape the kernel is not built
    for raises: there is no other path behind this call (``afm_grid_supported`` says beforehand)."""
    su, si, fu, fi, att_w = (_mat(t.detach(), w).contiguous() for t, w in (
        (su, "su"), (si, "si"), (fu, "fu"), (fi, "fi"), (att_w, "att_w")))
    att_b, att_h, out_w = _f32_vectors("afm_grid_scores", "att_b, att_h and out_w", att_b, att_h, out_w)
    nu, ni = su.shape[0], si.shape[0]
    dim, att = att_w.shape
    if su.shape[1] != 4 or si.shape[1] != 3:
        raise ValueError("afm_grid_scores: su must be (num_users, 4) and si (num_items, 3)")
    if fu.shape != (nu, 4 * dim) or fi.shape != (ni, 2 * dim):
        raise ValueError("afm_grid_scores: fu must be (num_users, 4E) and fi (num_items, 2E) for att_w (E, A)")
    if att_b.numel() != att or att_h.numel() != att or out_w.numel() != dim:
        raise ValueError("afm_grid_scores: att_b and att_h hold one element per column of att_w, out_w one per row")
    user0, rows, out = _grid_rows("afm_grid_scores", users, user0, rows, nu, ni, out, su.device)
    # algorithmic: every table row of the call read once (the user tiles re-read item rows from cache), the scores
    # written; per pair the eight products, their attention maps, the dots with att_h and out_w, the softmax
    rc = _timed("afm_grid_scores",
                lambda: (4 * (rows * (4 + 4 * dim) + ni * (3 + 2 * dim) + rows * ni) + (8 * rows if users is not None else 0),
                         rows * ni * AFM_GRID_CROSS * (3 * dim + 2 * dim * att + 3 * att + 8)),
                _lib.load().ctr_afm_grid_scores, su.data_ptr(), si.data_ptr(), fu.data_ptr(), fi.data_ptr(), nu, ni,
                dim, att, att_w.data_ptr(), att_b.data_ptr(), att_h.data_ptr(), out_w.data_ptr(),
                _lib.ptr(users) if users is not None and rows else None, user0, rows,
                _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
    _lib.check(rc, "ctr_afm_grid_scores")
    return out


# ---------------------------------------------------------------------------
# a biased low-rank product over the user x item grid (csrc/lowrank_grid.hip): MF, FFM, LR
# ---------------------------------------------------------------------------
LOWRANK_GRID_MAX_RANK = 256
LOWRANK_GRID_ITEM_TILE = _lib.CTR_LOWRANK_GRID_ITEM_TILE     # items of a workgroup (a wave: 32 of them)
LOWRANK_GRID_USER_TILE = _lib.CTR_LOWRANK_GRID_USER_TILE     # users staged at a time = rows of the matrix-core tile


def lowrank_grid_supported(rank) -> bool:
    """whether ``ctr_lowrank_grid_scores`` takes this rank: 0 (the biases alone) and every multiple of 16 up to 256"""
    rank = int(rank)
    return 0 <= rank <= LOWRANK_GRID_MAX_RANK and rank % 16 == 0


def lowrank_grid_scores(cu: Optional[torch.Tensor], ci: Optional[torch.Tensor], a: Optional[torch.Tensor],
                        b: Optional[torch.Tensor], *, users: Optional[torch.Tensor] = None, user0: int = 0,
                        rows: Optional[int] = None, out: Optional[torch.Tensor] = None,
                        row_blocks: int = 0) -> torch.Tensor:
    """(rows, num_items) float32: ``sigmoid((a[u] + b[i]) + <cu[u], ci[i]>)`` for the users ``users`` (1-D int64,
    validated by the caller) or ``user0 .. user0 + rows`` against every item (ctr_lowrank_grid_scores).  ``cu`` (U, K) and
    ``ci`` (I, K) are read as they are (no copy where they are contiguous); ``a`` (U) / ``b`` (I): None is zeros.  Rank 0
    is ``cu = ci = None`` with both ``a`` and ``b``.  ``row_blocks``: workgroups that share an item tile's user tiles,
    0 for the launch's own choice; the scores do not depend on it.  A rank the kernel is not built for raises: there is
    no other path behind this call (``lowrank_grid_supported`` says beforehand)."""
    if (cu is None) != (ci is None):
        raise ValueError("lowrank_grid_scores: cu and ci come together")
    if cu is not None:
        cu, ci = _mat(cu.detach(), "cu").contiguous(), _mat(ci.detach(), "ci").contiguous()
        nu, ni, rank = cu.shape[0], ci.shape[0], cu.shape[1]
        if ci.shape[1] != rank:
            raise ValueError("lowrank_grid_scores: cu and ci differ in width")
    else:
        if a is None or b is None:
            raise ValueError("lowrank_grid_scores: rank 0 needs both a and b")
        nu, ni, rank = a.numel(), b.numel(), 0
    if a is not None:
        (a,) = _f32_vectors("lowrank_grid_scores", "a", a)
    if b is not None:
        (b,) = _f32_vectors("lowrank_grid_scores", "b", b)
    if (a is not None and a.numel() != nu) or (b is not None and b.numel() != ni):
        raise ValueError("lowrank_grid_scores: a holds one element per row of cu, b one per row of ci")
    device = cu.device if cu is not None else a.device
    user0, rows, out = _grid_rows("lowrank_grid_scores", users, user0, rows, nu, ni, out, device)
    # algorithmic: every table row of the call read once (the user tiles re-read item rows from cache), the scores
    # written; per pair the dot, the biases and the sigmoid
    rc = _timed("lowrank_grid_scores",
                lambda: (4 * ((rows + ni) * (rank + 1) + rows * ni) + (8 * rows if users is not None else 0),
                         rows * ni * (2 * rank + 2)),
                _lib.load().ctr_lowrank_grid_scores, cu.data_ptr() if rank else None, ci.data_ptr() if rank else None,
                a.data_ptr() if a is not None else None, b.data_ptr() if b is not None else None, nu, ni, rank,
                _lib.ptr(users) if users is not None and rows else None, user0, rows,
                _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
    _lib.check(rc, "ctr_lowrank_grid_scores")
    return out


# ---------------------------------------------------------------------------
# Wide & Deep over the user x item grid (csrc/deepfm_grid.hip: the DeepFM template without its FM dot)
# ---------------------------------------------------------------------------
WIDEDEEP_GRID_HIDDEN = DEEPFM_GRID_HIDDEN   # hidden_units[1:]; hidden_units[0] is free (folded into the table rows)
WIDEDEEP_GRID_ITEM_TILE = _lib.CTR_WIDEDEEP_GRID_ITEM_TILE
WIDEDEEP_GRID_USER_TILE = _lib.CTR_WIDEDEEP_GRID_USER_TILE


def widedeep_grid_supported(hidden_units) -> bool:
    """whether ``ctr_widedeep_grid_scores`` takes a Wide & Deep of these ``hidden_units``, at any embedding width"""
    hidden = tuple(int(h) for h in hidden_units)
    return len(hidden) == 4 and hidden[0] >= 1 and hidden[1:] == WIDEDEEP_GRID_HIDDEN


def widedeep_grid_scores(zu: torch.Tensor, zi: torch.Tensor, a: torch.Tensor, b: torch.Tensor, w2: torch.Tensor,
                         b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, out_w: torch.Tensor, out_b: torch.Tensor,
                         *, users: Optional[torch.Tensor] = None, user0: int = 0, rows: Optional[int] = None,
                         out: Optional[torch.Tensor] = None, row_blocks: int = 0) -> torch.Tensor:
    """(rows, num_items) float32: ``sigmoid(out_w[0] (a[u] + b[i]) + out_w[1] relu(w3 . relu(w2 relu(zu[u] + zi[i]) +
    b2) + b3) + out_b)`` for the users ``users`` (1-D int64, validated by the caller) or ``user0 .. user0 + rows``
    against every item (ctr_widedeep_grid_scores): ``deepfm_grid_scores`` without ``su`` and ``si``.  A shape the kernel
    is not built for raises: there is no other path behind this call (``widedeep_grid_supported`` says beforehand)."""
    zu, zi, w2 = (_mat(t.detach(), w).contiguous() for t, w in ((zu, "zu"), (zi, "zi"), (w2, "w2")))
    a, b, b2, w3, b3, out_w, out_b = _f32_vectors("widedeep_grid_scores", "a, b and the weights", a, b, b2, w3, b3,
                                                  out_w, out_b)
    nu, ni = zu.shape[0], zi.shape[0]
    n2, n1 = w2.shape
    if a.numel() != nu or b.numel() != ni:
        raise ValueError("widedeep_grid_scores: the rows of a side differ in number")
    if zu.shape[1] != n1 or zi.shape[1] != n1 or b2.numel() != n2 or w3.numel() != n2:
        raise ValueError("widedeep_grid_scores: zu / zi must be as wide as a row of w2, b2 and w3 one element per unit "
                         "of w2")
    if b3.numel() != 1 or out_w.numel() != 2 or out_b.numel() != 1:
        raise ValueError("widedeep_grid_scores: b3 and out_b hold one element, out_w two")
    user0, rows, out = _grid_rows("widedeep_grid_scores", users, user0, rows, nu, ni, out, zu.device)
    # algorithmic: as deepfm_grid_scores, without the FM rows and their dot
    rc = _timed("widedeep_grid_scores",
                lambda: (4 * ((rows + ni) * (n1 + 1) + rows * ni) + (8 * rows if users is not None else 0),
                         rows * ni * (2 * n1 * n2 + n1 + 2 * n2)),
                _lib.load().ctr_widedeep_grid_scores, zu.data_ptr(), zi.data_ptr(), a.data_ptr(), b.data_ptr(), nu, ni,
                n1, n2, w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), out_w.data_ptr(), out_b.data_ptr(),
                _lib.ptr(users) if users is not None and rows else None, user0, rows,
                _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
    _lib.check(rc, "ctr_widedeep_grid_scores")
    return out


# ---------------------------------------------------------------------------
# feature interactions
# ---------------------------------------------------------------------------
USER_COL, ITEM_COL, DENSE_COL0, NUM_DENSE = 0, 1, 2, 43  # the (B,45) layout of data/reader.py:98-112


ALLPAIRS_MAX_VECTORS = 32  # ctr_allpairs_bwd's limit: the backward every shape but the pinned 26 x 16 takes


def _allpairs_admit(nvec: int) -> None:
    if not 2 <= nvec <= ALLPAIRS_MAX_VECTORS:
        raise ValueError(f"allpairs: 2..{ALLPAIRS_MAX_VECTORS} vectors per sample, got {nvec}")


def allpairs_fwd(emb: torch.Tensor, nvec: int, dim: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inner products of all pairs of a sample's ``nvec`` vectors, i < j lexicographic.  Admits what ``allpairs_bwd``
    can differentiate and nothing else: the lane-group forward (csrc/fields.hip) would take up to 64 vectors, but the
    backward of such a shape is refused by ctr_fields_pairs_bwd and then by ctr_allpairs_bwd (at most 32 vectors), so
    both raise ``ValueError`` above 32 vectors instead of a forward that succeeds and a backward that cannot."""
    _allpairs_admit(nvec)
    emb = _mat(emb, "emb")
    batch = emb.shape[0]
    npairs = nvec * (nvec - 1) // 2
    if out is None:
        out = torch.empty((batch, npairs), dtype=torch.float32, device=emb.device)
    many = nvec > 8 and dim in (8, 16, 32, 64)   # lane-group kernel (fields.hip) instead of the six-field LDS tiles
    rc = _timed("allpairs_fwd", lambda: (4 * batch * (nvec * dim + npairs), 2 * batch * npairs * dim),
                _lib.load().ctr_fields_pairs_fwd if many else _lib.load().ctr_allpairs_fwd, emb.data_ptr(), _ld(emb),
                batch, nvec, dim, out.data_ptr(), _ld(out), _lib.stream_ptr())
    if many and rc in _REFUSED:
        rc = _lib.load().ctr_allpairs_fwd(emb.data_ptr(), _ld(emb), batch, nvec, dim, out.data_ptr(), _ld(out),
                                          _lib.stream_ptr())
    _lib.check(rc, "ctr_allpairs_fwd")
    return out


def allpairs_bwd(emb, nvec, dim, gp, gemb, accumulate: bool) -> None:
    """backward of ``allpairs_fwd``; the same admission (``ValueError`` outside 2..32 vectors)"""
    _allpairs_admit(nvec)
    emb, gp, gemb = _mat(emb, "emb"), _mat(gp, "gp"), _mat(gemb, "gemb")
    batch = emb.shape[0]
    npairs = nvec * (nvec - 1) // 2
    many = nvec > 8 and dim in (8, 16, 32, 64)
    rc = _timed("allpairs_bwd", lambda: (4 * batch * ((2 + int(accumulate)) * nvec * dim + npairs),
                                         2 * batch * npairs * dim * 2),
                _lib.load().ctr_fields_pairs_bwd if many else _lib.load().ctr_allpairs_bwd, emb.data_ptr(), _ld(emb),
                batch, nvec, dim, gp.data_ptr(), _ld(gp), gemb.data_ptr(), _ld(gemb), int(accumulate), _lib.stream_ptr())
    if many and rc in _REFUSED:
        rc = _lib.load().ctr_allpairs_bwd(emb.data_ptr(), _ld(emb), batch, nvec, dim, gp.data_ptr(), _ld(gp),
                                          gemb.data_ptr(), _ld(gemb), int(accumulate), _lib.stream_ptr())
    _lib.check(rc, "ctr_allpairs_bwd")


def _wide_args(x, user1, item1, w, b):
    x = _mat(x, "x")
    _lib.require_device(user1, item1, w, b)
    return (x.data_ptr(), _ld(x), USER_COL, ITEM_COL, DENSE_COL0, w.shape[1], user1.data_ptr(), user1.shape[0],
            item1.data_ptr(), item1.shape[0], w.data_ptr(), b.data_ptr())


def fm_wide_fwd(emb, nvec, dim, x, user1, item1, wide_w, wide_b, out, err_flag=None) -> None:
    emb, out = _mat(emb, "emb"), _mat(out, "out")
    batch = emb.shape[0]
    rc = _timed("fm_wide_fwd", lambda: (4 * batch * (nvec * dim + 45 + 3), 4 * batch * nvec * dim),
                _lib.load().ctr_fm_wide_fwd, emb.data_ptr(), _ld(emb), batch, nvec, dim,
                *_wide_args(x, user1, item1, wide_w, wide_b), out.data_ptr(), _ld(out), _lib.ptr(err_flag),
                _lib.stream_ptr())
    _lib.check(rc, "ctr_fm_wide_fwd")


ROWS1_IN_LDS = os.environ.get("CTR_ROWS1_LDS", "1") != "0"   # 0: the interaction kernels' own per-sample atomics (A/B)


def _rows1_small(x, guser1, gitem1) -> bool:
    """the (V, 1) first-order gradients of SMALL tables leave ``fm_wide_bwd``: per-sample 4-byte atomics on a few dozen cache
    lines queue up at the memory side (csrc/rows_sum.hip, ctr_rows1_scatter).  Measured (profiles/r03_rows1_ab.txt): logistic
    regression 66.5 -> 58.0 us per step, Wide & Deep / AFM unchanged; under ``ffm_fused_bwd`` the atomics only cost 5 us and
    the extra launch 10, so FFM keeps them in the kernel."""
    if not ROWS1_IN_LDS or x.shape[0] < 4096 or (guser1 is None and gitem1 is None):
        return False
    rows = (guser1.shape[0] if guser1 is not None else 1) + (gitem1.shape[0] if gitem1 is not None else 1)
    return rows <= _lib.CTR_ROWS1_MAX_ROWS


def rows1_scatter(x, g, prob, guser1, gitem1) -> None:
    """guser1[x[:, 0]] += v, gitem1[x[:, 1]] += v, v = g (* p (1 - p) when ``prob`` is given)"""
    x, g = _mat(x, "x"), _mat(g, "g")
    batch = x.shape[0]
    nu = guser1.shape[0] if guser1 is not None else 1
    ni = gitem1.shape[0] if gitem1 is not None else 1
    rc = _timed("rows1_scatter", lambda: (batch * (8 + 4 + (4 if prob is not None else 0)) + 8 * (nu + ni), 2 * batch),
                _lib.load().ctr_rows1_scatter, x.data_ptr(), _ld(x), USER_COL, ITEM_COL, g.data_ptr(), _ld(g),
                _lib.ptr(prob), _ld(prob) if prob is not None else 0, batch, _lib.ptr(guser1), nu, _lib.ptr(gitem1), ni,
                _lib.stream_ptr())
    _lib.check(rc, "ctr_rows1_scatter")


def fm_wide_bwd(emb, nvec, dim, x, user1, item1, wide_w, wide_b, gout, guser1, gitem1, gwide_w, gwide_b, gemb,
                accumulate: bool) -> None:
    emb, gout = _mat(emb, "emb"), _mat(gout, "gout")
    batch = emb.shape[0]
    ws = _scratch(emb.device)
    if _rows1_small(x, guser1, gitem1):
        rows1_scatter(x, gout, None, guser1, gitem1)
        guser1 = gitem1 = None
    rc = _timed("fm_wide_bwd", lambda: (4 * batch * ((2 + int(accumulate)) * nvec * dim + 45 + 5),
                                        4 * batch * nvec * dim),
                _lib.load().ctr_fm_wide_bwd, emb.data_ptr(), _ld(emb), batch, nvec, dim,
                *_wide_args(x, user1, item1, wide_w, wide_b), gout.data_ptr(), _ld(gout), _lib.ptr(guser1),
                _lib.ptr(gitem1), _lib.ptr(gwide_w), _lib.ptr(gwide_b), _lib.ptr(gemb),
                _ld(gemb) if gemb is not None else 0, int(accumulate), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "ctr_fm_wide_bwd")


def _ptr_array(tensors):
    """host array of device pointers (NULL for None); None -> NULL array"""
    if tensors is None:
        return None
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def fields_fm_fwd(idx, tables, first, bias, emb, fm, err_flag=None) -> None:
    """N id fields: gather into ``emb`` (B, F*E) + FM second order + first-order sum into ``fm`` (B,1) -- one launch"""
    _lib.require_device(idx, emb, fm, *tables)
    emb, fm = _mat(emb, "emb"), _mat(fm, "fm")
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.stride(1) != 1:
        raise ValueError("fields_fm_fwd: idx must be a (B,F) int64 matrix with unit inner stride")
    batch, nf = idx.shape
    dim = tables[0].shape[1]
    vocabs = (C.c_int64 * nf)(*[t.shape[0] for t in tables])
    n1 = 0 if first is None else sum(1 for t in first if t is not None)
    rc = _timed("fields_fm_fwd", lambda: (batch * (nf * (dim * 8 + 8) + 4 * n1 + 4), 4 * batch * nf * dim),
                _lib.load().ctr_fields_fm_fwd, idx.data_ptr(), idx.stride(0), batch, nf, dim, _ptr_array(tables), vocabs,
                _ptr_array(first), _lib.ptr(bias), emb.data_ptr(), _ld(emb), fm.data_ptr(), _ld(fm),
                _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_fields_fm_fwd")


def fields_fm_bwd(idx, vocabs, dim, emb, gdeep, gfm, gtables, gfirst, gbias) -> None:
    """backward of ``fields_fm_fwd``: scatter-add ``gdeep + gfm * (S - v)`` into the dense table gradients"""
    emb = _mat(emb, "emb")
    batch, nf = idx.shape
    gdeep = _mat(gdeep, "gdeep") if gdeep is not None else None
    gfm = _mat(gfm, "gfm") if gfm is not None else None
    ws = _scratch(emb.device) if gbias is not None else None
    n1 = 0 if gfirst is None else sum(1 for t in gfirst if t is not None)
    rc = _timed("fields_fm_bwd", lambda: (batch * (nf * (dim * 4 * (2 + (gdeep is not None)) + 8) + 8 * n1 + 4),
                                          3 * batch * nf * dim),
                _lib.load().ctr_fields_fm_bwd, idx.data_ptr(), idx.stride(0), batch, nf, dim,
                (C.c_int64 * nf)(*vocabs), emb.data_ptr(), _ld(emb), _lib.ptr(gdeep),
                _ld(gdeep) if gdeep is not None else 0, _lib.ptr(gfm), _ld(gfm) if gfm is not None else 0,
                _ptr_array(gtables), _ptr_array(gfirst), _lib.ptr(gbias), _lib.ptr(ws),
                ws.numel() if ws is not None else 0, _lib.stream_ptr())
    _lib.check(rc, "ctr_fields_fm_bwd")


def _pair_array(pairs):
    flat = [v for p in pairs for v in p]
    return (C.c_int32 * len(flat))(*flat)


def ffm_fused_fwd(x, tables, user1, item1, lin_w, lin_b, emb, prob, err_flag=None) -> None:
    """FFM forward in one launch: the 12 field-aware vectors into ``emb`` (B, 12k), the probability into ``prob``"""
    x, emb, prob = _mat(x, "x"), _mat(emb, "emb"), _mat(prob, "prob")
    _lib.require_device(user1, item1, lin_w, lin_b, *tables)
    batch, dim = x.shape[0], tables[0].shape[1]
    rc = _timed("ffm_fused_fwd", lambda: (4 * batch * (45 + 4 * dim + 2 + 12 * dim + 1), 2 * batch * (15 + 86) * dim),
                _lib.load().ctr_ffm_fused_fwd, x.data_ptr(), _ld(x), batch, dim, _ptr_array(tables), user1.shape[0],
                item1.shape[0], user1.data_ptr(), item1.data_ptr(), lin_w.data_ptr(), lin_b.data_ptr(), emb.data_ptr(),
                _ld(emb), prob.data_ptr(), _ld(prob), _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_ffm_fused_fwd")


def ffm_fused_bwd(x, emb, num_users, num_items, lin_w, prob, gprob, guser1, gitem1, glin_w, glin_b, gemb) -> None:
    """backward of ``ffm_fused_fwd``'s head + dots: small gradients directly, ``gemb`` for the embedding backward"""
    x, emb, prob, gprob, gemb = _mat(x, "x"), _mat(emb, "emb"), _mat(prob, "prob"), _mat(gprob, "gprob"), _mat(gemb, "gemb")
    batch, dim = x.shape[0], emb.shape[1] // 12
    ws = _scratch(emb.device)
    rc = _timed("ffm_fused_bwd", lambda: (4 * batch * (45 + 24 * dim + 4), 4 * batch * 15 * dim),
                _lib.load().ctr_ffm_fused_bwd, x.data_ptr(), _ld(x), batch, dim, emb.data_ptr(), _ld(emb), num_users,
                num_items, lin_w.data_ptr(), prob.data_ptr(), _ld(prob), gprob.data_ptr(), _ld(gprob), _lib.ptr(guser1),
                _lib.ptr(gitem1), _lib.ptr(glin_w), _lib.ptr(glin_b), gemb.data_ptr(), _ld(gemb), ws.data_ptr(),
                ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "ctr_ffm_fused_bwd")


def ffm_head_fwd(emb, nvec, dim, pairs, x, user1, item1, lin_w, lin_b, prob, err_flag=None) -> None:
    emb, prob = _mat(emb, "emb"), _mat(prob, "prob")
    batch = emb.shape[0]
    rc = _timed("ffm_head_fwd", lambda: (4 * batch * (nvec * dim + 45 + 3), 2 * batch * len(pairs) * dim),
                _lib.load().ctr_ffm_head_fwd, emb.data_ptr(), _ld(emb), batch, nvec, dim, _pair_array(pairs),
                len(pairs), *_wide_args(x, user1, item1, lin_w, lin_b), prob.data_ptr(), _ld(prob),
                _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_ffm_head_fwd")


def ffm_head_bwd(emb, nvec, dim, pairs, x, user1, item1, lin_w, lin_b, prob, gprob, guser1, gitem1, glin_w, glin_b,
                 gemb) -> None:
    emb, prob, gprob, gemb = _mat(emb, "emb"), _mat(prob, "prob"), _mat(gprob, "gprob"), _mat(gemb, "gemb")
    batch = emb.shape[0]
    ws = _scratch(emb.device)
    rc = _timed("ffm_head_bwd", lambda: (4 * batch * (2 * nvec * dim + 45 + 6), 4 * batch * len(pairs) * dim),
                _lib.load().ctr_ffm_head_bwd, emb.data_ptr(), _ld(emb), batch, nvec, dim, _pair_array(pairs),
                len(pairs), *_wide_args(x, user1, item1, lin_w, lin_b), prob.data_ptr(), _ld(prob),
                gprob.data_ptr(), _ld(gprob), _lib.ptr(guser1), _lib.ptr(gitem1), _lib.ptr(glin_w),
                _lib.ptr(glin_b), gemb.data_ptr(), _ld(gemb), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "ctr_ffm_head_bwd")


def act_bwd(y, gy, act: int, out, accumulate: bool) -> None:
    y, gy, out = _mat(y, "y"), _mat(gy, "gy"), _mat(out, "out")
    m, n = y.shape
    rc = _timed(f"act_bwd[{m}x{n}]", lambda: (4 * m * n * (3 + int(accumulate)), m * n),
                _lib.load().ctr_act_bwd, y.data_ptr(), _ld(y), gy.data_ptr(), _ld(gy), out.data_ptr(), _ld(out),
                m, n, act, int(accumulate), _lib.stream_ptr())
    _lib.check(rc, "ctr_act_bwd")


def biinteract_fwd(emb, nvec, dim, out) -> torch.Tensor:
    """NFM bi-interaction: out[b, e] = sum_{i<j} v_i[e] * v_j[e]"""
    emb, out = _mat(emb, "emb"), _mat(out, "out")
    batch = emb.shape[0]
    rc = _timed("biinteract_fwd", lambda: (4 * batch * (nvec + 1) * dim, batch * dim * nvec * (nvec - 1)),
                _lib.load().ctr_biinteract_fwd, emb.data_ptr(), _ld(emb), batch, nvec, dim, out.data_ptr(), _ld(out),
                _lib.stream_ptr())
    _lib.check(rc, "ctr_biinteract_fwd")
    return out


def biinteract_bwd(emb, nvec, dim, gout, gemb, accumulate: bool) -> None:
    emb, gout, gemb = _mat(emb, "emb"), _mat(gout, "gout"), _mat(gemb, "gemb")
    batch = emb.shape[0]
    rc = _timed("biinteract_bwd", lambda: (4 * batch * ((2 + int(accumulate)) * nvec + 1) * dim, 3 * batch * dim * nvec),
                _lib.load().ctr_biinteract_bwd, emb.data_ptr(), _ld(emb), batch, nvec, dim, gout.data_ptr(), _ld(gout),
                gemb.data_ptr(), _ld(gemb), int(accumulate), _lib.stream_ptr())
    _lib.check(rc, "ctr_biinteract_bwd")


def pairprod_fwd(emb, nvec, dim, out) -> torch.Tensor:
    """AFM: out[(b*np + idx(i,j)), :] = v_i * v_j for every pair i < j"""
    emb, out = _mat(emb, "emb"), _mat(out, "out")
    batch, npairs = emb.shape[0], nvec * (nvec - 1) // 2
    rc = _timed("pairprod_fwd", lambda: (4 * batch * (nvec + npairs) * dim, batch * npairs * dim),
                _lib.load().ctr_pairprod_fwd, emb.data_ptr(), _ld(emb), batch, nvec, dim, out.data_ptr(), _ld(out),
                _lib.stream_ptr())
    _lib.check(rc, "ctr_pairprod_fwd")
    return out


def pairprod_bwd(emb, nvec, dim, gp, attn, gpool, gemb, accumulate: bool) -> None:
    emb, gp, gemb = _mat(emb, "emb"), _mat(gp, "gp"), _mat(gemb, "gemb")
    if gpool is not None:
        gpool = _mat(gpool, "gpool")
    batch, npairs = emb.shape[0], nvec * (nvec - 1) // 2
    rc = _timed("pairprod_bwd", lambda: (4 * batch * (2 * nvec + npairs + 1) * dim, 4 * batch * npairs * dim),
                _lib.load().ctr_pairprod_bwd, emb.data_ptr(), _ld(emb), batch, nvec, dim, gp.data_ptr(), _ld(gp),
                _lib.ptr(attn), _lib.ptr(gpool), _ld(gpool) if gpool is not None else 0, gemb.data_ptr(), _ld(gemb),
                int(accumulate), _lib.stream_ptr())
    _lib.check(rc, "ctr_pairprod_bwd")


def cross_fwd(x0, u, xl, bias, out) -> torch.Tensor:
    """Deep & Cross combine: out = x0 * u + bias + xl"""
    x0, u, xl, out = _mat(x0, "x0"), _mat(u, "u"), _mat(xl, "xl"), _mat(out, "out")
    m, d = x0.shape
    rc = _timed(f"cross_fwd[{m}x{d}]", lambda: (16 * m * d, 3 * m * d),
                _lib.load().ctr_cross_fwd, x0.data_ptr(), _ld(x0), u.data_ptr(), _ld(u), xl.data_ptr(), _ld(xl),
                bias.data_ptr(), out.data_ptr(), _ld(out), m, d, _lib.stream_ptr())
    _lib.check(rc, "ctr_cross_fwd")
    return out


def cross_bwd(x0, u, gy, gu, gx0, gbias) -> None:
    """gu = gy * x0; gx0 += gy * u; gbias += gy.sum(0)"""
    x0, u, gy, gu, gx0 = _mat(x0, "x0"), _mat(u, "u"), _mat(gy, "gy"), _mat(gu, "gu"), _mat(gx0, "gx0")
    m, d = x0.shape
    ws = _scratch(x0.device)
    rc = _timed(f"cross_bwd[{m}x{d}]", lambda: (24 * m * d, 3 * m * d),
                _lib.load().ctr_cross_bwd, x0.data_ptr(), _ld(x0), u.data_ptr(), _ld(u), gy.data_ptr(), _ld(gy),
                gu.data_ptr(), _ld(gu), gx0.data_ptr(), _ld(gx0), gbias.data_ptr(), m, d, ws.data_ptr(), ws.numel(),
                _lib.stream_ptr())
    _lib.check(rc, "ctr_cross_bwd")


# ---------------------------------------------------------------------------
# DIN / DIEN sequence attention and GRU
# ---------------------------------------------------------------------------
def linear_group_fwd(x, w, bias, res, group: int, act: int = ACT_NONE, out=None, sign_bits=None) -> torch.Tensor:
    """out = act(x @ w.T + bias + res[row // group]): one residual row per ``group`` consecutive rows (DIN: the
    per-sample term of the first attention layer on the E-wide operand).  ``sign_bits``: an int32 (m, n/32) tensor
    that receives bit (j & 31) of word j // 32 = (out[i, j] > 0) -- the ReLU derivative for ``linear_dx_masked``."""
    x, w, res = _mat(x, "x"), _mat(w, "w"), _mat(res, "res")
    m, k = x.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    out = _mat(out, "out")
    if sign_bits is not None:
        _lib.require_device(sign_bits)
        if sign_bits.dtype != torch.int32 or sign_bits.dim() != 2 or sign_bits.stride(1) != 1 or n % 32 or \
                sign_bits.shape[0] != m or sign_bits.shape[1] < n // 32:
            raise ValueError("linear_group_fwd: sign_bits must be an int32 (m, n/32) tensor with n % 32 == 0")
    rc = _timed(f"linear_group_fwd[{m}x{n}x{k}]",
                lambda: (4 * (m * k + n * k + m * n + (m // group) * n) + (m * n // 8 if sign_bits is not None else 0),
                         2 * m * n * k),
                _lib.load().ctr_linear_group_fwd, x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), _lib.ptr(bias),
                res.data_ptr(), _ld(res), group, out.data_ptr(), _ld(out), _lib.ptr(sign_bits),
                sign_bits.stride(0) if sign_bits is not None else 0, m, n, k, act, _lib.stream_ptr())
    _lib.check(rc, "ctr_linear_group_fwd")
    return out


def linear_dx_masked(w, y, gy, act: int, xin, act_in: int, gx, gsum=None, group: int = 0, sign_bits=None) -> None:
    """gx = ((gy * act'(y)) @ w) * act_in'(xin);  gsum[row // group] += gx[row] (optional).  With ``sign_bits`` (what
    ``linear_group_fwd`` wrote for xin, act_in = ReLU) xin is not read and may be None."""
    w, gy, gx = _mat(w, "w"), _mat(gy, "gy"), _mat(gx, "gx")
    m, n = gy.shape
    k = w.shape[1]
    if sign_bits is not None:
        _lib.require_device(sign_bits)
        if sign_bits.dtype != torch.int32 or sign_bits.dim() != 2 or sign_bits.stride(1) != 1 or \
                sign_bits.shape[0] != m or sign_bits.shape[1] * 32 < k:
            raise ValueError("linear_dx_masked: sign_bits must be an int32 (m, k/32) tensor")
        xin = None
    mask_bytes = (m * k // 8) if sign_bits is not None else (4 * m * k if act_in != ACT_NONE else 0)
    rc = _timed(f"linear_dx_masked[{m}x{n}x{k}]",
                lambda: (4 * (m * n * (2 if act != ACT_NONE else 1) + n * k + m * k) + mask_bytes, 2 * m * n * k),
                _lib.load().ctr_linear_dx_masked, w.data_ptr(), _ld(w), _lib.ptr(y), _ld(y) if y is not None else 0,
                gy.data_ptr(), _ld(gy), act, _lib.ptr(xin), _ld(xin) if xin is not None else 0, act_in,
                _lib.ptr(sign_bits), sign_bits.stride(0) if sign_bits is not None else 0, gx.data_ptr(),
                _ld(gx), _lib.ptr(gsum), _ld(gsum) if gsum is not None else 0, group, m, n, k, _lib.stream_ptr())
    _lib.check(rc, "ctr_linear_dx_masked")


def linear_fwd_dot(x, w, b, act: int, u, c):
    """(y, out) with y = act(x @ w.T + b) and out = y @ u.T + c for a single-unit ``u`` (1, n): the second layer is
    formed in the first one's epilogue (n <= 128), so y is not re-read for it"""
    x, w, u = _mat(x, "x"), _mat(w, "w"), _mat(u, "u")
    m, k = x.shape
    n = w.shape[0]
    if u.shape != (1, n):
        raise ValueError(f"linear_fwd_dot: u must be (1, {n})")
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    out = torch.empty((m, 1), dtype=torch.float32, device=x.device)
    rc = _timed(f"linear_fwd_dot[{m}x{n}x{k}]", lambda: (4 * (m * k + n * k + n + m * n + m), 2 * m * n * (k + 1)),
                _lib.load().ctr_linear_fwd_dot, x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), _lib.ptr(b), y.data_ptr(),
                _ld(y), u.data_ptr(), _lib.ptr(c), out.data_ptr(), 1, m, n, k, act, _lib.stream_ptr())
    _lib.check(rc, "ctr_linear_fwd_dot")
    return y, out


def linear_dx_scatter(w, gy, idx, attn, gpool, group: int, gtable) -> None:
    """gtable[idx[i]] += gy[i] @ w + attn[i] * gpool[i // group]: the input gradient of a layer whose input rows were
    gathered from ``gtable``'s table, added where the rows came from without storing the (m, k) gradient (DIN)"""
    w, gy, gpool, gtable = _mat(w, "w"), _mat(gy, "gy"), _mat(gpool, "gpool"), _mat(gtable, "gtable")
    _lib.require_device(idx, attn)
    m, n = gy.shape
    k = w.shape[1]
    if idx.dtype != torch.int64 or not idx.is_contiguous() or idx.numel() != m or attn.numel() != m or \
            not attn.is_contiguous() or attn.dtype != torch.float32:
        raise ValueError("linear_dx_scatter: idx (int64) and attn (float32) must be contiguous with one entry per row")
    if gtable.shape[1] != k or not gtable.is_contiguous():
        raise ValueError("linear_dx_scatter: gtable must be a contiguous (vocab, k) tensor")
    rc = _timed(f"linear_dx_scatter[{m}x{n}x{k}]", lambda: (4 * (m * n + n * k + 3 * m + 3 * m * k), 2 * m * n * k),
                _lib.load().ctr_linear_dx_scatter, w.data_ptr(), _ld(w), gy.data_ptr(), _ld(gy), idx.data_ptr(),
                attn.data_ptr(), gpool.data_ptr(), _ld(gpool), group, gtable.data_ptr(), gtable.shape[0], m, n, k,
                _lib.stream_ptr())
    _lib.check(rc, "ctr_linear_dx_scatter")


def linear_n1_bwd_masked(x, w, gy, act_in: int, gx, gw=None, gb=None) -> None:
    """backward of the single-unit layer y = x @ w.T + b whose input x is the previous layer's activation output:
    gx = (gy @ w) * act_in'(x) (``gx`` may be ``x`` itself), gw += gy.T @ x, gb += gy.sum()"""
    x, w, gy, gx = _mat(x, "x"), _mat(w, "w"), _mat(gy, "gy"), _mat(gx, "gx")
    m, k = x.shape
    if w.shape[0] != 1 or gy.shape != (m, 1) or gx.shape != (m, k):
        raise ValueError("linear_n1_bwd_masked: w must be (1, k), gy (m, 1), gx (m, k)")
    ws = _scratch(x.device) if gw is not None else None
    rc = _timed(f"linear_n1_bwd_masked[{m}x1x{k}]", lambda: (4 * (2 * m * k + m + 2 * k), 4 * m * k),
                _lib.load().ctr_linear_n1_bwd_masked, x.data_ptr(), _ld(x), w.data_ptr(), gy.data_ptr(), _ld(gy), act_in,
                gx.data_ptr(), _ld(gx), _lib.ptr(gw), _lib.ptr(gb), m, k, _lib.ptr(ws),
                ws.numel() if ws is not None else 0, _lib.stream_ptr())
    _lib.check(rc, "ctr_linear_n1_bwd_masked")


def din_scatter_bwd(hist, vocab, dim, gh, attn, gpool, summed: bool, gtable) -> None:
    """history positions' rows of the table gradient: gh + attn * gpool, scatter-added by hist ids"""
    gh, gpool = _mat(gh, "gh"), _mat(gpool, "gpool")
    batch, length = hist.shape
    rc = _timed("din_scatter_bwd", lambda: (batch * length * (8 + 4 + 4 * dim * (3 if summed else 4)), 0),
                _lib.load().ctr_din_scatter_bwd, hist.data_ptr(), vocab, batch, length, dim, gh.data_ptr(), _ld(gh),
                attn.data_ptr(), gpool.data_ptr(), _ld(gpool), int(summed), gtable.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_din_scatter_bwd")


def din_concat_fwd(table, hist, target, c, tvec, err_flag=None, pair: bool = False, h_only: bool = False) -> None:
    """attention operand per position: [h, h-t, t] (the reference's cat), ``pair``: [h, t], ``h_only``: [h]"""
    _lib.require_device(table, hist, target)
    c = _mat(c, "c")
    batch, length = hist.shape
    dim = table.shape[1]
    width = 1 if h_only else (2 if pair else 3)
    rc = _timed("din_concat_fwd", lambda: (batch * length * (dim * 4 + 8 + 4 * width * dim) + batch * (8 + 8 * dim), 0),
                _lib.load().ctr_din_concat_fwd, table.data_ptr(), table.shape[0], dim, hist.data_ptr(),
                target.data_ptr(), batch, length, c.data_ptr(), _ld(c), _lib.ptr(tvec),
                _ld(tvec) if tvec is not None else 0,
                _lib.DIN_H if h_only else (_lib.DIN_PAIR if pair else _lib.DIN_TRIPLE),
                _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_din_concat_fwd")


def din_pool_fwd(score, hsrc, batch, length, dim, attn, out, summed: bool) -> None:
    hsrc, out = _mat(hsrc, "hsrc"), _mat(out, "out")
    rc = _timed("din_pool_fwd", lambda: (4 * batch * length * (2 + dim * (1 if summed else 2)), 2 * batch * length * dim),
                _lib.load().ctr_din_pool_fwd, score.data_ptr(), hsrc.data_ptr(), _ld(hsrc), batch, length, dim,
                attn.data_ptr(), out.data_ptr(), _ld(out), int(summed), _lib.stream_ptr())
    _lib.check(rc, "ctr_din_pool_fwd")


def din_pool_bwd(attn, hsrc, batch, length, dim, gout, summed: bool, gscore) -> None:
    hsrc, gout = _mat(hsrc, "hsrc"), _mat(gout, "gout")
    rc = _timed("din_pool_bwd", lambda: (4 * batch * length * (2 + dim * (1 if summed else 2)), 2 * batch * length * dim),
                _lib.load().ctr_din_pool_bwd, attn.data_ptr(), hsrc.data_ptr(), _ld(hsrc), batch, length, dim,
                gout.data_ptr(), _ld(gout), int(summed), gscore.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_din_pool_bwd")


def din_concat_bwd(hist, target, vocab, dim, gc, attn, gout, summed: bool, gt_extra, gtable,
                   pair: bool = False) -> None:
    gc, gout = _mat(gc, "gc"), _mat(gout, "gout")
    batch, length = hist.shape
    width = 2 if pair else 3
    rc = _timed("din_concat_bwd", lambda: (batch * length * (8 + 4 + 4 * width * dim + 8 * dim) + batch * 16 * dim, 0),
                _lib.load().ctr_din_concat_bwd, hist.data_ptr(), target.data_ptr(), vocab, batch, length, dim,
                gc.data_ptr(), _ld(gc), attn.data_ptr(), gout.data_ptr(), _ld(gout), int(summed),
                _lib.ptr(gt_extra), _ld(gt_extra) if gt_extra is not None else 0,
                _lib.DIN_PAIR if pair else _lib.DIN_TRIPLE, gtable.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_din_concat_bwd")


def gru_fwd(gi, w_hh, b_hh, batch, length, dim, hbuf, last) -> None:
    gi = _mat(gi, "gi")
    rc = _timed("gru_fwd", lambda: (4 * batch * length * 4 * dim, 6 * batch * length * dim * dim),
                _lib.load().ctr_gru_fwd, gi.data_ptr(), _ld(gi), w_hh.data_ptr(), b_hh.data_ptr(), batch, length, dim,
                hbuf.data_ptr(), _lib.ptr(last), _ld(last) if last is not None else 0, _lib.stream_ptr())
    _lib.check(rc, "ctr_gru_fwd")


def gru_fused_fwd(x, w_ih, b_ih, w_hh, b_hh, batch, length, dim, hbuf, last) -> bool:
    """the GRU with its input projection inside (x rows instead of gi).  False: shape not taken, nothing ran --
    form gi with ``linear_fwd`` and call ``gru_fwd``."""
    x = _mat(x, "x")
    rc = _timed("gru_fused_fwd", lambda: (4 * batch * length * 2 * dim, 12 * batch * length * dim * dim),
                _lib.load().ctr_gru_fused_fwd, x.data_ptr(), _ld(x), w_ih.data_ptr(), b_ih.data_ptr(), w_hh.data_ptr(),
                b_hh.data_ptr(), batch, length, dim, hbuf.data_ptr(), _lib.ptr(last),
                _ld(last) if last is not None else 0, _lib.stream_ptr())
    if _refused(rc, "gru_fused_fwd"):
        return False
    _lib.check(rc, "ctr_gru_fused_fwd")
    return True


def gru_fused_bwd(x, w_ih, b_ih, w_hh, b_hh, hbuf, batch, length, dim, glast, gx, gw_ih, gb_ih, gw_hh, gb_hh) -> None:
    """backward of ``gru_fused_fwd``: gx = dgi W_ih and the four parameter gradients (accumulated), nothing of size
    3*dim per step stored"""
    x, glast, gx = _mat(x, "x"), _mat(glast, "glast"), _mat(gx, "gx")
    ws = _scratch(x.device)
    rc = _timed("gru_fused_bwd", lambda: (4 * batch * length * 3 * dim, 36 * batch * length * dim * dim),
                _lib.load().ctr_gru_fused_bwd, x.data_ptr(), _ld(x), w_ih.data_ptr(), b_ih.data_ptr(), w_hh.data_ptr(),
                b_hh.data_ptr(), hbuf.data_ptr(), batch, length, dim, glast.data_ptr(), _ld(glast), gx.data_ptr(),
                _ld(gx), gw_ih.data_ptr(), gb_ih.data_ptr(), gw_hh.data_ptr(), gb_hh.data_ptr(), ws.data_ptr(),
                ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "ctr_gru_fused_bwd")


def gru_bwd(gi, w_hh, b_hh, hbuf, batch, length, dim, glast, dgi, dgh) -> None:
    gi, glast = _mat(gi, "gi"), _mat(glast, "glast")
    rc = _timed("gru_bwd", lambda: (4 * batch * length * 10 * dim, 12 * batch * length * dim * dim),
                _lib.load().ctr_gru_bwd, gi.data_ptr(), _ld(gi), w_hh.data_ptr(), b_hh.data_ptr(), hbuf.data_ptr(),
                batch, length, dim, glast.data_ptr(), _ld(glast), dgi.data_ptr(), dgh.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_gru_bwd")


TOPK_MAX_K = 4096


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
    rc = _timed("topk_rows", lambda: (4 * rows * n + 8 * rows * k, 0), _lib.load().ctr_topk_rows,
                _lib.ptr(scores) if rows else None, scores.stride(1 - along), scores.stride(along), rows, n, k,
                _lib.ptr(out) if rows else None, None, _lib.stream_ptr())
    _lib.check(rc, "ctr_topk_rows")
    return out if along == 1 else out.t()


CF_KNN_MAX_K = 64   # CTR_CF_KNN_MAX_K: the longest list (k + 1 entries) ctr_cf_knn keeps per row


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
    lib = _lib.load()
    ws = C.c_int64()
    _lib.check(lib.ctr_gdcf_workspace_bytes(m, n, k, C.byref(ws)), "ctr_gdcf_workspace_bytes")
    parts = torch.empty(ws.value // 8, dtype=torch.float64, device=p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    gp = torch.empty_like(p) if grad else None
    rc = _timed("gdcf_rows" if grad else "gdcf_rows_loss",
                lambda: (4 * (m * k + n * k) + m * y.shape[1] + (4 * m * k if grad else 0),
                         (4 if grad else 2) * m * n * k),
                lib.ctr_gdcf_rows, p.data_ptr(), q.data_ptr(), m, n, k, y.data_ptr(), y.shape[1], loss.data_ptr(),
                _lib.ptr(gp), parts.data_ptr(), ws.value, _lib.stream_ptr())
    _lib.check(rc, "ctr_gdcf_rows")
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
    rc = _timed("gdcf_cols", lambda: (4 * (m * k + 2 * n * k) + n * yt.shape[1], 4 * m * n * k),
                _lib.load().ctr_gdcf_cols, p.data_ptr(), q.data_ptr(), m, n, k, yt.data_ptr(), yt.shape[1],
                gout.data_ptr(), gq.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_gdcf_cols")
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
    rc = _timed("softmax_full_rows" if grad else "softmax_full_rows_loss",
                lambda: (4 * (b * k + n * k) + 8 * b + 8 * b + (4 * b * k if grad else 0) + 2 * nbytes,
                         (4 if grad else 2) * b * n * k),
                _lib.load().ctr_softmax_full_rows, x.data_ptr(), q.data_ptr(), b, n, k, target.data_ptr(),
                nll.data_ptr(), lse.data_ptr(), _lib.ptr(gx), int(splits), _lib.ptr(ws), nbytes, _lib.ptr(err_flag),
                _lib.stream_ptr())
    _lib.check(rc, "ctr_softmax_full_rows")
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
    rc = _timed("softmax_full_cols", lambda: (4 * (b * k + 2 * n * k) + 20 * b + 2 * nbytes, 4 * b * n * k),
                _lib.load().ctr_softmax_full_cols, x.data_ptr(), q.data_ptr(), b, n, k, target.data_ptr(),
                lse.data_ptr(), _lib.ptr(nll), gout.data_ptr(), gq.data_ptr(), int(splits), _lib.ptr(ws), nbytes, _lib.stream_ptr())
    _lib.check(rc, "ctr_softmax_full_cols")
    return gq


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
    rc = _timed("als_gram", lambda: (4 * rows * k + 2 * nbytes + 4 * k * k, rows * k * (k + 16)),
                _lib.load().ctr_als_gram, y.data_ptr(), rows, k, gram.data_ptr(), ws.data_ptr(), nbytes,
                _lib.stream_ptr())
    _lib.check(rc, "ctr_als_gram")
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
    _lib.require_device(y, gram, indptr, indices, rows, out, err_flag)
    if gram.shape != (k, k) or gram.dtype != torch.float32 or not gram.is_contiguous():
        raise ValueError(f"als: gram must be a contiguous ({k}, {k}) float32 tensor, got {tuple(gram.shape)} {gram.dtype}")
    if indptr.dim() != 1 or indptr.dtype != torch.int64 or not indptr.is_contiguous() or indptr.numel() < 2:
        raise ValueError("als: indptr must be a contiguous (csr_rows + 1,) int64 tensor")
    if indices.dim() != 1 or indices.dtype != torch.int32 or not indices.is_contiguous():
        raise ValueError("als: indices must be a contiguous 1-D int32 tensor")
    csr_rows = indptr.numel() - 1
    if rows is not None and (rows.dim() != 1 or rows.dtype != torch.int64 or not rows.is_contiguous()):
        raise ValueError("als: rows must be a contiguous 1-D int64 tensor")
    count = csr_rows if rows is None else rows.numel()
    if count >= 1 << 31:
        raise ValueError("als: at most 2^31 - 1 rows a call")
    reg, alpha = float(reg), float(alpha)
    if reg != reg or alpha != alpha:
        raise ValueError("als: reg and alpha must be numbers")
    if err_flag is not None and (err_flag.dtype != torch.int32 or err_flag.numel() != 1):
        raise ValueError("als: err_flag must be one int32")
    if out is None:
        out = torch.empty((count, k), dtype=torch.float32, device=y.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape != (count, k) or \
            (count > 0 and out.stride(1) != 1) or (count > 1 and out.stride(0) < k):
        raise ValueError(f"als: out must be a ({count}, {k}) float32 tensor with unit inner stride")
    if count == 0:
        return out
    ldo = out.stride(0) if count > 1 else k
    nnz = indices.numel()

    def meta():      # 2 k^2 per list entry of the rows solved plus k^3 / 3 per row; read only under a profiler
        at = None if rows is None else rows.clamp(0, csr_rows - 1)
        entries = nnz if rows is None else int((indptr[at + 1] - indptr[at]).sum())
        return (4 * entries * (k + 1) + 16 * count + 4 * count * k + 4 * k * k,
                2 * k * k * entries + count * (k ** 3) // 3)
    rc = _timed("als_solve_rows", meta,
                _lib.load().ctr_als_solve_rows, y.data_ptr(), y.shape[0], k, gram.data_ptr(), indptr.data_ptr(),
                _lib.ptr(indices) if nnz else None, csr_rows, _lib.ptr(rows), count, reg, alpha, out.data_ptr(), ldo,
                _lib.ptr(err_flag), _lib.stream_ptr())
    _lib.check(rc, "ctr_als_solve_rows")
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
    if indptr.dim() != 1 or indptr.dtype != torch.int64 or not indptr.is_contiguous() or indptr.numel() < 2:
        raise ValueError("als: indptr must be a contiguous (csr_rows + 1,) int64 tensor")
    if indices.dim() != 1 or indices.dtype != torch.int32 or not indices.is_contiguous():
        raise ValueError("als: indices must be a contiguous 1-D int32 tensor")
    if values.dim() != 1 or values.dtype != torch.float32 or not values.is_contiguous() or \
            values.numel() != indices.numel():
        raise ValueError("als: values must be a contiguous 1-D float32 tensor of the length of indices")
    csr_rows = indptr.numel() - 1
    if rows is not None and (rows.dim() != 1 or rows.dtype != torch.int64 or not rows.is_contiguous()):
        raise ValueError("als: rows must be a contiguous 1-D int64 tensor")
    count = csr_rows if rows is None else rows.numel()
    if count >= 1 << 31:
        raise ValueError("als: at most 2^31 - 1 rows a call")
    try:
        (w0, w1), (t0, t1) = (float(v) for v in w), (float(v) for v in t)
    except (TypeError, ValueError):
        raise ValueError("als: w and t must be pairs of numbers (w0, w1), (t0, t1)") from None
    reg, reg_per_entry = float(reg), float(reg_per_entry)
    if any(v != v for v in (w0, w1, t0, t1, reg, reg_per_entry)):
        raise ValueError("als: w, t, reg and reg_per_entry must be numbers")
    if err_flag is not None and (err_flag.dtype != torch.int32 or err_flag.numel() != 1):
        raise ValueError("als: err_flag must be one int32")
    _lib.require_device(y, gram, indptr, indices, values, rows, out, err_flag)      # after what needs no device to tell
    if out is None:
        out = torch.empty((count, k), dtype=torch.float32, device=y.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape != (count, k) or \
            (count > 0 and out.stride(1) != 1) or (count > 1 and out.stride(0) < k):
        raise ValueError(f"als: out must be a ({count}, {k}) float32 tensor with unit inner stride")
    if count == 0:
        return out
    ldo = out.stride(0) if count > 1 else k
    nnz = indices.numel()

    def meta():      # als_solve_rows' with 4 B more read per entry; the dense part only where there is one
        at = None if rows is None else rows.clamp(0, csr_rows - 1)
        entries = nnz if rows is None else int((indptr[at + 1] - indptr[at]).sum())
        return (4 * entries * (k + 2) + 16 * count + 4 * count * k + (4 * k * k if gram is not None else 0),
                2 * k * k * entries + count * (k ** 3) // 3)
    rc = _timed("als_solve_rows_weighted", meta,
                _lib.load().ctr_als_solve_rows_weighted, y.data_ptr(), y.shape[0], k, _lib.ptr(gram),
                indptr.data_ptr(), _lib.ptr(indices) if nnz else None, _lib.ptr(values) if nnz else None, csr_rows,
                _lib.ptr(rows), count, w0, w1, t0, t1, reg, reg_per_entry, out.data_ptr(), ldo, _lib.ptr(err_flag),
                _lib.stream_ptr())
    _lib.check(rc, "ctr_als_solve_rows_weighted")
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


def _graph_indptr(indptr) -> int:
    if not isinstance(indptr, torch.Tensor) or indptr.dim() != 1 or indptr.dtype != torch.int64 or \
            not indptr.is_contiguous() or indptr.numel() < 2:
        raise ValueError("graph: indptr must be a contiguous (num_rows + 1,) int64 tensor")
    if indptr.numel() - 1 >= 1 << 31:
        raise ValueError("graph: a CSR must have fewer than 2^31 rows")
    return indptr.numel() - 1


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
    num_rows = _graph_indptr(indptr)
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
    num_rows = _graph_indptr(indptr)
    if not isinstance(indices, torch.Tensor) or indices.dim() != 1 or indices.dtype != torch.int32 or \
            not indices.is_contiguous():
        raise ValueError("graph: indices must be a contiguous 1-D int32 tensor")
    nnz = indices.numel()
    if nnz >= 1 << 31:
        raise ValueError("graph: a CSR must have fewer than 2^31 entries")
    _graph_scale(scale_in, x_rows, "scale_in")
    _graph_scale(scale_out, num_rows, "scale_out")
    if rows is not None and (not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.dtype != torch.int64 or
                             not rows.is_contiguous()):
        raise ValueError("graph: rows must be a contiguous 1-D int64 tensor")
    count = num_rows if rows is None else rows.numel()
    if count >= 1 << 31:
        raise ValueError("graph: at most 2^31 - 1 rows a call")
    if plan is not None:
        if not isinstance(plan, GraphPlan):
            raise ValueError("graph: plan must come from graph_plan()")
        if rows is not None:
            raise ValueError("graph: a plan covers all rows in order; pass rows or a plan, not both")
        if plan.num_rows != num_rows or plan.indptr.data_ptr() != indptr.data_ptr():
            raise ValueError("graph: the plan was built for another CSR")
    if err_flag is not None and (err_flag.dtype != torch.int32 or err_flag.numel() != 1):
        raise ValueError("graph: err_flag must be one int32")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2 or
                            out.shape != (count, k)):
        raise ValueError(f"graph: out must be a ({count}, {k}) float32 tensor")
    ldo = k if out is None or count == 0 else layout(out, count, "out")
    _lib.require_device(x, indptr, indices, scale_in, scale_out, rows, out, err_flag)
    if out is None:
        out = torch.empty((count, k), dtype=torch.float32, device=x.device)
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
        at = None if rows is None else rows.clamp(0, num_rows - 1)
        entries = nnz if rows is None else int((indptr[at + 1] - indptr[at]).sum())
        return 4 * entries * (k + 1) + 4 * count * (k + 4) + 2 * nbytes, 2 * entries * k
    rc = _timed("graph_propagate", meta,
                _lib.load().ctr_graph_propagate, x.data_ptr(), x_rows, ldx, k, indptr.data_ptr(),
                _lib.ptr(indices) if nnz else None, num_rows, nnz, _lib.ptr(scale_in), _lib.ptr(scale_out),
                _lib.ptr(rows), count, _lib.ptr(work), 0 if work is None else work.shape[0], _lib.ptr(merge),
                0 if merge is None else merge.shape[0], out.data_ptr(), ldo, _lib.ptr(ws), nbytes, flag.data_ptr(),
                _lib.stream_ptr())
    _lib.check(rc, "ctr_graph_propagate")
    if err_flag is None:
        bits = int(flag.item())
        if bits & GRAPH_ERR_INDEX:
            raise IndexError("graph: an index of the CSR is outside the table it indexes (or a row is outside the CSR)")
        if bits:
            raise RuntimeError(f"graph: the plan does not fit the call (error bits {bits:#x})")
    return out


# ---------------------------------------------------------------------------
# top-k ranking evaluation (csrc/rank_eval.hip); the CSRs are (offsets (rows + 1), ids) int64 device tensors, the
# offsets already sliced to the rows of the call (they index ``ids`` absolutely)
# ---------------------------------------------------------------------------
RANK_MASK_BITS = 0xFFFFFFFF
RANK_ERR_OFFSETS, RANK_ERR_LENGTH, RANK_ERR_SURVIVOR, RANK_ERR_COUNT = 1, 2, 4, 8
RANK_MAX_ROWS = 1 << 24
_RANK_TABLE_SLOTS = 1 << 25   # hash-set workspace of rank_metrics_lists: at most 256 MB (or one user's table)


def _i64(*tensors):
    _lib.require_device(*tensors)
    for t in tensors:
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous()):
            raise ValueError("expected contiguous int64 tensors")


def rank_filter(rec: torch.Tensor, ex_off: torch.Tensor, ex_ids: torch.Tensor, err: torch.Tensor):
    """remove_itemid's compaction: (out (rows, len), out_len (rows,)); out[u, out_len[u]:] is unwritten (zeros)"""
    _i64(rec, ex_off, ex_ids)
    rows, length = rec.shape
    out = torch.zeros((rows, length), dtype=torch.int64, device=rec.device)
    out_len = torch.empty(rows, dtype=torch.int64, device=rec.device)
    rc = _timed("rank_filter", lambda: (16 * rows * length, 0), _lib.load().ctr_rank_filter,
                _lib.ptr(rec) if rec.numel() else None, length, rows, length, ex_off.data_ptr(),
                _lib.ptr(ex_ids) if ex_ids.numel() else None, ex_ids.numel(), _lib.ptr(out) if out.numel() else None,
                length, out_len.data_ptr(), err.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_rank_filter")
    return out, out_len


def rank_metrics_lists(pred: torch.Tensor, pred_len: torch.Tensor, act_off: torch.Tensor, act_ids: torch.Tensor,
                       alen: torch.Tensor, k: int, err: torch.Tensor) -> torch.Tensor:
    """(rows, 7) float64 partials (same, rec, real, ap, dcg, idcg, rr) of explicit predicted rows"""
    _i64(pred, pred_len, act_off, act_ids, alen)
    rows, length = pred.shape
    lib = _lib.load()
    slots = C.c_int64()
    _lib.check(lib.ctr_rank_table_slots(k, length, C.byref(slots)), "ctr_rank_table_slots")
    cap = slots.value
    table = torch.empty(max(cap, min(rows, max(1, _RANK_TABLE_SLOTS // cap)) * cap), dtype=torch.int64,
                        device=pred.device)
    parts = torch.empty((rows, 7), dtype=torch.float64, device=pred.device)
    rc = _timed("rank_metrics_lists", lambda: (8 * rows * length + 8 * act_ids.numel(), 0), lib.ctr_rank_metrics_lists,
                _lib.ptr(pred) if pred.numel() else None, length, pred_len.data_ptr(), rows, length, act_off.data_ptr(),
                _lib.ptr(act_ids) if act_ids.numel() else None, act_ids.numel(), alen.data_ptr(), k,
                table.data_ptr(), table.numel(), parts.data_ptr(), err.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_rank_metrics_lists")
    return parts


def rank_mask(scores: torch.Tensor, ex_off: torch.Tensor, ex_ids: torch.Tensor, err: torch.Tensor) -> None:
    """write RANK_MASK_BITS over every excluded item of the (rows, n) float32 chunk, in place"""
    _lib.require_device(scores)
    _i64(ex_off, ex_ids)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError("rank_mask expects a row-major 2-D float32 tensor")
    rows, n = scores.shape
    rc = _timed("rank_mask", lambda: (8 * ex_ids.numel() + 4 * ex_ids.numel(), 0), _lib.load().ctr_rank_mask,
                scores.data_ptr(), scores.stride(0), rows, n, ex_off.data_ptr(),
                _lib.ptr(ex_ids) if ex_ids.numel() else None, ex_ids.numel(), err.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_rank_mask")


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
    rc = _timed("rank_metrics_scores", lambda: (4 * rows * n + 8 * top.numel() + 56 * rows, 0),
                _lib.load().ctr_rank_metrics_scores, scores.data_ptr(), scores.stride(0), rows, n, top.data_ptr(),
                top.shape[1], k, act_off.data_ptr(), _lib.ptr(act_ids) if act_ids.numel() else None, act_ids.numel(),
                alen.data_ptr(), n_real.data_ptr(), pad.data_ptr(), parts.data_ptr(), err.data_ptr(),
                _lib.stream_ptr())
    _lib.check(rc, "ctr_rank_metrics_scores")


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
    rc = _timed("eval_candidates", lambda: (16 * n + 8 * n * (1 + k), 0), _lib.load().ctr_eval_candidates,
                _lib.ptr(users) if n else None, _lib.ptr(items) if n else None, n, indptr.data_ptr(),
                _lib.ptr(indices) if indices.numel() else None, indices.numel(), int(num_users), int(num_items), int(k),
                int(seed), _lib.ptr(out) if n else None, ld, err.data_ptr(), fail.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_eval_candidates")
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
    rc = _timed("group_rank", lambda: (4 * n * (1 + k) + (4 * n if ranks is not None else 0), 0),
                _lib.load().ctr_group_rank, _lib.ptr(scores) if n else None, ld, n, int(k), _lib.ptr(ranks),
                hist.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_group_rank")


# ---------------------------------------------------------------------------
# score-level evaluation (csrc/score_eval.hip)
# ---------------------------------------------------------------------------
SCORE_CHUNK = _lib.CTR_SCORE_CHUNK
GAUC_SMALL, GAUC_SLAB = _lib.CTR_GAUC_SMALL, _lib.CTR_GAUC_SLAB


def _flat_f32(name, what, t, n=None):
    if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or (n is not None and t.shape[0] != n):
        raise ValueError(f"{name}: {what} must be a contiguous (N,) float32 tensor")


def _flat_int(name, what, t, dtype, n):
    if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.shape[0] != n:
        raise ValueError(f"{name}: {what} must be a contiguous ({n},) {str(dtype).replace('torch.', '')} tensor")


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
    rc = _timed("score_counts", lambda: (8 * n + 32 * chunks, 0), _lib.load().ctr_score_counts,
                _lib.ptr(prob) if n else None, _lib.ptr(target) if n else None, n, counts.data_ptr(),
                _lib.ptr(sums) if n else None, _lib.stream_ptr())
    _lib.check(rc, "ctr_score_counts")


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
    rc = _timed("gauc_groups", lambda: (12 * n + 24 * groups, 0), _lib.load().ctr_gauc_groups, nz(prob), nz(target), n,
                nz(order), offsets.data_ptr(), groups, nz(small_groups), small_groups.numel(), nz(slab_group),
                nz(slab_first), slab_group.numel(), nz(pos), nz(neg), nz(u2), err.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ctr_gauc_groups")
