"""Dense layers (csrc/linear*.hip, gemm_*.hip, mlp_*.hip, fold_head.hip, cross.hip): ``nn.Linear`` and stacks of it,
layer by layer or fused into one launch, the folded head, activation masks and the Deep & Cross combine.  The fused
embed + stack launch takes field specs, so this module imports ``embed`` (which imports no family module)."""
import ctypes as C
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import ACT_NONE
from ._call import _call, _ld, _mat, _profiling, _refused, _scratch, _timed
from .embed import FieldSpec, _embed_bytes, _field_array


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
    _call(f"linear_fwd[{m}x{n}x{k}]", "ctr_linear_fwd",
          lambda: (4 * (m * k + n * k + n + m * n * (2 if residual is not None else 1)), 2 * m * n * k), x.data_ptr(),
          _ld(x), w.data_ptr(), _ld(w), _lib.ptr(b), _lib.ptr(residual), _ld(residual) if residual is not None else 0,
          out.data_ptr(), _ld(out), m, n, k, act, _lib.stream_ptr())
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

    if not _profiling():
        _lib.check(fn(*call(gx, gw, gb)), "ctr_linear_bwd")
        return
    # profiling: one C call per kernel so each gets its own event pair
    if gx is not None:
        _lib.check(_timed(f"linear_bwd_dx[{m}x{n}x{k}]", lambda: (ygy + 4 * (n * k + m * k), 2 * m * n * k),
                          fn, *call(gx, None, None)), "ctr_linear_bwd")
    if gw is not None:
        _lib.check(_timed(f"linear_bwd_dw[{m}x{n}x{k}]", lambda: (ygy + 4 * (m * k + 2 * n * k), 2 * m * n * k),
                          fn, *call(None, gw, gb)), "ctr_linear_bwd")


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


# narrow stacks run as one launch (ctr_mlp_fwd/bwd) when their shape allows.  The package re-exports the switch and
# callers assign ``ops.FUSED_MLP``, which does not reach this global: ``_fusable`` reads the package's at call time
FUSED_MLP = True


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
    if not sys.modules[__package__].FUSED_MLP or len(layers) < 2 or len(layers) > 8:
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
        # a refusal is an error here: the input columns were never written
        _call("mlp_fused_bwd", "ctr_embed_mlp_head_bwd", meta, farr, len(gather_specs), m, arr, len(layers), C.byref(hg),
              C.byref(fg) if fg is not None else None, gx_first.data_ptr(), _ld(gx_first), ws.data_ptr(), ws.numel(),
              _lib.ptr(zero), zero.numel() if zero is not None else 0, _lib.stream_ptr())
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


def act_mask_bwd(g, y, act: int) -> None:
    """g *= act'(y) in place (ctr_act_mask_bwd)"""
    g, y = _mat(g, "g"), _mat(y, "y")
    m, n = g.shape
    _call("act_mask_bwd", "ctr_act_mask_bwd", lambda: (12 * m * n, m * n), g.data_ptr(), _ld(g), y.data_ptr(), _ld(y), m, n,
          act, _lib.stream_ptr())


def act_bwd(y, gy, act: int, out, accumulate: bool) -> None:
    y, gy, out = _mat(y, "y"), _mat(gy, "gy"), _mat(out, "out")
    m, n = y.shape
    _call(f"act_bwd[{m}x{n}]", "ctr_act_bwd", lambda: (4 * m * n * (3 + int(accumulate)), m * n), y.data_ptr(), _ld(y),
          gy.data_ptr(), _ld(gy), out.data_ptr(), _ld(out), m, n, act, int(accumulate), _lib.stream_ptr())


def cross_fwd(x0, u, xl, bias, out) -> torch.Tensor:
    """Deep & Cross combine: out = x0 * u + bias + xl"""
    x0, u, xl, out = _mat(x0, "x0"), _mat(u, "u"), _mat(xl, "xl"), _mat(out, "out")
    m, d = x0.shape
    _call(f"cross_fwd[{m}x{d}]", "ctr_cross_fwd", lambda: (16 * m * d, 3 * m * d), x0.data_ptr(), _ld(x0), u.data_ptr(),
          _ld(u), xl.data_ptr(), _ld(xl), bias.data_ptr(), out.data_ptr(), _ld(out), m, d, _lib.stream_ptr())
    return out


def cross_bwd(x0, u, gy, gu, gx0, gbias) -> None:
    """gu = gy * x0; gx0 += gy * u; gbias += gy.sum(0)"""
    x0, u, gy, gu, gx0 = _mat(x0, "x0"), _mat(u, "u"), _mat(gy, "gy"), _mat(gu, "gu"), _mat(gx0, "gx0")
    m, d = x0.shape
    ws = _scratch(x0.device)
    _call(f"cross_bwd[{m}x{d}]", "ctr_cross_bwd", lambda: (24 * m * d, 3 * m * d), x0.data_ptr(), _ld(x0), u.data_ptr(),
          _ld(u), gy.data_ptr(), _ld(gy), gu.data_ptr(), _ld(gu), gx0.data_ptr(), _ld(gx0), gbias.data_ptr(), m, d,
          ws.data_ptr(), ws.numel(), _lib.stream_ptr())
