"""DIN / DIEN sequence attention and the GRU (csrc/din.hip, gru.hip, linear_skinny.hip, linear_n1.hip)."""
import torch

from .. import _lib
from .._lib import ACT_NONE
from ._call import _call, _ld, _mat, _refused, _scratch, _timed


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
    _call(f"linear_group_fwd[{m}x{n}x{k}]", "ctr_linear_group_fwd",
          lambda: (4 * (m * k + n * k + m * n + (m // group) * n) + (m * n // 8 if sign_bits is not None else 0),
                   2 * m * n * k),
          x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), _lib.ptr(bias), res.data_ptr(), _ld(res), group, out.data_ptr(),
          _ld(out), _lib.ptr(sign_bits), sign_bits.stride(0) if sign_bits is not None else 0, m, n, k, act,
          _lib.stream_ptr())
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
    _call(f"linear_dx_masked[{m}x{n}x{k}]", "ctr_linear_dx_masked",
          lambda: (4 * (m * n * (2 if act != ACT_NONE else 1) + n * k + m * k) + mask_bytes, 2 * m * n * k), w.data_ptr(),
          _ld(w), _lib.ptr(y), _ld(y) if y is not None else 0, gy.data_ptr(), _ld(gy), act, _lib.ptr(xin),
          _ld(xin) if xin is not None else 0, act_in, _lib.ptr(sign_bits),
          sign_bits.stride(0) if sign_bits is not None else 0, gx.data_ptr(), _ld(gx), _lib.ptr(gsum),
          _ld(gsum) if gsum is not None else 0, group, m, n, k, _lib.stream_ptr())


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
    _call(f"linear_fwd_dot[{m}x{n}x{k}]", "ctr_linear_fwd_dot",
          lambda: (4 * (m * k + n * k + n + m * n + m), 2 * m * n * (k + 1)), x.data_ptr(), _ld(x), w.data_ptr(), _ld(w),
          _lib.ptr(b), y.data_ptr(), _ld(y), u.data_ptr(), _lib.ptr(c), out.data_ptr(), 1, m, n, k, act, _lib.stream_ptr())
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
    _call(f"linear_dx_scatter[{m}x{n}x{k}]", "ctr_linear_dx_scatter",
          lambda: (4 * (m * n + n * k + 3 * m + 3 * m * k), 2 * m * n * k), w.data_ptr(), _ld(w), gy.data_ptr(), _ld(gy),
          idx.data_ptr(), attn.data_ptr(), gpool.data_ptr(), _ld(gpool), group, gtable.data_ptr(), gtable.shape[0], m, n, k,
          _lib.stream_ptr())


def linear_n1_bwd_masked(x, w, gy, act_in: int, gx, gw=None, gb=None) -> None:
    """backward of the single-unit layer y = x @ w.T + b whose input x is the previous layer's activation output:
    gx = (gy @ w) * act_in'(x) (``gx`` may be ``x`` itself), gw += gy.T @ x, gb += gy.sum()"""
    x, w, gy, gx = _mat(x, "x"), _mat(w, "w"), _mat(gy, "gy"), _mat(gx, "gx")
    m, k = x.shape
    if w.shape[0] != 1 or gy.shape != (m, 1) or gx.shape != (m, k):
        raise ValueError("linear_n1_bwd_masked: w must be (1, k), gy (m, 1), gx (m, k)")
    ws = _scratch(x.device) if gw is not None else None
    _call(f"linear_n1_bwd_masked[{m}x1x{k}]", "ctr_linear_n1_bwd_masked", lambda: (4 * (2 * m * k + m + 2 * k), 4 * m * k),
          x.data_ptr(), _ld(x), w.data_ptr(), gy.data_ptr(), _ld(gy), act_in, gx.data_ptr(), _ld(gx), _lib.ptr(gw),
          _lib.ptr(gb), m, k, _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr())


def din_scatter_bwd(hist, vocab, dim, gh, attn, gpool, summed: bool, gtable) -> None:
    """history positions' rows of the table gradient: gh + attn * gpool, scatter-added by hist ids"""
    gh, gpool = _mat(gh, "gh"), _mat(gpool, "gpool")
    batch, length = hist.shape
    _call("din_scatter_bwd", "ctr_din_scatter_bwd", lambda: (batch * length * (8 + 4 + 4 * dim * (3 if summed else 4)), 0),
          hist.data_ptr(), vocab, batch, length, dim, gh.data_ptr(), _ld(gh), attn.data_ptr(), gpool.data_ptr(), _ld(gpool),
          int(summed), gtable.data_ptr(), _lib.stream_ptr())


def din_concat_fwd(table, hist, target, c, tvec, err_flag=None, pair: bool = False, h_only: bool = False) -> None:
    """attention operand per position: [h, h-t, t] (the reference's cat), ``pair``: [h, t], ``h_only``: [h]"""
    _lib.require_device(table, hist, target)
    c = _mat(c, "c")
    batch, length = hist.shape
    dim = table.shape[1]
    width = 1 if h_only else (2 if pair else 3)
    _call("din_concat_fwd", "ctr_din_concat_fwd",
          lambda: (batch * length * (dim * 4 + 8 + 4 * width * dim) + batch * (8 + 8 * dim), 0), table.data_ptr(),
          table.shape[0], dim, hist.data_ptr(), target.data_ptr(), batch, length, c.data_ptr(), _ld(c), _lib.ptr(tvec),
          _ld(tvec) if tvec is not None else 0, _lib.DIN_H if h_only else (_lib.DIN_PAIR if pair else _lib.DIN_TRIPLE),
          _lib.ptr(err_flag), _lib.stream_ptr())


def din_pool_fwd(score, hsrc, batch, length, dim, attn, out, summed: bool) -> None:
    hsrc, out = _mat(hsrc, "hsrc"), _mat(out, "out")
    _call("din_pool_fwd", "ctr_din_pool_fwd",
          lambda: (4 * batch * length * (2 + dim * (1 if summed else 2)), 2 * batch * length * dim), score.data_ptr(),
          hsrc.data_ptr(), _ld(hsrc), batch, length, dim, attn.data_ptr(), out.data_ptr(), _ld(out), int(summed),
          _lib.stream_ptr())


def din_pool_bwd(attn, hsrc, batch, length, dim, gout, summed: bool, gscore) -> None:
    hsrc, gout = _mat(hsrc, "hsrc"), _mat(gout, "gout")
    _call("din_pool_bwd", "ctr_din_pool_bwd",
          lambda: (4 * batch * length * (2 + dim * (1 if summed else 2)), 2 * batch * length * dim), attn.data_ptr(),
          hsrc.data_ptr(), _ld(hsrc), batch, length, dim, gout.data_ptr(), _ld(gout), int(summed), gscore.data_ptr(),
          _lib.stream_ptr())


def din_concat_bwd(hist, target, vocab, dim, gc, attn, gout, summed: bool, gt_extra, gtable,
                   pair: bool = False) -> None:
    gc, gout = _mat(gc, "gc"), _mat(gout, "gout")
    batch, length = hist.shape
    width = 2 if pair else 3
    _call("din_concat_bwd", "ctr_din_concat_bwd",
          lambda: (batch * length * (8 + 4 + 4 * width * dim + 8 * dim) + batch * 16 * dim, 0), hist.data_ptr(),
          target.data_ptr(), vocab, batch, length, dim, gc.data_ptr(), _ld(gc), attn.data_ptr(), gout.data_ptr(), _ld(gout),
          int(summed), _lib.ptr(gt_extra), _ld(gt_extra) if gt_extra is not None else 0,
          _lib.DIN_PAIR if pair else _lib.DIN_TRIPLE, gtable.data_ptr(), _lib.stream_ptr())


def gru_fwd(gi, w_hh, b_hh, batch, length, dim, hbuf, last) -> None:
    gi = _mat(gi, "gi")
    _call("gru_fwd", "ctr_gru_fwd", lambda: (4 * batch * length * 4 * dim, 6 * batch * length * dim * dim), gi.data_ptr(),
          _ld(gi), w_hh.data_ptr(), b_hh.data_ptr(), batch, length, dim, hbuf.data_ptr(), _lib.ptr(last),
          _ld(last) if last is not None else 0, _lib.stream_ptr())


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
    _call("gru_fused_bwd", "ctr_gru_fused_bwd", lambda: (4 * batch * length * 3 * dim, 36 * batch * length * dim * dim),
          x.data_ptr(), _ld(x), w_ih.data_ptr(), b_ih.data_ptr(), w_hh.data_ptr(), b_hh.data_ptr(), hbuf.data_ptr(), batch,
          length, dim, glast.data_ptr(), _ld(glast), gx.data_ptr(), _ld(gx), gw_ih.data_ptr(), gb_ih.data_ptr(),
          gw_hh.data_ptr(), gb_hh.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())


def gru_bwd(gi, w_hh, b_hh, hbuf, batch, length, dim, glast, dgi, dgh) -> None:
    gi, glast = _mat(gi, "gi"), _mat(glast, "glast")
    _call("gru_bwd", "ctr_gru_bwd", lambda: (4 * batch * length * 10 * dim, 12 * batch * length * dim * dim), gi.data_ptr(),
          _ld(gi), w_hh.data_ptr(), b_hh.data_ptr(), hbuf.data_ptr(), batch, length, dim, glast.data_ptr(), _ld(glast),
          dgi.data_ptr(), dgh.data_ptr(), _lib.stream_ptr())
