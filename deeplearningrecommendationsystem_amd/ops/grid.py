"""The grid scorers (csrc/*_grid.hip): every model's scores over the user x item or history x item grid."""
from typing import Optional, Sequence

import torch

from .. import _lib
from .._lib import ACT_SIGMOID
from ._call import _call, _f32_vectors, _i64, _ld, _mat
from .dense import Layer


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
    _call("ncf_grid_scores", "ctr_ncf_grid_scores",
          lambda: (4 * ((rows + ni) * (width + mf) + rows * ni) + (8 * rows if users is not None else 0),
                   rows * ni * (2 * tower + 2 * (mf + fold_k) + width)),
          p_u.data_ptr(), p_i.data_ptr(), gmf_u.data_ptr(), gmf_i.data_ptr(), nu, ni, mf, width, arr, len(layers),
          wfold.data_ptr(), cfold.data_ptr(), fold_k, _lib.ptr(users) if users is not None and rows else None, user0, rows,
          act, _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, _lib.stream_ptr())
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
    _call("din_grid_pool", "ctr_din_grid_pool",
          lambda: (4 * (ni * (dim + n1) + rows * length * (2 + n1 + dim) + rows * ni * dim),
                   rows * ni * length * (2 * n1 * n2 + n1 + 2 * n2 + 2 * dim)),
          table.data_ptr(), ni, dim, at.data_ptr(), ah.data_ptr(), int(ah_by_position), w2.data_ptr(), b2.data_ptr(),
          w3.data_ptr(), n1, n2, hist.data_ptr() if hist.numel() else None, rows, length,
          _lib.ptr(out) if out.numel() else None, max(_ld(out), dim) if out.shape[0] else dim, _lib.ptr(err_flag),
          _lib.stream_ptr())
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
    _call("dien_grid_hidden", "ctr_dien_grid_hidden",
          lambda: (4 * (ni * n1 + rows * length * (2 + n1 + gates) + rows * ni * dim),
                   rows * ni * length * (2 * n1 * n2 + n1 + 2 * n2 + 2 * dim * gates + 4 * gates)),
          at.data_ptr(), hp.data_ptr(), int(hp_by_position), ni, dim, w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), n1, n2,
          b_ih.data_ptr(), w_hh.data_ptr(), b_hh.data_ptr(), hist.data_ptr(), rows, length, _lib.ptr(out),
          max(_ld(out), dim), _lib.ptr(err_flag), _lib.stream_ptr())
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
    _call("deepfm_grid_scores", "ctr_deepfm_grid_scores",
          lambda: (4 * ((rows + ni) * (n1 + dim + 1) + rows * ni) + (8 * rows if users is not None else 0),
                   rows * ni * (2 * n1 * n2 + n1 + 2 * n2 + 2 * dim)),
          zu.data_ptr(), zi.data_ptr(), su.data_ptr(), si.data_ptr(), a.data_ptr(), b.data_ptr(), nu, ni, dim, n1, n2,
          w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), out_w.data_ptr(), out_b.data_ptr(),
          _lib.ptr(users) if users is not None and rows else None, user0, rows, _lib.ptr(out) if out.numel() else None,
          _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
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
    _call("pnn_grid_scores", "ctr_pnn_grid_scores",
          lambda: (4 * (rows * (n1 + 4 * dim) + ni * (n1 + 2 * dim) + rows * ni) + (8 * rows if users is not None else 0),
                   rows * ni * 2 * (PNN_GRID_CROSS * dim + n1 * PNN_GRID_CROSS + n1 + n1 * n2 + n2 * n3 + n3)),
          zu.data_ptr(), zi.data_ptr(), fu.data_ptr(), fi.data_ptr(), g.data_ptr(), nu, ni, dim, n1, n2, n3,
          d2_w.data_ptr(), d2_b.data_ptr(), d3_w.data_ptr(), d3_b.data_ptr(), out_w.data_ptr(), out_b.data_ptr(),
          _lib.ptr(users) if users is not None and rows else None, user0, rows, _lib.ptr(out) if out.numel() else None,
          _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
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
    _call("afm_grid_scores", "ctr_afm_grid_scores",
          lambda: (4 * (rows * (4 + 4 * dim) + ni * (3 + 2 * dim) + rows * ni) + (8 * rows if users is not None else 0),
                   rows * ni * AFM_GRID_CROSS * (3 * dim + 2 * dim * att + 3 * att + 8)),
          su.data_ptr(), si.data_ptr(), fu.data_ptr(), fi.data_ptr(), nu, ni, dim, att, att_w.data_ptr(), att_b.data_ptr(),
          att_h.data_ptr(), out_w.data_ptr(), _lib.ptr(users) if users is not None and rows else None, user0, rows,
          _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
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
    _call("lowrank_grid_scores", "ctr_lowrank_grid_scores",
          lambda: (4 * ((rows + ni) * (rank + 1) + rows * ni) + (8 * rows if users is not None else 0),
                   rows * ni * (2 * rank + 2)),
          cu.data_ptr() if rank else None, ci.data_ptr() if rank else None, a.data_ptr() if a is not None else None,
          b.data_ptr() if b is not None else None, nu, ni, rank, _lib.ptr(users) if users is not None and rows else None,
          user0, rows, _lib.ptr(out) if out.numel() else None, _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
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
    _call("widedeep_grid_scores", "ctr_widedeep_grid_scores",
          lambda: (4 * ((rows + ni) * (n1 + 1) + rows * ni) + (8 * rows if users is not None else 0),
                   rows * ni * (2 * n1 * n2 + n1 + 2 * n2)),
          zu.data_ptr(), zi.data_ptr(), a.data_ptr(), b.data_ptr(), nu, ni, n1, n2, w2.data_ptr(), b2.data_ptr(),
          w3.data_ptr(), b3.data_ptr(), out_w.data_ptr(), out_b.data_ptr(),
          _lib.ptr(users) if users is not None and rows else None, user0, rows, _lib.ptr(out) if out.numel() else None,
          _ld(out) if rows else ni, int(row_blocks), _lib.stream_ptr())
    return out
