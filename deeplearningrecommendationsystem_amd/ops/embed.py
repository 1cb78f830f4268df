"""The embedding stage (csrc/embed*.hip): gather, bag pooling and concat in one launch, and its backward."""
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .. import _lib
from .._lib import FIELD_BAG, FIELD_ID_F32, FIELD_ID_I64, FIELD_PROD_I64, Field
from ._call import _call, _ld, _mat, _scratch


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


def embed_fwd(specs: Sequence[FieldSpec], x: Optional[torch.Tensor], batch: int, out: torch.Tensor,
              err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fused gather + bag pooling + concat into ``out`` (B, >= sum widths)"""
    out = _mat(out, "out")
    if x is not None:
        x = _mat(x, "x")
    arr = _field_array(specs)
    _call("embed_fwd", "ctr_embed_fwd", lambda: (_embed_bytes(specs, batch, False), 0), arr, len(specs), _lib.ptr(x),
          _ld(x) if x is not None else 0, batch, out.data_ptr(), _ld(out), _lib.ptr(err_flag), _lib.stream_ptr())
    return out


def embed_bwd(specs: Sequence[FieldSpec], x: Optional[torch.Tensor], batch: int, gout: torch.Tensor,
              grads: dict) -> None:
    """accumulate into ``grads[id(table)]`` (dense, same shape as the table)"""
    gout = _mat(gout, "gout")
    if x is not None:
        x = _mat(x, "x")
    arr = _field_array(specs, grads)
    ws = _scratch(gout.device)  # bag partials + the small-table sort buffers
    _call("embed_bwd", "ctr_embed_bwd", lambda: (_embed_bytes(specs, batch, True), 0), arr, len(specs), _lib.ptr(x),
          _ld(x) if x is not None else 0, batch, gout.data_ptr(), _ld(gout), _lib.ptr(ws),
          ws.numel() if ws is not None else 0, _lib.stream_ptr())
