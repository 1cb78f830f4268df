"""Feature interactions (csrc/interact.hip, fields.hip, ffm_fused.hip, rows_sum.hip): all pairs, FM with the wide
part, N id fields with FM, FFM, bi-interaction and pair products."""
import ctypes as C
import os
from typing import Optional

import torch

from .. import _lib
from ._call import _REFUSED, _call, _ld, _mat, _scratch, _timed


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
    args = (emb.data_ptr(), _ld(emb), batch, nvec, dim, out.data_ptr(), _ld(out), _lib.stream_ptr())
    rc = _timed("allpairs_fwd", lambda: (4 * batch * (nvec * dim + npairs), 2 * batch * npairs * dim),
                _lib.load().ctr_fields_pairs_fwd if many else _lib.load().ctr_allpairs_fwd, *args)
    if many and rc in _REFUSED:
        rc = _lib.load().ctr_allpairs_fwd(*args)
    _lib.check(rc, "ctr_allpairs_fwd")
    return out


def allpairs_bwd(emb, nvec, dim, gp, gemb, accumulate: bool) -> None:
    """backward of ``allpairs_fwd``; the same admission (``ValueError`` outside 2..32 vectors)"""
    _allpairs_admit(nvec)
    emb, gp, gemb = _mat(emb, "emb"), _mat(gp, "gp"), _mat(gemb, "gemb")
    batch = emb.shape[0]
    npairs = nvec * (nvec - 1) // 2
    many = nvec > 8 and dim in (8, 16, 32, 64)
    args = (emb.data_ptr(), _ld(emb), batch, nvec, dim, gp.data_ptr(), _ld(gp), gemb.data_ptr(), _ld(gemb),
            int(accumulate), _lib.stream_ptr())
    rc = _timed("allpairs_bwd", lambda: (4 * batch * ((2 + int(accumulate)) * nvec * dim + npairs),
                                         2 * batch * npairs * dim * 2),
                _lib.load().ctr_fields_pairs_bwd if many else _lib.load().ctr_allpairs_bwd, *args)
    if many and rc in _REFUSED:
        rc = _lib.load().ctr_allpairs_bwd(*args)
    _lib.check(rc, "ctr_allpairs_bwd")


def _wide_args(x, user1, item1, w, b):
    x = _mat(x, "x")
    _lib.require_device(user1, item1, w, b)
    return (x.data_ptr(), _ld(x), USER_COL, ITEM_COL, DENSE_COL0, w.shape[1], user1.data_ptr(), user1.shape[0],
            item1.data_ptr(), item1.shape[0], w.data_ptr(), b.data_ptr())


def fm_wide_fwd(emb, nvec, dim, x, user1, item1, wide_w, wide_b, out, err_flag=None) -> None:
    emb, out = _mat(emb, "emb"), _mat(out, "out")
    batch = emb.shape[0]
    _call("fm_wide_fwd", "ctr_fm_wide_fwd", lambda: (4 * batch * (nvec * dim + 45 + 3), 4 * batch * nvec * dim),
          emb.data_ptr(), _ld(emb), batch, nvec, dim, *_wide_args(x, user1, item1, wide_w, wide_b), out.data_ptr(),
          _ld(out), _lib.ptr(err_flag), _lib.stream_ptr())


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
    _call("rows1_scatter", "ctr_rows1_scatter",
          lambda: (batch * (8 + 4 + (4 if prob is not None else 0)) + 8 * (nu + ni), 2 * batch), x.data_ptr(), _ld(x),
          USER_COL, ITEM_COL, g.data_ptr(), _ld(g), _lib.ptr(prob), _ld(prob) if prob is not None else 0, batch,
          _lib.ptr(guser1), nu, _lib.ptr(gitem1), ni, _lib.stream_ptr())


def fm_wide_bwd(emb, nvec, dim, x, user1, item1, wide_w, wide_b, gout, guser1, gitem1, gwide_w, gwide_b, gemb,
                accumulate: bool) -> None:
    emb, gout = _mat(emb, "emb"), _mat(gout, "gout")
    batch = emb.shape[0]
    ws = _scratch(emb.device)
    if _rows1_small(x, guser1, gitem1):
        rows1_scatter(x, gout, None, guser1, gitem1)
        guser1 = gitem1 = None
    _call("fm_wide_bwd", "ctr_fm_wide_bwd", lambda: (4 * batch * ((2 + int(accumulate)) * nvec * dim + 45 + 5),
                                                     4 * batch * nvec * dim),
          emb.data_ptr(), _ld(emb), batch, nvec, dim, *_wide_args(x, user1, item1, wide_w, wide_b), gout.data_ptr(),
          _ld(gout), _lib.ptr(guser1), _lib.ptr(gitem1), _lib.ptr(gwide_w), _lib.ptr(gwide_b), _lib.ptr(gemb),
          _ld(gemb) if gemb is not None else 0, int(accumulate), ws.data_ptr(), ws.numel(), _lib.stream_ptr())


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
    _call("fields_fm_fwd", "ctr_fields_fm_fwd", lambda: (batch * (nf * (dim * 8 + 8) + 4 * n1 + 4), 4 * batch * nf * dim),
          idx.data_ptr(), idx.stride(0), batch, nf, dim, _ptr_array(tables), vocabs, _ptr_array(first), _lib.ptr(bias),
          emb.data_ptr(), _ld(emb), fm.data_ptr(), _ld(fm), _lib.ptr(err_flag), _lib.stream_ptr())


def fields_fm_bwd(idx, vocabs, dim, emb, gdeep, gfm, gtables, gfirst, gbias) -> None:
    """backward of ``fields_fm_fwd``: scatter-add ``gdeep + gfm * (S - v)`` into the dense table gradients"""
    emb = _mat(emb, "emb")
    batch, nf = idx.shape
    gdeep = _mat(gdeep, "gdeep") if gdeep is not None else None
    gfm = _mat(gfm, "gfm") if gfm is not None else None
    ws = _scratch(emb.device) if gbias is not None else None
    n1 = 0 if gfirst is None else sum(1 for t in gfirst if t is not None)
    _call("fields_fm_bwd", "ctr_fields_fm_bwd",
          lambda: (batch * (nf * (dim * 4 * (2 + (gdeep is not None)) + 8) + 8 * n1 + 4),
                   3 * batch * nf * dim),
          idx.data_ptr(), idx.stride(0), batch, nf, dim, (C.c_int64 * nf)(*vocabs), emb.data_ptr(), _ld(emb),
          _lib.ptr(gdeep), _ld(gdeep) if gdeep is not None else 0, _lib.ptr(gfm), _ld(gfm) if gfm is not None else 0,
          _ptr_array(gtables), _ptr_array(gfirst), _lib.ptr(gbias), _lib.ptr(ws), ws.numel() if ws is not None else 0,
          _lib.stream_ptr())


def _pair_array(pairs):
    flat = [v for p in pairs for v in p]
    return (C.c_int32 * len(flat))(*flat)


def ffm_fused_fwd(x, tables, user1, item1, lin_w, lin_b, emb, prob, err_flag=None) -> None:
    """FFM forward in one launch: the 12 field-aware vectors into ``emb`` (B, 12k), the probability into ``prob``"""
    x, emb, prob = _mat(x, "x"), _mat(emb, "emb"), _mat(prob, "prob")
    _lib.require_device(user1, item1, lin_w, lin_b, *tables)
    batch, dim = x.shape[0], tables[0].shape[1]
    _call("ffm_fused_fwd", "ctr_ffm_fused_fwd",
          lambda: (4 * batch * (45 + 4 * dim + 2 + 12 * dim + 1), 2 * batch * (15 + 86) * dim), x.data_ptr(), _ld(x), batch,
          dim, _ptr_array(tables), user1.shape[0], item1.shape[0], user1.data_ptr(), item1.data_ptr(), lin_w.data_ptr(),
          lin_b.data_ptr(), emb.data_ptr(), _ld(emb), prob.data_ptr(), _ld(prob), _lib.ptr(err_flag), _lib.stream_ptr())


def ffm_fused_bwd(x, emb, num_users, num_items, lin_w, prob, gprob, guser1, gitem1, glin_w, glin_b, gemb) -> None:
    """backward of ``ffm_fused_fwd``'s head + dots: small gradients directly, ``gemb`` for the embedding backward"""
    x, emb, prob, gprob, gemb = _mat(x, "x"), _mat(emb, "emb"), _mat(prob, "prob"), _mat(gprob, "gprob"), _mat(gemb, "gemb")
    batch, dim = x.shape[0], emb.shape[1] // 12
    ws = _scratch(emb.device)
    _call("ffm_fused_bwd", "ctr_ffm_fused_bwd", lambda: (4 * batch * (45 + 24 * dim + 4), 4 * batch * 15 * dim),
          x.data_ptr(), _ld(x), batch, dim, emb.data_ptr(), _ld(emb), num_users, num_items, lin_w.data_ptr(),
          prob.data_ptr(), _ld(prob), gprob.data_ptr(), _ld(gprob), _lib.ptr(guser1), _lib.ptr(gitem1), _lib.ptr(glin_w),
          _lib.ptr(glin_b), gemb.data_ptr(), _ld(gemb), ws.data_ptr(), ws.numel(), _lib.stream_ptr())


def ffm_head_fwd(emb, nvec, dim, pairs, x, user1, item1, lin_w, lin_b, prob, err_flag=None) -> None:
    emb, prob = _mat(emb, "emb"), _mat(prob, "prob")
    batch = emb.shape[0]
    _call("ffm_head_fwd", "ctr_ffm_head_fwd", lambda: (4 * batch * (nvec * dim + 45 + 3), 2 * batch * len(pairs) * dim),
          emb.data_ptr(), _ld(emb), batch, nvec, dim, _pair_array(pairs), len(pairs),
          *_wide_args(x, user1, item1, lin_w, lin_b), prob.data_ptr(), _ld(prob), _lib.ptr(err_flag), _lib.stream_ptr())


def ffm_head_bwd(emb, nvec, dim, pairs, x, user1, item1, lin_w, lin_b, prob, gprob, guser1, gitem1, glin_w, glin_b,
                 gemb) -> None:
    emb, prob, gprob, gemb = _mat(emb, "emb"), _mat(prob, "prob"), _mat(gprob, "gprob"), _mat(gemb, "gemb")
    batch = emb.shape[0]
    ws = _scratch(emb.device)
    _call("ffm_head_bwd", "ctr_ffm_head_bwd", lambda: (4 * batch * (2 * nvec * dim + 45 + 6), 4 * batch * len(pairs) * dim),
          emb.data_ptr(), _ld(emb), batch, nvec, dim, _pair_array(pairs), len(pairs),
          *_wide_args(x, user1, item1, lin_w, lin_b), prob.data_ptr(), _ld(prob), gprob.data_ptr(), _ld(gprob),
          _lib.ptr(guser1), _lib.ptr(gitem1), _lib.ptr(glin_w), _lib.ptr(glin_b), gemb.data_ptr(), _ld(gemb), ws.data_ptr(),
          ws.numel(), _lib.stream_ptr())


def biinteract_fwd(emb, nvec, dim, out) -> torch.Tensor:
    """NFM bi-interaction: out[b, e] = sum_{i<j} v_i[e] * v_j[e]"""
    emb, out = _mat(emb, "emb"), _mat(out, "out")
    batch = emb.shape[0]
    _call("biinteract_fwd", "ctr_biinteract_fwd", lambda: (4 * batch * (nvec + 1) * dim, batch * dim * nvec * (nvec - 1)),
          emb.data_ptr(), _ld(emb), batch, nvec, dim, out.data_ptr(), _ld(out), _lib.stream_ptr())
    return out


def biinteract_bwd(emb, nvec, dim, gout, gemb, accumulate: bool) -> None:
    emb, gout, gemb = _mat(emb, "emb"), _mat(gout, "gout"), _mat(gemb, "gemb")
    batch = emb.shape[0]
    _call("biinteract_bwd", "ctr_biinteract_bwd",
          lambda: (4 * batch * ((2 + int(accumulate)) * nvec + 1) * dim, 3 * batch * dim * nvec), emb.data_ptr(), _ld(emb),
          batch, nvec, dim, gout.data_ptr(), _ld(gout), gemb.data_ptr(), _ld(gemb), int(accumulate), _lib.stream_ptr())


def pairprod_fwd(emb, nvec, dim, out) -> torch.Tensor:
    """AFM: out[(b*np + idx(i,j)), :] = v_i * v_j for every pair i < j"""
    emb, out = _mat(emb, "emb"), _mat(out, "out")
    batch, npairs = emb.shape[0], nvec * (nvec - 1) // 2
    _call("pairprod_fwd", "ctr_pairprod_fwd", lambda: (4 * batch * (nvec + npairs) * dim, batch * npairs * dim),
          emb.data_ptr(), _ld(emb), batch, nvec, dim, out.data_ptr(), _ld(out), _lib.stream_ptr())
    return out


def pairprod_bwd(emb, nvec, dim, gp, attn, gpool, gemb, accumulate: bool) -> None:
    emb, gp, gemb = _mat(emb, "emb"), _mat(gp, "gp"), _mat(gemb, "gemb")
    if gpool is not None:
        gpool = _mat(gpool, "gpool")
    batch, npairs = emb.shape[0], nvec * (nvec - 1) // 2
    _call("pairprod_bwd", "ctr_pairprod_bwd", lambda: (4 * batch * (2 * nvec + npairs + 1) * dim, 4 * batch * npairs * dim),
          emb.data_ptr(), _ld(emb), batch, nvec, dim, gp.data_ptr(), _ld(gp), _lib.ptr(attn), _lib.ptr(gpool),
          _ld(gpool) if gpool is not None else 0, gemb.data_ptr(), _ld(gemb), int(accumulate), _lib.stream_ptr())
