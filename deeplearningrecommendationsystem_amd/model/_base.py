"""shared host-side pieces of the model mirrors"""
from __future__ import annotations

import os
from types import SimpleNamespace as Params

import numpy as np
import torch
from torch import nn

from .. import _lib, ops, sparse, topn
from .._lib import FIELD_BAG, FIELD_ID_F32
from ..ops import FieldSpec, Layer
from ._grid import UserGridScorer


class CtrModule(nn.Module):
    """nn.Module whose forward/backward are libctrhip kernels.

    Index validation: kernels never fault on a bad id -- the forward reads it as row 0 and
    raises a device flag, the backward adds its gradient to no row.  The flag is read where
    the host syncs anyway: ``Trainer.model_eval`` (next to its ``loss.item()``), the sharded
    lookup's count exchange, or ``check_bad_index()`` called by hand -- each raises the
    ``IndexError`` ``nn.Embedding`` raises on CPU.  With ``CTRHIP_CHECK_INDEX=1`` (or
    ``self.check_index = True``) it is read after every forward (one sync per call).
    """

    check_index = os.environ.get("CTRHIP_CHECK_INDEX", "0") == "1"

    def _err_flag(self, device):
        flag = getattr(self, "_err", None)
        if flag is None or flag.device != device:
            flag = torch.zeros(1, dtype=torch.int32, device=device)
            object.__setattr__(self, "_err", flag)
        return flag

    def check_bad_index(self):
        """read the device flag (one sync) and raise IndexError if any lookup since the last check saw an
        id outside its table"""
        flag = getattr(self, "_err", None)
        if flag is not None and int(flag.item()) != 0:
            flag.zero_()
            raise IndexError("index out of range in self")

    def _raise_if_bad_index(self):
        if self.check_index:
            self.check_bad_index()

    @staticmethod
    def _need_device(*tensors):
        _lib.require_device(*tensors)

    # ---- the way into the autograd node
    @staticmethod
    def _dense(t):
        """an input in the layout the kernels read"""
        return t.contiguous()

    def _run(self, inputs, p, exchanged=()):
        """``inputs`` and the named parameters ``p`` through ``_ModelFunction``.  ``exchanged`` names the entries of
        ``p`` that the caller replaced by rows of a sharded table (``_zero_grads``)."""
        flat, spec = _flatten(p)
        self._need_device(*inputs, *flat)
        inputs = [self._dense(t) for t in inputs]
        object.__setattr__(self, "_flag", self._err_flag(inputs[0].device))
        out = _ModelFunction.apply(self, spec, exchanged, len(inputs), *inputs, *flat)
        self._raise_if_bad_index()
        return out

    def _zero_grads(self, flat, rows=()):
        """{id(t): zero gradient} for a backward pass: one flat buffer for the parameters ``flat``.  The exchanged
        ``rows`` of a sharded table are an activation, not a replicated parameter: their gradient gets a buffer of
        its own, so that the data-parallel all-reduce of the flat one does not carry it."""
        own = {id(t) for t in rows}
        zeros = ops.zero_grads([t for t in flat if id(t) not in own])
        for t in rows:
            zeros[id(t)] = torch.zeros_like(t)
        return zeros

    # ---- opt-in sparse mode of the big tables' gradients (sparse.py)
    def sparse_ids(self, inputs, p):
        """[(table out of ``p``, [id tensors scattered into that table])] -- models whose tables can run in sparse
        mode override this; ``inputs is None`` asks for the tables alone"""
        return []

    def sparse_grads(self, enable: bool = True, min_rows: int = 65536):
        """switch the tables with at least ``min_rows`` rows to the sparse gradient mode (or back).  Call after the
        module is on its device; train with ``deeplearningrecommendationsystem_amd.optim.Adam`` (it updates the
        pending rows; a stock torch optimizer would see ``grad is None`` and skip these tables)."""
        tables = [t for t, _ in self.sparse_ids(None, self._params())]
        if enable and not tables:
            raise NotImplementedError(f"{type(self).__name__} has no sparse-mode tables")
        for p in tables:
            if enable and p.shape[0] >= min_rows:
                if sparse.state_of(p) is None:
                    p._ctr_sparse = sparse.SparseRows(p)
            elif sparse.state_of(p) is not None:
                del p._ctr_sparse
        return self

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none)
        sparse.discard(self.parameters())


def _flatten(p):
    """named parameters -> (the tensors in the order autograd sees them, what ``_rebuild`` needs besides them).  An
    entry of ``p`` is a tensor, an ``ops.Layer`` (weight, then bias) or a list of entries."""
    flat = []

    def walk(v):
        if isinstance(v, Layer):
            flat.extend((v.weight, v.bias))
            return Layer(None, None, v.act)
        if isinstance(v, (list, tuple)):
            return [walk(item) for item in v]
        flat.append(v)
        return None

    spec = {name: walk(v) for name, v in vars(p).items()}
    return tuple(flat), spec


def _rebuild(spec, flat):
    """the named parameters of ``_flatten`` around the tensors ``flat``"""
    flat = iter(flat)

    def walk(s):
        if isinstance(s, Layer):
            return Layer(next(flat), next(flat), s.act)
        return next(flat) if s is None else [walk(item) for item in s]

    return Params(**{name: walk(s) for name, s in spec.items()})


class _ModelFunction(torch.autograd.Function):
    """one autograd node per model: ``impl.run_forward(inputs, p)`` returns ``(output, state)``;
    ``impl.run_backward(state, inputs, p, gout, zeros)`` leaves every parameter's gradient in ``zeros`` (keyed by
    ``id``).  Forward and backward are straight sequences of libctrhip launches on torch's current stream."""

    @staticmethod
    def forward(ctx, impl, spec, exchanged, n_inputs, *tensors):
        out, state = impl.run_forward(tensors[:n_inputs], _rebuild(spec, tensors[n_inputs:]))
        ctx.impl, ctx.state, ctx.spec, ctx.exchanged, ctx.n_inputs = impl, state, spec, exchanged, n_inputs
        ctx.save_for_backward(*tensors)
        return out

    @staticmethod
    def backward(ctx, gout):
        tensors = ctx.saved_tensors
        inputs, flat = tensors[:ctx.n_inputs], tensors[ctx.n_inputs:]
        p, gout = _rebuild(ctx.spec, flat), gout.contiguous()
        zeros = ctx.impl._zero_grads(flat, [getattr(p, name) for name in ctx.exchanged])
        ctx.impl.run_backward(ctx.state, inputs, p, gout, zeros)
        ctx.state = None
        grads = [zeros[id(t)] for t in flat]
        if any(sparse.state_of(t) is not None for t in flat):
            # sparse mode: the scatter went into the tables' persistent buffers; list the rows it touched and
            # hand autograd no dense gradient for those tables
            slot = {id(t): k for k, t in enumerate(flat)}
            jobs = []
            for table, id_list in ctx.impl.sparse_ids(inputs, p):
                if sparse.state_of(table) is not None:
                    jobs += [(table, ids) for ids in id_list]
                    grads[slot[id(table)]] = None
            sparse.mark(jobs)
        return (None,) * (4 + ctx.n_inputs) + tuple(grads)


def six_field_specs(tables, dim):
    """[user, item, age, gender, occupation, movie] vectors at columns f*dim
    (reference model/deepfm.py:45-54, model/pnn.py:113-121)"""
    user, item, age, gender, occ, movie = tables
    return [
        FieldSpec(FIELD_ID_F32, dim, 0 * dim, table=user, src_col=0),
        FieldSpec(FIELD_ID_F32, dim, 1 * dim, table=item, src_col=1),
        FieldSpec(FIELD_BAG, dim, 2 * dim, table=age, src_col=2, bag_size=1),
        FieldSpec(FIELD_BAG, dim, 3 * dim, table=gender, src_col=3, bag_size=2),
        FieldSpec(FIELD_BAG, dim, 4 * dim, table=occ, src_col=5, bag_size=21),
        FieldSpec(FIELD_BAG, dim, 5 * dim, table=movie, src_col=26, bag_size=19),
    ]


class FeatureModel(CtrModule):
    """models fed by the (B,45) float feature matrix of data/reader.py:98-112"""

    @staticmethod
    def _dense(x):
        return x if x.stride(1) == 1 else x.contiguous()     # the kernels take a row stride

    def _run_model(self, x, p, exchanged=()):
        self._need_device(x)
        if x.dim() != 2 or x.shape[1] != 45 or x.dtype != torch.float32:
            raise ValueError(f"expected a (B,45) float32 feature matrix, got {tuple(x.shape)} {x.dtype}")
        return self._run([x], p, exchanged)

    def _aligned_weight(self, w, refresh=True):
        """weights whose rows are not a multiple of 4 floats long: the GEMM kernels stage 16-byte
        aligned rows several times faster, so they read a copy padded to a multiple of 4 columns
        (refreshed on every forward -- the optimizer updates ``w`` in place)."""
        k = w.shape[1]
        if k % 4 == 0:
            return w
        pad = getattr(self, "_padded", None)
        if pad is None:
            pad = {}
            object.__setattr__(self, "_padded", pad)
        buf = pad.get(id(w))
        if buf is None or buf.device != w.device or buf.shape[0] != w.shape[0]:
            buf = torch.zeros((w.shape[0], (k + 3) // 4 * 4), dtype=w.dtype, device=w.device)
            pad[id(w)] = buf
        if refresh:
            buf[:, :k].copy_(w.detach())
        return buf[:, :k]

    @staticmethod
    def _padded_rows(rows, width, device):
        """(rows, width) buffer whose row stride is a multiple of 4 floats"""
        return torch.empty((rows, (width + 3) // 4 * 4), dtype=torch.float32, device=device)[:, :width]

    def _rank_users(self, num_users, user_item, k, chunk: int = 1 << 18):
        """reference recommendation() (e.g. model/pnn.py:133-143): for every user, score the rows of the pandas
        frame ``user_item`` that carry its id and return the positions (within those rows) of the k best.  The
        reference filters the frame and calls forward once per user (943 host->device copies and forward calls);
        here the frame goes to the device once, the rows are grouped by user with one stable sort, scored in
        ``chunk``-row forward calls under no_grad, and ranked by one batched top-k."""
        dev = next(self.parameters()).device
        feats = torch.as_tensor(user_item.values, dtype=torch.float32).to(dev)
        uid = feats[:, 0].long()
        order = torch.argsort(uid, stable=True)                 # rows of a user keep their frame order
        feats = feats[order].contiguous()
        counts = torch.bincount(uid, minlength=num_users)[:num_users]
        scores = torch.empty(feats.shape[0], dtype=torch.float32, device=dev)
        with torch.no_grad():
            for lo in range(0, feats.shape[0], chunk):
                scores[lo:lo + chunk] = self.forward(feats[lo:lo + chunk]).view(-1)
        return _segment_topk(scores, counts, k)

    # ---- the user x item grid: a row scorer and a bounded-workspace ranker (no gradients, training paths untouched)
    def _table_sizes(self):
        """(num_users, num_items) of a six-field model's id tables"""
        if getattr(self, "num_fields", None) is not None:
            raise ValueError(f"{type(self).__name__} built with num_fields= has no user and item side: "
                             "catalogue_scorer() takes the six-field model only")
        for user, item in (("user_embedding", "item_embedding"), ("user_embed", "item_embed"), ("user", "item")):
            if hasattr(self, user) and hasattr(self, item):
                return getattr(self, user).weight.shape[0], getattr(self, item).weight.shape[0]
        raise NotImplementedError(f"{type(self).__name__} has no user and item id tables")

    def catalogue_scorer(self, assembler) -> "CatalogueScorer":
        """a ``CatalogueScorer`` of this model over ``assembler`` (``data.FeatureAssembler``: the side features of
        every user and every item): ``score_rows`` / ``score_grid`` / ``recommend`` over the whole catalogue without
        the (user, item) feature frame ``recommendation()`` needs"""
        return CatalogueScorer(self, assembler)


FORWARD_GRID_PAIRS = 1 << 18     # pairs per forward call of the "forward" path: 47 MB of features


class CatalogueScorer(UserGridScorer):
    """Scores of users against EVERY item for a model fed by the (B, 45) feature matrix.  The model does not own the
    side features, so the scorer holds the model and the assembler; it keeps no copy of a weight: every call reads
    the model's parameters as they are then, so a scorer is never stale after an optimizer step.

    ``path``: "forward" here -- ``assembler.feature`` and the model's own forward over ``FORWARD_GRID_PAIRS`` pairs a
    call, under ``no_grad``; a model with a grid kernel overrides ``_scores`` (``DeepFM``: "grid")."""

    path = "forward"

    def __init__(self, model: FeatureModel, assembler):
        super().__init__(*model._table_sizes(), assembler.user_features.device)
        users, items = tuple(assembler.user_features.shape), tuple(assembler.item_features.shape)
        if len(users) != 2 or len(items) != 2 or 2 + users[1] + items[1] != 45:
            raise ValueError(f"the assembler's features are {users} and {items}: expected (U, 24) and (I, 19)")
        if (users[0], items[0]) != (self.num_users, self.num_items):
            raise ValueError(f"the assembler was built for {users[0]} x {items[0]}, the model's tables are "
                             f"{self.num_users} x {self.num_items}")
        self.model, self.assembler = model, assembler

    def _device(self):
        return self.device

    def _scores(self, users, start, stop, shared=None) -> torch.Tensor:
        rows = users.numel() if users is not None else stop - start
        out = torch.empty((rows, self.num_items), dtype=torch.float32, device=self.device)
        topn.forward_grid(out, FORWARD_GRID_PAIRS, lambda r, i: self.model.forward(
            self.assembler.feature(users[r] if users is not None else r + start, i)))
        return out


_USER_FIELDS, _ITEM_FIELDS = (0, 2, 3, 4), (1, 5)   # of six_field_specs: user, age, gender, occupation / item, movie


class SixFieldGridScorer(CatalogueScorer):
    """A six-field model on the user x item grid: every field vector belongs to the user or to the item, so what the
    model computes ahead of its first nonlinearity splits into rows of a user-side and an item-side table, and a kernel
    scores the pairs from those.  The rows of BOTH sides are made for the whole table at every public call (the weights
    are read then), in passes of ``side_chunk`` rows at fixed positions: a table row's bits then do not depend on which
    users were asked for.  A model supplies ``_side_buffers``, ``_side_rows`` and ``_grid_scores``; ``_side_prepare``
    and ``_operands`` are for what a model makes beside the two sides' buffers, ``_field_specs`` for a model whose
    embedding stage is not ``six_field_specs`` over its tables; such a model also says through ``_tables`` which tables
    those are, through ``_stage`` how wide a row of its stage is (FFM: twelve vectors; Wide & Deep: the 5E + 1 stack)
    and through ``_zero_other`` which of its columns are the other side's."""

    path = "grid"
    row_blocks = 0               # 0: the launch's own geometry (tests set 1, 2 to reach the tile loop at small shapes)
    side_chunk = 1 << 16         # table rows per pass of _side: bounds its (rows, 6E) buffer and the hook's own

    def _field_specs(self, p, dim, dev) -> list:
        """the embedding stage's field list of the six vectors at columns f * dim; a model whose tables are not the six
        of ``six_field_specs`` brings its own"""
        return six_field_specs([t.detach() for t in p.tables], dim)

    def _tables(self, p) -> list:
        """the embedding tables of ``p``, every one of them ``dim`` wide"""
        return p.tables

    def _stage(self, rows, dim, dev) -> tuple:
        """(the buffer the embedding stage fills for ``rows`` feature rows, the same by field vector -- or None)"""
        emb = torch.empty((rows, 6 * dim), dtype=torch.float32, device=dev)
        return emb, emb.view(rows, 6, dim)

    def _side_prepare(self, p) -> None:
        """runs once a side, in front of its allocations and its passes: what ``_side_rows`` reads and does not make"""

    def _side_buffers(self, p, rows, dim, user_side: bool, dev) -> tuple:
        """what ``_side`` returns for one side's table of ``rows`` rows, allocated"""
        raise NotImplementedError

    def _side_rows(self, p, x, emb, vec, lo, hi, user_side: bool, buffers) -> None:
        """fill rows [lo, hi) of ``buffers`` from the feature rows ``x`` and their field vectors ``emb`` (``vec``: the
        same as (rows, 6, E)); ``_zero_other`` in front of whatever reads ``emb`` as one side's"""
        raise NotImplementedError

    def _operands(self, p) -> tuple:
        return ()                # what ``_shared`` returns behind the two sides; made before them

    def _grid_scores(self, shared, users, user0, rows) -> torch.Tensor:
        """the one kernel call, for ``rows`` >= 1"""
        raise NotImplementedError

    @staticmethod
    def _fields(user_side: bool):
        return _USER_FIELDS if user_side else _ITEM_FIELDS

    def _zero_other(self, vec, user_side: bool) -> None:
        vec[:, self._fields(not user_side), :] = 0.0             # the other side's columns add exact zeros

    def _side(self, p, user_side: bool):
        asm = self.assembler
        dev, dim = self._device(), self._tables(p)[0].shape[1]
        rows = self.num_users if user_side else self.num_items
        self._side_prepare(p)
        buffers = self._side_buffers(p, rows, dim, user_side, dev)
        flag = self.model._err_flag(dev)
        for lo in range(0, rows, self.side_chunk):
            hi = min(rows, lo + self.side_chunk)
            ids, zero = torch.arange(lo, hi, device=dev), torch.zeros(hi - lo, dtype=torch.int64, device=dev)
            x = asm.feature(ids, zero) if user_side else asm.feature(zero, ids)
            # the field vectors exactly as the forward gathers them
            emb, vec = self._stage(hi - lo, dim, dev)
            ops.embed_fwd(self._field_specs(p, dim, dev), x, hi - lo, emb, flag)
            self._side_rows(p, x, emb, vec, lo, hi, user_side, buffers)
        return buffers

    def _shared(self):
        p = self.model._params()
        self.model._need_device(self._tables(p)[0], self.assembler.user_features)
        rest = self._operands(p)
        return (p, self._side(p, True), self._side(p, False)) + rest

    def _scores(self, users, start, stop, shared=None):
        rows = users.numel() if users is not None else stop - start
        if rows == 0:
            return torch.empty((0, self.num_items), dtype=torch.float32, device=self._device())
        return self._grid_scores(shared, users, start, rows)


def _segment_topk(scores: torch.Tensor, counts: torch.Tensor, k: int) -> np.ndarray:
    """top-k positions inside consecutive segments of ``scores`` (segment u has ``counts[u]`` entries)"""
    n_seg, longest = counts.numel(), int(counts.max()) if counts.numel() else 0
    if k > int(counts.min()):
        raise RuntimeError(f"selected index k out of range: a user has {int(counts.min())} candidate rows, k = {k}")
    if int(counts.min()) == longest:                                     # the usual case: every user x every item
        grid = scores.view(n_seg, longest)
    else:
        starts = torch.cumsum(counts, 0) - counts
        pos = torch.arange(longest, device=scores.device).unsqueeze(0)
        valid = pos < counts.unsqueeze(1)
        grid = torch.full((n_seg, longest), float("-inf"), device=scores.device)
        grid[valid] = scores[(starts.unsqueeze(1) + pos)[valid]]
    return ops.topk_rows(grid, k).cpu().numpy()
