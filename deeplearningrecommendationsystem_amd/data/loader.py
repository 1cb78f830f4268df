"""Device-side mini-batch loader: shuffled epochs over sample tensors that live on the device, one
``ctr_load_batch`` launch per batch (csrc/loader.hip).  The reference trains full-batch and leaves its
data/dataloader.py and data/dataset.py empty; this fills that slot for sample sets larger than one step.

Position ``p`` of epoch ``e`` reads sample ``perm(seed, e, p)``, a stateless keyed permutation defined in the kernel
file's header comment: no ``randperm``, no N-sized index tensor, no ``index_select`` per tensor.

Batches and ranks (pure host arithmetic, ``batch_ranges``).  With F = N // batch_size full batches, every rank takes
F // world of them, rank r the batches r, r + world, ... of the SAME permutation, so all ranks run the same number of
full steps.  The positions behind those batches, [(F // world) * world * batch_size, N), are dropped with
``drop_last``; otherwise they are cut into ``world`` contiguous pieces (the first ``rest % world`` one sample longer)
and piece r is rank r's tail batch.  With world == 1 that is the usual N % batch_size tail.

The loader owns one set of static full-size batch buffers -- what a captured training graph reads, see
``Trainer.train_epoch`` -- and a separately allocated set for the tail batch.  ``epoch()`` yields views of them: a batch
is valid until the next one is drawn.  There is no CPU fallback.

Drawn negatives.  A loader built with ``negatives=k`` and ``observed=ObservedPairs(...)`` is given the positives only
and emits, per epoch, every positive once and k negatives per positive, drawn inside the same launch and shuffled in
with the positives (``ctr_load_batch_neg``; the definition stands in the kernel file's header comment).  Everything
above then speaks of the virtual epoch of ``num_samples = num_positives * (1 + k)`` positions.  An unshuffled pass --
what ``valid_epoch`` / ``test_epoch`` ask for -- shows each positive followed by its k negatives, the same ones every
time.

Grouped epochs.  The shuffle of the virtual epoch scatters a positive and its negatives over the batches.  A loader built
with ``grouped=True`` shuffles the positives instead and keeps each one's k negatives behind it
(``ctr_load_batch_groups``; the definition stands in the kernel file's header comment): every batch is a run of whole
groups of ``1 + k`` samples, the positive first -- what ``loss.BPRLoss`` / ``loss.SampledSoftmaxLoss`` read.  The
samples of an epoch are the ungrouped loader's, in another order.  ``batch_size`` must be a multiple of ``1 + k``; the
batch ranges are those of ``num_positives`` groups in batches of ``batch_size // (1 + k)``, scaled by ``1 + k``, so
neither a tail piece nor the ``world > 1`` split cuts a group.

Weighted negatives.  With ``item_sampler=ItemSampler(...)`` (``data/sampler.py``) the draws follow the sampler's alias
table instead of the uniform distribution (``ctr_load_batch_neg_pop`` / ``ctr_load_batch_groups_pop``; kernel file's
header comment), grouped or not, every family; for user u the drawn items follow ``q_i / (1 - Q_u)``, Q_u the table
mass of u's observed items.  Every buffer set then owns a log-q column, ``log_q_of(rating)``: ``log q(item)`` of each
sample of the batch, what ``loss.SampledSoftmaxLoss(log_q=loader)`` subtracts.  ``item_sampler=None`` is the uniform
path, call for call.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib


def batch_ranges(n: int, batch_size: int, drop_last: bool = False, rank: int = 0, world: int = 1):
    """[(first position, count)] of one rank's batches in an epoch of ``n`` samples (module docstring)"""
    if n < 1 or batch_size < 1:
        raise ValueError("batch_ranges(): n and batch_size must be positive")
    if world < 1 or not 0 <= rank < world:
        raise ValueError("batch_ranges(): need 0 <= rank < world")
    per_rank = (n // batch_size) // world
    out = [((k * world + rank) * batch_size, batch_size) for k in range(per_rank)]
    used = per_rank * world * batch_size
    rest = n - used
    if not drop_last and rest > 0:
        base, extra = divmod(rest, world)
        count = base + (1 if rank < extra else 0)
        if count:
            out.append((used + rank * base + min(rank, extra), count))
    return out


class ObservedPairs:
    """The (user, item) pairs no negative may repeat, as a CSR over users: ``indptr`` (num_users + 1) int64, ``indices``
    int32 item ids, ascending and distinct within a row -- 4 B per pair whatever ``num_items`` is.  ``users`` / ``items``
    are 1-D int64 tensors, or sequences of them to union (train | valid | test).  Built once with torch ops on the
    device the ids live on."""

    def __init__(self, users, items, num_users, num_items):
        users = torch.cat([t.reshape(-1) for t in users]) if isinstance(users, (list, tuple)) else users
        items = torch.cat([t.reshape(-1) for t in items]) if isinstance(items, (list, tuple)) else items
        self.num_users, self.num_items = int(num_users), int(num_items)
        if self.num_users < 1 or self.num_items < 1:
            raise ValueError("ObservedPairs: num_users and num_items must be positive")
        if self.num_items >= 1 << 31:
            raise ValueError("ObservedPairs: num_items must be below 2^31 (item ids are stored as int32)")
        if self.num_users >= 1 << 31:
            raise ValueError("ObservedPairs: num_users must be below 2^31")
        if users.dtype != torch.int64 or items.dtype != torch.int64 or users.dim() != 1 or users.shape != items.shape:
            raise ValueError("ObservedPairs: users and items must be 1-D int64 tensors of one length")
        if users.numel() and bool(((users < 0) | (users >= self.num_users) | (items < 0) | (items >= self.num_items)).any()):
            raise IndexError("index out of range in self")
        keys = torch.unique(users * self.num_items + items)          # sorted: by user, then by item
        rows = torch.div(keys, self.num_items, rounding_mode="floor")
        self.indices = (keys - rows * self.num_items).to(torch.int32)
        self.indptr = torch.zeros(self.num_users + 1, dtype=torch.int64, device=users.device)
        torch.cumsum(torch.bincount(rows, minlength=self.num_users), 0, out=self.indptr[1:])

    def __len__(self):
        return self.indices.shape[0]

    def contains(self, users, items) -> torch.Tensor:
        """bool tensor: is (users[b], items[b]) observed; ids outside the tables are not"""
        inside = (users >= 0) & (users < self.num_users) & (items >= 0) & (items < self.num_items)
        rows = torch.repeat_interleave(torch.arange(self.num_users, device=self.indptr.device), self.indptr.diff())
        keys = rows * self.num_items + self.indices
        query = torch.where(inside, users * self.num_items + items, torch.full_like(users, -1))
        at = torch.searchsorted(keys, query).clamp_(max=max(len(self) - 1, 0))
        return inside & (keys[at] == query) if len(self) else torch.zeros_like(inside)


class _Column:
    """an (N,) or (N, w) int64 / float32 source copied row by row"""

    def __init__(self, name, src):
        if src.dtype not in (torch.int64, torch.float32) or src.dim() not in (1, 2):
            raise ValueError(f"DeviceLoader: {name} must be an (N,) or (N, w) int64 or float32 tensor")
        self.src = src.contiguous()
        self.width = 1 if src.dim() == 1 else src.shape[1]
        if self.width < 1:
            raise ValueError(f"DeviceLoader: {name} has no columns")

    def buffer(self, rows):
        return torch.empty((rows,) + tuple(self.src.shape[1:]), dtype=self.src.dtype, device=self.src.device)

    def describe(self, col, dst):
        col.src, col.dst = self.src.data_ptr(), dst.data_ptr()
        col.lds = col.ldd = col.width = self.width
        col.elem_bytes = self.src.element_size()


class _Buffers:
    """one set of batch outputs and the descriptor that fills them"""

    def __init__(self, loader, rows):
        self.desc = d = _lib.Loader()
        d.n = loader.num_positives
        d.ncols = len(loader._columns)
        self.cols = []
        for k, c in enumerate(loader._columns):
            self.cols.append(c.buffer(rows))
            c.describe(d.cols[k], self.cols[k])
        self.feat = self.hist = None
        dev = loader.device
        if loader._feature is not None:
            asm, users, items = loader._feature
            self.feat = torch.empty((rows, asm.width), dtype=torch.float32, device=dev)
            d.feat_users, d.feat_items = users.data_ptr(), items.data_ptr()
            d.user_feat, d.item_feat = asm.user_features.data_ptr(), asm.item_features.data_ptr()
            d.num_users, d.user_width = asm.user_features.shape
            d.num_items, d.item_width = asm.item_features.shape
            d.feat_out, d.feat_ldo = self.feat.data_ptr(), self.feat.stride(0)
        if loader._history is not None:
            history, users = loader._history
            self.hist = torch.empty((rows, history.shape[1]), dtype=torch.int64, device=dev)
            d.hist_users, d.history = users.data_ptr(), history.data_ptr()
            d.hist_rows, d.hist_len = history.shape
            d.ld_history = history.stride(0)
            d.hist_out, d.hist_ldo = self.hist.data_ptr(), self.hist.stride(0)
        d.err_flag = loader._err.data_ptr()
        self.logq = self.pop = None
        if loader._sampler is not None:                    # the log-q column of these rows and the descriptor that fills it
            sampler, items = loader._sampler
            self.logq = torch.empty(rows, dtype=torch.float32, device=dev)
            self.pop = w = _lib.LoaderPop()
            w.table, w.pos_items, w.log_q = sampler.table.data_ptr(), items.data_ptr(), sampler.log_q.data_ptr()
            w.logq_out, w.logq_ldo = self.logq.data_ptr(), 1

    def batch(self, family):
        rating = self.cols[-1]
        if family == "pairs":
            return (self.cols[0], self.cols[1]), rating
        if family == "features":
            return (self.feat,), rating
        return (self.hist, self.cols[0]), rating


class DeviceLoader:
    """Shuffled mini-batches of device-resident samples; build one with ``pairs``, ``features`` or ``sequences``.

    ``for args, rating in loader.epoch(e)`` draws this rank's batches of epoch ``e``: ``model(*args)`` against
    ``rating``.  ``len(loader)`` batches; the full-size ones are views of ``static_batch()``."""

    def __init__(self, family, columns, ids, feature, history, batch_size, seed, shuffle, drop_last, rank, world,
                 negatives=0, observed=None, grouped=False, item_sampler=None):
        if int(batch_size) < 1:
            raise ValueError("DeviceLoader: batch_size must be positive")
        if int(world) < 1 or not 0 <= int(rank) < int(world):
            raise ValueError("DeviceLoader: need 0 <= rank < world")
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("DeviceLoader: seed must fit an unsigned 64-bit integer")
        self.negatives = int(negatives)
        if self.negatives < 0 or (self.negatives > 0) != (observed is not None):
            raise ValueError("DeviceLoader: negatives > 0 and observed=ObservedPairs(...) go together")
        self.grouped = bool(grouped)
        if self.grouped and (self.negatives < 1 or int(batch_size) % (1 + self.negatives)):
            raise ValueError("DeviceLoader: grouped=True needs negatives >= 1 and a batch_size that is a multiple of "
                             "1 + negatives")
        samples = [t for _, t in columns] + list(ids)
        tables = [feature.user_features, feature.item_features] if feature is not None else []
        _lib.require_device(*samples, *tables, history)
        if any(t.dtype != torch.int64 or t.dim() != 1 for t in ids):
            raise ValueError("DeviceLoader: the id columns must be 1-D int64 tensors")
        self._columns = [_Column(name, t) for name, t in columns]
        n = samples[0].shape[0]
        if n < 1 or any(t.shape[0] != n for t in samples):
            raise ValueError("DeviceLoader: the sample tensors must have one length, at least 1")
        if history is not None and (history.dtype != torch.int64 or history.dim() != 2 or 0 in history.shape):
            raise ValueError("DeviceLoader: history must be a (U, L) int64 matrix")
        # the epoch: every positive, and `negatives` drawn samples per positive
        self.family, self.num_positives, self.device = family, n, samples[0].device
        self.num_samples = n = n * (1 + self.negatives)
        self.batch_size, self.seed, self.shuffle = int(batch_size), int(seed), bool(shuffle)
        self.drop_last, self.rank, self.world = bool(drop_last), int(rank), int(world)
        ids = [t.contiguous() for t in ids]
        self._users = ids[0]                               # every family: the users come first
        self._feature = None if feature is None else (feature, ids[0], ids[1])
        self._history = None if history is None else (history.contiguous(), ids[0])
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._neg = self._fail = self._sampler = None
        if self.negatives:
            self._describe_negatives(observed, ids[0])
        if item_sampler is not None:
            self._describe_sampler(item_sampler, observed, ids[1])
        if self.grouped:    # the ranges of the groups, scaled: no batch, tail piece or rank boundary cuts a group
            per = 1 + self.negatives
            groups = batch_ranges(self.num_positives, self.batch_size // per, self.drop_last, self.rank, self.world)
            self._ranges = [(first * per, count * per) for first, count in groups]
        else:
            self._ranges = batch_ranges(n, self.batch_size, self.drop_last, self.rank, self.world)
        # a tail piece that happens to hold batch_size samples is still the tail: it has its own buffers
        self._num_full = (n // self.batch_size) // self.world
        tail = self._ranges[-1][1] if len(self._ranges) > self._num_full else 0
        self._full = _Buffers(self, self.batch_size) if self._num_full else None
        self._tail = _Buffers(self, tail) if tail else None

    def _describe_negatives(self, observed, users):
        """the ``ctr_loader_neg_t`` both buffer sets share"""
        _lib.require_device(observed.indptr, observed.indices)
        rating = self._columns[-1]                         # every family: the ratings come last
        if rating.width != 1 or rating.src.dtype != torch.float32:
            raise ValueError("DeviceLoader: with negatives the ratings must be (N,) or (N, 1) float32")
        self._fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._neg_keep = (observed, users)                 # what the descriptor points into
        self._neg = g = _lib.LoaderNeg()
        g.negatives = self.negatives
        g.item_col = {"pairs": 1, "features": -1, "sequences": 0}[self.family]    # items / (in the join) / targets
        g.rating_col = len(self._columns) - 1
        g.users = users.data_ptr()
        g.num_users, g.num_items = observed.num_users, observed.num_items
        g.indptr, g.indices = observed.indptr.data_ptr(), observed.indices.data_ptr()
        g.fail_flag = self._fail.data_ptr()

    def _describe_sampler(self, sampler, observed, items):
        """weighted negatives: what every buffer set's ``ctr_loader_pop_t`` points into; ``items``: the positives'"""
        if self.negatives < 1:
            raise ValueError("DeviceLoader: item_sampler needs negatives >= 1 (and observed=ObservedPairs(...))")
        if sampler.num_items != observed.num_items:
            raise ValueError(f"DeviceLoader: the item_sampler covers {sampler.num_items} items, the observed pairs "
                             f"{observed.num_items}")
        _lib.require_device(sampler.table, sampler.log_q)
        # one gather: a positive the table never draws has log q = -inf, and the corrected loss would see it (an id
        # outside the table is the kernel's business, as everywhere: *err_flag)
        inside = (items >= 0) & (items < sampler.num_items)
        log_q = sampler.log_q[items.clamp(0, sampler.num_items - 1)]
        if bool((inside & torch.isinf(log_q)).any()):
            raise ValueError("DeviceLoader: a positive's item has probability 0 under the item_sampler (log q = -inf)")
        self._sampler = (sampler, items)

    # -- constructors ------------------------------------------------------------------------------------------
    @classmethod
    def pairs(cls, users, items, ratings, batch_size, seed=0, shuffle=True, drop_last=False, rank=0, world=1,
              negatives=0, observed=None, grouped=False, item_sampler=None):
        """MF / NeuralCF: batches ``(user_idx (B,), item_idx (B,)), rating`` -- rating (N,) or (N, 1) float32.
        ``negatives=k, observed=ObservedPairs(...)`` (every constructor): the samples are positives, and each epoch adds
        k drawn negatives per positive, rating 0; ``grouped=True`` (every constructor) keeps each positive's negatives
        behind it (module docstring)"""
        cols = [("users", users), ("items", items), ("ratings", ratings)]
        return cls("pairs", cols, [users, items], None, None, batch_size, seed, shuffle, drop_last, rank, world,
                   negatives, observed, grouped, item_sampler)

    @classmethod
    def features(cls, assembler, users, items, ratings, batch_size, seed=0, shuffle=True, drop_last=False, rank=0,
                 world=1, negatives=0, observed=None, grouped=False, item_sampler=None):
        """feature models: batches ``(x (B, assembler.width),), rating`` -- x as ``assembler.feature`` builds it (for a
        negative: from the drawn item's row)"""
        return cls("features", [("ratings", ratings)], [users, items], assembler, None, batch_size, seed, shuffle,
                   drop_last, rank, world, negatives, observed, grouped, item_sampler)

    @classmethod
    def sequences(cls, history, users, targets, ratings, batch_size, seed=0, shuffle=True, drop_last=False, rank=0,
                  world=1, negatives=0, observed=None, grouped=False, item_sampler=None):
        """DIN / DIEN: batches ``(hist (B, L), target (B,)), rating`` -- hist row = ``history[users[sample]]``,
        ``history`` one (U, L) int64 row per USER (a negative replaces the target and keeps the row)"""
        cols = [("targets", targets), ("ratings", ratings)]
        return cls("sequences", cols, [users, targets], None, history, batch_size, seed, shuffle, drop_last, rank, world,
                   negatives, observed, grouped, item_sampler)

    # -- batches -----------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self._ranges)

    @property
    def ranges(self):
        """[(first position, count)] of this rank's batches"""
        return list(self._ranges)

    @property
    def num_rank_samples(self):
        return sum(count for _, count in self._ranges)

    def static_batch(self):
        """``(args, rating)`` over the static full-size buffers (what every full batch is written to), or None when
        this rank has no full batch"""
        return None if self._full is None else self._full.batch(self.family)

    def _launch(self, buffers, epoch, first, count, shuffle):
        if self._sampler is not None:
            name = "ctr_load_batch_groups_pop" if self.grouped else "ctr_load_batch_neg_pop"
            rc = getattr(_lib.load(), name)(C.addressof(buffers.desc), C.addressof(self._neg), C.addressof(buffers.pop),
                                            self.seed, epoch, first, count, int(shuffle), _lib.stream_ptr())
            _lib.check(rc, name)
            return
        if self._neg is not None:
            name = "ctr_load_batch_groups" if self.grouped else "ctr_load_batch_neg"
            rc = getattr(_lib.load(), name)(C.addressof(buffers.desc), C.addressof(self._neg), self.seed, epoch, first,
                                            count, int(shuffle), _lib.stream_ptr())
            _lib.check(rc, name)
            return
        rc = _lib.load().ctr_load_batch(C.addressof(buffers.desc), self.seed, epoch, first, count, int(shuffle),
                                        _lib.stream_ptr())
        _lib.check(rc, "ctr_load_batch")

    def epoch(self, epoch: int, shuffle=None):
        """yield ``(args, rating)`` for every batch of this rank; ``shuffle`` overrides the loader's setting (an
        evaluation pass asks for the identity order)"""
        if int(epoch) < 0:
            raise ValueError("DeviceLoader.epoch(): epoch must be non-negative")
        shuffle = self.shuffle if shuffle is None else bool(shuffle)
        for k, (first, count) in enumerate(self._ranges):
            buffers = self._full if k < self._num_full else self._tail
            self._launch(buffers, int(epoch), first, count, shuffle)
            yield buffers.batch(self.family)

    def log_q_of(self, rating: torch.Tensor) -> torch.Tensor:
        """the (rows,) float32 log-q column that belongs to the rating buffer ``rating`` -- what the last batch drawn
        into that buffer set wrote: ``log q(item)`` of every sample, a positive's own item or a negative's drawn one.
        The buffer is told by its storage address and length (a tail of ``batch_size`` samples has buffers of its
        own); any other tensor, or a loader without ``item_sampler``, is a ValueError."""
        if self._sampler is None:
            raise ValueError("DeviceLoader.log_q_of(): the loader was built without item_sampler")
        for buffers in (self._full, self._tail):
            if buffers is not None and torch.is_tensor(rating) and rating.is_cuda:
                own = buffers.cols[-1]
                if rating.data_ptr() == own.data_ptr() and rating.shape[0] == own.shape[0] and rating.numel() == own.numel():
                    return buffers.logq
        raise ValueError("DeviceLoader.log_q_of(): not one of this loader's rating buffers")

    def indices(self, epoch: int, first: int = 0, count=None, shuffle=None) -> torch.Tensor:
        """sample indices of positions [first, first + count) of epoch ``epoch`` (int64, on the device); with negatives
        the index v over the virtual epoch: positive ``v // (1 + k)``, slot ``v % (1 + k)`` (grouped: the slot is the
        position's, the positive its group's)"""
        count = self.num_samples - first if count is None else count
        if epoch < 0 or first < 0 or count < 0 or first + count > self.num_samples:
            raise ValueError("DeviceLoader.indices(): position range outside the epoch")
        shuffle = self.shuffle if shuffle is None else bool(shuffle)
        if self.grouped:
            return self._group_indices(int(epoch), int(first), int(count), shuffle)
        out = torch.empty(count, dtype=torch.int64, device=self.device)
        rc = _lib.load().ctr_loader_indices(self.num_samples, self.seed, int(epoch), int(first), int(count), int(shuffle),
                                            out.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "ctr_loader_indices")
        return out

    def _group_indices(self, epoch, first, count, shuffle):
        """v = perm_N(group) * (1 + k) + slot of positions [first, first + count): the permutation of the groups that
        the range touches by ``ctr_loader_indices`` over N, the rest by torch ops"""
        per = 1 + self.negatives
        pos = torch.arange(first, first + count, dtype=torch.int64, device=self.device)
        if count == 0:
            return pos
        g0, g1 = first // per, (first + count - 1) // per + 1
        order = torch.empty(g1 - g0, dtype=torch.int64, device=self.device)
        rc = _lib.load().ctr_loader_indices(self.num_positives, self.seed, epoch, g0, g1 - g0, int(shuffle),
                                            order.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "ctr_loader_indices")
        group = torch.div(pos, per, rounding_mode="floor")
        return order[group - g0] * per + (pos - group * per)

    def user_ids(self) -> torch.Tensor:
        """(num_samples,) int64 user of every sample of the unshuffled epoch: with ``negatives=k`` sample v has the
        user of positive ``v // (1 + k)``, grouped or not -- what ``evaluator.UserGroups`` is built from"""
        return self._users.repeat_interleave(1 + self.negatives) if self.negatives else self._users

    def check_bad_index(self):
        """raise the IndexError of an id outside its join table seen by any batch since the last call, or the
        RuntimeError of a negative that could not be drawn"""
        if int(self._err.item()):
            self._err.zero_()
            raise IndexError("index out of range in self")
        if self._fail is not None and int(self._fail.item()):
            self._fail.zero_()
            raise RuntimeError("negative sampling: a user has (practically) no item outside the observed pairs")
