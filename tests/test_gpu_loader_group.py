"""Grouped epochs of the device loader (ctr_load_batch_groups; data/loader.py ``grouped=True``).

Reference: loader_group_numpy.epoch_samples, a numpy restatement of the definition in the header comment of
csrc/loader.hip, and plain host indexing with what it returns (test_gpu_loader_neg's helpers and data: twelve users
whose observed rows reach the search's edges).  The loader draws integers and copies, so every comparison is
bit-equality."""
import functools

import numpy as np
import pytest
import torch

import loader_group_numpy as lgn
import loader_numpy as ln
import test_gpu_loader_neg as base

pytestmark = pytest.mark.gpu
DEV, SEED, NU, NI = base.DEV, base.SEED, base.NU, base.NI


@functools.lru_cache(maxsize=None)
def _restated(n, k, epoch, shuffle):
    """the whole grouped epoch of the standard data, computed once for all families and tests; read-only"""
    return lgn.epoch_samples(SEED, epoch, np.arange(n * (1 + k)), base._sources(n)["users"].numpy(), k, NI, base.OBSERVED,
                             shuffle=shuffle, num_users=NU)


def _group_ranges(n, k, batch, drop_last=False, rank=0, world=1):
    per = 1 + k
    return [(first * per, count * per) for first, count in ln.batch_ranges(n, batch // per, drop_last, rank, world)]


# (N, groups per batch).  With 1 + k = 5 a batch of 13 groups is 65 positions and one of 77 groups 385: every launch but
# the first starts inside a 64-position tile of the epoch, and the tiles of a launch cut groups (5 does not divide 64).
#   N = 1: the tail buffers alone;  N = 13: two full batches and a tail of three groups;  N = 1000: 12 full batches of
#   seven tiles (the last one partial) and a tail of 76 groups
SHAPES = [(1, 3), (13, 5), (1000, 77)]


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n,per_batch", SHAPES)
@pytest.mark.parametrize("family", ["pairs", "features", "sequences"])
def test_every_batch_is_bit_equal_to_the_restatement(family, n, per_batch, k):
    src = base._sources(n)
    per = 1 + k
    m, batch = n * per, per_batch * per
    for shuffle in (True, False):
        loader = base._loader(family, src, batch, k, shuffle=shuffle, grouped=True)
        assert loader.grouped and (loader.num_positives, loader.num_samples, loader.negatives) == (n, m, k)
        assert loader.ranges == _group_ranges(n, k, batch) and loader.num_rank_samples == m
        assert all(first % per == 0 and count % per == 0 for first, count in loader.ranges)
        if n == 1000:
            assert any(first % 64 for first, _ in loader.ranges) and batch % 64
        for epoch in (0, 3):
            out = _restated(n, k, epoch, shuffle)
            assert not out["failed"].any()
            base._assert_epoch(loader, family, src, out, epoch)
            for _, rating in loader.epoch(epoch):         # the shape a group loss reads: the positive first
                assert (rating.view(-1, per)[:, 0] > 0).all() and (rating.view(-1, per)[:, 1:] == 0).all()
            assert np.array_equal(loader.indices(epoch).cpu().numpy(), out["v"])
            lo, cnt = min(7, m - 1), min(11, m - min(7, m - 1))          # a range that starts and ends inside groups
            assert np.array_equal(loader.indices(epoch, lo, cnt).cpu().numpy(), out["v"][lo:lo + cnt])
            assert loader.indices(epoch, lo, 0).numel() == 0
        loader.check_bad_index()
        if loader._full is not None and loader._tail is not None:      # the full and tail buffer sets are distinct
            full, tail = loader._full.batch(family), loader._tail.batch(family)
            assert full[1].data_ptr() != tail[1].data_ptr()
            assert all(a.data_ptr() != b.data_ptr() for a, b in zip(full[0], tail[0]))
            assert full[1].shape[0] == batch and tail[1].shape[0] == loader.ranges[-1][1]
    # the loader's setting can be overridden per pass (what an evaluation pass does)
    base._assert_epoch(loader, family, src, _restated(n, k, 0, True), 0, shuffle=True)


@pytest.mark.parametrize("family", ["pairs", "features", "sequences"])
def test_unshuffled_equals_the_ungrouped_loader_and_shuffled_emits_the_same_samples(family):
    n, k, batch = 1000, 4, 385
    src = base._sources(n)
    grouped = base._loader(family, src, batch, k, grouped=True)
    flat = base._loader(family, src, batch, k)
    assert grouped.ranges == flat.ranges
    for (args, rating), (args0, rating0) in zip(grouped.epoch(1, shuffle=False), flat.epoch(1, shuffle=False)):
        assert torch.equal(rating, rating0) and all(torch.equal(a, b) for a, b in zip(args, args0))

    def emitted(loader, epoch):
        rows = []
        for args, rating in loader.epoch(epoch):
            rows.append(torch.cat([a.reshape(a.shape[0], -1).double() for a in args] + [rating.double()], 1).cpu())
        rows = torch.cat(rows)
        return rows[np.lexsort(rows.numpy().T[::-1])]

    a, b = emitted(grouped, 2), emitted(flat, 2)
    assert a.shape == b.shape == (n * (1 + k), a.shape[1]) and torch.equal(a, b)      # one multiset of samples


def test_ranks_partition_one_grouped_epoch():
    n, k, batch, world = 1000, 4, 320, 3
    src = base._sources(n)
    out = _restated(n, k, 2, True)
    covered = np.zeros(n * (1 + k), dtype=np.int64)
    for rank in range(world):
        loader = base._loader("pairs", src, batch, k, rank=rank, world=world, grouped=True)
        assert loader.ranges == _group_ranges(n, k, batch, False, rank, world)
        base._assert_epoch(loader, "pairs", src, out, 2)      # the same positions of the world = 1 epoch
        for first, count in loader.ranges:
            assert first % (1 + k) == 0 and count % (1 + k) == 0
            covered[first:first + count] += 1
    assert (covered == 1).all()


def test_an_exhausted_user_raises_and_the_flag_clears():
    """the existing flag, not a fault: user 5 has observed every item, the last draw is written and the flag raised"""
    n, k = 8, 1
    users = torch.tensor([0, 1, 5, 2, 3, 5, 4, 6])
    src = dict(users=users, items=torch.arange(n), y=torch.ones(n, 1))
    rows = dict(base.OBSERVED)
    rows[5] = set(range(NI))
    loader = base._loader("pairs", src, 16, k, observed=base._observed(rows), grouped=True)
    out = lgn.epoch_samples(SEED, 0, np.arange(n * (1 + k)), users.numpy(), k, NI, rows, num_users=NU)
    assert out["failed"].sum() == 2
    base._assert_epoch(loader, "pairs", src, out, 0)
    with pytest.raises(RuntimeError, match="negative sampling"):
        loader.check_bad_index()
    loader.check_bad_index()                              # the flag was cleared
