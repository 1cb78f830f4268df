"""CPU: the grouped epochs of the mini-batch loader as restated in loader_group_numpy.py (the GPU tests compare the
kernel with that restatement bit for bit): the three properties that follow from the definition, the host arithmetic
over groups, and the entry point's and the constructor's argument validation."""
import ctypes

import numpy as np
import pytest
import torch

import loader_group_numpy as lgn
import loader_neg_numpy as lnn
import loader_numpy as ln

SEED = 20
NUM_USERS, NUM_ITEMS = 12, 40


def _data(n, seed=3):
    """n positives of 12 users over 40 items; observed = the positives plus a dense row for user 5 (30 items)"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, NUM_USERS, size=n)
    observed = {}
    for u, i in zip(users, rng.integers(0, NUM_ITEMS, size=n)):
        observed.setdefault(int(u), set()).add(int(i))
    observed.setdefault(5, set()).update(range(30))
    return users, observed


@pytest.mark.parametrize("n", [1, 2, 5, 63, 64, 65, 1000])
def test_the_order_of_groups_is_a_bijection(n):
    for k in (1, 4):
        per = 1 + k
        for epoch in (0, 3):
            v = lgn.group_index(SEED, epoch, np.arange(n * per), n, k)
            assert np.array_equal(v % per, np.tile(np.arange(per), n)), "a position keeps its slot: positive first"
            groups = (v // per).reshape(n, per)
            assert (groups == groups[:, :1]).all(), "the positions of a group read one positive"
            assert np.array_equal(np.sort(groups[:, 0]), np.arange(n)), "every positive heads exactly one group"
            assert np.array_equal(groups[:, 0], ln.perm(SEED, epoch, np.arange(n), n)), "the permutation over N"
    if n >= 63:
        a, b = (lgn.group_index(SEED, e, np.arange(n * 2), n, 1) for e in (0, 1))
        assert (a != b).mean() > 0.5, "epochs differ"


@pytest.mark.parametrize("n,k", [(1, 1), (37, 1), (65, 3), (1000, 4)])
def test_unshuffled_is_the_ungrouped_loader(n, k):
    users, observed = _data(n)
    m = n * (1 + k)
    for epoch in (0, 3):
        want = lnn.epoch_samples(SEED, epoch, np.arange(m), users, k, NUM_ITEMS, observed, shuffle=False, num_users=NUM_USERS)
        got = lgn.epoch_samples(SEED, epoch, np.arange(m), users, k, NUM_ITEMS, observed, shuffle=False, num_users=NUM_USERS)
        for key in want:
            assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_an_epoch_emits_the_samples_of_the_ungrouped_epoch(n, k):
    users, observed = _data(n)
    m = n * (1 + k)
    for epoch in (0, 2):
        flat = lnn.epoch_samples(SEED, epoch, np.arange(m), users, k, NUM_ITEMS, observed, num_users=NUM_USERS)
        grouped = lgn.epoch_samples(SEED, epoch, np.arange(m), users, k, NUM_ITEMS, observed, num_users=NUM_USERS)
        a, b = np.argsort(flat["v"]), np.argsort(grouped["v"])
        assert np.array_equal(flat["v"][a], np.arange(m)) and np.array_equal(grouped["v"][b], np.arange(m))
        for key in ("sample", "slot", "item", "tries", "failed", "bad"):
            assert np.array_equal(flat[key][a], grouped[key][b]), key      # the draw depends on (seed, e, v) only
        if n >= 65:
            assert not np.array_equal(flat["v"], grouped["v"])


def test_a_position_does_not_depend_on_who_else_is_asked():
    n, k = 1000, 4
    users, observed = _data(n)
    whole = lgn.epoch_samples(SEED, 2, np.arange(n * (1 + k)), users, k, NUM_ITEMS, observed)
    part = lgn.epoch_samples(SEED, 2, np.arange(253, 500), users, k, NUM_ITEMS, observed)      # starts inside a group
    for key in whole:
        assert np.array_equal(part[key], whole[key][253:500]), key


def _group_ranges(n, k, batch, drop_last, rank, world):
    """the rule of data/loader.py's docstring: the ranges of n groups in batches of batch // (1 + k), scaled"""
    per = 1 + k
    return [(first * per, count * per) for first, count in ln.batch_ranges(n, batch // per, drop_last, rank, world)]


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_batch_ranges_in_groups_never_cut_a_group(world, drop_last):
    from deeplearningrecommendationsystem_amd.data.loader import batch_ranges
    for n, k, batch in ((37, 1, 128), (65, 3, 64), (1000, 4, 320), (1, 1, 2), (13, 4, 5), (64, 4, 320)):
        per = 1 + k
        covered = np.zeros(n * per, dtype=np.int64)
        fulls = {len(batch_ranges(n, batch // per, True, rank, world)) for rank in range(world)}
        for rank in range(world):
            groups = batch_ranges(n, batch // per, drop_last, rank, world)
            ranges = [(first * per, count * per) for first, count in groups]
            assert ranges == _group_ranges(n, k, batch, drop_last, rank, world)
            for first, count in ranges:
                assert first % per == 0 and count % per == 0 and 0 < count <= batch, (n, k, batch, rank)
                covered[first:first + count] += 1
        assert len(fulls) == 1, "every rank runs the same number of full steps"
        assert covered.max() <= 1
        if not drop_last:
            assert (covered == 1).all(), (n, k, batch, world)
        else:
            assert covered.sum() == (n // (batch // per)) // world * world * batch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def test_groups_entry_point_validation_without_gpu(lib):
    h = lib.load()
    d, g = lib.Loader(), lib.LoaderNeg()
    at, neg = ctypes.addressof(d), ctypes.addressof(g)
    keep = [(ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)(), (ctypes.c_float * 4)(), (ctypes.c_float * 4)(),
            (ctypes.c_int64 * 3)(), (ctypes.c_int32 * 4)()]
    d.n, d.ncols = 4, 2
    for col, src, dst, size in ((d.cols[0], keep[0], keep[1], 8), (d.cols[1], keep[2], keep[3], 4)):
        col.src, col.dst = ctypes.addressof(src), ctypes.addressof(dst)
        col.lds = col.ldd = col.width = 1
        col.elem_bytes = size

    def valid():
        g.negatives, g.item_col, g.rating_col = 2, 0, 1
        g.users, g.indptr, g.indices = ctypes.addressof(keep[0]), ctypes.addressof(keep[4]), ctypes.addressof(keep[5])
        g.num_users, g.num_items = 2, 40

    def call(first=0, count=3):
        return h.ctr_load_batch_groups(at, neg, 1, 0, first, count, 1, None)

    valid()
    # an empty batch is a no-op, whatever the pointers are
    assert h.ctr_load_batch_groups(None, None, 1, 0, 0, 0, 1, None) == 0 and call(count=0) == 0
    assert h.ctr_load_batch_groups(at, None, 1, 0, 0, 3, 1, None) == -1       # no negative descriptor
    assert h.ctr_load_batch_groups(None, neg, 1, 0, 0, 3, 1, None) == -1      # no loader descriptor
    assert h.ctr_load_batch_groups(None, None, 1, 0, 0, 3, 1, None) == -1
    assert call(count=-1) == -1
    assert call(first=10, count=3) == -1                                       # M = 12: a range beyond it
    assert h.ctr_load_batch_groups(at, neg, 1, -1, 0, 3, 1, None) == -1       # negative epoch
    # every refusal below is the only thing wrong with an otherwise valid call
    for field, value in (("negatives", 0), ("negatives", -1), ("rating_col", 2), ("rating_col", 0), ("item_col", 1),
                         ("num_items", 1 << 31), ("num_items", 0), ("num_users", 0), ("users", None), ("indptr", None),
                         ("indices", None)):
        valid()
        setattr(g, field, value)
        assert call() == -1, (field, value)
    valid()
    d.n = (1 << 62) // 3 + 1                                                   # n * (1 + k) beyond 2^62
    assert call() == -1


def test_device_loader_grouped_validation_without_gpu(lib):
    from deeplearningrecommendationsystem_amd.data import DeviceLoader, ObservedPairs
    u, i, y = torch.arange(6), torch.arange(6), torch.ones(6)
    obs = ObservedPairs(u, i, 6, 6)
    with pytest.raises(ValueError, match="grouped"):
        DeviceLoader.pairs(u, i, y, 4, grouped=True)                                   # negatives = 0
    with pytest.raises(ValueError, match="grouped"):
        DeviceLoader.pairs(u, i, y, 4, negatives=2, observed=obs, grouped=True)        # 4 % 3
    with pytest.raises(ValueError, match="grouped"):
        DeviceLoader.sequences(torch.zeros(6, 3, dtype=torch.int64), u, i, y, 7, negatives=1, observed=obs, grouped=True)
    with pytest.raises(lib.CtrHipError):
        DeviceLoader.pairs(u, i, y, 6, negatives=2, observed=obs, grouped=True)        # valid, but no CPU fallback
