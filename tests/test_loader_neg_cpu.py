"""CPU: the drawn negatives of the mini-batch loader as restated in loader_neg_numpy.py (the GPU tests compare the
kernel with that restatement bit for bit), the entry point's argument validation, and the host arithmetic over the
virtual epoch."""
import ctypes

import numpy as np
import pytest
import torch

import loader_neg_numpy as lnn
import loader_numpy as ln

SEED = 20
NUM_USERS, NUM_ITEMS = 12, 40


def _data(n, seed=3):
    """n positives of 12 users over 40 items; observed = the positives plus a dense row for user 5 (30 items)"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, NUM_USERS, size=n)
    items = rng.integers(0, NUM_ITEMS, size=n)
    observed = {}
    for u, i in zip(users, items):
        observed.setdefault(int(u), set()).add(int(i))
    observed.setdefault(5, set()).update(range(30))
    return users, items, observed


@pytest.mark.parametrize("n,k", [(1, 1), (37, 1), (37, 3), (1000, 4)])
def test_an_epoch_is_every_positive_once_and_k_negatives_each(n, k):
    users, _, observed = _data(n)
    m = n * (1 + k)
    for epoch in (0, 1):
        out = lnn.epoch_samples(SEED, epoch, np.arange(m), users, k, NUM_ITEMS, observed, num_users=NUM_USERS)
        assert np.array_equal(np.sort(out["v"]), np.arange(m)), "v is a permutation of [0, M)"
        positive = out["slot"] == 0
        assert np.array_equal(np.sort(out["sample"][positive]), np.arange(n)), "every positive exactly once"
        assert np.array_equal(np.bincount(out["sample"][~positive], minlength=n), np.full(n, k)), "k slots per positive"
        assert (out["item"][positive] == -1).all() and not out["failed"].any() and not out["bad"].any()
        # exclusion: no emitted negative is observed, and every one is an item
        for s, item in zip(out["sample"][~positive], out["item"][~positive]):
            assert 0 <= item < NUM_ITEMS and int(item) not in observed.get(int(users[s]), ())
    flat = lnn.epoch_samples(SEED, 0, np.arange(m), users, k, NUM_ITEMS, observed, shuffle=False)
    assert np.array_equal(flat["sample"], np.repeat(np.arange(n), 1 + k)), "unshuffled: a positive, then its k negatives"
    assert np.array_equal(flat["slot"], np.tile(np.arange(1 + k), n))


def test_a_position_does_not_depend_on_who_else_is_asked():
    n, k = 1000, 4
    users, _, observed = _data(n)
    whole = lnn.epoch_samples(SEED, 2, np.arange(n * (1 + k)), users, k, NUM_ITEMS, observed)
    part = lnn.epoch_samples(SEED, 2, np.arange(250, 500), users, k, NUM_ITEMS, observed)
    for key in whole:
        assert np.array_equal(part[key], whole[key][250:500]), key


def _uniformity_setup(epoch):
    users = np.zeros(100, dtype=np.int64)
    return lnn.epoch_samples(7, epoch, np.arange(500), users, 4, 50, {0: set(range(0, 50, 5))}, shuffle=False)


def test_epochs_draw_different_negatives():
    a, b = _uniformity_setup(0), _uniformity_setup(1)
    negative = a["slot"] != 0
    assert np.array_equal(a["slot"], b["slot"])
    changed = float((a["item"][negative] != b["item"][negative]).mean())
    print("negative slots whose item changes between epochs 0 and 1:", changed)
    assert changed > 0.5


def test_draws_are_uniform_over_the_allowed_items():
    """40 000 draws over 40 allowed items: every count within 5 standard deviations (156) of 1000 and chi-square below
    72.1 (p = 0.001 at 39 degrees of freedom); 1 / 0.8 tries per draw are expected"""
    counts = np.zeros(50, dtype=np.int64)
    tries = total = 0
    for epoch in range(100):
        out = _uniformity_setup(epoch)
        negative = out["slot"] != 0
        counts += np.bincount(out["item"][negative], minlength=50)
        tries += int(out["tries"][negative].sum())
        total += int(negative.sum())
    allowed = np.array([i for i in range(50) if i % 5])
    assert total == 40_000 and counts[::5].sum() == 0 and counts.sum() == total
    chi2 = float(((counts[allowed] - 1000.0) ** 2 / 1000.0).sum())
    print("counts", counts[allowed].min(), "to", counts[allowed].max(), "chi-square", chi2, "tries per draw", tries / total)
    assert np.abs(counts[allowed] - 1000).max() <= 156
    assert chi2 < 72.1
    assert abs(tries / total - 1.25) < 0.02


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def test_neg_struct_matches_the_header(lib):
    from test_loader_cpu import _c_sizeof
    assert ctypes.sizeof(lib.LoaderNeg) == _c_sizeof("ctr_loader_neg_t") == 64


def test_neg_entry_point_validation_without_gpu(lib):
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

    def call(first=0, count=4):
        return h.ctr_load_batch_neg(at, neg, 1, 0, first, count, 1, None)

    valid()
    # an empty batch is a no-op, whatever the pointers are
    assert h.ctr_load_batch_neg(None, None, 1, 0, 0, 0, 1, None) == 0 and call(count=0) == 0
    assert h.ctr_load_batch_neg(at, None, 1, 0, 0, 4, 1, None) == -1       # no negative descriptor
    assert h.ctr_load_batch_neg(None, neg, 1, 0, 0, 4, 1, None) == -1      # no loader descriptor
    assert call(count=-1) == -1
    assert call(first=10, count=4) == -1                                    # M = 12: a range beyond it
    assert h.ctr_load_batch_neg(at, neg, 1, -1, 0, 4, 1, None) == -1       # negative epoch
    # every refusal below is the only thing wrong with an otherwise valid call
    for field, value in (("negatives", 0), ("negatives", -1), ("rating_col", 2), ("rating_col", -1), ("rating_col", 0),
                         ("item_col", 2), ("item_col", -2), ("item_col", 1), ("num_items", 1 << 31), ("num_items", 0),
                         ("num_users", 0), ("users", None), ("indptr", None), ("indices", None)):
        valid()
        setattr(g, field, value)
        assert call() == -1, (field, value)
    valid()
    d.n = (1 << 62) // 3 + 1                                                # n * (1 + k) beyond 2^62
    assert call() == -1
    d.n = 4
    d.ncols = lib.CTR_MAX_FIELDS + 1
    assert call() == -1


@pytest.mark.parametrize("world", [1, 2, 3])
def test_batch_ranges_tile_the_virtual_epoch(world):
    from deeplearningrecommendationsystem_amd.data.loader import batch_ranges
    for n, k, batch in ((37, 1, 128), (65, 3, 64), (1000, 4, 256), (1, 1, 1)):
        m = n * (1 + k)
        covered = np.zeros(m, dtype=np.int64)
        for rank in range(world):
            ranges = batch_ranges(m, batch, False, rank, world)
            assert ranges == ln.batch_ranges(m, batch, False, rank, world)
            for first, count in ranges:
                covered[first:first + count] += 1
        assert (covered == 1).all(), (n, k, batch, world)


def test_observed_pairs_on_the_host():
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    u = torch.tensor([3, 0, 3, 3, 0, 2])
    i = torch.tensor([7, 1, 0, 7, 39, 5])
    obs = ObservedPairs(u, i, 5, 40)
    assert obs.indptr.tolist() == [0, 2, 2, 3, 5, 5] and obs.indices.tolist() == [1, 39, 5, 0, 7]
    assert obs.indptr.dtype == torch.int64 and obs.indices.dtype == torch.int32 and len(obs) == 5
    assert (obs.num_users, obs.num_items) == (5, 40)
    both = ObservedPairs([u, torch.tensor([4, 3])], [i, torch.tensor([2, 7])], 5, 40)          # a union
    assert both.indptr.tolist() == [0, 2, 2, 3, 5, 6] and both.indices.tolist() == [1, 39, 5, 0, 7, 2]
    qu, qi = torch.tensor([0, 0, 1, 3, 3, 4, 4, 5, -1, 0]), torch.tensor([1, 2, 0, 0, 7, 2, 39, 0, 0, 40])
    assert both.contains(qu, qi).tolist() == [True, False, False, True, True, True, False, False, False, False]
    empty = ObservedPairs(u[:0], i[:0], 5, 40)
    assert empty.indptr.tolist() == [0] * 6 and not empty.contains(qu, qi).any()
    for bad_u, bad_i in ((5, 0), (-1, 0), (0, 40), (0, -1)):
        with pytest.raises(IndexError):
            ObservedPairs(torch.tensor([bad_u]), torch.tensor([bad_i]), 5, 40)
    with pytest.raises(ValueError):
        ObservedPairs(u, i, 5, 1 << 31)
    with pytest.raises(ValueError):
        ObservedPairs(u, i[:-1], 5, 40)


def test_device_loader_negatives_validation_without_gpu(lib):
    from deeplearningrecommendationsystem_amd.data import DeviceLoader, ObservedPairs
    u, i, y = torch.arange(6), torch.arange(6), torch.ones(6)
    obs = ObservedPairs(u, i, 6, 6)
    with pytest.raises(ValueError):
        DeviceLoader.pairs(u, i, y, 4, negatives=2)                 # no observed set
    with pytest.raises(ValueError):
        DeviceLoader.pairs(u, i, y, 4, observed=obs)                # an observed set and nothing to draw
    with pytest.raises(ValueError):
        DeviceLoader.pairs(u, i, y, 4, negatives=-1, observed=obs)
    with pytest.raises(lib.CtrHipError):
        DeviceLoader.pairs(u, i, y, 4, negatives=2, observed=obs)   # no CPU fallback
