"""CPU: the sampled leave-one-out evaluation as restated in group_eval_numpy.py (the GPU tests compare the kernels of
csrc/group_eval.hip with it): properties of the candidate draw, the metrics pinned to the reference's ``Ranking`` on
tests/golden/group_eval/small.npz (dev/make_group_eval_golden.py), the host-side argument checks of the two entry
points through the loaded library, and the batch ranges a LeaveOneOut loader gets."""
import os

import numpy as np
import pytest

import group_eval_numpy as gn
import loader_numpy as ln

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group_eval", "small.npz")
SEEDS = (0, 12345, (1 << 64) - 1)


def _csr(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.array([x for r in rows for x in sorted(r)], dtype=np.int32)
    return indptr, indices


def _observed(num_users, num_items, lo, hi, seed):
    gen = np.random.default_rng(seed)
    return [set(gen.choice(num_items, int(gen.integers(lo, hi + 1)), replace=False).tolist()) for _ in range(num_users)]


@pytest.mark.parametrize("num_items", [1, 2, 3, 4, 5, 16, 17, 64, 65])
def test_group_permutation_is_a_bijection(num_items):
    for seed in SEEDS:
        for s in (0, 1, 77):
            assert sorted(gn.group_perm(seed, s, num_items).tolist()) == list(range(num_items))
    # groups draw from different permutations (from 5 items on two of them differing is certain enough: 1/120 each)
    if num_items >= 16:
        assert gn.group_perm(0, 0, num_items).tolist() != gn.group_perm(0, 1, num_items).tolist()


@pytest.mark.parametrize("num_items,k,row", [(1682, 99, (20, 737)), (40, 9, (0, 25))])
def test_candidates_are_distinct_unobserved_and_not_the_positive(num_items, k, row):
    num_users = 30
    rows = _observed(num_users, num_items, row[0], row[1], 3)
    indptr, indices = _csr(rows)
    gen = np.random.default_rng(4)
    users = gen.integers(0, num_users, 50)
    items = np.array([sorted(rows[u])[0] if rows[u] and s % 2 else int(gen.integers(0, num_items))
                      for s, u in enumerate(users)])          # positives inside and outside the observed set
    cand, err, fail = gn.candidates(users, items, indptr, indices, num_users, num_items, k, 9)
    assert not err and not fail
    assert (cand[:, 0] == items).all()
    for s, u in enumerate(users):
        neg = cand[s, 1:].tolist()
        assert len(set(neg)) == k and min(neg) >= 0 and max(neg) < num_items
        assert items[s] not in neg and not (set(neg) & rows[u])
    # prefix property: the draw with k' < k is the first k' of the draw with k
    for kk in (1, k // 2):
        part, _, _ = gn.candidates(users, items, indptr, indices, num_users, num_items, kk, 9)
        assert (part == cand[:, :1 + kk]).all()
    other, _, _ = gn.candidates(users, items, indptr, indices, num_users, num_items, k, 10)
    assert (other != cand).any()


def test_exact_fit_fills_the_row_and_a_shortfall_writes_minus_one():
    num_items, k = 17, 6
    rows = [set(range(10)), set(range(11)), set()]          # eligible: 17 - 10 - 1 = 6 (positive 16), 5, 16
    indptr, indices = _csr(rows)
    cand, err, fail = gn.candidates([0], [16], indptr, indices, 3, num_items, k, 1)
    assert not err and not fail and sorted(cand[0, 1:].tolist()) == [10, 11, 12, 13, 14, 15]
    cand, err, fail = gn.candidates([0, 1, 2], [16, 16, 3], indptr, indices, 3, num_items, k, 1)
    assert fail and not err
    assert sorted(cand[1, 1:6].tolist()) == [11, 12, 13, 14, 15] and cand[1, 6] == -1
    assert (cand[0] >= 0).all() and (cand[2] >= 0).all()
    # a positive inside the observed row takes nothing from the eligible items: 17 - 11 = 6 fit exactly
    cand, err, fail = gn.candidates([1], [4], indptr, indices, 3, num_items, k, 1)
    assert not fail and sorted(cand[0, 1:].tolist()) == [11, 12, 13, 14, 15, 16]
    # user id out of range: zeros and the error flag; an inconsistent row is read as empty and flagged
    cand, err, fail = gn.candidates([3, -1], [2, 2], indptr, indices, 3, num_items, k, 1)
    assert err and not fail and (cand[:, 1:] == 0).all() and (cand[:, 0] == 2).all()
    bad = indptr.copy()
    bad[1] = 99
    cand, err, fail = gn.candidates([0], [16], bad, indices, 3, num_items, k, 1)
    assert err and not fail and len(set(cand[0, 1:].tolist())) == k


def test_rank_rule_counts_ties_and_nan_against_the_positive():
    nan, inf = np.nan, np.inf
    rows = np.array([[3, 3, 3, 3],          # all equal: rank k
                     [5, 1, 2, 3],          # strictly best: 0
                     [2, 2, 1, 3],          # one tie, one above
                     [nan, 0, 0, 0],        # NaN positive loses to everything
                     [1, nan, 0, 0],        # a NaN negative counts against it
                     [inf, inf, 0, -inf],
                     [-inf, -inf, 0, nan]], dtype=np.float32)
    assert gn.ranks(rows, 3).tolist() == [3, 0, 2, 3, 1, 1, 3]
    assert gn.histogram(gn.ranks(rows, 3), 3).tolist() == [1, 2, 1, 3]


@pytest.mark.parametrize("tag", ["ties", "inf"])
def test_metrics_are_the_references_on_one_item_ground_truths(tag):
    """1e-12 absolute: both sides are float64 sums of a few hundred terms in [0, 1] (observed: 3e-17)"""
    z = np.load(GOLDEN)
    k = int(z["negatives"])
    scores, order = z[f"{tag}_scores"], z[f"{tag}_order"]
    rank = gn.ranks(scores, k)
    # the stored orderings are the pessimistic ones: the positive (slot 0) stands at its rank
    assert (np.argmax(order == 0, axis=1) == rank).all()
    assert len(set(rank.tolist())) > 3 and (rank == k).any() and (rank == 0).any()
    cutoffs = [int(c) for c in z["cutoffs"]]
    assert cutoffs == [1, 3, 10, 20]
    hr, ndcg, mrr_at, mrr = gn.metrics(gn.histogram(rank, k), cutoffs)
    for row, c in zip(z[f"{tag}_recall_ndcg_map"], cutoffs):
        assert abs(hr[c] - row[0]) <= 1e-12
        assert abs(ndcg[c] - row[1]) <= 1e-12
        assert abs(mrr_at[c] - row[2]) <= 1e-12
    assert abs(mrr - float(z[f"{tag}_mrr"])) <= 1e-12


def test_host_metrics_of_the_package_equal_the_restatement():
    from deeplearningrecommendationsystem_amd.evaluator.sampled import metrics_from_histogram
    hist = np.array([5, 0, 3, 1, 0, 0, 7, 2, 0, 0, 11, 4], dtype=np.int64)
    got = metrics_from_histogram(hist, cutoffs=(1, 5, 10, 50))
    hr, ndcg, mrr_at, mrr = gn.metrics(hist, (1, 5, 10, 50))
    assert got.hr == hr and got.ndcg == ndcg and got.mrr_at == mrr_at and got.mrr == mrr
    assert got.groups == 33 and got.histogram.tolist() == hist.tolist()
    assert "HR@10" in got.report() and "MRR" in got.report()


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib.load()


def test_group_rank_argument_validation_without_gpu(handle):
    one = 8   # any non-null address: the checks return before anything is read or launched
    assert handle.ctr_group_rank(one, 10, 4, 0, None, one, None) == -1        # k = 0
    assert handle.ctr_group_rank(one, 5000, 4, 4096, None, one, None) == -1   # k = 4096
    assert handle.ctr_group_rank(one, 9, 4, 9, None, one, None) == -1         # ld < 1 + k
    assert handle.ctr_group_rank(None, 10, 4, 9, None, one, None) == -1       # null scores
    assert handle.ctr_group_rank(one, 10, 4, 9, None, None, None) == -1       # null hist
    assert handle.ctr_group_rank(one, 10, -1, 9, None, one, None) == -1
    assert handle.ctr_group_rank(None, 10, 0, 9, None, None, None) == 0       # N = 0: a no-op


def test_eval_candidates_argument_validation_without_gpu(handle):
    one = 8

    def call(users=one, items=one, n=4, indptr=one, indices=one, nnz=3, nu=5, ni=40, k=9, cand=one, ld=10):
        return handle.ctr_eval_candidates(users, items, n, indptr, indices, nnz, nu, ni, k, 0, cand, ld, None, None, None)

    assert call(k=0) == -1 and call(k=4096, ld=5000) == -1 and call(ld=9) == -1
    assert call(users=None) == -1 and call(items=None) == -1 and call(indptr=None) == -1 and call(cand=None) == -1
    assert call(indices=None) == -1 and call(ni=0) == -1 and call(ni=1 << 31) == -1 and call(nu=0) == -1
    assert call(n=-1) == -1 and call(nnz=-1) == -1
    assert call(n=0, users=None, items=None, indptr=None, indices=None, cand=None) == 0


@pytest.mark.parametrize("groups,k,batch", [(50, 9, 64), (7, 4, 5), (3, 99, 1000)])
def test_leave_one_out_batches_keep_the_groups_contiguous(groups, k, batch):
    """world = 1: the unshuffled batches tile [0, N (1 + k)) in order, so the gathered predictions lie in groups"""
    from deeplearningrecommendationsystem_amd.data.loader import batch_ranges
    n = groups * (1 + k)
    ranges = batch_ranges(n, batch)
    assert ranges == ln.batch_ranges(n, batch)
    at = 0
    for first, count in ranges:
        assert first == at and count >= 1
        at += count
    assert at == n
