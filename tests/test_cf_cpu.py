"""CPU: the numpy restatement of the neighbourhood-CF semantics (tests/cf_numpy.py) against the fixtures made from
the reference's UserCF_Final.py / ItemCF_Final.py (dev/make_cf_golden.py), and the C-ABI refusals of the CF entry
points, which need no GPU."""
import ctypes
import os

import numpy as np
import pytest

import cf_numpy as cfn
from golden_util import GOLDEN_DIR, assert_same_ranking

FIXTURES = [("usercf.npz", "user"), ("itemcf.npz", "item")]


def _load(name):
    z = np.load(os.path.join(GOLDEN_DIR, "cf", name), allow_pickle=False)
    nu, ni = int(z["num_users"]), int(z["num_items"])
    m = np.unpackbits(z["bitmap"])[:nu * ni].reshape(nu, ni)
    return z, m


def _model(m, kind, k, users):
    rows = m if kind == "user" else m.T
    nbr, nsim = cfn.neighbors(rows, k)
    pred = (cfn.predict_user if kind == "user" else cfn.predict_item)(m, nbr, nsim, users)
    return nbr, nsim, pred


@pytest.mark.parametrize("name,kind", FIXTURES)
def test_similarity_matches_sklearn(name, kind):
    z, m = _load(name)
    rows = m if kind == "user" else m.T
    got = cfn.similarity(rows[z["sim_rows"]], rows)
    np.testing.assert_allclose(got, z["sim_sample"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("name,kind", FIXTURES)
def test_restatement_reproduces_fixture_b(name, kind):
    z, m = _load(name)
    users = z["users"]
    nbr, _, pred = _model(m, kind, int(z["k"]), users)
    np.testing.assert_array_equal(nbr, z["b_neighbors"])
    recs = cfn.recommend(pred, int(z["n"]))
    assert_same_ranking(recs, z["b_recs"], pred, tol=1e-6)
    # the reference's float64 predictions of its list, against ours of the same items
    np.testing.assert_allclose(np.take_along_axis(pred, z["b_recs"].astype(np.int64), 1), z["b_preds"], rtol=1e-6)
    full = np.full((m.shape[0], recs.shape[1]), -1, dtype=np.int64)
    full[users] = recs
    got = cfn.metrics(full, z["test_users"], z["test_items"], users, int(z["divisor"]))
    np.testing.assert_allclose(got, z["b_metrics"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("name,kind", FIXTURES)
def test_restatement_agrees_with_fixture_a_where_unambiguous(name, kind):
    """with sklearn's float64 similarity the reference may order float32-tied neighbours differently.  UserCF: where
    a user's neighbour set equals ours, the whole list must agree (up to prediction ties).  ItemCF: a prediction
    depends on its item's neighbour set only, so with the items whose set differs taken out of both lists, the
    reference's remaining items must be the head of our ranking of the unaffected items."""
    z, m = _load(name)
    users = z["users"]
    nbr, _, pred = _model(m, kind, int(z["k"]), users)
    same = np.array([set(a) == set(b) for a, b in zip(nbr.tolist(), z["a_neighbors"].tolist())])
    assert same.mean() > 0.5
    n = int(z["n"])
    if kind == "user":
        sel = np.flatnonzero(same[users])
        assert sel.size > 0.5 * len(users)
        recs = cfn.recommend(pred, n)
        assert_same_ranking(recs[sel], z["a_recs"][sel], pred[sel], tol=1e-6)
        return
    ambiguous = np.flatnonzero(~same)
    assert 0 < ambiguous.size < 0.1 * same.size
    masked = pred.copy()
    masked[:, ambiguous] = -np.inf
    ours = cfn.recommend(masked, n)
    compared = 0
    for r in range(len(users)):
        want = [int(i) for i in z["a_recs"][r] if i >= 0 and i not in set(ambiguous.tolist())]
        got = ours[r, :len(want)]
        assert_same_ranking(got[None, :], np.array([want]), masked[r:r + 1], tol=1e-6)
        compared += len(want) > 0
    assert compared == len(users)


def test_library_metric_matches_restatement():
    from deeplearningrecommendationsystem_amd.cf import recall_precision_f1
    z, m = _load("itemcf.npz")
    recs = np.full((m.shape[0], 20), -1, dtype=np.int64)
    recs[z["users"]] = z["b_recs"]
    recs[3] = -1   # an empty list: precision 0 instead of the reference's division by zero
    got = recall_precision_f1(recs, z["test_users"], z["test_items"], users=z["users"], divisor=int(z["divisor"]))
    want = cfn.metrics(recs, z["test_users"], z["test_items"], z["users"], int(z["divisor"]))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    r, p, f = recall_precision_f1(np.array([[1, 2, -1]]), [0], [2])
    assert (r, p) == (1.0, 0.5) and abs(f - 2 / 3) < 1e-12


def test_synthetic_split_shape():
    from deeplearningrecommendationsystem_amd import synth
    tu, ti, su, si = synth.implicit_split(120, 90, 1500, 4, seed=2)
    assert len(tu) == 1500 and len(su) == 120 * 4
    m = cfn.dense(tu, ti, 120, 90)
    assert m.sum() == 1500 and m.any(1).all() and m.any(0).all()
    assert not cfn.dense(su, si, 120, 90)[m != 0].any()
    assert (np.bincount(su.numpy(), minlength=120) == 4).all()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib.load()


def test_cf_entry_points_refuse_bad_arguments(lib):
    EINVAL, ELIMIT, EALIGN = -1, -2, -4
    p = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4097)
    knn = lib.ctr_cf_knn
    assert knn(None, 10, 64, p, 0, 10, 11, p, p, None) == EINVAL
    assert knn(p, 10, 64, None, 0, 10, 11, p, p, None) == EINVAL
    assert knn(p, 10, 64, p, 0, 10, 11, None, p, None) == EINVAL
    assert knn(p, 10, 64, p, 0, 10, 11, p, None, None) == EINVAL
    assert knn(p, 10, 96, p, 0, 10, 11, p, p, None) == EINVAL      # cols_pad not a multiple of 64
    assert knn(p, 0, 64, p, 0, 0, 11, p, p, None) == EINVAL
    assert knn(p, 10, 64, p, 5, 6, 11, p, p, None) == EINVAL       # query rows past the end
    assert knn(p, 10, 64, p, -1, 2, 11, p, p, None) == EINVAL
    assert knn(p, 10, 64, p, 0, 10, 0, p, p, None) == EINVAL
    assert knn(p, 10, 64, p, 0, 10, 65, p, p, None) == ELIMIT
    assert knn(odd, 10, 64, p, 0, 10, 11, p, p, None) == EALIGN
    assert knn(None, 10, 64, None, 0, 0, 11, None, None, None) == 0   # nothing to do
    for fn in (lib.ctr_usercf_scores, lib.ctr_itemcf_scores):
        assert fn(None, 5, 64, 10, p, p, 3, p, 2, p, 10, None) == EINVAL
        assert fn(p, 5, 64, 10, None, p, 3, p, 2, p, 10, None) == EINVAL
        assert fn(p, 5, 64, 10, p, p, 3, None, 2, p, 10, None) == EINVAL
        assert fn(p, 5, 64, 10, p, p, 3, p, 2, None, 10, None) == EINVAL
        assert fn(p, 5, 64, 70, p, p, 3, p, 2, p, 70, None) == EINVAL     # more items than the padded row
        assert fn(p, 5, 64, 10, p, p, 3, p, 2, p, 9, None) == EINVAL      # ldo < num_items
        assert fn(p, 5, 64, 10, p, p, -1, p, 2, p, 10, None) == EINVAL
        assert fn(p, 5, 64, 10, p, p, 65, p, 2, p, 10, None) == ELIMIT
        assert fn(odd, 5, 64, 10, p, p, 3, p, 2, p, 10, None) == EALIGN
        assert fn(None, 5, 64, 10, None, None, 3, None, 0, None, 10, None) == 0   # empty batch


def test_python_refuses_k_above_limit():
    from deeplearningrecommendationsystem_amd import cf, ops
    assert ops.CF_KNN_MAX_K == 64
    with pytest.raises(ValueError, match="64"):
        cf.UserCF(64)
    with pytest.raises(ValueError, match="64"):
        cf.ItemCF(100)
    cf.UserCF(63)
