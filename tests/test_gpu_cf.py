"""GPU: the neighbourhood-CF kernels (csrc/knn_cf.hip) against the numpy restatement tests/cf_numpy.py -- neighbour
lists and similarities bitwise, predictions bitwise, rankings equal -- and against the reference-derived fixtures
tests/golden/cf/*.npz (dev/make_cf_golden.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cf_numpy as cfn
from golden_util import GOLDEN_DIR, assert_same_ranking

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cf():
    from deeplearningrecommendationsystem_amd import cf
    return cf


def _matrix(m):
    u, i = np.nonzero(m)
    return _cf().implicit_matrix(u, i, m.shape[0], m.shape[1])


def _check_model(m, k, users, n):
    cf = _cf()
    mat = _matrix(m)
    for cls, rows, pred in ((cf.UserCF, m, cfn.predict_user), (cf.ItemCF, m.T, cfn.predict_item)):
        model = cls(k).fit(mat)
        nbr, nsim = cfn.neighbors(rows, k)
        np.testing.assert_array_equal(model.neighbors.cpu().numpy(), nbr, err_msg=cls.__name__)
        assert np.array_equal(model.neighbor_sims.cpu().numpy().view(np.uint32), nsim.view(np.uint32)), cls.__name__
        want = pred(m, nbr, nsim, users)
        got = model.predict(users).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), cls.__name__
        np.testing.assert_array_equal(model.recommend(users, n).cpu().numpy(), cfn.recommend(want, n),
                                      err_msg=cls.__name__)


def test_i8_counts_exact_on_asymmetric_rows():
    """rows of distinct, unrelated densities: every intersection count (so every similarity) must come out exact,
    which fails if the i8 operand map pairs A and B bytes of different k"""
    rng = np.random.default_rng(3)
    m = (rng.random((300, 448)) < rng.random((300, 1)) * 0.6).astype(np.uint8)
    x = torch.from_numpy(m.astype(np.int8)).cuda()
    from deeplearningrecommendationsystem_amd import ops
    idx, sim = ops.cf_knn(x, x.sum(1, dtype=torch.int32), 64)
    want_idx, want_sim = cfn.ranking(cfn.similarity(m), 64)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(sim.cpu().numpy().view(np.uint32), want_sim.view(np.uint32))


def test_zipf_slice_against_all_rows():
    rng = np.random.default_rng(11)
    rows, cols = 20000, 5000
    pop = 1.0 / np.arange(1, cols + 1)
    pop = pop[rng.permutation(cols)]
    per_row = rng.integers(1, 120, rows)
    u = np.repeat(np.arange(rows), per_row)
    i = rng.choice(cols, size=u.size, p=pop / pop.sum())
    cf = _cf()
    mat = cf.implicit_matrix(u, i, rows, cols)
    from deeplearningrecommendationsystem_amd import ops
    x = mat.data
    q0, nq = 7 * 1024 + 13, 256
    idx, sim = ops.cf_knn(x, x.sum(1, dtype=torch.int32), 11, q0, nq)
    m = mat.dense()
    want_idx, want_sim = cfn.ranking(cfn.similarity(m[q0:q0 + nq], m), 11)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(sim.cpu().numpy().view(np.uint32), want_sim.view(np.uint32))


def test_edge_cases_small():
    # zero rows and zero items, identical rows (position 0 is not self), items not a multiple of 64
    m = np.zeros((9, 70), dtype=np.uint8)
    m[1, [3, 5, 69]] = 1
    m[2, [3, 5, 69]] = 1          # identical to row 1
    m[4, [0, 3]] = 1
    m[5, :] = 1                   # rated everything: no unrated item
    m[6, :68] = 1                 # two unrated items, fewer than n
    m[7, [5, 60]] = 1
    m[8, [60, 61, 62]] = 1        # rows 0 and 3 stay empty, items 1, 2, ... untouched by most users
    _check_model(m, 3, np.arange(9), 5)
    nbr, _ = cfn.neighbors(m, 3)
    assert nbr[2, 0] == 2         # row 2's position 0 was row 1 (tie at 1.0, lower index)


def test_duplicate_pairs_count_once():
    cf = _cf()
    a = cf.implicit_matrix([0, 0, 0, 1, 1], [2, 2, 3, 3, 3], 3, 5)
    b = cf.implicit_matrix([0, 0, 1], [2, 3, 3], 3, 5)
    assert torch.equal(a.data, b.data)
    assert a.counts.tolist() == [2, 1, 0]


def test_rows_at_most_k():
    m = np.array([[1, 0, 1], [1, 1, 0], [0, 1, 1]], dtype=np.uint8)
    _check_model(m, 5, np.arange(3), 4)   # 3 rows, k + 1 = 6: lists shorter than k, -1 padded
    model = _cf().UserCF(5).fit(_matrix(m))
    assert (model.neighbors.cpu().numpy()[:, 2:] == -1).all()


def test_k_limit():
    cf = _cf()
    rng = np.random.default_rng(5)
    m = (rng.random((150, 100)) < 0.2).astype(np.uint8)
    _check_model(m, 63, np.arange(0, 150, 7), 20)   # k + 1 = 64 accepted
    with pytest.raises(ValueError, match="64"):
        cf.UserCF(64)
    from deeplearningrecommendationsystem_amd import ops
    x = _matrix(m).data
    with pytest.raises(ValueError, match="64"):
        ops.cf_knn(x, x.sum(1, dtype=torch.int32), 65)


def test_empty_user_batch():
    cf = _cf()
    m = np.eye(4, 6, dtype=np.uint8)
    for cls in (cf.UserCF, cf.ItemCF):
        model = cls(2).fit(_matrix(m))
        assert model.predict([]).shape == (0, 6)
        assert model.recommend([], 3).shape == (0, 3)


def test_random_against_restatement():
    rng = np.random.default_rng(17)
    m = (rng.random((333, 517)) < rng.random((1, 517)) * 0.15).astype(np.uint8)
    _check_model(m, 10, np.arange(333), 20)


def test_score_chunks_stitch(monkeypatch):
    """predict() / recommend() over several user chunks give the single-chunk answer"""
    from deeplearningrecommendationsystem_amd import topn
    cf = _cf()
    rng = np.random.default_rng(23)
    m = (rng.random((97, 150)) < 0.1).astype(np.uint8)
    users = rng.permutation(97)[:61]
    for cls in (cf.UserCF, cf.ItemCF):
        model = cls(6).fit(_matrix(m))
        want_p = model.predict(users).cpu().numpy()
        want_r = model.recommend(users, 12).cpu().numpy()
        monkeypatch.setattr(topn, "MAX_ROWS", 7)
        monkeypatch.setattr(topn, "SCORE_CHUNK_FLOATS", 150 * 5)   # 5 users per recommend() chunk
        got_p = model.predict(users).cpu().numpy()
        got_r = model.recommend(users, 12).cpu().numpy()
        monkeypatch.undo()
        assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), cls.__name__
        np.testing.assert_array_equal(got_r, want_r, err_msg=cls.__name__)
        np.testing.assert_array_equal(want_r, cfn.recommend(want_p, 12), err_msg=cls.__name__)


@pytest.mark.parametrize("num_items,batch", [(4500, 37), (40000, 30)])
def test_itemcf_scores_item_blocks_and_user_groups(num_items, batch):
    """several 2048-item blocks, a last user group smaller than the rest, and (40 000 items: 5 000-byte bitmaps)
    groups of fewer than 16 users -- against the restatement on a random neighbour table with -1 entries"""
    from deeplearningrecommendationsystem_amd import ops
    rng = np.random.default_rng(num_items)
    num_users, k = 45, 5
    m = (rng.random((num_users, num_items)) < 0.02).astype(np.uint8)
    nbr = rng.integers(0, num_items, (num_items, k)).astype(np.int64)
    nbr[rng.random((num_items, k)) < 0.1] = -1
    nsim = rng.random((num_items, k)).astype(np.float32)
    nsim[nbr < 0] = 0
    users = rng.integers(0, num_users, batch)
    x = _matrix(m).data
    got = ops.itemcf_scores(x, num_items, torch.from_numpy(nbr).cuda(), torch.from_numpy(nsim).cuda(),
                            torch.from_numpy(users).cuda()).cpu().numpy()
    want = cfn.predict_item(m, nbr, nsim, users)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _fixture(name):
    return np.load(os.path.join(GOLDEN_DIR, "cf", name), allow_pickle=False)


@pytest.mark.parametrize("name,cls_name", [("usercf.npz", "UserCF"), ("itemcf.npz", "ItemCF")])
def test_fixture_b(name, cls_name):
    z = _fixture(name)
    nu, ni = int(z["num_users"]), int(z["num_items"])
    m = np.unpackbits(z["bitmap"])[:nu * ni].reshape(nu, ni)
    k, n = int(z["k"]), int(z["n"])
    cf = _cf()
    model = getattr(cf, cls_name)(k).fit(_matrix(m))
    rows = m if cls_name == "UserCF" else m.T
    nbr, nsim = cfn.neighbors(rows, k)
    np.testing.assert_array_equal(model.neighbors.cpu().numpy(), z["b_neighbors"])
    assert np.array_equal(model.neighbor_sims.cpu().numpy().view(np.uint32), nsim.view(np.uint32))
    users = z["users"]
    recs = model.recommend(users, n).cpu().numpy()
    scores = model.predict(users).cpu().numpy()
    assert_same_ranking(recs, z["b_recs"], scores, tol=1e-6)
    full = np.full((nu, n), -1, dtype=np.int64)
    full[users] = recs
    got = cf.recall_precision_f1(full, z["test_users"], z["test_items"], users=users, divisor=int(z["divisor"]))
    np.testing.assert_allclose(got, z["b_metrics"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("script", ["usercf.py", "itemcf.py"])
def test_scripts_run(script):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    last = out.stdout.strip().splitlines()[-1]
    assert "recall" in last and "precision" in last and "F1" in last, last
