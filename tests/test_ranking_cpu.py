"""CPU: the numpy restatement of the ranking evaluation (tests/ranking_numpy.py) against the fixtures made from the
reference's evaluator/ranking.py and data/reader.py (dev/make_ranking_golden.py), the import of the mirror without a
GPU, and the C-ABI refusals of the ranking entry points."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ranking_numpy as rn
from golden_util import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _z(name):
    return np.load(os.path.join(GOLDEN_DIR, "ranking", name + ".npz"), allow_pickle=False)


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(np.asarray(a).astype(np.int64)).tobytes()).digest(),
                         dtype=np.uint8)


def _check(parts, metrics, z, tag, k):
    want = z[f"{tag}_k{k}_metrics"]
    assert list(metrics[:3]) == want[:3].tolist()
    np.testing.assert_allclose(metrics, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(parts[:, 3], z[f"{tag}_k{k}_ap"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(parts[:, 6], z[f"{tag}_k{k}_rr"])
    nd = [d / i if i > 0 else 0 for d, i in zip(parts[:, 4], parts[:, 5])]
    np.testing.assert_allclose(nd, z[f"{tag}_k{k}_ndcg"], rtol=1e-12, atol=0)


def test_restatement_reproduces_ml100k_fixture():
    z = _z("ml100k")
    nu, ni = int(z["num_users"]), int(z["num_items"])
    tu, ti = np.nonzero(np.unpackbits(z["bitmap"])[:nu * ni].reshape(nu, ni))
    train_real = rn.itemid_matrix(tu, ti)
    valid_real = rn.itemid_matrix(z["valid_users"], z["valid_items"])
    test_real = rn.itemid_matrix(z["test_users"], z["test_items"])
    for name, a in (("train_real", train_real), ("valid_real", valid_real), ("test_real", test_real)):
        assert np.array_equal(_sha(a), z[name + "_sha"]) and list(a.shape) == z[name + "_shape"].tolist(), name
    scores = (z["emb_user"].astype(np.int32) @ z["emb_item"].astype(np.int32).T).astype(np.float32)
    roc = rn.full_ranking(scores)
    assert np.array_equal(_sha(roc), z["roc_sha"])
    first = rn.remove_itemid(roc, train_real)
    assert np.array_equal(_sha(first), z["valid_roc1_sha"])
    valid_roc, test_roc = rn.remove_itemid(first, test_real), rn.remove_itemid(first, valid_real)
    for name, a in (("valid_roc", valid_roc), ("test_roc", test_roc)):
        assert np.array_equal(_sha(a), z[name + "_sha"]) and list(a.shape) == z[name + "_shape"].tolist(), name
        assert str(a.dtype) == bytes(z[name + "_dtype"]).decode()
    for k in (10, 50):
        for tag, real, rec in (("valid", valid_real, valid_roc), ("test", test_real, test_roc)):
            _check(rn.partials(real, rec, k), rn.metrics(real, rec, k), z, tag, k)


def test_restatement_reproduces_small_fixture():
    z = _z("small")
    np.testing.assert_array_equal(rn.full_ranking(z["scores"]), z["roc"])
    f1 = rn.remove_itemid(z["roc"], z["ex1"])
    np.testing.assert_array_equal(f1, z["filtered1"])
    f2 = rn.remove_itemid(f1, z["ex2"])
    np.testing.assert_array_equal(f2, z["filtered2"])
    assert f2.dtype == z["filtered2"].dtype
    assert (f2 == -1).sum(1).max() > 0 and ((f2 >= 0).sum(1) < 10).any()   # pads fall inside p[:k]
    off, ids = z["act_off"], z["act_ids"]
    ragged = [ids[off[u]:off[u + 1]].tolist() for u in range(len(off) - 1)]
    for k in (10, 50):
        _check(rn.partials(ragged, f2, k), rn.metrics(ragged, f2, k), z, "ragged", k)
        _check(rn.partials(z["actual_padded"], f2, k), rn.metrics(z["actual_padded"], f2, k), z, "padded", k)
    np.testing.assert_array_equal(rn.itemid_matrix(z["frame_users"], z["frame_items"]), z["itemid"])
    with pytest.raises(ZeroDivisionError):
        rn.metrics([[1, 2], []], [[1, 3], [4]], 2)      # an empty actual row: apk divides by len(a) = 0
    with pytest.raises(ZeroDivisionError):
        rn.metrics([[1, 2]], [[3, 4]], 2)               # P + R = 0


def test_library_itemid_matrix_matches_fixture():
    """itemid_matrix is host code in the library: frames and pairs give the reference's array"""
    import pandas as pd
    from deeplearningrecommendationsystem_amd.evaluator.ranking import itemid_matrix
    z = _z("small")
    u, i = z["frame_users"], z["frame_items"]
    for data in (pd.DataFrame({"user_id": u, "item_id": i}), (u, i)):
        got = itemid_matrix(data)
        np.testing.assert_array_equal(got, z["itemid"])
        assert got.dtype == z["itemid"].dtype


def test_compat_import_resolves_to_mirror_without_gpu():
    code = ("import evaluator.ranking as r, torch; from evaluator.ranking import Ranking; "
            "print(Ranking.__module__, torch.cuda.is_available())")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "compat"), HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[0] == "deeplearningrecommendationsystem_amd.evaluator.ranking"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib.load()


def test_rank_entry_points_refuse_bad_arguments(lib):
    EINVAL, ELIMIT = -1, -2
    p = ctypes.c_void_p(4096)
    filt = lib.ctr_rank_filter
    assert filt(p, 10, -1, 10, p, p, 3, p, 10, p, p, None) == EINVAL
    assert filt(p, 9, 4, 10, p, p, 3, p, 10, p, p, None) == EINVAL          # ld_rec < len
    assert filt(p, 10, 4, 10, p, p, 3, p, 9, p, p, None) == EINVAL          # ld_out < len
    assert filt(p, 10, 4, 10, None, p, 3, p, 10, p, p, None) == EINVAL
    assert filt(p, 10, 4, 10, p, None, 3, p, 10, p, p, None) == EINVAL      # nnz > 0 without ids
    assert filt(None, 10, 4, 10, p, p, 3, p, 10, p, p, None) == EINVAL
    assert filt(p, 10, 4, 10, p, p, -3, p, 10, p, p, None) == EINVAL
    assert filt(p, 10, (1 << 24) + 1, 10, p, p, 3, p, 10, p, p, None) == ELIMIT
    assert filt(None, 10, 0, 10, None, None, 0, None, 10, None, None, None) == 0   # nothing to do
    slots = ctypes.c_int64()
    for k, n, want in ((50, 1682, 128), (5000, 1682, 4096), (1, 1, 64)):
        assert lib.ctr_rank_table_slots(k, n, ctypes.byref(slots)) == 0 and slots.value == want
    assert lib.ctr_rank_table_slots(0, 10, ctypes.byref(slots)) == EINVAL
    lists = lib.ctr_rank_metrics_lists
    assert lists(p, 10, p, 4, 10, p, p, 3, p, 0, p, 64, p, p, None) == EINVAL      # k < 1
    assert lists(p, 10, p, 4, 10, p, p, 3, p, 5, p, 63, p, p, None) == EINVAL      # table smaller than one user's
    assert lists(p, 10, p, 4, 10, None, p, 3, p, 5, p, 64, p, p, None) == EINVAL
    assert lists(p, 10, p, 4, 10, p, None, 3, p, 5, p, 64, p, p, None) == EINVAL
    assert lists(p, 10, p, 4, 10, p, p, 3, None, 5, p, 64, p, p, None) == EINVAL
    assert lists(p, 10, p, 4, 10, p, p, 3, p, 5, p, 64, None, p, None) == EINVAL
    assert lists(p, 10, p, 4, 10, p, p, 3, p, 5, None, 64, p, p, None) == EINVAL
    assert lists(p, 9, p, 4, 10, p, p, 3, p, 5, p, 64, p, p, None) == EINVAL       # ld_pred < len
    assert lists(None, 10, None, 0, 10, None, None, 0, None, 5, None, 0, None, None, None) == 0
    mask = lib.ctr_rank_mask
    assert mask(p, 10, 4, 0, p, p, 3, p, None) == EINVAL
    assert mask(p, 9, 4, 10, p, p, 3, p, None) == EINVAL
    assert mask(None, 10, 4, 10, p, p, 3, p, None) == EINVAL
    assert mask(p, 10, 4, 10, p, None, 3, p, None) == EINVAL
    assert mask(p, 10, 4, 10, p, p, -1, p, None) == EINVAL
    assert mask(p, 1 << 31, 4, 1 << 31, p, p, 3, p, None) == ELIMIT
    sc = lib.ctr_rank_metrics_scores
    ok = (p, 100, 4, 100, p, 10, 10, p, p, 3, p, p, p, p, p, None)
    args = list(ok)
    args[6] = 0
    args[5] = 0
    assert sc(*args) == EINVAL                                                      # k < 1
    args = list(ok)
    args[5] = 9
    assert sc(*args) == EINVAL                                                      # kt != min(k, n)
    for i in (0, 4, 7, 8, 10, 11, 12, 13, 14):
        args = list(ok)
        args[i] = None
        assert sc(*args) == EINVAL, i
    args = list(ok)
    args[2] = (1 << 24) + 1
    assert sc(*args) == ELIMIT
