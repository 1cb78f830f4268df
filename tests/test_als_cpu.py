"""CPU: the restatement tests/als_numpy.py -- its float64 row solves against a brute-force dense least squares, the
closed form of the loss against the dense sum, the float32 restatement against the solve criterion, and the criterion's
discriminating power (the exact solution of a system with one list entry dropped fails it on every GPU parity case) --
then the host-side refusals of the three ``ctr_als_*`` entries and what ``ops`` and ``ALS`` decide before a device is
touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import als_numpy as an

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ELIMIT = 0, -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def _toy(num_users, num_items, k, pairs, seed):
    rs = np.random.RandomState(seed)
    cells = rs.choice(num_users * num_items, pairs, replace=False)
    Yui = np.zeros((num_users, num_items))
    Yui[cells // num_items, cells % num_items] = 1.0
    P, Q = rs.normal(0, 0.1, (num_users, k)), rs.normal(0, 0.1, (num_items, k))
    return Yui, P, Q


# ---- the restatement
@pytest.mark.parametrize("alpha,reg", an.PARITY_PARAMS)
def test_float64_row_solves_minimise_the_dense_objective(alpha, reg):
    num_users, num_items, k = 7, 9, 16
    Yui, P, Q = _toy(num_users, num_items, k, 20, 3)
    Yui[2] = 0.0                                                   # a user without a pair
    lists = [np.flatnonzero(row) for row in Yui]
    got = an.half_sweep64(Q, lists, reg, alpha)
    assert not got[2].any()                                        # an empty list: exact zeros
    for u in range(num_users):
        # brute force: weighted least squares over EVERY item, the regulariser as k more rows
        w = np.sqrt(1.0 + alpha * Yui[u])
        design = np.vstack([Q * w[:, None], np.sqrt(reg) * np.eye(k)])
        target = np.concatenate([Yui[u] * w, np.zeros(k)])
        want = np.linalg.lstsq(design, target, rcond=None)[0]
        np.testing.assert_allclose(got[u], want, rtol=1e-9, atol=1e-12)
    # and the objective itself: no perturbation of the solved rows lowers it
    rs = np.random.RandomState(4)
    best = an.dense_loss(got, Q, Yui, reg, alpha)
    assert best <= an.dense_loss(P, Q, Yui, reg, alpha)
    for _ in range(20):
        assert best <= an.dense_loss(got + rs.normal(0, 1e-3, got.shape), Q, Yui, reg, alpha)


@pytest.mark.parametrize("alpha,reg", an.PARITY_PARAMS)
def test_closed_form_loss_equals_the_dense_sum(alpha, reg):
    Yui, P, Q = _toy(7, 9, 16, 25, 5)
    users, items = np.nonzero(Yui)
    dense = an.dense_loss(P, Q, Yui, reg, alpha)
    assert abs(an.loss(P, Q, users, items, reg, alpha) - dense) <= 1e-12 * abs(dense)


def _parity_cases():
    return [(n, k, init, alpha, reg) for n, k in an.PARITY_SHAPES for init in an.PARITY_INITS
            for alpha, reg in an.PARITY_PARAMS]


@pytest.mark.parametrize("n,k,init,alpha,reg", _parity_cases())
def test_criterion_holds_for_the_restatement_and_fails_a_dropped_entry(n, k, init, alpha, reg):
    Y, lists, rho_ref = an.parity_case(n, k, init, alpha, reg)
    assert [len(lst) for lst in lists] == an.list_lengths(n, an.CHUNK)
    closest = np.inf
    for lst, ref in zip(lists, rho_ref):
        assert ref <= an.threshold(ref)                            # trivially its own criterion
        assert ref <= 64 * an.U                                    # ... which is no loose one: a few units of roundoff
        if len(lst) == 0:
            assert ref == 0.0
            continue
        # the exact solution of the system with one entry dropped must NOT pass
        for drop in (0, len(lst) - 1):
            x = an.solve64(Y, np.delete(lst, drop), reg, alpha)
            closest = min(closest, an.rho(x, Y, lst, reg, alpha) / an.threshold(ref))
    print(f"als criterion n {n} k {k} {init} alpha {alpha} reg {reg}: a dropped entry is at least {closest:.2f}x the "
          f"threshold, rho_ref up to {max(rho_ref) / an.U:.2f}u")
    assert closest > 1.0


def test_many_row_check_is_the_same_criterion():
    """``worst_ratio_many`` skips the restatement for rows under the 8u floor of every threshold: it must pass what the
    row-by-row criterion passes and fail a dropped entry"""
    Y, lists, rho_ref = an.parity_case(200, 64, "normal", 40.0, 0.1)
    good = [an.solve32(Y, lst, 0.1, 40.0) for lst in lists]
    worst, _ = an.worst_ratio_many(good, Y, lists, 0.1, 40.0)
    assert worst <= 1.0 and an.worst_ratio(good, Y, lists, rho_ref, 0.1, 40.0) <= 1.0
    dropped = [an.solve64(Y, lst[1:], 0.1, 40.0) if len(lst) else np.zeros(64) for lst in lists]
    for r in range(1, len(lists)):
        one = list(good)
        one[r] = dropped[r]
        assert an.worst_ratio_many(one, Y, lists, 0.1, 40.0)[0] > 1.0


def test_float32_restatement_loss_does_not_increase():
    num_users, num_items, k, alpha, reg = 20, 30, 16, 40.0, 0.1
    Yui, P, Q = _toy(num_users, num_items, k, 150, 6)
    users, items = np.nonzero(Yui)
    user_lists = [np.flatnonzero(row) for row in Yui]
    item_lists = [np.flatnonzero(col) for col in Yui.T]
    P, Q = P.astype(np.float32), Q.astype(np.float32)
    last = an.loss(P, Q, users, items, reg, alpha)
    for _ in range(3):
        P = an.half_sweep32(Q, user_lists, reg, alpha)
        now = an.loss(P, Q, users, items, reg, alpha)
        assert now <= last * (1 + 1e-6)
        Q = an.half_sweep32(P, item_lists, reg, alpha)
        last, mid = an.loss(P, Q, users, items, reg, alpha), now
        assert last <= mid * (1 + 1e-6)


def test_float32_restatement_is_close_to_float64():
    Y, lists, _ = an.parity_case(200, 64, "normal", 40.0, 0.1)
    for lst in lists[1:]:
        x32, x64 = an.solve32(Y, lst, 0.1, 40.0), an.solve64(Y, lst, 0.1, 40.0)
        assert np.abs(x32 - x64).max() <= 1e-3 * np.abs(x64).max()


# ---- the header and the C entries: every refusal below is decided on the host, before a launch
def test_header_declares_the_entries_and_the_limit(lib):
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    define = int(re.search(r"#define\s+CTR_ALS_MAX_DIM\s+(\d+)", text).group(1))
    assert lib.CTR_ALS_MAX_DIM == define == ops.ALS_MAX_DIM == 128
    handle = lib.load()
    for name in ("ctr_als_gram_workspace_bytes", "ctr_als_gram", "ctr_als_solve_rows"):
        assert name in text and name in lib.SIGNATURES and hasattr(handle, name)


def test_supported_dims():
    from deeplearningrecommendationsystem_amd import ops
    assert [k for k in range(0, 200) if ops.als_supported(k)] == list(range(16, 129, 16))
    assert not ops.als_supported(16.0) and not ops.als_supported(True)


def test_c_entries_refuse_before_a_launch(lib):
    h = lib.load()
    buf = (ctypes.c_float * 64)()            # host memory, never dereferenced: nothing below reaches a launch
    p = ctypes.addressof(buf)
    nbytes = ctypes.c_int64(-1)
    assert h.ctr_als_gram_workspace_bytes(1000, 64, ctypes.byref(nbytes)) == OK
    assert nbytes.value == 2 * 64 * 64 * 4                         # two slabs of an.SLAB rows
    assert -(-1000 // an.SLAB) == 2
    assert h.ctr_als_gram_workspace_bytes(1000, 64, None) == EINVAL
    assert h.ctr_als_gram_workspace_bytes(0, 64, ctypes.byref(nbytes)) == EINVAL
    for k in (24, 8, 144, 256):
        assert h.ctr_als_gram_workspace_bytes(1000, k, ctypes.byref(nbytes)) == ELIMIT
        assert h.ctr_als_gram(p, 1000, k, p, p, 1 << 30, None) == ELIMIT
        assert h.ctr_als_solve_rows(p, 10, k, p, p, p, 5, None, 5, 0.1, 40.0, p, k, None, None) == ELIMIT
    assert h.ctr_als_gram(None, 1000, 64, p, p, 1 << 30, None) == EINVAL
    assert h.ctr_als_gram(p, 1000, 64, None, p, 1 << 30, None) == EINVAL
    assert h.ctr_als_gram(p, 1000, 64, p, None, 1 << 30, None) == EINVAL
    assert h.ctr_als_gram(p, 1000, 64, p, p, 2 * 64 * 64 * 4 - 1, None) == EINVAL      # workspace too small
    assert h.ctr_als_gram(p, 0, 64, p, p, 1 << 30, None) == EINVAL
    # count == 0: CTR_OK, nothing enqueued, whatever the pointers are
    assert h.ctr_als_solve_rows(None, 10, 64, None, None, None, 5, None, 0, 0.1, 40.0, None, 64, None, None) == OK
    assert h.ctr_als_solve_rows(None, 10, 64, p, p, p, 5, None, 5, 0.1, 40.0, p, 64, None, None) == EINVAL
    assert h.ctr_als_solve_rows(p, 10, 64, None, p, p, 5, None, 5, 0.1, 40.0, p, 64, None, None) == EINVAL
    assert h.ctr_als_solve_rows(p, 10, 64, p, None, p, 5, None, 5, 0.1, 40.0, p, 64, None, None) == EINVAL
    assert h.ctr_als_solve_rows(p, 10, 64, p, p, p, 5, None, 5, 0.1, 40.0, None, 64, None, None) == EINVAL
    assert h.ctr_als_solve_rows(p, 10, 64, p, p, p, 5, None, 5, 0.1, 40.0, p, 63, None, None) == EINVAL   # ldo < k
    assert h.ctr_als_solve_rows(p, 10, 64, p, p, p, 5, None, -1, 0.1, 40.0, p, 64, None, None) == EINVAL
    assert h.ctr_als_solve_rows(p, 0, 64, p, p, p, 5, None, 5, 0.1, 40.0, p, 64, None, None) == EINVAL
    assert h.ctr_als_solve_rows(p, 10, 64, p, p, p, 5, None, 5, float("nan"), 40.0, p, 64, None, None) == EINVAL


# ---- ops and the model, without a device
def test_ops_refuse_bad_shapes_and_have_no_cpu_fallback(lib):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    indptr, indices = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1], dtype=torch.int32)
    for k in (24, 144, 8):
        with pytest.raises(ValueError):
            ops.als_gram(torch.zeros(5, k))
        with pytest.raises(ValueError):
            ops.als_solve_rows(torch.zeros(5, k), torch.zeros(k, k), indptr, indices, 0.1, 40.0)
    with pytest.raises(ValueError):
        ops.als_gram(torch.zeros(5, 16, dtype=torch.float64))
    with pytest.raises(CtrHipError):
        ops.als_gram(torch.zeros(5, 16))
    with pytest.raises(CtrHipError):
        ops.als_solve_rows(torch.zeros(5, 16), torch.zeros(16, 16), indptr, indices, 0.1, 40.0)


def test_model_argument_errors_need_no_device(lib):
    import deeplearningrecommendationsystem_amd as pkg
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    for kwargs in (dict(reg=0.0), dict(reg=-1.0), dict(alpha=-0.5), dict(k=24), dict(k=144), dict(k=0),
                   dict(reg=float("nan"))):
        with pytest.raises(ValueError):
            pkg.ALS(5, 6, **{"k": 16, **kwargs})
    with pytest.raises(ValueError):
        pkg.ALS(0, 6, k=16)
    model = pkg.ALS(5, 6, k=16, device="cpu")
    assert model.P.shape == (5, 16) and model.Q.shape == (6, 16) and model.P.dtype == torch.float32
    assert not isinstance(model.P, torch.nn.Parameter)
    # P before Q from one RandomState, N(0, 0.01)
    rs = np.random.RandomState(0)
    np.testing.assert_array_equal(model.P.numpy(), rs.normal(0.0, 0.01, (5, 16)).astype(np.float32))
    np.testing.assert_array_equal(model.Q.numpy(), rs.normal(0.0, 0.01, (6, 16)).astype(np.float32))
    with pytest.raises(RuntimeError):
        model.sweep()
    observed = ObservedPairs(torch.tensor([0, 1, 4]), torch.tensor([2, 2, 5]), 5, 6)
    with pytest.raises(ValueError):
        model.fit(ObservedPairs(torch.tensor([0]), torch.tensor([2]), 5, 7))
    with pytest.raises(CtrHipError):
        model.fit(observed)                                       # well formed, but no device: no CPU fallback
