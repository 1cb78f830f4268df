"""CPU: the restatement tests/als_weighted_numpy.py -- its float64 weighted row solves against brute-force weighted
least squares (over every cell for confidences, over the observed cells for explicit ratings), the closed forms of both
losses against the dense sums, and the criterion's discriminating power on the cases the GPU test uses (the exact
solution of the system with every value replaced by the list's mean is at least 16x over the threshold, the one with
the last entry dropped is over it) -- then ``data.Interactions``, the host-side refusals of
``ctr_als_solve_rows_weighted`` and what ``ops`` and ``ALS`` decide before a device is touched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import als_numpy as an
import als_weighted_numpy as aw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ELIMIT = 0, -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def _toy(num_users, num_items, k, pairs, seed, palette):
    """(stored mask, values on the stored cells, P, Q)"""
    rs = np.random.RandomState(seed)
    cells = rs.choice(num_users * num_items, pairs, replace=False)
    stored = np.zeros((num_users, num_items), dtype=bool)
    stored[cells // num_items, cells % num_items] = True
    V = np.where(stored, np.asarray(palette)[rs.randint(0, len(palette), stored.shape)], 0.0).astype(np.float32)
    P, Q = rs.normal(0, 0.1, (num_users, k)), rs.normal(0, 0.1, (num_items, k))
    return stored, V, P.astype(np.float32), Q.astype(np.float32)


def _lists(stored, V):
    return [np.flatnonzero(row) for row in stored], [V[u][np.flatnonzero(row)] for u, row in enumerate(stored)]


# ---- the restatement
@pytest.mark.parametrize("alpha,reg", an.PARITY_PARAMS)
def test_float64_confidence_solves_minimise_the_dense_objective(alpha, reg):
    num_users, num_items, k = 7, 9, 16
    stored, V, P, Q = _toy(num_users, num_items, k, 20, 3, aw.CONFIDENCE_VALUES)
    stored[2] = False                                              # a user without a pair
    V[2] = 0.0
    lists, values = _lists(stored, V)
    ob = aw.confidences(alpha, reg)
    got = aw.half_sweep64(Q, lists, values, ob)
    assert not got[2].any()
    for u in range(num_users):
        # brute force: weighted least squares over EVERY item, the regulariser as k more rows
        c = 1.0 + np.float64(np.float32(alpha)) * V[u].astype(np.float64) * stored[u]
        design = np.vstack([Q.astype(np.float64) * np.sqrt(c)[:, None], np.sqrt(np.float64(np.float32(reg))) * np.eye(k)])
        target = np.concatenate([stored[u] * np.sqrt(c), np.zeros(k)])
        want = np.linalg.lstsq(design, target, rcond=None)[0]
        np.testing.assert_allclose(got[u], want, rtol=1e-6, atol=1e-9)
    rs = np.random.RandomState(4)
    a32, r32 = float(np.float32(alpha)), float(np.float32(reg))
    best = aw.dense_loss_confidences(got, Q, V, stored, r32, a32)
    assert best <= aw.dense_loss_confidences(P, Q, V, stored, r32, a32)
    for _ in range(20):
        assert best <= aw.dense_loss_confidences(got + rs.normal(0, 1e-3, got.shape), Q, V, stored, r32, a32)


@pytest.mark.parametrize("reg", [0.05, 0.5])
def test_float64_explicit_solves_minimise_the_observed_objective(reg):
    num_users, num_items, k = 7, 40, 16
    stored, V, P, Q = _toy(num_users, num_items, k, 150, 8, aw.RATINGS)
    stored[2] = False
    V[2] = 0.0
    lists, values = _lists(stored, V)
    ob = aw.explicit(reg)
    got = aw.half_sweep64(Q, lists, values, ob)
    assert not got[2].any()
    r32 = np.float64(np.float32(reg))
    for u in range(num_users):
        if not len(lists[u]):
            continue
        # brute force over the OBSERVED cells, the regulariser times the list length as k more rows
        design = np.vstack([Q[lists[u]].astype(np.float64), np.sqrt(r32 * len(lists[u])) * np.eye(k)])
        target = np.concatenate([values[u].astype(np.float64), np.zeros(k)])
        want = np.linalg.lstsq(design, target, rcond=None)[0]
        np.testing.assert_allclose(got[u], want, rtol=1e-6, atol=1e-9)
    rs = np.random.RandomState(5)
    best = aw.dense_loss_explicit(got, Q, V, stored, float(r32))
    assert best <= aw.dense_loss_explicit(P, Q, V, stored, float(r32))
    for _ in range(20):
        assert best <= aw.dense_loss_explicit(got + rs.normal(0, 1e-3, got.shape), Q, V, stored, float(r32))


@pytest.mark.parametrize("alpha,reg", an.PARITY_PARAMS)
def test_closed_form_losses_equal_the_dense_sums(alpha, reg):
    stored, V, P, Q = _toy(7, 9, 16, 25, 5, aw.CONFIDENCE_VALUES)
    users, items = np.nonzero(stored)
    dense = aw.dense_loss_confidences(P, Q, V, stored, reg, alpha)
    assert abs(aw.loss_confidences(P, Q, users, items, V[users, items], reg, alpha) - dense) <= 1e-12 * abs(dense)
    # all-ones values: the unit model's loss
    ones = stored.astype(np.float32)
    assert abs(aw.loss_confidences(P, Q, users, items, ones[users, items], reg, alpha)
               - an.loss(P, Q, users, items, reg, alpha)) <= 1e-12 * abs(dense)
    stored, V, P, Q = _toy(7, 9, 16, 25, 6, aw.RATINGS)
    users, items = np.nonzero(stored)
    dense = aw.dense_loss_explicit(P, Q, V, stored, reg)
    assert abs(aw.loss_explicit(P, Q, users, items, V[users, items], reg) - dense) <= 1e-12 * abs(dense)


def _parity_cases():
    return [(n, k, init, ob) for n, k in an.PARITY_SHAPES for init in an.PARITY_INITS for ob in aw.PARITY_OBJECTIVES]


@pytest.mark.parametrize("n,k,init,ob", _parity_cases(), ids=lambda v: v.name if isinstance(v, aw.Objective) else None)
def test_criterion_holds_for_the_restatement_and_tells_ignored_values_and_a_dropped_entry(n, k, init, ob):
    """on the cases tests/test_gpu_als_weighted.py runs: the restatement's own residual is a few units of roundoff, the
    exact float64 solution with every value replaced by the list's mean is at least 16x over the threshold on every
    list of two or more entries, the one with the last entry dropped is over it on every list"""
    Y, lists, values, rho_ref = aw.parity_case(n, k, init, ob)
    assert [len(lst) for lst in lists] == an.list_lengths(n, an.CHUNK)
    ignored, dropped = np.inf, np.inf
    for lst, v, ref in zip(lists, values, rho_ref):
        assert ref <= 64 * aw.U
        if len(lst) == 0:
            assert ref == 0.0
            continue
        x = aw.solve64(Y, lst[:-1], v[:-1], ob)
        dropped = min(dropped, aw.rho(x, Y, lst, v, ob) / aw.threshold(ref))
        if len(lst) >= 2:
            assert not (v == v[0]).all()
            x = aw.solve64(Y, lst, np.full(len(lst), v.astype(np.float64).mean(), dtype=np.float32), ob)
            ignored = min(ignored, aw.rho(x, Y, lst, v, ob) / aw.threshold(ref))
    print(f"als weighted criterion n {n} k {k} {init} {ob.name}: ignored values at least {ignored:.1f}x the threshold, "
          f"a dropped last entry at least {dropped:.2f}x, rho_ref up to {max(rho_ref) / aw.U:.2f}u")
    assert dropped > 1.0
    assert ignored >= 16.0 or all(len(lst) < 2 for lst in lists)


def test_unit_objective_is_the_unit_system():
    """values that are all ones with (alpha, 0, 1 + alpha, 0) give als_numpy's system"""
    Y, lists, _ = an.parity_case(200, 64, "normal", 40.0, 0.1)
    ob = aw.unit(40.0, 0.1)
    for lst in lists[1:4]:
        A, b = aw.system64(Y, lst, np.ones(len(lst), np.float32), ob)
        A0, b0 = an.system64(Y, lst, float(np.float32(0.1)), 40.0)
        np.testing.assert_allclose(A, A0, rtol=1e-12)
        np.testing.assert_allclose(b, b0, rtol=1e-12)


def test_many_row_check_is_the_same_criterion():
    ob = aw.PARITY_OBJECTIVES[0]
    Y, lists, values, rho_ref = aw.parity_case(200, 64, "normal", ob)
    good = [aw.solve32(Y, lst, v, ob) for lst, v in zip(lists, values)]
    assert aw.worst_ratio_many(good, Y, lists, values, ob)[0] <= 1.0
    assert max(aw.ratios(good, Y, lists, values, rho_ref, ob)) <= 1.0
    for r in range(1, len(lists)):
        one = list(good)
        one[r] = aw.solve64(Y, lists[r][:-1], values[r][:-1], ob)
        assert aw.worst_ratio_many(one, Y, lists, values, ob)[0] > 1.0


# ---- Interactions
def _triples(seed=0, n=400, num_users=30, num_items=50, integer=False):
    rs = np.random.RandomState(seed)
    u, i = rs.randint(0, num_users, n), rs.randint(0, num_items, n)
    v = rs.randint(1, 6, n).astype(np.float32) if integer else rs.rand(n).astype(np.float32) * 3.0 + 0.1
    return torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(v), num_users, num_items


def _dense(inter):
    p = inter.pairs
    rows = np.repeat(np.arange(p.num_users), np.diff(p.indptr.numpy()))
    M = np.zeros((p.num_users, p.num_items), dtype=np.float32)
    M[rows, p.indices.numpy()] = inter.values.numpy()
    return M


def _tree_sum(vs):
    """the float32 sum by the tree of ``data.interactions._segment_sums``: in pass s = 1, 2, 4, ... the element of rank
    r (a multiple of 2s) takes in the element of rank r + s"""
    vs = [np.float32(c) for c in vs]
    stride = 1
    while stride < len(vs):
        for r in range(0, len(vs) - stride, 2 * stride):
            vs[r] = np.float32(vs[r] + vs[r + stride])
        stride *= 2
    return vs[0]


def test_interactions_align_with_observed_pairs_and_reduce_duplicates():
    from deeplearningrecommendationsystem_amd.data import Interactions, ObservedPairs
    u, i, v, U_, I_ = _triples()
    pairs = ObservedPairs(u, i, U_, I_)
    assert len(pairs) < u.numel()                                   # the draw has repeated pairs
    for rule in ("sum", "mean"):
        inter = Interactions(u, i, v, U_, I_, duplicates=rule)
        assert torch.equal(inter.pairs.indptr, pairs.indptr) and torch.equal(inter.pairs.indices, pairs.indices)
        assert inter.values.dtype == torch.float32 and inter.values.shape == (len(pairs),) and len(inter) == len(pairs)
        assert (inter.num_users, inter.num_items) == (U_, I_)
        # every stored value: the float32 sum of its pair's values, in the order they were given, by the fixed tree
        want = {}
        for a, b, c in zip(u.tolist(), i.tolist(), v.numpy()):
            want.setdefault((a, b), []).append(c)
        M = _dense(inter)
        for (a, b), vs in want.items():
            s = _tree_sum(vs)
            assert abs(float(s) - float(np.sum(np.asarray(vs, np.float64)))) <= 1e-5 * float(s)
            assert M[a, b] == (s if rule == "sum" else np.float32(s / np.float32(len(vs)))), (a, b, vs)
        assert np.count_nonzero(M) == len(want)
    with pytest.raises(ValueError):
        Interactions(u, i, v, U_, I_, duplicates="error")
    with pytest.raises(ValueError):
        Interactions(u, i, v, U_, I_, duplicates="max")
    # sequences are concatenated, as ObservedPairs takes them
    parts = Interactions([u[:100], u[100:]], [i[:100], i[100:]], [v[:100], v[100:]], U_, I_)
    assert torch.equal(parts.values, Interactions(u, i, v, U_, I_).values)
    # distinct pairs pass "error" and keep their values
    keys = torch.unique(u * I_ + i)
    du, di = keys // I_, keys % I_
    dv = torch.arange(keys.numel(), dtype=torch.float32) + 0.5
    perm = torch.from_numpy(np.random.RandomState(1).permutation(keys.numel()))
    distinct = Interactions(du[perm], di[perm], dv[perm], U_, I_, duplicates="error")
    assert torch.equal(distinct.values, dv)                         # back in CSR order
    empty = Interactions(u[:0], i[:0], v[:0], U_, I_)
    assert len(empty) == 0 and empty.values.shape == (0,) and len(empty.transpose()) == 0


def test_interactions_same_bits_on_two_calls_with_non_integer_values():
    from deeplearningrecommendationsystem_amd.data import Interactions
    u, i, v, U_, I_ = _triples(seed=3, n=5000, num_users=20, num_items=25)      # ~10 values a pair
    for rule in ("sum", "mean"):
        a, b = Interactions(u, i, v, U_, I_, rule), Interactions(u, i, v, U_, I_, rule)
        assert torch.equal(a.values, b.values)
        assert torch.equal(a.values.view(torch.int32), b.values.view(torch.int32))
    want = {}
    for x, y, c in zip(u.tolist(), i.tolist(), v.numpy()):
        want.setdefault((x, y), []).append(c)
    M = _dense(Interactions(u, i, v, U_, I_, "sum"))
    assert max(len(vs) for vs in want.values()) >= 16             # trees of five levels
    assert all(M[x, y] == _tree_sum(vs) for (x, y), vs in want.items())


def test_interactions_transpose_round_trip():
    from deeplearningrecommendationsystem_amd.data import Interactions, ObservedPairs
    u, i, v, U_, I_ = _triples(seed=5)
    inter = Interactions(u, i, v, U_, I_)
    t = inter.transpose()
    assert (t.num_users, t.num_items) == (I_, U_)
    ref = ObservedPairs(i, u, I_, U_)
    assert torch.equal(t.pairs.indptr, ref.indptr) and torch.equal(t.pairs.indices, ref.indices)
    assert np.array_equal(_dense(t), _dense(inter).T)               # asymmetric values: a wrong alignment shows
    back = t.transpose()
    assert torch.equal(back.pairs.indptr, inter.pairs.indptr) and torch.equal(back.pairs.indices, inter.pairs.indices)
    assert torch.equal(back.values, inter.values)


def test_interactions_refusals():
    from deeplearningrecommendationsystem_amd.data import Interactions
    u, i, v, U_, I_ = _triples(n=10)
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = v.clone()
        w[4] = bad
        with pytest.raises(ValueError):
            Interactions(u, i, w, U_, I_)
    with pytest.raises(IndexError):
        Interactions(torch.tensor([0, U_]), torch.tensor([0, 0]), torch.ones(2), U_, I_)
    with pytest.raises(IndexError):
        Interactions(torch.tensor([0, 1]), torch.tensor([0, -1]), torch.ones(2), U_, I_)
    with pytest.raises(ValueError):
        Interactions(u, i, v.double(), U_, I_)
    with pytest.raises(ValueError):
        Interactions(u, i, v[:-1], U_, I_)
    with pytest.raises(ValueError):
        Interactions(u.int(), i, v, U_, I_)
    with pytest.raises(ValueError):
        Interactions(u, i, v, 0, I_)
    with pytest.raises(ValueError):
        Interactions(u, i, v, U_, 1 << 31)


# ---- the C entry: every refusal below is decided on the host, before a launch
def test_header_declares_the_weighted_entry(lib):
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    assert "ctr_als_solve_rows_weighted" in text and "ctr_als_solve_rows_weighted" in lib.SIGNATURES
    assert hasattr(lib.load(), "ctr_als_solve_rows_weighted")
    assert lib.ABI_VERSION == lib.load().ctr_version()


def test_weighted_entry_refuses_before_a_launch(lib):
    h = lib.load()
    buf = (ctypes.c_float * 64)()            # host memory, never dereferenced: nothing below reaches a launch
    p = ctypes.addressof(buf)

    def call(y=p, y_rows=10, k=64, gram=p, indptr=p, indices=p, values=p, csr_rows=5, rows=None, count=5,
             scalars=(0.0, 40.0, 1.0, 40.0, 0.1, 0.0), out=p, ldo=None):
        return h.ctr_als_solve_rows_weighted(y, y_rows, k, gram, indptr, indices, values, csr_rows, rows, count,
                                             *scalars, out, k if ldo is None else ldo, None, None)

    for k in (24, 8, 144, 256):
        assert call(k=k) == ELIMIT
    # count == 0: CTR_OK, nothing enqueued, whatever the pointers are
    assert call(y=None, gram=None, indptr=None, indices=None, values=None, out=None, count=0) == OK
    assert call(values=None) == EINVAL                             # a CSR with pairs and no values
    assert call(y=None) == EINVAL
    assert call(indptr=None) == EINVAL
    assert call(out=None) == EINVAL
    assert call(ldo=63) == EINVAL
    assert call(count=-1) == EINVAL
    assert call(y_rows=0) == EINVAL
    assert call(csr_rows=0) == EINVAL
    for at in range(6):                                            # a NaN in any of the six scalars
        scalars = [0.0, 40.0, 1.0, 40.0, 0.1, 0.0]
        scalars[at] = float("nan")
        assert call(scalars=tuple(scalars)) == EINVAL


# ---- ops and the model, without a device
def test_ops_refuse_bad_arguments_and_have_no_cpu_fallback(lib):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    indptr, indices = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1], dtype=torch.int32)
    values = torch.ones(3)
    w, t = (0.0, 40.0), (1.0, 40.0)
    y, g = torch.zeros(5, 16), torch.zeros(16, 16)
    for k in (24, 144, 8):
        with pytest.raises(ValueError):
            ops.als_solve_rows_weighted(torch.zeros(5, k), torch.zeros(k, k), indptr, indices, values, w, t, 0.1)
    for bad in (dict(values=values[:2]), dict(values=values.double()), dict(w=(0.0,)), dict(w=(0.0, float("nan"))),
                dict(t=1.0), dict(reg=float("nan")), dict(reg_per_entry=float("nan")), dict(gram=torch.zeros(16, 8))):
        kw = dict(y=y, gram=g, indptr=indptr, indices=indices, values=values, w=w, t=t, reg=0.1, reg_per_entry=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.als_solve_rows_weighted(**kw)
    with pytest.raises(CtrHipError):
        ops.als_solve_rows_weighted(y, g, indptr, indices, values, w, t, 0.1)
    with pytest.raises(CtrHipError):
        ops.als_solve_rows_weighted(y, None, indptr, indices, values, (1.0, 0.0), (0.0, 1.0), 0.0, 0.05)


def test_model_refusals_need_no_device(lib):
    import deeplearningrecommendationsystem_amd as pkg
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    from deeplearningrecommendationsystem_amd.data import Interactions, ObservedPairs
    for objective in ("ranking", "", "Implicit", None):
        with pytest.raises(ValueError):
            pkg.ALS(5, 6, k=16, objective=objective)
    assert pkg.ALS(5, 6, k=16, device="cpu").objective == "implicit"
    u, i = torch.tensor([0, 1, 4]), torch.tensor([2, 2, 5])
    pairs = ObservedPairs(u, i, 5, 6)
    implicit = pkg.ALS(5, 6, k=16, device="cpu")
    with pytest.raises(ValueError):                                 # a negative confidence value
        implicit.fit(Interactions(u, i, torch.tensor([1.0, -0.5, 2.0]), 5, 6))
    with pytest.raises(ValueError):
        implicit.fold_in(Interactions(u, i, torch.tensor([1.0, -0.5, 2.0]), 5, 6))
    with pytest.raises(CtrHipError):                                # well formed (a zero value too), but no device
        implicit.fit(Interactions(u, i, torch.tensor([1.0, 0.0, 2.0]), 5, 6))
    explicit = pkg.ALS(5, 6, k=16, device="cpu", objective="explicit")
    with pytest.raises(ValueError):                                 # a set has no ratings
        explicit.fit(pairs)
    with pytest.raises(ValueError):
        explicit.fold_in(pairs)
    with pytest.raises(ValueError):
        explicit.fit(Interactions(u, i, torch.ones(3), 5, 7))
    with pytest.raises(CtrHipError):                                # negative ratings are fine; no device is not
        explicit.fit(Interactions(u, i, torch.tensor([1.0, -0.5, 2.0]), 5, 6))
    with pytest.raises(RuntimeError):
        explicit.loss()
    # predict is plain torch
    got = implicit.predict([0, 4], [2, 5])
    assert torch.equal(got, (implicit.P[[0, 4]] * implicit.Q[[2, 5]]).sum(1)) and got.dtype == torch.float32
    with pytest.raises(IndexError):
        implicit.predict([5], [0])
    with pytest.raises(IndexError):
        implicit.predict([0], [6])
