"""GPU: the weighted arm of the ALS row solves (csrc/als.hip, ``ctr_als_solve_rows_weighted``) against the restatement
tests/als_weighted_numpy.py -- per-pair confidences and explicit ratings by the scaled residual against the float32
restatement's own (rho <= 4 rho_ref + 8u) on both sides of every chunk boundary and on 3000 rows in one launch, the
plumbing, locality and fold-in bitwise, the unit arm untouched, the guards, the model under both objectives and the
script.

Every parity check prints its worst rho / threshold; the worst seen on the MI355X is quoted in DESIGN.md section 4s."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import als_numpy as an
import als_weighted_numpy as aw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF, EXPLICIT = aw.PARITY_OBJECTIVES[0], aw.PARITY_OBJECTIVES[2]


def _pkg():
    import deeplearningrecommendationsystem_amd as pkg
    from deeplearningrecommendationsystem_amd import ops
    return pkg, ops


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared cases are read-only


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _solve(Y, lists, values, ob, gram=None, rows=None):
    """(rows of x as a device tensor, flag value) of one als_solve_rows_weighted call over the CSR of ``lists``"""
    _, ops = _pkg()
    y = _dev(Y)
    indptr, indices, vals = aw.csr(lists, values)
    if ob.dense and gram is None:
        gram = ops.als_gram(y)
    flag = _flag()
    out = ops.als_solve_rows_weighted(y, gram if ob.dense else None, _dev(indptr), _dev(indices), _dev(vals),
                                      (ob.w0, ob.w1), (ob.t0, ob.t1), ob.reg, ob.reg_per_entry,
                                      rows=None if rows is None else _dev(np.asarray(rows, dtype=np.int64)),
                                      err_flag=flag)
    return out, int(flag.item())


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("ob", aw.PARITY_OBJECTIVES, ids=lambda ob: ob.name)
@pytest.mark.parametrize("init", an.PARITY_INITS)
@pytest.mark.parametrize("n,k", an.PARITY_SHAPES)
def test_solve_parity(n, k, init, ob):
    Y, lists, values, rho_ref = aw.parity_case(n, k, init, ob)
    out, bits = _solve(Y, lists, values, ob)
    X = out.cpu().numpy()
    assert bits == 0 and np.isfinite(X).all()
    assert not X[0].any()                                     # the empty list: exact zeros
    ratios = aw.ratios(X, Y, lists, values, rho_ref, ob)
    print(f"als_solve_rows_weighted n {n} k {k} {init} {ob.name}: worst rho / threshold {max(ratios):.4f} "
          f"(list length {len(lists[int(np.argmax(ratios))])})")
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("ob", [CONF, EXPLICIT], ids=lambda ob: ob.name)
@pytest.mark.parametrize("k", [64, 128])
def test_solve_parity_many_rows_in_one_launch(k, ob):
    """3000 rows in ONE launch, every one held to the criterion, and again as a permuted launch, bitwise"""
    n, rows = 1000, 3000
    rs = np.random.RandomState(k)
    Y = an.case_table(n, k, "normal", 50 + k)
    lists = [np.sort(rs.choice(n, rs.randint(0, 41), replace=False)).astype(np.int64) for _ in range(rows)]
    values = aw.case_values(lists, ob.palette, 9 + k)
    out, bits = _solve(Y, lists, values, ob)
    X = out.cpu().numpy()
    assert bits == 0 and np.isfinite(X).all()
    empty = [r for r, lst in enumerate(lists) if len(lst) == 0]
    assert empty and not X[empty].any()
    assert all(X[r].any() for r, lst in enumerate(lists) if len(lst))      # no row was silently zeroed
    worst, slow = aw.worst_ratio_many(X, Y, lists, values, ob)
    print(f"als_solve_rows_weighted {rows} rows in one launch, k {k} {ob.name}: worst rho / threshold {worst:.4f} "
          f"({slow} rows needed the restatement)")
    assert worst <= 1.0
    perm = np.random.RandomState(1).permutation(rows)
    permuted, bits = _solve(Y, lists, values, ob, rows=perm)
    assert bits == 0 and torch.equal(permuted, out[_dev(perm)])


def test_all_ones_values_meet_the_unit_criterion():
    """c = 1 + alpha * 1 is the unit system; not bitwise the unit arm's row (fma(alpha, s, s) is not (1 + alpha) s)"""
    for n, k, init, (alpha, reg) in [(200, 64, "uniform", an.PARITY_PARAMS[0]), (300, 128, "normal", an.PARITY_PARAMS[1]),
                                     (65, 16, "normal", an.PARITY_PARAMS[0])]:
        Y, lists, rho_ref = an.parity_case(n, k, init, alpha, reg)
        ones = [np.ones(len(lst), dtype=np.float32) for lst in lists]
        out, bits = _solve(Y, lists, ones, aw.confidences(alpha, reg))
        assert bits == 0
        worst = an.worst_ratio(out.cpu().numpy(), Y, lists, rho_ref, reg, alpha)
        print(f"als_solve_rows_weighted all-ones n {n} k {k} {init}: worst rho / threshold of the unit system {worst:.4f}")
        assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ bitwise
def test_values_times_two_with_half_alpha_is_the_same_row():
    Y, lists, values, _ = aw.parity_case(200, 64, "normal", CONF)
    out, bits = _solve(Y, lists, values, aw.confidences(40.0, 0.1))
    doubled, bits2 = _solve(Y, lists, [2.0 * v for v in values], aw.confidences(20.0, 0.1))
    assert bits == 0 == bits2 and torch.equal(out, doubled)
    other, _ = _solve(Y, lists, [2.0 * v for v in values], aw.confidences(40.0, 0.1))
    assert not torch.equal(out[1:], other[1:])               # the values do reach the kernel


@pytest.mark.parametrize("ob", [CONF, EXPLICIT], ids=lambda ob: ob.name)
def test_locality_and_determinism(ob):
    Y, lists, values, _ = aw.parity_case(200, 64, "uniform", ob)
    _, ops = _pkg()
    gram = ops.als_gram(_dev(Y))
    every, _ = _solve(Y, lists, values, ob, gram)
    again, _ = _solve(Y, lists, values, ob, gram)
    assert torch.equal(every, again)
    count = len(lists)
    explicit, _ = _solve(Y, lists, values, ob, gram, rows=np.arange(count))
    assert torch.equal(every, explicit)
    perm = np.random.RandomState(3).permutation(count)
    permuted, _ = _solve(Y, lists, values, ob, gram, rows=perm)
    assert torch.equal(permuted, every[_dev(perm)])
    repeats = np.array([5, 5, count - 1, 0, 5, count - 1, 2])
    repeated, _ = _solve(Y, lists, values, ob, gram, rows=repeats)
    assert torch.equal(repeated, every[_dev(repeats)])
    for row in (0, 4, count - 1):
        single, _ = _solve(Y, lists, values, ob, gram, rows=[row])
        assert torch.equal(single[0], every[row])
    # a row alone in its own CSR: the same list and values at another offset
    for row in (4, count - 1):
        alone, _ = _solve(Y, [lists[row]], [values[row]], ob, gram)
        assert torch.equal(alone[0], every[row])


def test_unit_arm_is_the_same_before_and_after_a_weighted_call():
    _, ops = _pkg()
    alpha, reg = an.PARITY_PARAMS[0]
    Y, lists, _ = an.parity_case(200, 64, "normal", alpha, reg)
    y = _dev(Y)
    indptr, indices = (_dev(a) for a in an.csr(lists))
    gram = ops.als_gram(y)
    before = ops.als_solve_rows(y, gram, indptr, indices, reg, alpha)
    _, lists_w, values, _ = aw.parity_case(200, 64, "normal", CONF)
    _solve(Y, lists_w, values, CONF, gram)
    _solve(Y, lists_w, values, EXPLICIT)
    after = ops.als_solve_rows(y, ops.als_gram(y), indptr, indices, reg, alpha)
    assert torch.equal(before, after)


# ------------------------------------------------------------------------------------------------------------ guards
@pytest.mark.parametrize("bad", ["y_rows", -1])
def test_bad_index_at_the_end_of_the_arrays_is_never_read(bad):
    """the bad index is the LAST entry of the LAST row: its index and its value end their allocations, and a kernel
    that read one entry past a list's end would leave the arrays"""
    ob = CONF
    Y, lists, values, _ = aw.parity_case(65, 16, "normal", ob)
    order = [r for r in range(len(lists)) if r != 5] + [5]     # the 33-entry list last: the bad index opens chunk 2
    lists, values = [lists[r] for r in order], [values[r] for r in order]
    assert len(lists[-1]) == 33
    clean, _ = _solve(Y, lists, values, ob)
    broken = [lst.copy() for lst in lists]
    broken[-1][-1] = 65 if bad == "y_rows" else -1
    out, bits = _solve(Y, broken, values, ob)
    _, ops = _pkg()
    assert bits == ops.ALS_ERR_INDEX
    assert not out[-1].any()
    assert torch.equal(out[:-1], clean[:-1])


@pytest.mark.parametrize("ob", [CONF, EXPLICIT], ids=lambda ob: ob.name)
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_non_finite_value_gives_a_zero_row_and_the_pivot_bit(poison, ob):
    _, ops = _pkg()
    Y, lists, values, _ = aw.parity_case(200, 48, "uniform", ob)
    clean, _ = _solve(Y, lists, values, ob)
    hit = [3, len(lists) - 1]                                  # 31 entries (the value in the last slot) and the whole table
    bad = [v.copy() for v in values]
    bad[hit[0]][-1] = poison
    bad[hit[1]][40] = poison
    out, bits = _solve(Y, lists, bad, ob)
    assert bits == ops.ALS_ERR_PIVOT
    assert bool(torch.isfinite(out).all())
    assert not out[hit].any()
    miss = [r for r in range(len(lists)) if r not in hit]
    assert torch.equal(out[miss], clean[miss])


def test_infinite_scalar_gives_zero_rows_and_the_pivot_bit():
    _, ops = _pkg()
    Y, lists, values, _ = aw.parity_case(65, 16, "normal", CONF)
    out, bits = _solve(Y, lists, values, aw.confidences(float("inf"), 0.1))
    assert bits == ops.ALS_ERR_PIVOT and not out.any() and bool(torch.isfinite(out).all())


def test_pivot_guard_zero_system():
    _, ops = _pkg()
    Y = np.zeros((40, 16), dtype=np.float32)
    lists = [np.arange(0), np.arange(3), np.arange(40)]
    values = [np.ones(len(lst), dtype=np.float32) for lst in lists]
    for ob in (aw.confidences(40.0, 0.0), aw.explicit(0.0)):
        out, bits = _solve(Y, lists, values, ob)
        assert bits == ops.ALS_ERR_PIVOT
        assert not out.any() and bool(torch.isfinite(out).all())


def test_negative_weights_are_caught_by_the_pivot_guard():
    """w_e < 0 is the caller's business: an indefinite system ends in the guard, not in a NaN"""
    _, ops = _pkg()
    Y, lists, values, _ = aw.parity_case(65, 16, "uniform", EXPLICIT)
    ob = aw.Objective("negative", -1.0, 0.0, 0.0, 1.0, 0.0, 0.0, False, aw.RATINGS)
    out, bits = _solve(Y, lists, values, ob)
    assert bits == ops.ALS_ERR_PIVOT and not out.any()


def test_count_zero_launches_nothing():
    from deeplearningrecommendationsystem_amd import _lib
    lib = _lib.load()
    assert lib.ctr_als_solve_rows_weighted(None, 1, 16, None, None, None, None, 1, None, 0, 0.0, 40.0, 1.0, 40.0, 0.1,
                                           0.0, None, 16, None, None) == 0
    Y, lists, values, _ = aw.parity_case(65, 16, "normal", CONF)
    out, bits = _solve(Y, lists, values, CONF, rows=np.zeros(0, dtype=np.int64))
    assert out.shape == (0, 16) and bits == 0


def test_a_csr_without_a_pair():
    """nnz == 0: indices and values go in as NULL and every row is an empty list"""
    _, ops = _pkg()
    y = _dev(an.case_table(10, 16, "normal", 1))
    flag = _flag()
    out = ops.als_solve_rows_weighted(y, None, torch.zeros(4, dtype=torch.int64, device="cuda"),
                                      torch.zeros(0, dtype=torch.int32, device="cuda"),
                                      torch.zeros(0, dtype=torch.float32, device="cuda"), (1.0, 0.0), (0.0, 1.0), 0.0,
                                      0.05, err_flag=flag)
    assert out.shape == (3, 16) and not out.any() and int(flag.item()) == 0


# ------------------------------------------------------------------------------------------------------------ data
@pytest.mark.parametrize("rule", ["sum", "mean"])
def test_interactions_on_the_device_reduce_duplicates_as_on_the_host(rule):
    """the stable sort and the segmented sum give, on the device, the bits the host gives: each pair's values added in
    the order they were given"""
    from deeplearningrecommendationsystem_amd.data import Interactions
    rs = np.random.RandomState(2)
    u, i = rs.randint(0, 20, 5000), rs.randint(0, 25, 5000)       # ~10 values a pair
    v = (rs.rand(5000) * 3.0 + 0.1).astype(np.float32)
    host = Interactions(torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(v), 20, 25, rule)
    dev = Interactions(_dev(u), _dev(i), _dev(v), 20, 25, rule)
    again = Interactions(_dev(u), _dev(i), _dev(v), 20, 25, rule)
    assert dev.values.is_cuda and torch.equal(dev.values, again.values)
    assert torch.equal(dev.pairs.indptr.cpu(), host.pairs.indptr) and torch.equal(dev.pairs.indices.cpu(), host.pairs.indices)
    assert torch.equal(dev.values.cpu(), host.values)
    t = dev.transpose()
    assert torch.equal(t.transpose().values, dev.values)


# ------------------------------------------------------------------------------------------------------------ model
NUM_USERS, NUM_ITEMS = 60, 40


def _toy(objective):
    """ALS(60, 40, k=16) on about 900 valued pairs -- the value depends on (user, item) asymmetrically, so a transposed
    CSR whose values are misaligned shows"""
    pkg, _ = _pkg()
    from deeplearningrecommendationsystem_amd.data import Interactions
    rs = np.random.RandomState(13)
    cells = rs.choice(NUM_USERS * NUM_ITEMS, 900, replace=False)
    users, items = cells // NUM_ITEMS, cells % NUM_ITEMS
    if objective == "explicit":
        vals = (1 + (3 * users + 7 * items) % 5).astype(np.float32)              # ratings 1..5
    else:
        vals = np.asarray(aw.CONFIDENCE_VALUES, dtype=np.float32)[(3 * users + 5 * items) % 7]
    inter = Interactions(_dev(users.astype(np.int64)), _dev(items.astype(np.int64)), _dev(vals), NUM_USERS, NUM_ITEMS,
                         duplicates="error")
    V = np.zeros((NUM_USERS, NUM_ITEMS), dtype=np.float32)
    stored = np.zeros((NUM_USERS, NUM_ITEMS), dtype=bool)
    V[users, items], stored[users, items] = vals, True
    model = pkg.ALS(NUM_USERS, NUM_ITEMS, k=16, reg=0.1, alpha=40.0, objective=objective).fit(inter, sweeps=0)
    return model, inter, V, stored


def _lists_of(side):
    indptr, indices = side.pairs.indptr.cpu().numpy(), side.pairs.indices.cpu().numpy()
    values = side.values.cpu().numpy()
    rows = range(len(indptr) - 1)
    return ([indices[indptr[r]:indptr[r + 1]].astype(np.int64) for r in rows],
            [values[indptr[r]:indptr[r + 1]] for r in rows])


@pytest.mark.parametrize("objective", ["implicit", "explicit"])
def test_model_sweeps_loss_recommend_and_predict(objective):
    model, inter, V, stored = _toy(objective)
    ob = aw.confidences(model.alpha, model.reg) if objective == "implicit" else aw.explicit(model.reg)
    user_lists, user_values = _lists_of(model._users)
    item_lists, item_values = _lists_of(model._items)
    # the transposed side carries every value to its place
    for u, (lst, v) in enumerate(zip(user_lists, user_values)):
        assert np.array_equal(v, V[u, lst])
    for i, (lst, v) in enumerate(zip(item_lists, item_values)):
        assert np.array_equal(v, V[lst, i])
    last = model.loss()
    worst = 0.0
    for half in range(6):
        if half % 2 == 0:
            fixed, lists, values = model.Q.cpu().numpy().copy(), user_lists, user_values
            model.solve_users()
            solved = model.P.cpu().numpy()
        else:
            fixed, lists, values = model.P.cpu().numpy().copy(), item_lists, item_values
            model.solve_items()
            solved = model.Q.cpu().numpy()
        G = an.gram32(fixed) if ob.dense else None               # on the operands this half-sweep read
        rho_ref = [aw.rho(aw.solve32(fixed, lst, v, ob, G), fixed, lst, v, ob) for lst, v in zip(lists, values)]
        ratio = max(aw.ratios(solved, fixed, lists, values, rho_ref, ob))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (half, ratio)
        now = model.loss()
        assert now <= last * (1.0 + 1e-6), (half, last, now)
        last = now
    print(f"ALS {objective} model: worst rho / threshold over 6 half-sweeps {worst:.4f}, loss {last:.6f}")

    # the closed form of loss() against the dense sum
    P, Q = model.P.cpu().numpy(), model.Q.cpu().numpy()
    if objective == "implicit":
        dense = aw.dense_loss_confidences(P, Q, V, stored, model.reg, model.alpha)
    else:
        dense = aw.dense_loss_explicit(P, Q, V, stored, model.reg)
    assert abs(last - dense) <= 1e-9 * abs(dense)

    grid = model.score_grid().cpu().numpy()
    rec = model.recommend(n=10, exclude=inter.pairs).cpu().numpy()
    masked = np.where(stored, -np.inf, grid)
    assert np.array_equal(rec, np.argsort(-masked, axis=1, kind="stable")[:, :10])
    assert not stored[np.arange(NUM_USERS)[:, None], rec].any()

    users, items = np.nonzero(stored)
    got = model.predict(users, items)
    assert got.dtype == torch.float32 and got.shape == (users.size,)
    assert torch.equal(got, (model.P[_dev(users)] * model.Q[_dev(items)]).sum(1))
    if objective == "explicit":                                  # three sweeps fit the ratings better than their mean
        rmse = float(np.sqrt(np.mean((got.cpu().numpy() - V[users, items]) ** 2)))
        assert rmse < float(np.std(V[users, items]))


def test_explicit_launches_no_gram(monkeypatch):
    _, ops = _pkg()
    model, *_ = _toy("explicit")

    def no_gram(*args, **kwargs):
        raise AssertionError("the explicit objective has no dense part: als_gram must not be launched")

    monkeypatch.setattr(ops, "als_gram", no_gram)
    model.sweep()
    model.fold_in(_fold_in_lists(model, [0, 3]))
    implicit, *_ = _toy("implicit")
    with pytest.raises(AssertionError):
        implicit.sweep()                                         # the patch does bite where there is a Gram


def _fold_in_lists(model, picked):
    """an Interactions of new users that copy the lists and values of ``picked``"""
    from deeplearningrecommendationsystem_amd.data import Interactions
    side = model._users
    indptr = side.pairs.indptr.cpu().numpy()
    at = np.concatenate([np.arange(indptr[u], indptr[u + 1]) for u in picked])
    new_users = np.concatenate([np.full(indptr[u + 1] - indptr[u], j) for j, u in enumerate(picked)]).astype(np.int64)
    at = _dev(at)
    return Interactions(_dev(new_users), side.pairs.indices[at].long(), side.values[at], len(picked), NUM_ITEMS,
                        duplicates="error")


@pytest.mark.parametrize("objective", ["implicit", "explicit"])
def test_fold_in_is_the_user_solve(objective):
    model, *_ = _toy(objective)
    model.sweep()
    P, Q = model.P.clone(), model.Q.clone()
    picked = [0, 17, 59]
    folded = model.fold_in(_fold_in_lists(model, picked))
    assert torch.equal(model.P, P) and torch.equal(model.Q, Q)            # untouched
    assert bool(folded.any()) and torch.equal(folded, model.solve_users(picked))
    assert model.solve_users() is None and torch.equal(model.P[picked], folded)


def test_implicit_model_still_takes_a_set_and_matches_the_unit_arm():
    """``fit(ObservedPairs)`` is the unit kernel: bitwise the row ``ops.als_solve_rows`` gives"""
    pkg, ops = _pkg()
    model, inter, *_ = _toy("implicit")
    unit = pkg.ALS(NUM_USERS, NUM_ITEMS, k=16, reg=0.1, alpha=40.0).fit(inter.pairs, sweeps=0)
    q = unit.Q.clone()
    unit.solve_users()
    want = ops.als_solve_rows(q, ops.als_gram(q), inter.pairs.indptr, inter.pairs.indices, 0.1, 40.0)
    assert torch.equal(unit.P, want)
    model.solve_users()
    assert not torch.equal(model.P, unit.P)                      # the confidences differ from the set's


# ------------------------------------------------------------------------------------------------------------ script
@pytest.mark.parametrize("objective", ["implicit", "explicit"])
def test_script_runs_and_the_loss_falls(objective):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "als_weighted.py"), "--objective", objective,
                          "--sweeps", "2", "--k", "16"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(line.split("loss")[1].split()[0]) for line in out.stdout.splitlines() if line.startswith("sweep")]
    assert len(losses) == 2 and losses[1] <= losses[0], out.stdout
