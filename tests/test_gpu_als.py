"""GPU: ALS (csrc/als.hip) against the restatement tests/als_numpy.py -- the Gram against float64 with a bound that
holds for any summation order, the row solves by the scaled residual against the float32 restatement's own
(rho <= 4 rho_ref + 8u) on the edge-length lists and on 3000 rows in one launch, locality and determinism (bitwise),
the guards, memory, the model and the script.

Every parity check prints its worst rho / threshold; the worst seen on the MI355X is quoted in DESIGN.md section 4s."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import als_numpy as an

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import deeplearningrecommendationsystem_amd as pkg
    from deeplearningrecommendationsystem_amd import ops
    return pkg, ops


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared cases are read-only


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _solve(Y, lists, reg, alpha, gram=None, rows=None, flag=None):
    """(rows of x as a device tensor, flag value) of one als_solve_rows call over the CSR of ``lists``"""
    _, ops = _pkg()
    y = _dev(Y)
    indptr, indices = an.csr(lists)
    gram = ops.als_gram(y) if gram is None else gram
    flag = _flag() if flag is None else flag
    out = ops.als_solve_rows(y, gram, _dev(indptr), _dev(indices), reg, alpha,
                             rows=None if rows is None else _dev(np.asarray(rows, dtype=np.int64)), err_flag=flag)
    return out, int(flag.item())


# ------------------------------------------------------------------------------------------------------------ Gram
@pytest.mark.parametrize("k", [16, 128])
@pytest.mark.parametrize("rows", [1, an.SLAB - 1, an.SLAB, an.SLAB + 1, 2 * an.SLAB - 1, 2 * an.SLAB, 2 * an.SLAB + 1,
                                  1682])
def test_gram_against_float64(rows, k):
    _, ops = _pkg()
    rs = np.random.RandomState(rows + k)
    Y = rs.normal(0.0, 1.0, (rows, k)).astype(np.float32)
    y = _dev(Y)
    g1, g2 = ops.als_gram(y), ops.als_gram(y)
    assert torch.equal(g1, g2)                                # no atomics: bitwise reproducible
    G = g1.cpu().numpy()
    assert np.array_equal(G, G.T)
    Y64 = Y.astype(np.float64)
    bound = rows * an.U * (np.abs(Y64).T @ np.abs(Y64))       # holds for any summation order
    err = np.abs(G - Y64.T @ Y64)
    print(f"als_gram rows {rows} k {k}: worst error / bound {(err / bound).max():.4f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------------------ solves
@pytest.mark.parametrize("alpha,reg", an.PARITY_PARAMS)
@pytest.mark.parametrize("init", an.PARITY_INITS)
@pytest.mark.parametrize("n,k", an.PARITY_SHAPES)
def test_solve_parity(n, k, init, alpha, reg):
    Y, lists, rho_ref = an.parity_case(n, k, init, alpha, reg)
    out, bits = _solve(Y, lists, reg, alpha)
    X = out.cpu().numpy()
    assert bits == 0 and np.isfinite(X).all()
    assert not X[0].any()                                     # the empty list: exact zeros
    ratios = [an.rho(x, Y, lst, reg, alpha) / an.threshold(r) for x, lst, r in zip(X, lists, rho_ref)]
    print(f"als_solve_rows n {n} k {k} {init} alpha {alpha} reg {reg}: worst rho / threshold {max(ratios):.4f} "
          f"(list length {len(lists[int(np.argmax(ratios))])})")
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("k", [64, 128])
def test_solve_parity_many_rows_in_one_launch(k):
    """3000 rows in ONE launch: more rows than the device holds workgroups at once (four a CU at k = 64, two at
    k = 128), every one held to the criterion, and again as a permuted launch, bitwise"""
    n, rows, alpha, reg = 1000, 3000, 40.0, 0.1
    rs = np.random.RandomState(k)
    Y = an.case_table(n, k, "normal", 50 + k)
    lists = [np.sort(rs.choice(n, rs.randint(0, 41), replace=False)).astype(np.int64) for _ in range(rows)]
    out, bits = _solve(Y, lists, reg, alpha)
    X = out.cpu().numpy()
    assert bits == 0 and np.isfinite(X).all()
    empty = [r for r, lst in enumerate(lists) if len(lst) == 0]
    assert empty and not X[empty].any()
    assert all(X[r].any() for r, lst in enumerate(lists) if len(lst))      # no row was silently zeroed
    worst, slow = an.worst_ratio_many(X, Y, lists, reg, alpha)
    print(f"als_solve_rows {rows} rows in one launch, k {k}: worst rho / threshold {worst:.4f} "
          f"({slow} rows needed the restatement)")
    assert worst <= 1.0
    perm = np.random.RandomState(1).permutation(rows)
    permuted, bits = _solve(Y, lists, reg, alpha, rows=perm)
    assert bits == 0 and torch.equal(permuted, out[_dev(perm)])


def test_locality_and_determinism():
    n, k, alpha, reg = 200, 64, 40.0, 0.1
    Y, lists, _ = an.parity_case(n, k, "uniform", alpha, reg)
    _, ops = _pkg()
    gram = ops.als_gram(_dev(Y))
    every, _ = _solve(Y, lists, reg, alpha, gram)
    again, _ = _solve(Y, lists, reg, alpha, gram)
    assert torch.equal(every, again)
    count = len(lists)
    explicit, _ = _solve(Y, lists, reg, alpha, gram, rows=np.arange(count))
    assert torch.equal(every, explicit)
    perm = np.random.RandomState(3).permutation(count)
    permuted, _ = _solve(Y, lists, reg, alpha, gram, rows=perm)
    assert torch.equal(permuted, every[_dev(perm)])
    repeats = np.array([5, 5, count - 1, 0, 5, count - 1, 2])
    repeated, _ = _solve(Y, lists, reg, alpha, gram, rows=repeats)
    assert torch.equal(repeated, every[_dev(repeats)])
    for row in (0, 4, count - 1):
        single, _ = _solve(Y, lists, reg, alpha, gram, rows=[row])
        assert torch.equal(single[0], every[row])


# ------------------------------------------------------------------------------------------------------------ guards
@pytest.mark.parametrize("bad", ["y_rows", -1])
def test_bad_index_is_never_read(bad):
    n, k, alpha, reg = 65, 16, 40.0, 0.1
    Y, lists, _ = an.parity_case(n, k, "normal", alpha, reg)
    clean, _ = _solve(Y, lists, reg, alpha)
    row = 5                                                   # a list of 33 entries: the bad index sits in its first chunk
    broken = [lst.copy() for lst in lists]
    broken[row][len(broken[row]) // 2] = n if bad == "y_rows" else -1
    out, bits = _solve(Y, broken, reg, alpha)
    _, ops = _pkg()
    assert bits == ops.ALS_ERR_INDEX
    assert not out[row].any()
    keep = [r for r in range(len(lists)) if r != row]
    assert torch.equal(out[keep], clean[keep])


def test_bad_row_id_is_never_read():
    n, k, alpha, reg = 65, 16, 40.0, 0.1
    Y, lists, _ = an.parity_case(n, k, "normal", alpha, reg)
    clean, _ = _solve(Y, lists, reg, alpha)
    out, bits = _solve(Y, lists, reg, alpha, rows=[3, len(lists), -1, 4])
    assert bits == 1
    assert not out[1].any() and not out[2].any()
    assert torch.equal(out[0], clean[3]) and torch.equal(out[3], clean[4])


def test_offsets_that_run_backwards_are_flagged():
    _, ops = _pkg()
    Y, lists, _ = an.parity_case(65, 16, "normal", 40.0, 0.1)
    indptr, indices = an.csr(lists)
    clean, _ = _solve(Y, lists, 0.1, 40.0)
    indptr = indptr.copy()
    indptr[3] = indptr[2] - 1                                 # row 2 runs backwards; row 3 starts one entry early
    flag = _flag()
    y = _dev(Y)
    out = ops.als_solve_rows(y, ops.als_gram(y), _dev(indptr), _dev(indices), 0.1, 40.0, err_flag=flag)
    assert int(flag.item()) == ops.ALS_ERR_INDEX
    assert not out[2].any() and bool(torch.isfinite(out).all())
    assert torch.equal(out[4:], clean[4:])


def test_model_raises_index_error_on_a_bad_pair():
    pkg, _ = _pkg()
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    rs = np.random.RandomState(0)
    u, i = _dev(rs.randint(0, 20, 100)), _dev(rs.randint(0, 30, 100))
    model = pkg.ALS(20, 30, k=16).fit(ObservedPairs(u, i, 20, 30), sweeps=0)
    model._users.pairs.indices[3] = 30
    with pytest.raises(IndexError):
        model.solve_users()
    assert int(model._flag.item()) == 0                        # read once and cleared


def test_pivot_guard_zero_system():
    _, ops = _pkg()
    Y = np.zeros((40, 16), dtype=np.float32)
    lists = [np.arange(0), np.arange(3), np.arange(40)]
    out, bits = _solve(Y, lists, 0.0, 40.0)
    assert bits == ops.ALS_ERR_PIVOT
    assert not out.any() and bool(torch.isfinite(out).all())


def test_pivot_guard_nan_in_the_table():
    n, k, alpha, reg = 200, 48, 1.0, 0.01
    Y, lists, _ = an.parity_case(n, k, "uniform", alpha, reg)
    _, ops = _pkg()
    gram = ops.als_gram(_dev(Y))                               # of the clean table
    clean, _ = _solve(Y, lists, reg, alpha, gram)
    poisoned = Y.copy()
    victim = int(lists[4][0])
    poisoned[victim, 7] = np.nan
    out, bits = _solve(poisoned, lists, reg, alpha, gram)
    assert bits == ops.ALS_ERR_PIVOT
    assert bool(torch.isfinite(out).all())
    hit = [r for r, lst in enumerate(lists) if victim in lst]
    miss = [r for r in range(len(lists)) if r not in hit]
    assert len(hit) >= 2 and len(miss) >= 2
    assert not out[hit].any()
    assert torch.equal(out[miss], clean[miss])


def test_count_zero_launches_nothing():
    _, ops = _pkg()
    from deeplearningrecommendationsystem_amd import _lib
    lib = _lib.load()
    assert lib.ctr_als_solve_rows(None, 1, 16, None, None, None, 1, None, 0, 0.1, 1.0, None, 16, None, None) == 0
    Y, lists, _ = an.parity_case(65, 16, "normal", 40.0, 0.1)
    out, bits = _solve(Y, lists, 0.1, 40.0, rows=np.zeros(0, dtype=np.int64))
    assert out.shape == (0, 16) and bits == 0


# ------------------------------------------------------------------------------------------------------------ memory
def test_no_rows_by_k_by_k_tensor():
    _, ops = _pkg()
    rows, k, n = 4096, 128, 1000
    rs = np.random.RandomState(1)
    y = _dev(rs.normal(0.0, 0.1, (n, k)).astype(np.float32))
    lens = rs.randint(0, 40, rows)
    indptr = _dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    indices = _dev(rs.randint(0, n, int(lens.sum())).astype(np.int32))
    flag = _flag()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    gram = ops.als_gram(y)
    out = ops.als_solve_rows(y, gram, indptr, indices, 0.1, 40.0, err_flag=flag)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    allowed = out.numel() * 4 + gram.numel() * 4 + ops.als_gram_workspace_bytes(n, k) + (1 << 20)
    print(f"als memory: peak grew {grew} B, allowed {allowed} B, a (rows, k, k) batch {rows * k * k * 4} B")
    assert grew <= allowed
    assert int(flag.item()) == 0 and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------ model
def _toy():
    """ALS(70, 130, k=16) on about 900 random pairs, with one held-out item per user"""
    pkg, _ = _pkg()
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    rs = np.random.RandomState(11)
    num_users, num_items = 70, 130
    cells = rs.choice(num_users * num_items, 900, replace=False)
    users, items = cells // num_items, cells % num_items
    taken = np.zeros((num_users, num_items), dtype=bool)
    taken[users, items] = True
    test_items = np.array([rs.choice(np.flatnonzero(~taken[u])) for u in range(num_users)])
    observed = ObservedPairs(_dev(users.astype(np.int64)), _dev(items.astype(np.int64)), num_users, num_items)
    model = pkg.ALS(num_users, num_items, k=16).fit(observed, sweeps=0)
    return model, observed, taken, test_items


def _lists_of(pairs):
    indptr, indices = pairs.indptr.cpu().numpy(), pairs.indices.cpu().numpy()
    return [indices[indptr[r]:indptr[r + 1]].astype(np.int64) for r in range(len(indptr) - 1)]


def test_model_sweeps_recommend_and_metrics():
    from deeplearningrecommendationsystem_amd.evaluator.ranking import ranking_metrics
    model, observed, taken, test_items = _toy()
    user_lists, item_lists = _lists_of(model._users.pairs), _lists_of(model._items.pairs)
    assert sum(len(lst) for lst in user_lists) == 900 == sum(len(lst) for lst in item_lists)
    last = model.loss()
    worst = 0.0
    for half in range(6):
        if half % 2 == 0:
            fixed, lists = model.Q.cpu().numpy().copy(), user_lists
            model.solve_users()
            solved = model.P.cpu().numpy()
        else:
            fixed, lists = model.P.cpu().numpy().copy(), item_lists
            model.solve_items()
            solved = model.Q.cpu().numpy()
        ref = an.half_sweep32(fixed, lists, model.reg, model.alpha)     # on the operands this half-sweep read
        rho_ref = [an.rho(x, fixed, lst, model.reg, model.alpha) for x, lst in zip(ref, lists)]
        ratio = an.worst_ratio(solved, fixed, lists, rho_ref, model.reg, model.alpha)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (half, ratio)
        now = model.loss()
        assert now <= last * (1.0 + 1e-6), (half, last, now)
        last = now
    print(f"ALS model: worst rho / threshold over 6 half-sweeps {worst:.4f}, loss {last:.6f}")

    # the closed form of loss() against the dense sum
    P, Q = model.P.cpu().numpy(), model.Q.cpu().numpy()
    dense = an.dense_loss(P, Q, taken, model.reg, model.alpha)
    assert abs(last - dense) <= 1e-9 * abs(dense)

    grid = model.score_grid().cpu().numpy()
    assert np.array_equal(grid, model.score_rows(0, 70).cpu().numpy())
    rec = model.recommend(n=10, exclude=observed).cpu().numpy()
    masked = np.where(taken, -np.inf, grid)
    want = np.argsort(-masked, axis=1, kind="stable")[:, :10]
    assert np.array_equal(rec, want)
    assert not taken[np.arange(70)[:, None], rec].any()

    users = np.arange(70, dtype=np.int64)
    m = ranking_metrics(model.score_rows, (_dev(users), _dev(test_items.astype(np.int64))), 10,
                        exclude=((_dev(np.nonzero(taken)[0]), _dev(np.nonzero(taken)[1])),), num_users=70)
    assert all(np.isfinite(v) for v in (m.precision, m.recall, m.map, m.ndcg, m.mrr))


def test_fold_in_is_the_user_solve():
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    model, observed, taken, _ = _toy()
    model.sweep()
    P, Q = model.P.clone(), model.Q.clone()
    picked = [0, 17, 69]
    new_users = np.concatenate([np.full(int(taken[u].sum()), j) for j, u in enumerate(picked)]).astype(np.int64)
    new_items = np.concatenate([np.flatnonzero(taken[u]) for u in picked]).astype(np.int64)
    folded = model.fold_in(ObservedPairs(_dev(new_users), _dev(new_items), len(picked), 130))
    assert torch.equal(model.P, P) and torch.equal(model.Q, Q)            # untouched
    assert torch.equal(folded, model.solve_users(picked))
    assert model.solve_users() is None and torch.equal(model.P[picked], folded)      # all rows: stored, not returned


def test_calls_before_fit_and_bad_ids():
    pkg, _ = _pkg()
    model = pkg.ALS(20, 30, k=16)
    for call in (model.sweep, model.solve_users, model.solve_items, model.loss):
        with pytest.raises(RuntimeError):
            call()
    fitted, *_ = _toy()
    with pytest.raises(IndexError):
        fitted.solve_users([0, 70])
    with pytest.raises(IndexError):
        fitted.solve_items([-1])


# ------------------------------------------------------------------------------------------------------------ script
def test_script_runs_and_the_loss_falls():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "als.py"), "--sweeps", "2", "--k", "16"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(line.split("loss")[1].split()[0]) for line in out.stdout.splitlines() if line.startswith("sweep")]
    assert len(losses) == 2 and losses[1] <= losses[0], out.stdout
