"""numpy restatement of the weighted row solve of csrc/als.hip (``ctr_als_solve_rows_weighted``) beside
tests/als_numpy.py, whose Cholesky, criterion constants and parity shapes it shares:

    (G + sum_e w_e y_e y_e^T + (reg + reg_per_entry n) I) x = sum_e t_e y_e
    w_e = fma(w1, v_e, w0),   t_e = fma(t1, v_e, t0),   n = the list length,   G = Y^T Y or 0

the float64 system, solve and the two losses; a float32 restatement with the longest chains any summation order can have
(sequential chains of (w_e x) x^T and t_e x in list order); and the same scaled residual
``rho(x) = max|A x - b| / (|Abar|_inf max|x| + max|bbar|)`` with ``Abar`` from ``|Y|`` and ``|w_e|`` and the same
diagonal, ``bbar = sum |t_e| |y_e|``, accepted when ``rho <= 4 rho_ref + 8u`` (``als_numpy.threshold``).
"""
from collections import namedtuple

import numpy as np

import als_numpy as an

F32 = np.float32
U = an.U

# one objective: the six scalars, whether the dense part G = Y^T Y is in the system, and how its values are drawn
Objective = namedtuple("Objective", "name w0 w1 t0 t1 reg reg_per_entry dense palette")

CONFIDENCE_VALUES = (0.0, 0.5, 1.0, 2.0, 3.0, 7.0, 20.0)
RATINGS = (1.0, 2.0, 3.0, 4.0, 5.0)


def confidences(alpha, reg):
    """c = 1 + alpha v, preference 1 on every stored pair"""
    return Objective(f"confidences({alpha:g}, {reg:g})", 0.0, alpha, 1.0, alpha, reg, 0.0, True, CONFIDENCE_VALUES)


def explicit(reg_per_entry):
    """least squares over the observed cells, the regulariser times the list length"""
    return Objective(f"explicit({reg_per_entry:g})", 1.0, 0.0, 0.0, 1.0, 0.0, reg_per_entry, False, RATINGS)


def unit(alpha, reg):
    """the unit-confidence system of als_numpy, for values that are all ones"""
    return Objective(f"unit({alpha:g}, {reg:g})", alpha, 0.0, 1.0 + alpha, 0.0, reg, 0.0, True, (1.0,))


PARITY_OBJECTIVES = [confidences(40.0, 0.1), confidences(1.0, 0.01), explicit(0.05)]


def fma32(a, x, b):
    """a * x + b of float32 operands: the product is exact in float64, so this is one rounding to 53 bits and one to
    24 -- a fused multiply-add up to that double rounding"""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(x, F32).astype(np.float64)
            + np.asarray(b, F32).astype(np.float64)).astype(F32)


# ---------------------------------------------------------------------------------------------------------- float64
def weights64(vals, ob):
    """(w, t) in float64 from the float32 weights the kernel forms"""
    vals = np.asarray(vals, dtype=F32)
    return (fma32(ob.w1, vals, ob.w0).astype(np.float64), fma32(ob.t1, vals, ob.t0).astype(np.float64))


def system64(Y, lst, vals, ob, G=None, absolute=False):
    """(A, b) in float64 from the (float32) inputs as they are; ``G``: Y^T Y when at hand.  ``absolute``: the
    comparison system (Abar, bbar) of the criterion -- pass |Y| (and its G)"""
    Y = np.asarray(Y, dtype=np.float64)
    k = Y.shape[1]
    X = Y[np.asarray(lst, dtype=np.int64)]
    w, t = weights64(vals, ob)
    if absolute:
        w, t = np.abs(w), np.abs(t)
    A = (X * w[:, None]).T @ X + (float(F32(ob.reg)) + float(F32(ob.reg_per_entry)) * len(lst)) * np.eye(k)
    if ob.dense:
        A = A + (Y.T @ Y if G is None else np.asarray(G, dtype=np.float64))
    return A, (X * t[:, None]).sum(0)


def solve64(Y, lst, vals, ob, G=None):
    if len(lst) == 0:
        return np.zeros(np.asarray(Y).shape[1])       # the kernel's rule: an empty list is exact zeros
    A, b = system64(Y, lst, vals, ob, G)
    return np.linalg.solve(A, b)


def half_sweep64(Y, lists, values, ob):
    Y = np.asarray(Y, dtype=np.float64)
    G = Y.T @ Y
    return np.stack([solve64(Y, lst, vals, ob, G) for lst, vals in zip(lists, values)])


def dense_loss_confidences(P, Q, V, stored, reg, alpha):
    """sum over ALL cells of c (y - s)^2 + reg(|P|^2 + |Q|^2), c = 1 + alpha v and y = 1 on the stored cells"""
    P, Q, V = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(V, np.float64)
    Yui = np.asarray(stored, np.float64)
    C = 1.0 + alpha * V * Yui
    return float((C * (Yui - P @ Q.T) ** 2).sum() + reg * ((P ** 2).sum() + (Q ** 2).sum()))


def loss_confidences(P, Q, users, items, vals, reg, alpha):
    """the closed form ALS.loss() takes: <P^T P, Q^T Q> + sum_obs((1 + alpha v)(1 - s)^2 - s^2) + reg(|P|^2 + |Q|^2)"""
    P, Q, vals = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(vals, np.float64)
    s = (P[users] * Q[items]).sum(1)
    return float(((P.T @ P) * (Q.T @ Q)).sum() + ((1.0 + alpha * vals) * (1.0 - s) ** 2 - s ** 2).sum()
                 + reg * ((P ** 2).sum() + (Q ** 2).sum()))


def dense_loss_explicit(P, Q, V, stored, reg):
    """sum over the stored cells of (v - s)^2, every row's and column's norm weighted by its count"""
    P, Q, V = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(V, np.float64)
    M = np.asarray(stored, np.float64)
    return float((M * (V - P @ Q.T) ** 2).sum()
                 + reg * ((M.sum(1) * (P ** 2).sum(1)).sum() + (M.sum(0) * (Q ** 2).sum(1)).sum()))


def loss_explicit(P, Q, users, items, vals, reg):
    """the closed form: sum_obs (v - s)^2 + reg (sum_u n_u |p_u|^2 + sum_i n_i |q_i|^2)"""
    P, Q, vals = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(vals, np.float64)
    s = (P[users] * Q[items]).sum(1)
    n_u, n_i = np.bincount(users, minlength=P.shape[0]), np.bincount(items, minlength=Q.shape[0])
    return float(((vals - s) ** 2).sum() + reg * ((n_u * (P ** 2).sum(1)).sum() + (n_i * (Q ** 2).sum(1)).sum()))


# ---------------------------------------------------------------------------------------------------------- float32
def solve32(Y, lst, vals, ob, G=None):
    """the float32 restatement of one row; ``G``: an.gram32(Y) when at hand"""
    Y = np.asarray(Y, dtype=F32)
    k = Y.shape[1]
    if len(lst) == 0:
        return np.zeros(k, dtype=F32)
    vals = np.asarray(vals, dtype=F32)
    w, t = fma32(ob.w1, vals, ob.w0), fma32(ob.t1, vals, ob.t0)
    S = np.zeros((k, k), dtype=F32)
    s = np.zeros(k, dtype=F32)
    for x, we, te in zip(Y[np.asarray(lst, dtype=np.int64)], w, t):
        S = (S + np.outer((we * x).astype(F32), x).astype(F32)).astype(F32)
        s = (s + (te * x).astype(F32)).astype(F32)
    A = S
    if ob.dense:
        A = ((an.gram32(Y) if G is None else np.asarray(G, dtype=F32)) + S).astype(F32)
    diag = fma32(ob.reg_per_entry, F32(len(lst)), ob.reg)
    A[np.diag_indices(k)] = (A[np.diag_indices(k)] + diag).astype(F32)
    return an.cholesky_solve32(A, s)


# ---------------------------------------------------------------------------------------------------------- criterion
def rho(x, Y, lst, vals, ob, G=None, Gabs=None):
    """the scaled residual against the float64 system built from the float32 inputs.  ``G`` / ``Gabs``: the float64
    Y^T Y and |Y|^T |Y| when at hand"""
    A, b = system64(Y, lst, vals, ob, G)
    Abar, bbar = system64(np.abs(np.asarray(Y, dtype=np.float64)), lst, vals, ob, Gabs, absolute=True)
    x = np.asarray(x, dtype=np.float64)
    den = np.abs(Abar).sum(1).max() * np.abs(x).max() + np.abs(bbar).max()
    num = np.abs(A @ x - b).max()
    if len(lst) == 0 or den == 0.0:      # an empty list and x = 0: solved exactly
        return 0.0 if not x.any() else float("inf")
    return float(num / den)


threshold = an.threshold


def case_values(lists, palette, seed):
    """one float32 array per list, drawn from ``palette``.  The values of a list of two or more entries are not all
    equal (replacing them by their mean would change nothing, and the margin against a kernel that ignores the values
    could not be asserted): where the draw is constant its first value moves to the next one of the palette."""
    rs = np.random.RandomState(seed)
    out = []
    for lst in lists:
        v = np.asarray(palette, dtype=F32)[rs.randint(0, len(palette), len(lst))]
        if len(palette) > 1 and len(v) >= 2 and (v == v[0]).all():
            v[0] = palette[(palette.index(float(v[0])) + 1) % len(palette)]
        out.append(v)
    return out


_CASES = {}


def parity_case(n, k, init, ob):
    """(Y, lists, values, rho_ref) of one weighted parity case: the table and lists of ``an.parity_case`` (both sides
    of every chunk boundary), values drawn from the objective's palette, and the restatement's own scaled residual on
    every list; made once and shared (nothing in it is written to afterwards).

    The seed of the values carries a ``+ 1``: without it the 95-entry list of (300, 128, uniform, confidences(40, 0.1))
    ends in an entry that the other 94 already predict at 1.025 = t_e / w_e, so that dropping it moves the residual
    to 0.45x the threshold only -- a case on which the criterion could not tell a dropped last entry.  With it (and
    with + 2 and + 3 alike) the worst dropped last entry is at 3.8x; tests/test_als_weighted_cpu.py asserts both
    margins on exactly these cases."""
    key = (n, k, init, ob)
    if key not in _CASES:
        Y, lists, _ = an.parity_case(n, k, init, *an.PARITY_PARAMS[0])
        values = case_values(lists, ob.palette, 77 * n + k + len(ob.name) + 1)
        G = an.gram32(Y) if ob.dense else None
        rho_ref = [rho(solve32(Y, lst, v, ob, G), Y, lst, v, ob) for lst, v in zip(lists, values)]
        for v in values:
            v.setflags(write=False)
        _CASES[key] = (Y, lists, values, rho_ref)
    return _CASES[key]


def ratios(X, Y, lists, values, rho_ref, ob):
    """rho(x) / threshold(rho_ref) of every row"""
    return [rho(x, Y, lst, v, ob) / threshold(r) for x, lst, v, r in zip(X, lists, values, rho_ref)]


def worst_ratio_many(X, Y, lists, values, ob):
    """(worst rho / threshold, rows that needed the restatement) over MANY rows of one table, as
    ``an.worst_ratio_many``: the restatement runs only for the rows above the 8u floor of every threshold"""
    Y64 = np.asarray(Y, dtype=np.float64)
    G, Gabs = Y64.T @ Y64, np.abs(Y64).T @ np.abs(Y64)
    G32 = None
    worst, slow = 0.0, 0
    for x, lst, v in zip(X, lists, values):
        r = rho(x, Y, lst, v, ob, G, Gabs)
        if r <= 8.0 * U:
            worst = max(worst, r / (8.0 * U))
            continue
        if ob.dense and G32 is None:
            G32 = an.gram32(Y)
        slow += 1
        worst = max(worst, r / threshold(rho(solve32(Y, lst, v, ob, G32), Y, lst, v, ob, G, Gabs)))
    return worst, slow


def csr(lists, values):
    indptr, indices = an.csr(lists)
    vals = np.concatenate([np.asarray(v, dtype=F32) for v in values]) if lists else np.zeros(0, F32)
    return indptr, indices, vals.astype(F32)
