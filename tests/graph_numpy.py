"""float64 restatement of the graph propagation (csrc/graph_prop.hip) and of LightGCN (model/lightgcn.py), the kernel's
constants, and the case builders the CPU and GPU tests share.  A helper, not a test."""
import functools

import numpy as np

U = 2.0 ** -24                 # unit roundoff of float32
SEGMENT = 512                  # CTR_GRAPH_SEGMENT: a list is cut every SEGMENT entries from its own start
UNROLL = 4                     # wave-instructions of row loads in flight
KS = (16, 48, 64, 256)         # the parity widths: 16, 5 (four idle lanes), 4 and 1 entries per wave-instruction


def entries_per_instruction(k):
    """list entries one wave-instruction of 16-byte loads covers: a row is k / 4 lanes wide"""
    return 64 // (k // 4)


def gamma(m):
    return m * U / (1.0 - m * U)


# ------------------------------------------------------------------------------------------------------ one propagation
def propagate64(x, indptr, indices, s_in=None, s_out=None, rows=None, skip=()):
    """(out, mag) in float64: out[j] = s_out[r] sum_e s_in[idx_e] x[idx_e], r = rows[j], and the magnitude
    mag[j] = |s_out[r]| sum_e |s_in[idx_e] x[idx_e]| the error bound is stated in.  Entries whose index is outside the
    table add nothing; positions of ``indices`` listed in ``skip`` neither."""
    x = np.asarray(x, dtype=np.float64)
    num_rows = len(indptr) - 1
    rows = np.arange(num_rows) if rows is None else np.asarray(rows)
    si = np.ones(x.shape[0]) if s_in is None else np.asarray(s_in, dtype=np.float64)
    so = np.ones(num_rows) if s_out is None else np.asarray(s_out, dtype=np.float64)
    out, mag = np.zeros((len(rows), x.shape[1])), np.zeros((len(rows), x.shape[1]))
    skip = set(skip)
    for j, r in enumerate(rows):
        at = [e for e in range(indptr[r], indptr[r + 1]) if e not in skip and 0 <= indices[e] < x.shape[0]]
        idx = np.asarray(indices)[at].astype(np.int64)
        terms = si[idx, None] * x[idx]
        out[j] = so[r] * terms.sum(0)
        mag[j] = abs(so[r]) * np.abs(terms).sum(0)
    return out, mag


def bound(indptr, mag, rows=None):
    """elementwise: gamma(n + 2) mag, n the list length -- n additions in any order, the two scales"""
    n = np.diff(indptr)
    n = n if rows is None else n[np.asarray(rows)]
    return gamma(n + 2.0)[:, None] * mag


def worst_ratio(got, ref, limit):
    """max |got - ref| / limit; an element whose limit is 0 must be exact"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if (err[limit == 0.0] != 0.0).any():
        return np.inf
    return float((err[limit > 0.0] / limit[limit > 0.0]).max()) if (limit > 0.0).any() else 0.0


def dense_adjacency(indptr, indices, num_cols):
    a = np.zeros((len(indptr) - 1, num_cols))
    for r in range(len(indptr) - 1):
        for e in range(indptr[r], indptr[r + 1]):
            a[r, indices[e]] += 1.0
    return a


def transpose_csr(indptr, indices, num_cols):
    """the CSR of the transposed matrix, lists ascending"""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    order = np.lexsort((rows, indices))
    t_indptr = np.zeros(num_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=num_cols), out=t_indptr[1:])
    return t_indptr, rows[order].astype(np.int32)


# ------------------------------------------------------------------------------------------------------ kernel cases
def list_lengths():
    """the lengths of the parity CSR: empty and tiny lists, around the entries per wave-instruction and its unrolled
    multiple at every width of KS, 63 / 64 / 65, around one and two segments, and one list of five segments and a bit"""
    lengths = [0, 1, 2, 3, 63, 64, 65, SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT, 2 * SEGMENT + 1]
    for k in KS:
        e = entries_per_instruction(k)
        lengths += [e - 1, e, e + 1, UNROLL * e - 1, UNROLL * e, UNROLL * e + 1]
    return sorted(set(n for n in lengths if n >= 0)) + [5 * SEGMENT + 7]


X_ROWS, X_UNNAMED = 700, 50      # the parity table; its last X_UNNAMED rows are named by no list


@functools.lru_cache(maxsize=None)
def parity_csr():
    """(indptr int64, indices int32): one CSR with every length of ``list_lengths``, shuffled, indices into the first
    X_ROWS - X_UNNAMED rows"""
    rs = np.random.RandomState(11)
    lengths = np.asarray(list_lengths())[rs.permutation(len(list_lengths()))]
    indptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    indices = rs.randint(0, X_ROWS - X_UNNAMED, int(indptr[-1])).astype(np.int32)
    return indptr, indices


@functools.lru_cache(maxsize=None)
def parity_inputs(k, scaled):
    """(x float32, s_in, s_out): x ~ N(0, 1); the scales uniform in [0.05, 1], or None"""
    rs = np.random.RandomState(100 + k)
    x = rs.normal(0.0, 1.0, (X_ROWS, k)).astype(np.float32)
    if not scaled:
        return x, None, None
    num_rows = len(parity_csr()[0]) - 1
    return x, rs.uniform(0.05, 1.0, X_ROWS).astype(np.float32), rs.uniform(0.05, 1.0, num_rows).astype(np.float32)


@functools.lru_cache(maxsize=None)
def many_rows_csr():
    """3000 rows of 0 to 40 entries over a 1000-row table"""
    rs = np.random.RandomState(12)
    lengths = rs.randint(0, 41, 3000)
    indptr = np.zeros(3001, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    return indptr, rs.randint(0, 1000, int(indptr[-1])).astype(np.int32)


# ------------------------------------------------------------------------------------------------------ the model
GRAPHS = {"small": (37, 23, 150), "large": (300, 200, 4000)}


@functools.lru_cache(maxsize=None)
def model_graph(name):
    """(num_users, num_items, users, items): distinct pairs sorted by user then item.  "large": item 0 is held by every
    user that has a pair, and users 5 and 17 have none."""
    num_users, num_items, pairs = GRAPHS[name]
    rs = np.random.RandomState(len(name))
    if name == "small":
        cells = rs.choice(num_users * num_items, pairs, replace=False)
        users, items = cells // num_items, cells % num_items
    else:
        active = np.setdiff1d(np.arange(num_users), (5, 17))
        cells = rs.choice(len(active) * (num_items - 1), pairs - len(active), replace=False)
        users = np.concatenate([active, active[cells // (num_items - 1)]])
        items = np.concatenate([np.zeros(len(active), dtype=np.int64), 1 + cells % (num_items - 1)])
    order = np.lexsort((items, users))
    return num_users, num_items, users[order].astype(np.int64), items[order].astype(np.int64)


def normalised_adjacency(num_users, num_items, users, items):
    """the symmetric (U + I, U + I) operator [[0, S_U R S_I], [S_I R^T S_U, 0]], d^-1/2 with 0 for d = 0"""
    r = np.zeros((num_users, num_items))
    r[users, items] = 1.0
    with np.errstate(divide="ignore"):
        su = np.where(r.sum(1) > 0, r.sum(1) ** -0.5, 0.0)
        si = np.where(r.sum(0) > 0, r.sum(0) ** -0.5, 0.0)
    a = su[:, None] * r * si[None, :]
    n = num_users + num_items
    full = np.zeros((n, n))
    full[:num_users, num_users:] = a
    full[num_users:, :num_users] = a.T
    return full


def mean_of_layers(adj, layers):
    """M with F = M E^(0): the mean of adj^0 .. adj^layers"""
    m, power = np.eye(adj.shape[0]), np.eye(adj.shape[0])
    for _ in range(layers):
        power = adj @ power
        m = m + power
    return m / (layers + 1)


def horner_backward(adj, layers, gf):
    """the model's backward: g <- gF / (L + 1) + adj g, L times"""
    g0 = gf / (layers + 1)
    g = g0
    for _ in range(layers):
        g = g0 + adj @ g
    return g


def model64(w_u, w_i, graph, layers, users, items, weights):
    """(prob, grad of sum(weights * prob) in W_U, the same in W_I), float64, through the dense operator.  The
    gradient goes through the explicit transpose of the mean-of-layers matrix: no symmetry is assumed here."""
    num_users, num_items, gu, gi = graph
    m = mean_of_layers(normalised_adjacency(num_users, num_items, gu, gi), layers)
    e0 = np.concatenate([np.asarray(w_u, dtype=np.float64), np.asarray(w_i, dtype=np.float64)])
    f = m @ e0
    f_u, f_i = f[:num_users], f[num_users:]
    prob = 1.0 / (1.0 + np.exp(-(f_u[users] * f_i[items]).sum(1)))
    gz = np.asarray(weights, dtype=np.float64) * prob * (1.0 - prob)
    gf = np.zeros_like(f)
    np.add.at(gf, users, gz[:, None] * f_i[items])
    np.add.at(gf, num_users + items, gz[:, None] * f_u[users])
    ge = m.T @ gf
    return prob, ge[:num_users], ge[num_users:]


def model_batch(graph, seed=3, size=257):
    """257 (user, item) pairs with repeats and a weight per pair"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, graph[0], size), rs.randint(0, graph[1], size), rs.normal(0.0, 1.0, size)
