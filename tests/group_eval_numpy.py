"""Numpy restatement of csrc/group_eval.hip, written from the definitions in the kernel file's header comment and built
on loader_numpy's perm / mix64 (no import of the package).

    candidates, row s:
        cand[s, 0]    = items[s]
        gseed_s       = mix64(seed ^ mix64(s * 0x100000001B3 + 5))                     (uint64 arithmetic, wrapping)
        q_t           = perm_{num_items}(gseed_s, 0, t),  t = 0 .. num_items - 1
        cand[s, 1..k] = the first k of q_0, q_1, .. that are neither items[s] nor observed for users[s];
                        -1 from the first slot that cannot be filled; all 0 for a user id outside [0, num_users)
    ranks:
        rank[g] = #{ j in 1..k : not (scores[g, j] < scores[g, 0]) }      hist[r] = #{ g : rank[g] == r }
    metrics, w_r = hist[r] / N, float64:
        HR@c = sum_{r<c} w_r     NDCG@c = sum_{r<c} w_r / log2(r + 2)     MRR@c = sum_{r<c} w_r / (r + 1)     MRR = MRR@(k+1)
"""
import numpy as np

from loader_numpy import U64, mix64, perm


def group_seed(seed, s):
    with np.errstate(over="ignore"):
        return int(mix64(U64(seed) ^ mix64(U64(s) * U64(0x100000001B3) + U64(5))))


def group_perm(seed, s, num_items):
    """q_0 .. q_{num_items - 1} of group s"""
    return perm(group_seed(seed, s), 0, np.arange(num_items), num_items)


def candidates(users, items, indptr, indices, num_users, num_items, k, seed):
    """-> (cand (N, 1 + k) int64, err, fail)"""
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    cand = np.empty((len(users), 1 + k), dtype=np.int64)
    err = fail = False
    nnz = len(indices)
    for s, (u, pos) in enumerate(zip(users, items)):
        cand[s, 0] = pos
        if u < 0 or u >= num_users:
            cand[s, 1:] = 0
            err = True
            continue
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        if lo < 0 or hi < lo or hi > nnz:
            err = True
            lo = hi = 0
        q = group_perm(seed, s, num_items)
        keep = q[(q != pos) & ~np.isin(q, np.asarray(indices[lo:hi], dtype=np.int64))][:k]
        cand[s, 1:1 + len(keep)] = keep
        if len(keep) < k:
            cand[s, 1 + len(keep):] = -1
            fail = True
    return cand, err, fail


def ranks(scores, k):
    """scores: anything that reshapes to (N, 1 + k) float32"""
    s = np.asarray(scores, dtype=np.float32).reshape(-1, 1 + k)
    with np.errstate(invalid="ignore"):
        return (~(s[:, 1:] < s[:, :1])).sum(axis=1).astype(np.int32)


def histogram(rank, k):
    return np.bincount(np.asarray(rank, dtype=np.int64), minlength=k + 1).astype(np.int64)


def metrics(hist, cutoffs):
    """-> (hr, ndcg, mrr_at: dicts by cutoff; mrr) in float64"""
    hist = np.asarray(hist, dtype=np.int64)
    n = int(hist.sum())
    w = hist.astype(np.float64) / n
    r = np.arange(len(hist), dtype=np.float64)
    hr, ndcg, mrr_at = {}, {}, {}
    for c in cutoffs:
        hr[c] = float(np.sum(w[:c]))
        ndcg[c] = float(np.sum(w[:c] / np.log2(r[:c] + 2.0)))
        mrr_at[c] = float(np.sum(w[:c] / (r[:c] + 1.0)))
    return hr, ndcg, mrr_at, float(np.sum(w / (r + 1.0)))
