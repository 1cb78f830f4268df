"""numpy restatement of the score-level evaluation, written from the definitions in the header comment of
csrc/score_eval.hip (not from the kernels): the class rule, ctr_score_counts' counts and float64 chunk sums,
ctr_gauc_groups' integer counts, the UserGroups plan and the float64 GAUC composition.  Shared by test_score_cpu.py,
which pins it to sklearn, and test_gpu_score.py, which compares the kernels with it."""
import numpy as np

CHUNK, SMALL, SLAB = 65536, 64, 1024
FIXED_SIZES = [1, 2, 2, 3, 63, 64, 65, 127, 1023, 1024, 1025, 2049, 3000]


def positive(y):
    """target > 0.5 in float32; a NaN target is negative"""
    with np.errstate(invalid="ignore"):
        return np.asarray(y, dtype=np.float32) > np.float32(0.5)


def hard(p):
    with np.errstate(invalid="ignore"):
        return np.asarray(p, dtype=np.float32) >= np.float32(0.5)


# -- ctr_score_counts ------------------------------------------------------------------------------------------------
def counts(p, y):
    """{positives, negatives, tp, fp, fn, tn, bad, 0}"""
    p = np.asarray(p, dtype=np.float32)
    pos, hd = positive(y), hard(p)
    with np.errstate(invalid="ignore"):
        inside = (p >= 0) & (p <= 1)
    return np.array([pos.sum(), (~pos).sum(), (pos & hd).sum(), (~pos & hd).sum(), (pos & ~hd).sum(),
                     (~pos & ~hd).sum(), (~inside).sum(), 0], dtype=np.int64)


def bce_terms(p, y):
    """-(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) in float64; the max drops a NaN (fmax)"""
    p, y = np.asarray(p, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        lp = np.fmax(np.log(p), -100.0)
        l1p = np.fmax(np.log(1.0 - p), -100.0)
    return -(y * lp + (1.0 - y) * l1p)


def chunk_sums(p, y):
    """(ceil(n / CHUNK), 4) float64: sum BCE term, sum p, sum (p - y)^2, sum y of every chunk"""
    p, y = np.asarray(p, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n = p.shape[0]
    rows = np.zeros((-(-n // CHUNK), 4), dtype=np.float64)
    terms = bce_terms(p, y)
    p64, y64 = p.astype(np.float64), y.astype(np.float64)
    for c in range(rows.shape[0]):
        s = slice(c * CHUNK, min(n, (c + 1) * CHUNK))
        rows[c] = [terms[s].sum(), p64[s].sum(), ((p64[s] - y64[s]) ** 2).sum(), y64[s].sum()]
    return rows


# -- the plan --------------------------------------------------------------------------------------------------------
def user_groups(users):
    """dict of the UserGroups attributes: groups by ascending user id, the samples of a group in sample order"""
    users = np.asarray(users, dtype=np.int64)
    order = np.argsort(users, kind="stable")
    group_users, sizes = np.unique(users, return_counts=True)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    small = np.flatnonzero(sizes <= SMALL)
    slab_group, slab_first = [], []
    for g in np.flatnonzero(sizes > SMALL):
        for first in range(0, int(sizes[g]), SLAB):
            slab_group.append(g)
            slab_first.append(first)
    return dict(order=order.astype(np.int32), offsets=offsets, group_users=group_users, sizes=sizes,
                small_groups=small.astype(np.int32), slab_group=np.array(slab_group, dtype=np.int32),
                slab_first=np.array(slab_first, dtype=np.int32))


# -- ctr_gauc_groups -------------------------------------------------------------------------------------------------
def group_counts(p, y, order, offsets):
    """(pos, neg, u2, err): u2[g] = sum over (positive i, negative j) of 2 [p_j < p_i] + [p_j == p_i], IEEE compares;
    an order entry outside [0, n) is skipped and sets err"""
    p, y = np.asarray(p, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n, groups = p.shape[0], len(offsets) - 1
    pos, neg = np.zeros(groups, dtype=np.int32), np.zeros(groups, dtype=np.int32)
    u2, err = np.zeros(groups, dtype=np.int64), 0
    cls = positive(y)
    for g in range(groups):
        members = np.asarray(order[offsets[g]:offsets[g + 1]], dtype=np.int64)
        ok = (members >= 0) & (members < n)
        err |= int((~ok).any())
        members = members[ok]
        s, t = p[members][cls[members]], p[members][~cls[members]]
        pos[g], neg[g] = s.shape[0], t.shape[0]
        with np.errstate(invalid="ignore"):
            u2[g] = 2 * int((t[None, :] < s[:, None]).sum()) + int((t[None, :] == s[:, None]).sum())
    return pos, neg, u2, err


def gauc(pos, neg, u2):
    """(GAUC, unweighted mean of the user AUCs, users scored, samples scored) in float64"""
    pos, neg, u2 = (np.asarray(t, dtype=np.int64) for t in (pos, neg, u2))
    keep = (pos > 0) & (neg > 0)
    if not keep.any():
        return float("nan"), float("nan"), 0, 0
    auc = u2[keep] / (2.0 * pos[keep].astype(np.float64) * neg[keep].astype(np.float64))
    w = (pos[keep] + neg[keep]).astype(np.float64)
    return float((w * auc).sum() / w.sum()), float(auc.mean()), int(keep.sum()), int((pos[keep] + neg[keep]).sum())


# -- inputs ----------------------------------------------------------------------------------------------------------
def recipe():
    """the mixed input of the tests: (users, y, p) of 12 697 permuted samples in 213 groups -- the sizes around the
    small / slab thresholds plus 200 sizes from [1, 40), labels Bernoulli(0.3), every second group's scores rounded to
    sixteenths (ties), and the groups that have no AUC or a known one"""
    gen = np.random.default_rng(0)
    sizes = FIXED_SIZES + gen.integers(1, 40, 200).tolist()
    ids = gen.choice(10 ** 6, len(sizes), replace=False)
    users, ys, ps = [], [], []
    twos = 0
    for k, size in enumerate(sizes):
        y = (gen.random(size) < 0.3).astype(np.float32)
        p = gen.random(size, dtype=np.float32)
        if k % 2:
            p = np.round(p * 16) / np.float32(16)
        if k < len(FIXED_SIZES):
            if size == 2:
                y = np.array([[1, 0], [1, 1]][twos], dtype=np.float32)     # one scorable pair, one group all positive
                twos += 1
            elif size == 63:
                y[:] = 0                                                   # all negative
            elif size == 1025:
                p[:] = 0.5                                                 # constant: AUC 0.5 exactly
            elif size == 127:
                p[gen.choice(size, 5, replace=False)] = np.nan
        users.append(np.full(size, ids[k], dtype=np.int64))
        ys.append(y)
        ps.append(p.astype(np.float32))
    users, y, p = np.concatenate(users), np.concatenate(ys), np.concatenate(ps)
    perm = gen.permutation(users.shape[0])
    return users[perm], y[perm], p[perm]


SPECIALS = np.array([0.0, -0.0, 1.0, np.nan, -0.25, 1.5, np.inf, -np.inf], dtype=np.float32)


def with_specials(p, seed, every=7):
    """a copy of p with about one score in ``every`` replaced by +-0.0, 1.0, NaN or a value outside [0, 1]"""
    gen = np.random.default_rng(seed)
    p = np.array(p, dtype=np.float32)
    at = np.flatnonzero(gen.integers(0, every, p.shape[0]) == 0)
    p[at] = SPECIALS[gen.integers(0, SPECIALS.shape[0], at.shape[0])]
    return p
