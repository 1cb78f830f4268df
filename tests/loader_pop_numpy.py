"""Numpy restatement of the weighted negatives of csrc/loader.hip (ctr_load_batch_neg_pop, ctr_load_batch_groups_pop),
written from the definition in the kernel file's header comment and from nothing else (no import of the package);
perm / mix64 are loader_numpy's.

    table[c] = (thresh_c << 32) | alias_c;   a column that always keeps itself has alias_c == c
    slot v of user u, try t:
        h      = mix64(nkey ^ mix64(v * 0x100000001B3 + t)),   nkey = mix64(seed ^ mix64(e * 0x100000001B3 + 4))
        col    = ((h >> 32) * num_items) >> 32
        item_t = (h & 0xffffffff) < thresh_col ? col : alias_col
        item   = item_t for the first t < 2^14 with (u, item_t) not observed; the last one if there is none (failed)
        u outside [0, num_users): no draw, item 0 (bad)
    q_i = (kept_i + sum over c != i with alias_c == i of (2^32 - thresh_c)) / (num_items * 2^32),
          kept_i = 2^32 if alias_i == i else thresh_i
    log-q column of a position: float32(log q)[item], item = the positive's own or the drawn one; 0.0 for an item
    outside [0, num_items)
    ungrouped: v = perm_M(seed, e, p);  grouped: v = perm_N(seed, e, p // (1 + k)) * (1 + k) + p % (1 + k)
"""
import numpy as np

from loader_numpy import U64, mix64, perm

MAX_TRIES = 1 << 14
MULT = U64(0x100000001B3)
ONE = 1 << 32


def heavy_tail_weights(n, seed, zeros=0.2):
    """test weights: a Pareto tail (index 1.1) with about ``zeros`` of the entries exactly 0"""
    rng = np.random.default_rng(seed)
    w = rng.pareto(1.1, n) + 0.01
    w[rng.random(n) < zeros] = 0.0
    return w


def split_words(words):
    """(thresh, alias) int64 arrays of the uint64 table words"""
    words = np.asarray(words).view(U64) if np.asarray(words).dtype == np.int64 else np.asarray(words, dtype=U64)
    return (words >> U64(32)).astype(np.int64), (words & U64(0xffffffff)).astype(np.int64)


def implied_q(words):
    """(I,) float64 distribution of a table, from its integers (Python ints: no rounding before the one division)"""
    thresh, alias = split_words(words)
    n = thresh.shape[0]
    mass = [0] * n
    for c in range(n):
        if int(alias[c]) == c:
            mass[c] += ONE
        else:
            mass[c] += int(thresh[c])
            mass[int(alias[c])] += ONE - int(thresh[c])
    assert sum(mass) == n * ONE
    return np.array([m / (n * ONE) for m in mass], dtype=np.float64)     # int / int: correctly rounded


def log_q32(q):
    with np.errstate(divide="ignore"):
        return np.log(q).astype(np.float32)


def hashes(seed, epoch, v, tries):
    """h of slots ``v`` (array) x tries t = 0 .. tries - 1 -> uint64 array of shape v.shape + (tries,)"""
    with np.errstate(over="ignore"):
        nkey = mix64(U64(seed) ^ mix64(U64(epoch) * MULT + U64(4)))
        v = np.asarray(v, dtype=U64)
        inner = mix64(v[..., None] * MULT + np.arange(tries, dtype=U64))
        return mix64(nkey ^ inner)


def items_of(h, words):
    """item_t of every hash of ``h`` -> int64 array"""
    thresh, alias = split_words(words)
    n = U64(thresh.shape[0])
    col = (((h >> U64(32)) * n) >> U64(32)).astype(np.int64)
    low = (h & U64(0xffffffff)).astype(np.int64)
    return np.where(low < thresh[col], col, alias[col])


def uniform_items_of(h, num_items):
    """the uniform draw of the same hashes (loader_neg_numpy's), for the test that the statistic has teeth"""
    return (((h >> U64(32)) * U64(num_items)) >> U64(32)).astype(np.int64)


def negative(seed, epoch, v, user_items, words):
    """(item, tries used, failed) of negative slot v for a user whose observed items are the set ``user_items``"""
    done, block = 0, 16
    while done < MAX_TRIES:
        block = min(block, MAX_TRIES - done)
        d = items_of(hashes(seed, epoch, np.array([v]), done + block)[0, done:], words)
        for t, item in enumerate(d):
            if int(item) not in user_items:
                return int(item), done + t + 1, False
        done += block
        block *= 8
    return int(d[-1]), MAX_TRIES, True


def epoch_samples(seed, epoch, positions, users, pos_items, k, words, observed, shuffle=True, num_users=None,
                  grouped=False):
    """what positions ``positions`` of epoch ``epoch`` hold: dict of arrays over the positions -- v, sample (s), slot (j),
    item (the drawn item, -1 for a positive), tries, the flags failed / bad (bad: a user id or an item id outside its
    table), and logq (float32, the log-q column)"""
    users = np.asarray(users, dtype=np.int64)
    pos_items = np.asarray(pos_items, dtype=np.int64)
    n, per = users.shape[0], 1 + k
    pos = np.asarray(positions, dtype=np.int64)
    if grouped:
        group = pos // per
        v = (perm(seed, epoch, group, n) if shuffle else group) * per + pos % per
    else:
        v = perm(seed, epoch, pos, n * per) if shuffle else pos.copy()
    sample, slot = v // per, v % per
    num_items = np.asarray(words).shape[0]
    table_log_q = log_q32(implied_q(words))
    item = np.full(v.shape, -1, dtype=np.int64)
    tries = np.zeros(v.shape, dtype=np.int64)
    failed = np.zeros(v.shape, dtype=bool)
    bad = np.zeros(v.shape, dtype=bool)
    logq = np.zeros(v.shape, dtype=np.float32)
    for at in range(v.shape[0]):
        if slot[at]:
            u = int(users[sample[at]])
            if u < 0 or (num_users is not None and u >= num_users):
                item[at], bad[at] = 0, True
            else:
                item[at], tries[at], failed[at] = negative(seed, epoch, int(v[at]), observed.get(u, ()), words)
        which = int(item[at]) if slot[at] else int(pos_items[sample[at]])
        if 0 <= which < num_items:
            logq[at] = table_log_q[which]
        else:
            bad[at] = True
    return dict(v=v, sample=sample, slot=slot, item=item, tries=tries, failed=failed, bad=bad, logq=logq)
