"""Numpy restatement of the drawn negatives of csrc/loader.hip (ctr_load_batch_neg), written from the definition in
the kernel file's header comment and from nothing else (no import of the package); perm / mix64 are loader_numpy's.

    N positives, k negatives per positive, M = N * (1 + k) positions; position p of epoch e:
        v = perm_M(seed, e, p)  (v = p unshuffled);   s = v // (1 + k);   j = v % (1 + k)
        j == 0: the positive s
        j >= 1: a negative of u = users[s]:
            nkey   = mix64(seed ^ mix64(e * 0x100000001B3 + 4))
            draw_t = ((mix64(nkey ^ mix64(v * 0x100000001B3 + t)) >> 32) * num_items) >> 32,   t = 0, 1, ...
            item   = draw_t for the first t < 2^14 with (u, draw_t) not observed; the last draw if there is none (failed)
            u outside [0, num_users): no draw, item 0 (bad)
"""
import numpy as np

from loader_numpy import U64, mix64, perm

MAX_TRIES = 1 << 14
MULT = U64(0x100000001B3)


def draws(seed, epoch, v, tries, num_items):
    """draw_t of slot v for t = 0 .. tries - 1 -> int64 array"""
    with np.errstate(over="ignore"):
        nkey = mix64(U64(seed) ^ mix64(U64(epoch) * MULT + U64(4)))
        inner = mix64(U64(v) * MULT + np.arange(tries, dtype=U64))
        return (((mix64(nkey ^ inner) >> U64(32)) * U64(num_items)) >> U64(32)).astype(np.int64)


def negative(seed, epoch, v, user_items, num_items):
    """(item, tries used, failed) of negative slot v for a user whose observed items are the set ``user_items``"""
    done, block = 0, 16
    while done < MAX_TRIES:
        block = min(block, MAX_TRIES - done)
        d = draws(seed, epoch, v, done + block, num_items)[done:]
        for t, item in enumerate(d):
            if int(item) not in user_items:
                return int(item), done + t + 1, False
        done += block
        block *= 8
    return int(d[-1]), MAX_TRIES, True


def epoch_samples(seed, epoch, positions, users, k, num_items, observed, shuffle=True, num_users=None):
    """what positions ``positions`` of epoch ``epoch`` hold.  ``users``: user id of each of the N positives; ``observed``:
    {user: set of items} (a user without an entry has observed nothing).  Returns a dict of arrays over the positions:
    v, sample (s), slot (j), item (the drawn item, -1 for a positive), tries, and the flags failed / bad."""
    users = np.asarray(users, dtype=np.int64)
    m = users.shape[0] * (1 + k)
    pos = np.asarray(positions, dtype=np.int64)
    v = perm(seed, epoch, pos, m) if shuffle else pos.copy()
    sample, slot = v // (1 + k), v % (1 + k)
    item = np.full(v.shape, -1, dtype=np.int64)
    tries = np.zeros(v.shape, dtype=np.int64)
    failed = np.zeros(v.shape, dtype=bool)
    bad = np.zeros(v.shape, dtype=bool)
    for n in np.nonzero(slot)[0]:
        u = int(users[sample[n]])
        if u < 0 or (num_users is not None and u >= num_users):
            item[n], bad[n] = 0, True
            continue
        item[n], tries[n], failed[n] = negative(seed, epoch, int(v[n]), observed.get(u, ()), num_items)
    return dict(v=v, sample=sample, slot=slot, item=item, tries=tries, failed=failed, bad=bad)
