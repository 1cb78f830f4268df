"""Numpy restatement of the grouped epochs of csrc/loader.hip (ctr_load_batch_groups), written from the definition in
the kernel file's header comment and from nothing else (no import of the package); perm is loader_numpy's, the draw
loader_neg_numpy's.

    N positives, k negatives per positive; position p of epoch e:
        g = p // (1 + k);   j = p % (1 + k)
        s = perm_N(seed, e, g)   (s = g unshuffled);    v = s * (1 + k) + j
        outputs = what the ungrouped loader defines for virtual index v: j == 0 the positive s, j >= 1 the draw keyed
        by (seed, e, v) for u = users[s]
"""
import numpy as np

from loader_neg_numpy import negative
from loader_numpy import perm


def group_index(seed, epoch, positions, n, k, shuffle=True):
    """v of every position (array-like of ints in [0, n (1 + k))) -> int64 array"""
    pos = np.asarray(positions, dtype=np.int64)
    group, slot = pos // (1 + k), pos % (1 + k)
    sample = perm(seed, epoch, group, n) if shuffle else group
    return sample * (1 + k) + slot


def epoch_samples(seed, epoch, positions, users, k, num_items, observed, shuffle=True, num_users=None):
    """what positions ``positions`` of epoch ``epoch`` hold: loader_neg_numpy.epoch_samples' dict of arrays (v, sample,
    slot, item (-1 for a positive), tries, failed, bad), with v from the grouped map"""
    users = np.asarray(users, dtype=np.int64)
    v = group_index(seed, epoch, positions, users.shape[0], k, shuffle)
    sample, slot = v // (1 + k), v % (1 + k)
    item = np.full(v.shape, -1, dtype=np.int64)
    tries = np.zeros(v.shape, dtype=np.int64)
    failed = np.zeros(v.shape, dtype=bool)
    bad = np.zeros(v.shape, dtype=bool)
    for at in np.nonzero(slot)[0]:
        u = int(users[sample[at]])
        if u < 0 or (num_users is not None and u >= num_users):
            item[at], bad[at] = 0, True
            continue
        item[at], tries[at], failed[at] = negative(seed, epoch, int(v[at]), observed.get(u, ()), num_items)
    return dict(v=v, sample=sample, slot=slot, item=item, tries=tries, failed=failed, bad=bad)
