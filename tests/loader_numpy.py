"""Numpy restatement of the shuffled index of csrc/loader.hip and of the host arithmetic of data/loader.py, written
from the definition in the kernel file's header comment and from nothing else (no import of the package).

    perm(seed, epoch, p), 0 <= p < N:
        bits  = smallest even number >= 2 with 2^bits >= N;  half = bits / 2;  mask = 2^half - 1
        key_r = mix64(seed ^ mix64(epoch * 0x100000001B3 + r)),  r = 0..3          (uint64 arithmetic, wrapping)
        E(x):  (L, R) = (x >> half, x & mask);  four times, r = 0..3:  (L, R) = (R, L ^ ((mix64(key_r ^ R) >> 32) & mask))
               result (L << half) | R
        x = E(p);  while x >= N: x = E(x);  perm = x
"""
import numpy as np

U64 = np.uint64
ROUNDS = 4


def mix64(z):
    """the splitmix64 finaliser of csrc/sampler.hip, on uint64 arrays (wrapping)"""
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def half_bits(n):
    bits = 2
    while (1 << bits) < n:
        bits += 2
    return bits // 2


def round_keys(seed, epoch):
    with np.errstate(over="ignore"):
        inner = mix64(U64(epoch) * U64(0x100000001B3) + np.arange(ROUNDS, dtype=U64))
    return mix64(U64(seed) ^ inner)


def _network(x, keys, half):
    mask = U64((1 << half) - 1)
    left, right = x >> U64(half), x & mask
    for k in keys:
        left, right = right, left ^ ((mix64(k ^ right) >> U64(32)) & mask)
    return (left << U64(half)) | right


def perm(seed, epoch, positions, n):
    """sample index of every position (array-like of ints in [0, n)) -> int64 array"""
    pos = np.asarray(positions, dtype=np.int64)
    assert n >= 1 and (pos.size == 0 or (pos.min() >= 0 and pos.max() < n))
    keys, half = round_keys(seed, epoch), half_bits(n)
    x = _network(pos.astype(U64), keys, half)
    while True:
        walk = x >= U64(n)
        if not walk.any():
            return x.astype(np.int64)
        x[walk] = _network(x[walk], keys, half)


def batch_ranges(n, batch_size, drop_last=False, rank=0, world=1):
    """[(first position, count)] of one rank's batches, restated from the rule in data/loader.py's docstring:
    F = n // batch_size full batches; every rank takes F // world of them, rank r the batches r, r + world, ...;
    the positions behind them, [(F // world) * world * batch_size, n), are dropped with drop_last and otherwise cut
    into `world` contiguous pieces, the first `rest % world` one longer, piece r being rank r's tail batch."""
    per_rank = (n // batch_size) // world
    out = [((k * world + rank) * batch_size, batch_size) for k in range(per_rank)]
    used = per_rank * world * batch_size
    rest = n - used
    if not drop_last and rest > 0:
        base, extra = divmod(rest, world)
        first = used + rank * base + min(rank, extra)
        count = base + (1 if rank < extra else 0)
        if count:
            out.append((first, count))
    return out
