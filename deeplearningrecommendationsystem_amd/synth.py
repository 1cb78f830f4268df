"""Synthetic MovieLens-100k-shaped batches (host side, seeded).

The reference builds its inputs with pandas from ml-100k (data/reader.py:14-112)
whose licence forbids redistribution, and nothing in it is seeded, so benchmarks
and tests use generated batches with the same layout:

* feature models: ``(B,45)`` float32 -- col 0 user id, col 1 item id (as floats,
  scripts/pnn.py:41-43), col 2 age in [0,1) (reader.py:38-41), 3:5 gender
  one-hot, 5:26 occupation one-hot, 26:45 genre multi-hot (mean ~1.7 ones);
* id models: two int64 vectors (scripts/mf.py:24-62);
* sequence models: ``hist (B,L)`` int64 left-padded with id 0 and a target
  ``(B,)`` (scripts/din.py:23-31).
"""
from __future__ import annotations

import torch

NUM_USERS_ML100K = 943
NUM_ITEMS_ML100K = 1682
NUM_COLS = 45


def generator(seed: int = 1234) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def feature_batch(batch: int, num_users: int = NUM_USERS_ML100K, num_items: int = NUM_ITEMS_ML100K,
                  gen: torch.Generator | None = None, zero_genre_rows: int = 0) -> torch.Tensor:
    gen = gen or generator()
    x = torch.zeros(batch, NUM_COLS, dtype=torch.float32)
    x[:, 0] = torch.randint(0, num_users, (batch,), generator=gen).float()
    x[:, 1] = torch.randint(0, num_items, (batch,), generator=gen).float()
    x[:, 2] = torch.rand(batch, generator=gen)
    gender = torch.randint(0, 2, (batch,), generator=gen)
    occ = torch.randint(0, 21, (batch,), generator=gen)
    rows = torch.arange(batch)
    x[rows, 3 + gender] = 1.0
    x[rows, 5 + occ] = 1.0
    x[:, 26:45] = (torch.rand(batch, 19, generator=gen) < 0.09).float()
    if zero_genre_rows:
        x[:zero_genre_rows, 26:45] = 0.0
    return x


def id_batch(batch: int, num_users: int = NUM_USERS_ML100K, num_items: int = NUM_ITEMS_ML100K,
             gen: torch.Generator | None = None):
    gen = gen or generator()
    u = torch.randint(0, num_users, (batch,), generator=gen)
    i = torch.randint(0, num_items, (batch,), generator=gen)
    return u, i


def hist_batch(batch: int, hist_len: int, num_items: int, gen: torch.Generator | None = None,
               pad_fraction: float = 0.25):
    """histories are left-padded with id 0 for ``pad_fraction`` of the rows
    (random pad length), like scripts/din.py:23-31."""
    gen = gen or generator()
    hist = torch.randint(0, num_items, (batch, hist_len), generator=gen)
    npad = torch.randint(0, hist_len + 1, (batch,), generator=gen)
    padded = torch.rand(batch, generator=gen) < pad_fraction
    pos = torch.arange(hist_len).unsqueeze(0)
    hist = torch.where(padded.unsqueeze(1) & (pos < npad.unsqueeze(1)), torch.zeros_like(hist), hist)
    target = torch.randint(0, num_items, (batch,), generator=gen)
    return hist, target


def labels(batch: int, shape_2d: bool = True, gen: torch.Generator | None = None) -> torch.Tensor:
    gen = gen or generator()
    y = (torch.rand(batch, generator=gen) < 0.5).float()
    return y.view(-1, 1) if shape_2d else y


def implicit_split(num_users: int = NUM_USERS_ML100K, num_items: int = NUM_ITEMS_ML100K, train_pairs: int = 90_570,
                   test_per_user: int = 10, seed: int = 5, zipf: float = 1.0):
    """an implicit-feedback split shaped like ml-100k's ua.base / ua.test: every user has exactly ``test_per_user``
    test items (as ua.test), training pairs are spread over users with a skewed count and over items by a Zipf-like
    popularity, no pair is in both splits or twice in one, and every user and every item occurs in training.
    Returns 0-based int64 ``(train_users, train_items, test_users, test_items)``."""
    gen = generator(seed)
    if train_pairs + num_users * test_per_user > num_users * num_items // 2 or train_pairs < num_users + num_items:
        raise ValueError("split does not fit the matrix")
    pop = 1.0 / torch.arange(1, num_items + 1, dtype=torch.float64) ** zipf
    pop = pop[torch.randperm(num_items, generator=gen)]
    activity = torch.rand(num_users, generator=gen, dtype=torch.float64) ** 3 + 0.05
    taken = torch.zeros(num_users, num_items, dtype=torch.bool)
    # every item once in training, each with a random user
    first_users = torch.randint(0, num_users, (num_items,), generator=gen)
    taken[first_users, torch.arange(num_items)] = True
    # every user at least once
    for u in torch.nonzero(~taken.any(1)).flatten().tolist():
        taken[u, int(torch.multinomial(pop, 1, generator=gen))] = True
    # the rest by activity x popularity, without repeats (each round adds at most the pairs still missing)
    while int(taken.sum()) < train_pairs:
        left = train_pairs - int(taken.sum())
        u = torch.multinomial(activity, left, replacement=True, generator=gen)
        i = torch.multinomial(pop, left, replacement=True, generator=gen)
        taken[u, i] = True
    train_u, train_i = torch.nonzero(taken, as_tuple=True)
    # test: test_per_user unseen items per user, by popularity
    test = torch.zeros_like(taken)
    for u in range(num_users):
        w = pop.clone()
        w[taken[u]] = 0.0
        test[u, torch.multinomial(w, test_per_user, replacement=False, generator=gen)] = True
    test_u, test_i = torch.nonzero(test, as_tuple=True)
    assert bool(taken.any(1).all()) and bool(taken.any(0).all())
    return train_u, train_i, test_u, test_i


def valued_split(seed: int = 5, rank: int = 8, noise: float = 0.5, **split):
    """``implicit_split(seed=seed, **split)`` with a value on every pair, from a seeded affinity
    ``a_ui = <f_u, g_i>`` of unit variance (``rank`` factors) plus N(0, ``noise``^2): play counts
    ``1 + floor(exp(a + e))`` (float32, >= 1, heavy-tailed) on the training pairs and ratings
    ``clip(round(3 + a + e'), 1, 5)`` on both splits.  Returns 0-based int64 ids and float32 values
    ``(train_users, train_items, train_counts, train_ratings, test_users, test_items, test_ratings)``."""
    train_u, train_i, test_u, test_i = implicit_split(seed=seed, **split)
    num_users, num_items = int(train_u.max()) + 1, int(train_i.max()) + 1      # every user and item is in training
    gen = generator(seed + 1000)
    f = torch.randn(num_users, rank, generator=gen, dtype=torch.float64)
    g = torch.randn(num_items, rank, generator=gen, dtype=torch.float64) / rank ** 0.5

    def affinity(u, i):
        return (f[u] * g[i]).sum(1), torch.randn(u.numel(), generator=gen, dtype=torch.float64) * noise

    a, e = affinity(train_u, train_i)
    counts = (1.0 + torch.floor(torch.exp(a + e))).float()
    _, e = affinity(train_u, train_i)
    ratings = torch.clamp(torch.round(3.0 + a + e), 1.0, 5.0).float()
    a, e = affinity(test_u, test_i)
    test_ratings = torch.clamp(torch.round(3.0 + a + e), 1.0, 5.0).float()
    return train_u, train_i, counts, ratings, test_u, test_i, test_ratings
