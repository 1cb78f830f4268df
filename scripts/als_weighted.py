#!/usr/bin/env python3
"""ALS with a value on every pair, on the synthetic ml-100k-shaped split of ``synth.valued_split`` (943 x 1682, ~90k
training pairs with a play count and a rating each, 10 test items per user).

``--objective implicit``: the counts as confidences ``c = 1 + alpha count`` (``ALS.fit(Interactions)``) beside the same
pairs as a set (``ALS.fit(ObservedPairs)``): the loss of each over ALL user x item cells after every sweep, then the
top-50 ranking metrics of both with the training pairs left out.
``--objective explicit``: the ratings by weighted-lambda least squares over the observed cells: the loss and the train /
held-out RMSE after every sweep.

    python scripts/als_weighted.py [--objective implicit|explicit] [--sweeps 10] [--k 64] [--reg 0.1] [--alpha 40]
"""
import argparse

import _common as c

from deeplearningrecommendationsystem_amd import ALS, synth
from deeplearningrecommendationsystem_amd.data import Interactions
from deeplearningrecommendationsystem_amd.evaluator.ranking import ranking_metrics

ap = argparse.ArgumentParser()
ap.add_argument("--objective", choices=("implicit", "explicit"), default="implicit")
ap.add_argument("--sweeps", type=int, default=10)
ap.add_argument("--k", type=int, default=64, help="factors: a multiple of 16 up to 128")
ap.add_argument("--reg", type=float, default=0.1)
ap.add_argument("--alpha", type=float, default=40.0, help="implicit: the confidence of a pair is 1 + alpha count")
a = ap.parse_args()
device = c.device
depth = 50

train_u, train_i, counts, ratings, test_u, test_i, test_ratings = (t.to(device) for t in synth.valued_split())


def rmse(model, users, items, want):
    return float((model.predict(users, items) - want).square().mean().sqrt())


def report(name, m):
    print(f"""
                {name}
                - Precision@{depth}:  {m.precision}
                - Recall@{depth}:  {m.recall}
                - F1 Score@{depth}:  {m.f1}
                - MAP@{depth}: {m.map}
                - Mean NDCG@{depth}: {m.ndcg}
                - MRR: {m.mrr}
                """)


if a.objective == "explicit":
    inter = Interactions(train_u, train_i, ratings, c.NUM_USERS, c.NUM_ITEMS, duplicates="error")
    model = ALS(c.NUM_USERS, c.NUM_ITEMS, k=a.k, reg=a.reg, seed=0, device=device, objective="explicit")
    model.fit(inter, sweeps=0)
    for sweep in range(a.sweeps):
        model.sweep()
        print(f"sweep {sweep + 1}: loss {model.loss():.6f}  train RMSE {rmse(model, train_u, train_i, ratings):.4f}  "
              f"held-out RMSE {rmse(model, test_u, test_i, test_ratings):.4f}")
else:
    inter = Interactions(train_u, train_i, counts, c.NUM_USERS, c.NUM_ITEMS, duplicates="error")
    weighted = ALS(c.NUM_USERS, c.NUM_ITEMS, k=a.k, reg=a.reg, alpha=a.alpha, seed=0, device=device).fit(inter, sweeps=0)
    as_set = ALS(c.NUM_USERS, c.NUM_ITEMS, k=a.k, reg=a.reg, alpha=a.alpha, seed=0, device=device).fit(inter.pairs,
                                                                                                      sweeps=0)
    for sweep in range(a.sweeps):
        weighted.sweep()
        as_set.sweep()
        print(f"sweep {sweep + 1}: loss {weighted.loss():.6f}  (the pairs as a set: loss {as_set.loss():.6f})")
    for name, model in (("counts as confidences", weighted), ("the same pairs as a set", as_set)):
        report(name, ranking_metrics(model.score_rows, (test_u, test_i), depth, exclude=((train_u, train_i),),
                                     num_users=c.NUM_USERS))
    for u, row in enumerate(weighted.recommend(users=[0, 1, 2], n=10, exclude=inter.pairs).tolist()):
        print(f"    user {u}: {row}")
