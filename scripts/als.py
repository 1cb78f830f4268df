#!/usr/bin/env python3
"""Implicit-feedback matrix factorisation by alternating least squares (Hu, Koren & Volinsky 2008) on the synthetic
ml-100k-shaped implicit split of ``_common.implicit_split`` (943 x 1682, ~90k training pairs, 10 test items per
user): every sweep solves all users, then all items, exactly; the loss over ALL user x item cells is printed after each
sweep, then the top-50 ranking metrics with the training pairs left out (``ranking_metrics``) and the ten best unseen
items of the first three users (``model.recommend``).

    python scripts/als.py [--sweeps 10] [--k 64] [--reg 0.1] [--alpha 40]
"""
import argparse

import _common as c

from deeplearningrecommendationsystem_amd import ALS
from deeplearningrecommendationsystem_amd.data import ObservedPairs
from deeplearningrecommendationsystem_amd.evaluator.ranking import ranking_metrics

ap = argparse.ArgumentParser()
ap.add_argument("--sweeps", type=int, default=10)
ap.add_argument("--k", type=int, default=64, help="factors: a multiple of 16 up to 128")
ap.add_argument("--reg", type=float, default=0.1)
ap.add_argument("--alpha", type=float, default=40.0, help="confidence of an observed pair: 1 + alpha")
a = ap.parse_args()
device = c.device
depth = 50

train_u, train_i, test_u, test_i = (t.to(device) for t in c.implicit_split())
observed = ObservedPairs(train_u, train_i, c.NUM_USERS, c.NUM_ITEMS)
model = ALS(c.NUM_USERS, c.NUM_ITEMS, k=a.k, reg=a.reg, alpha=a.alpha, seed=0, device=device).fit(observed, sweeps=0)
for sweep in range(a.sweeps):
    model.sweep()
    print(f"sweep {sweep + 1}: loss {model.loss():.6f}")
m = ranking_metrics(model.score_rows, (test_u, test_i), depth, exclude=((train_u, train_i),), num_users=c.NUM_USERS)
for u, row in enumerate(model.recommend(users=[0, 1, 2], n=10, exclude=observed).tolist()):
    print(f"    user {u}: {row}")
print(f"""
                - Precision@{depth}:  {m.precision}
                - Recall@{depth}:  {m.recall}
                - F1 Score@{depth}:  {m.f1}
                - MAP@{depth}: {m.map}
                - Mean NDCG@{depth}: {m.ndcg}
                - MRR: {m.mrr}
                """)
