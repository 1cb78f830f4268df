#!/usr/bin/env python3
"""Matrix factorisation trained on the objective the sampled losses estimate: the cross entropy of each training
positive against EVERY item of the catalogue (``model.softmax_nll``: two fused matrix-core passes, no logit matrix, no
sampler, no negatives to draw, nothing to tune but the optimizer).  The loader runs over the positives alone; after each
epoch the whole catalogue is ranked (``model.score_rows``, training pairs left out) and the top 50 compared with the
users' test items.  The split is the synthetic ml-100k-shaped implicit split of ``_common.implicit_split``.

    python scripts/mf_softmax.py [--epochs 3] [--batch 8192] [--embedding 64]
"""
import argparse

import _common as c
import torch

from model.mf import MatrixFactorization

from deeplearningrecommendationsystem_amd import optim
from deeplearningrecommendationsystem_amd.data import DeviceLoader
from deeplearningrecommendationsystem_amd.evaluator.ranking import ranking_metrics

K = 50
ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--embedding", type=int, default=64, help="embedding size (at most 256)")
a = ap.parse_args()
device = c.device

train_u, train_i, test_u, test_i = (t.to(device) for t in c.implicit_split())
ones = torch.ones(train_u.shape[0], dtype=torch.float32, device=device)      # the loader's rating column, unused
train = DeviceLoader.pairs(train_u, train_i, ones, a.batch, seed=1, negatives=0)

model = MatrixFactorization(c.NUM_USERS, c.NUM_ITEMS, a.embedding).to(device)
optimizer = optim.Adam(model.parameters(), lr=0.01)
for epoch in range(a.epochs):
    total = torch.zeros((), dtype=torch.float64, device=device)
    for (u, i), _ in train.epoch(epoch):
        nll = model.softmax_nll(u, i)
        nll.mean().backward()
        optimizer.step()
        optimizer.zero_grad()
        total += nll.detach().sum()
    train.check_bad_index()
    model.check_bad_index()
    m = ranking_metrics(model.score_rows, (test_u, test_i), K, exclude=((train_u, train_i),), num_users=c.NUM_USERS)
    print(f"epoch {epoch + 1}: train nll {total.item() / train_u.shape[0]:.4f}  precision@{K} {m.precision:.4f}  "
          f"recall@{K} {m.recall:.4f}  NDCG@{K} {m.ndcg:.4f}  MRR {m.mrr:.4f}")
