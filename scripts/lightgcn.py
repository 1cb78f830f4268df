#!/usr/bin/env python3
"""LightGCN trained by BPR over groups of one positive and four drawn negatives (a grouped loader) and evaluated over
the WHOLE catalogue: every epoch each user's items are scored from the propagated tables (``model.score_rows``), the
training pairs are left out and the top 50 are compared with the user's test items (``ranking_metrics``); the ten best
unseen items of the first three users are printed beside it (``model.recommend``).  The graph is the TRAIN pairs; the
split is the synthetic ml-100k-shaped implicit split of ``_common.implicit_split``.  ``--layers 0`` is MF.

    python scripts/lightgcn.py [--layers 0..3] [--epochs 3] [--batch 8000] [--k 50] [--embed 64] [--graph]
"""
import argparse

import _common as c
import torch
from torch import optim

from model.lightgcn import LightGCN, grid_path
from trainer.trainer import Trainer

from deeplearningrecommendationsystem_amd.data import DeviceLoader, ObservedPairs
from deeplearningrecommendationsystem_amd.evaluator.ranking import ranking_metrics
from deeplearningrecommendationsystem_amd.loss import BPRLoss

NEGATIVES = 4
ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=3, choices=(0, 1, 2, 3), help="propagation layers; 0 is MF")
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--batch", type=int, default=8000, help="a multiple of 1 + 4")
ap.add_argument("--k", type=int, default=50, help="depth of the ranking evaluation")
ap.add_argument("--embed", type=int, default=64)
ap.add_argument("--graph", action="store_true", help="replay the full batches as one hipGraph")
a = ap.parse_args()
device = c.device
if a.batch % (1 + NEGATIVES):
    raise SystemExit("--batch must be a multiple of 5")

train_u, train_i, test_u, test_i = (t.to(device) for t in c.implicit_split())
observed = ObservedPairs([train_u, test_u], [train_i, test_i], c.NUM_USERS, c.NUM_ITEMS)
train_pairs = ObservedPairs(train_u, train_i, c.NUM_USERS, c.NUM_ITEMS)
ones = torch.ones(train_u.shape[0], dtype=torch.float32, device=device)      # forward returns (B,)
train = DeviceLoader.pairs(train_u, train_i, ones, a.batch, seed=1, negatives=NEGATIVES, observed=observed, grouped=True)

model = LightGCN(c.NUM_USERS, c.NUM_ITEMS, a.embed, a.layers).to(device).set_graph(train_pairs)
print(f"{a.layers} layers over {len(train_pairs)} training pairs; grid scorer path: {grid_path(a.embed)}")
trainer = Trainer(model, BPRLoss(NEGATIVES), optim.Adam(model.parameters(), lr=0.005, weight_decay=1e-5), graph=a.graph)
m = None
for epoch in range(a.epochs):
    trainer.train_epoch(train, epoch)
    train.check_bad_index()
    model.check_bad_index()
    m = ranking_metrics(model.score_rows, (test_u, test_i), a.k, exclude=((train_u, train_i),), num_users=c.NUM_USERS)
    top = model.recommend(users=[0, 1, 2], n=10, exclude=observed)
    print(f"epoch {epoch + 1}: train loss {trainer.train_loss.item():.4f}  precision@{a.k} {m.precision:.4f}  "
          f"recall@{a.k} {m.recall:.4f}  NDCG@{a.k} {m.ndcg:.4f}  MRR {m.mrr:.4f}")
    for u, row in enumerate(top.tolist()):
        print(f"    user {u}: {row}")
