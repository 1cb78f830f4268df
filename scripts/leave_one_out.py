#!/usr/bin/env python3
"""NeuralCF trained on positives with drawn negatives and evaluated the way that regime is: every test positive
ranked against 99 distinct unobserved items (HR@10 / NDCG@10 / MRR), all on the device.  The reference has neither
stage; the split is the synthetic ml-100k-shaped implicit split of ``_common.implicit_split`` (943 x 1682, ~90k
training pairs, 10 test items per user).

    python scripts/leave_one_out.py [--epochs 5] [--batch 8192] [--negatives 4] [--candidates 99]
"""
import argparse

import _common as c
import torch.nn
from torch import optim

from model.neuralcf import NeuralCF
from trainer.trainer import Trainer

from deeplearningrecommendationsystem_amd.data import DeviceLoader, LeaveOneOut, ObservedPairs

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--negatives", type=int, default=4, help="negatives drawn per training positive, fresh every epoch")
ap.add_argument("--candidates", type=int, default=99, help="distinct negatives each test positive is ranked against")
a = ap.parse_args()
device = c.device

train_u, train_i, test_u, test_i = (t.to(device) for t in c.implicit_split())
observed = ObservedPairs([train_u, test_u], [train_i, test_i], c.NUM_USERS, c.NUM_ITEMS)
ones = torch.ones((train_u.shape[0], 1), dtype=torch.float32, device=device)
train = DeviceLoader.pairs(train_u, train_i, ones, a.batch, seed=1, negatives=a.negatives, observed=observed)
held_out = LeaveOneOut(test_u, test_i, observed, negatives=a.candidates, seed=2)
held_out.check()
test = held_out.pairs(a.batch)
print(f"{train.num_positives} training positives x (1 + {a.negatives}) per epoch; {held_out.num_groups} test positives, "
      f"each against {a.candidates} distinct unobserved items")

model = NeuralCF(c.NUM_USERS, c.NUM_ITEMS, 64, [128, 64, 32, 16, 8]).to(device)
trainer = Trainer(model, torch.nn.BCELoss(), optim.Adam(model.parameters(), lr=0.001))
for epoch in range(a.epochs):
    trainer.train_epoch(train, epoch)
    m = trainer.rank_epoch(test, negatives=a.candidates, cutoffs=(10,))
    train.check_bad_index()
    print(f"epoch {epoch + 1}: train loss {trainer.train_loss.item():.4f}  test loss {trainer.rank_loss.item():.4f}  "
          f"HR@10 {m.hr[10]:.4f}  NDCG@10 {m.ndcg[10]:.4f}  MRR {m.mrr:.4f}")
print(trainer.rank_metrics.report())
