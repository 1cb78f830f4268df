#!/usr/bin/env python3
"""NeuralCF trained on the objective it is scored by: groups of one positive and four drawn negatives from a grouped
loader, under a pointwise (BCE), pairwise (BPR) or listwise (sampled softmax) loss, and every test positive ranked
against 99 distinct unobserved items after each epoch (HR@10 / NDCG@10 / MRR), all on the device.  The reference trains
with BCE alone; the split is the synthetic ml-100k-shaped implicit split of ``scripts/leave_one_out.py``.

    python scripts/pairwise.py [--loss bce|bpr|softmax] [--epochs 5] [--batch 8000] [--candidates 99] [--graph]
                               [--sampler uniform|popularity] [--alpha 0.75] [--logq]

``--sampler popularity`` draws the training negatives in proportion to ``count ** alpha`` over the observed pairs
(``data.ItemSampler.popularity``) instead of uniformly; ``--logq`` (softmax, popularity) subtracts log q(item) from the
logits (``SampledSoftmaxLoss(log_q=loader)``).  The evaluation candidates stay uniform and distinct.
"""
import argparse

import _common as c
import torch
from torch import optim

from model.neuralcf import NeuralCF
from trainer.trainer import Trainer

from deeplearningrecommendationsystem_amd.data import DeviceLoader, ItemSampler, LeaveOneOut, ObservedPairs
from deeplearningrecommendationsystem_amd.loss import BCELoss, BPRLoss, SampledSoftmaxLoss

NEGATIVES = 4
ap = argparse.ArgumentParser()
ap.add_argument("--loss", choices=("bce", "bpr", "softmax"), default="bpr")
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--batch", type=int, default=8000, help="a multiple of 1 + 4 and of 1 + candidates")
ap.add_argument("--candidates", type=int, default=99, help="distinct negatives each test positive is ranked against")
ap.add_argument("--graph", action="store_true", help="replay the full batches as one hipGraph")
ap.add_argument("--sampler", choices=("uniform", "popularity"), default="uniform", help="where the training negatives come from")
ap.add_argument("--alpha", type=float, default=0.75, help="popularity: weights count ** alpha")
ap.add_argument("--logq", action="store_true", help="softmax with --sampler popularity: the logQ correction")
a = ap.parse_args()
if a.logq and (a.loss != "softmax" or a.sampler != "popularity"):
    raise SystemExit("--logq goes with --loss softmax --sampler popularity")
device = c.device
if a.batch % (1 + NEGATIVES) or a.batch % (1 + a.candidates) or (1 + a.candidates) % (1 + NEGATIVES):
    # the evaluation pass hands the loss batches of whole test groups; they must be whole training-sized groups too
    raise SystemExit("--batch must be a multiple of 5 and of 1 + candidates, and 1 + candidates a multiple of 5")

train_u, train_i, test_u, test_i = (t.to(device) for t in c.implicit_split())
observed = ObservedPairs([train_u, test_u], [train_i, test_i], c.NUM_USERS, c.NUM_ITEMS)
ones = torch.ones((train_u.shape[0], 1), dtype=torch.float32, device=device)
item_sampler = ItemSampler.popularity(observed, a.alpha) if a.sampler == "popularity" else None
train = DeviceLoader.pairs(train_u, train_i, ones, a.batch, seed=1, negatives=NEGATIVES, observed=observed, grouped=True,
                           item_sampler=item_sampler)
held_out = LeaveOneOut(test_u, test_i, observed, negatives=a.candidates, seed=2)
held_out.check()
test = held_out.pairs(a.batch)
drawn = "uniform negatives" if item_sampler is None else f"negatives drawn by count^{a.alpha:g}" + (", logQ-corrected" if a.logq else "")
print(f"{train.num_positives} training positives in groups of 1 + {NEGATIVES}, loss {a.loss}, {drawn}; {held_out.num_groups} test "
      f"positives, each against {a.candidates} distinct unobserved items")

loss_fn = {"bce": BCELoss(), "bpr": BPRLoss(NEGATIVES), "softmax": SampledSoftmaxLoss(NEGATIVES, log_q=train if a.logq else None)}[a.loss]
model = NeuralCF(c.NUM_USERS, c.NUM_ITEMS, 64, [128, 64, 32, 16, 8]).to(device)
trainer = Trainer(model, loss_fn, optim.Adam(model.parameters(), lr=0.001), graph=a.graph)
for epoch in range(a.epochs):
    trainer.train_epoch(train, epoch)
    m = trainer.rank_epoch(test, negatives=a.candidates, cutoffs=(10,))
    train.check_bad_index()
    print(f"epoch {epoch + 1}: train loss {trainer.train_loss.item():.4f}  HR@10 {m.hr[10]:.4f}  NDCG@10 {m.ndcg[10]:.4f}  "
          f"MRR {m.mrr:.4f}")
print(trainer.rank_metrics.report())
