#!/usr/bin/env python3
"""DIEN trained on positives with drawn negatives through ``DeviceLoader.sequences`` and evaluated over the WHOLE
catalogue: every epoch each user's history row is scored against all 1682 items by the history x item grid kernel
(``model.history_scorer(history)``), the training pairs are left out, and the top 50 are compared with the user's test
items (``ranking_metrics``: precision, recall, F1, MAP, NDCG, MRR); the ten best unseen items of the first three users
are printed beside it (``model.recommend``).  The split is the synthetic ml-100k-shaped implicit split of
``_common.implicit_split`` (943 x 1682, ~90k training pairs, 10 test items per user); a user's history row is ten of
their training items (left-padded with item 0 where they have fewer).

    python scripts/dien_topk.py [--epochs 3] [--batch 8192] [--negatives 4] [--k 50]
"""
import argparse

import _common as c
import torch.nn
from torch import optim

from model.dien import DIEN
from trainer.trainer import Trainer

from deeplearningrecommendationsystem_amd.data import DeviceLoader, ObservedPairs
from deeplearningrecommendationsystem_amd.evaluator.ranking import ranking_metrics

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--negatives", type=int, default=4, help="negatives drawn per training positive, fresh every epoch")
ap.add_argument("--k", type=int, default=50, help="depth of the ranking evaluation")
a = ap.parse_args()
device = c.device
HIST_LEN = 10

train_u, train_i, test_u, test_i = (t.to(device) for t in c.implicit_split())
observed = ObservedPairs([train_u, test_u], [train_i, test_i], c.NUM_USERS, c.NUM_ITEMS)
seen = ObservedPairs(train_u, train_i, c.NUM_USERS, c.NUM_ITEMS)
# one history row per USER: the last HIST_LEN of the user's (ascending) training items, left-padded with item 0
at = seen.indptr[1:, None] - HIST_LEN + torch.arange(HIST_LEN, device=device)[None, :]
inside = at >= seen.indptr[:-1, None]
history = torch.where(inside, seen.indices[at.clamp_(min=0)].to(torch.int64), torch.zeros_like(at))
ones = torch.ones((train_u.shape[0], 1), dtype=torch.float32, device=device)
train = DeviceLoader.sequences(history, train_u, train_i, ones, a.batch, seed=1, negatives=a.negatives, observed=observed)

model = DIEN(c.NUM_ITEMS, 16).to(device)
trainer = Trainer(model, torch.nn.BCELoss(), optim.Adam(model.parameters(), lr=0.001, weight_decay=1e-5))
m = None
for epoch in range(a.epochs):
    trainer.train_epoch(train, epoch)
    train.check_bad_index()
    m = ranking_metrics(model.history_scorer(history), (test_u, test_i), a.k, exclude=((train_u, train_i),),
                        num_users=c.NUM_USERS)
    top = model.recommend(history[:3], n=10, exclude=observed, users=[0, 1, 2])
    print(f"epoch {epoch + 1}: train loss {trainer.train_loss.item():.4f}  precision@{a.k} {m.precision:.4f}  "
          f"recall@{a.k} {m.recall:.4f}  NDCG@{a.k} {m.ndcg:.4f}  MRR {m.mrr:.4f}")
    for u, row in enumerate(top.tolist()):
        print(f"    user {u}: {row}")
print(f"""
                - Precision@{a.k}:  {m.precision}
                - Recall@{a.k}:  {m.recall}
                - F1 Score@{a.k}:  {m.f1}
                - MAP@{a.k}: {m.map}
                - Mean NDCG@{a.k}: {m.ndcg}
                - MRR: {m.mrr}
                """)
