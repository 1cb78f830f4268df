#!/usr/bin/env python3
"""Wide & Deep trained on positives with drawn negatives and evaluated over the WHOLE catalogue: every epoch each user's
1682 items are scored by the grid kernel (``model.catalogue_scorer(features)``: no (user, item) feature frame is ever
built), the training pairs are left out, and the top 50 are compared with the user's test items (``ranking_metrics``:
precision, recall, F1, MAP, NDCG, MRR); the ten best unseen items of the first three users are printed beside it
(``scorer.recommend``).  The split is the synthetic ml-100k-shaped implicit split of ``_common.implicit_split``
(943 x 1682, ~90k training pairs, 10 test items per user); the side features are those of scripts/minibatch.py.

    python scripts/widedeep_topk.py [--epochs 3] [--batch 8192] [--negatives 4] [--k 50] [--embed 128]
"""
import argparse

import _common as c
import torch.nn
from torch import optim

from model.widedeep import WideDeep
from trainer.trainer import Trainer

from deeplearningrecommendationsystem_amd import synth
from deeplearningrecommendationsystem_amd.data import DeviceLoader, FeatureAssembler, ObservedPairs
from deeplearningrecommendationsystem_amd.evaluator.ranking import ranking_metrics

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--negatives", type=int, default=4, help="negatives drawn per training positive, fresh every epoch")
ap.add_argument("--k", type=int, default=50, help="depth of the ranking evaluation")
ap.add_argument("--embed", type=int, default=128, help="embedding size")
a = ap.parse_args()
device = c.device

train_u, train_i, test_u, test_i = (t.to(device) for t in c.implicit_split())
observed = ObservedPairs([train_u, test_u], [train_i, test_i], c.NUM_USERS, c.NUM_ITEMS)
ones = torch.ones((train_u.shape[0], 1), dtype=torch.float32, device=device)
features = FeatureAssembler(synth.feature_batch(c.NUM_USERS, gen=synth.generator(11))[:, 2:26].to(device),
                            synth.feature_batch(c.NUM_ITEMS, gen=synth.generator(12))[:, 26:45].to(device))
train = DeviceLoader.features(features, train_u, train_i, ones, a.batch, seed=1, negatives=a.negatives, observed=observed)

model = WideDeep(c.NUM_USERS, c.NUM_ITEMS, [512, 256, 128, 1], a.embed).to(device)
scorer = model.catalogue_scorer(features)       # reads the weights at every call: made once, never stale
print(f"catalogue scorer path: {scorer.path}")
trainer = Trainer(model, torch.nn.BCELoss(), optim.Adam(model.parameters(), lr=0.001, weight_decay=1e-5))
m = None
for epoch in range(a.epochs):
    trainer.train_epoch(train, epoch)
    train.check_bad_index()
    m = ranking_metrics(scorer, (test_u, test_i), a.k, exclude=((train_u, train_i),), num_users=c.NUM_USERS)
    top = scorer.recommend(users=[0, 1, 2], n=10, exclude=observed)
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
