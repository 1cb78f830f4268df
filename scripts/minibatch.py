#!/usr/bin/env python3
"""Mini-batch training through the device-side loader: NeuralCF, DeepFM and DIN, each for a few shuffled epochs on
synthetic ml-100k-shaped splits.  The reference's scripts train full-batch (the same tensors every epoch); here
``DeviceLoader`` draws shuffled batches on the device and ``Trainer.train_epoch`` / ``valid_epoch`` / ``test_epoch``
drive it.  ``--batch`` is smaller than the split, so an epoch is several full batches and a tail.

    python scripts/minibatch.py [--epochs 3] [--batch 4096] [--train 20000] [--graph] [--negatives K]

With ``--negatives K`` the loaders are given the positive part of each split and draw K negatives per positive
themselves: fresh ones every training epoch, fixed ones for the evaluation passes.
"""
import argparse

import _common as c
import torch.nn
from torch import optim

from model.deepfm import DeepFM
from model.din import DIN
from model.neuralcf import NeuralCF
from trainer.trainer import Trainer

from deeplearningrecommendationsystem_amd import synth
from deeplearningrecommendationsystem_amd.data import DeviceLoader, FeatureAssembler, ObservedPairs

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--train", type=int, default=20_000, help="training samples")
ap.add_argument("--graph", action="store_true", help="replay the full-size steps as one hipGraph")
ap.add_argument("--negatives", type=int, default=0, help="negatives the loaders draw per positive (0: the splits as they are)")
a = ap.parse_args()
device = c.device
HIST_LEN = 10


def assembler():
    """user rows (age, gender and occupation one-hot) and item rows (genre flags) in the layout of synth.feature_batch"""
    users = synth.feature_batch(c.NUM_USERS, gen=synth.generator(11))[:, 2:26]
    items = synth.feature_batch(c.NUM_ITEMS, gen=synth.generator(12))[:, 26:45]
    return FeatureAssembler(users.to(device), items.to(device))


def histories():
    """one left-padded history row per USER: the loader gathers it per sample"""
    hist, _ = synth.hist_batch(c.NUM_USERS, HIST_LEN, c.NUM_ITEMS, synth.generator(13))
    return hist.to(device)


def loaders(kind, splits):
    """train (shuffled) / valid / test loaders of one family over the id splits"""
    out = []
    for k, (users, items, rating) in enumerate(splits):
        kw = dict(batch_size=a.batch, seed=k, shuffle=k == 0, negatives=a.negatives, observed=observed)
        if kind == "pairs":
            out.append(DeviceLoader.pairs(users, items, rating, **kw))
        elif kind == "features":
            out.append(DeviceLoader.features(features, users, items, rating, **kw))
        else:
            out.append(DeviceLoader.sequences(history, users, items, rating, **kw))
    return out


def run(name, model, kind):
    print(f"\n==== {name}: {a.epochs} epochs, {len(train_split[0])} samples in batches of {a.batch} ====")
    if a.negatives:
        print(f"     (the positives of each split, and {a.negatives} drawn negatives per positive)")
    loss_fn = torch.nn.BCELoss()
    optimizer = optim.Adam(model.parameters(), lr=0.001, weight_decay=1e-5)
    trainer = Trainer(model, loss_fn, optimizer, graph=a.graph)
    train, valid, test = loaders(kind, splits)
    for epoch in range(a.epochs):
        trainer.train_epoch(train, epoch)
        trainer.valid_epoch(valid)
        trainer.test_epoch(test)
        if epoch % 5 == 4 or epoch == a.epochs - 1:
            for loader in (train, valid, test):
                loader.check_bad_index()
            trainer.model_eval(epoch)


splits = c.id_splits(a.train)
observed = None
if a.negatives:
    # as the reference's scripts: the positives of each split, negatives outside train | valid | test
    observed = ObservedPairs([u for u, _, _ in splits], [i for _, i, _ in splits], c.NUM_USERS, c.NUM_ITEMS)
    splits = [tuple(t[y.view(-1) > 0.5] for t in (u, i, y)) for u, i, y in splits]
train_split = splits[0]
features, history = assembler(), histories()
run("NeuralCF", NeuralCF(c.NUM_USERS, c.NUM_ITEMS, 256, [512, 256, 128, 64, 32]).to(device), "pairs")
run("DeepFM", DeepFM(c.NUM_USERS, c.NUM_ITEMS, [512, 256, 128, 1], 128).to(device), "features")
run("DIN", DIN(c.NUM_ITEMS, 64).to(device), "sequences")
