"""Counterpart of the reference's trainer/trainer.py:8-146: same constructor, same loop
methods and call convention, so a script written against the reference drives the HIP
modules unchanged.  ``graph=True`` additionally replays the training step as one hipGraph
(the reference's scripts pass the same full-batch tensors every epoch)."""
from __future__ import annotations

import torch

from ..evaluator import Evaluator


class Trainer:
    def __init__(self, model, loss_fn, optimizer, graph: bool = False):
        self.model = model
        self.loss_fn = loss_fn
        self.optimizer = optimizer
        self.train_loss = self.valid_loss = self.test_loss = None
        self.predictions_train = self.predictions_valid = self.predictions_test = None
        self.train_rating = self.valid_rating = self.test_rating = None
        self.rank_metrics = self.predictions_rank = self.rank_rating = self.rank_loss = None
        self.score_metrics = self.predictions_score = self.score_rating = self.score_loss = None
        self._graph = graph
        self._graphed = None
        self._graph_key = None

    def _forward(self, args):
        # trainer/trainer.py:28-35: two tensors -> model(a, b); one -> model(x)
        if len(args) not in (1, 2):
            raise ValueError("Invalid number of arguments provided to train_loop")
        return self.model(*args)

    def train_loop(self, *args, train_rating):
        """zero_grad, forward, loss, backward, optimizer.step (trainer/trainer.py:23-40)"""
        if len(args) not in (1, 2):
            raise ValueError("Invalid number of arguments provided to train_loop")
        self.model.train()
        if self._graph:
            key = tuple(t.data_ptr() for t in args) + (train_rating.data_ptr(),)
            if self._graphed is None or key != self._graph_key:
                from ..graph import GraphedStep
                self._graphed = GraphedStep(self.model, self.loss_fn, args, train_rating)
                self._graph_key = key
            self.train_loss = self._graphed()
            self.predictions_train = self._graphed.prob
        else:
            self.optimizer.zero_grad()
            self.predictions_train = self._forward(args)
            self.train_loss = self.loss_fn(self.predictions_train, train_rating)
            self.train_loss.backward()
        self.optimizer.step()
        self.train_rating = train_rating

    def _eval_loop(self, args, rating):
        self.model.eval()
        with torch.no_grad():
            pred = self._forward(args)
            loss = self.loss_fn(pred, rating)
        return pred, loss

    def valid_loop(self, *args, valid_rating):
        self.predictions_valid, self.valid_loss = self._eval_loop(args, valid_rating)
        self.valid_rating = valid_rating

    def test_loop(self, *args, test_rating):
        self.predictions_test, self.test_loss = self._eval_loop(args, test_rating)
        self.test_rating = test_rating

    # masked variants (trainer/trainer.py:81-113, used by the AutoRec scripts)
    def train_loop2(self, train_matrix, mask):
        self.model.train()
        self.optimizer.zero_grad()
        self.predictions_train = self.model(train_matrix)[mask]
        train_rating = train_matrix[mask]
        self.train_loss = self.loss_fn(self.predictions_train, train_rating)
        self.train_loss.backward()
        self.optimizer.step()
        self.train_rating = train_rating

    def valid_loop2(self, valid_matrix, mask):
        self.model.eval()
        with torch.no_grad():
            self.predictions_valid = self.model(valid_matrix)[mask]
            self.valid_rating = valid_matrix[mask]
            self.valid_loss = self.loss_fn(self.predictions_valid, self.valid_rating)

    def test_loop2(self, test_matrix, mask):
        self.model.eval()
        with torch.no_grad():
            self.predictions_test = self.model(test_matrix)[mask]
            self.test_rating = test_matrix[mask]
            self.test_loss = self.loss_fn(self.predictions_test, self.test_rating)

    # mini-batch epochs over a data.DeviceLoader (no counterpart in the reference, which trains full-batch)
    def _eager_batch(self, args, rating):
        """one eager step that leaves the captured graph usable: the graph's replays write the .grad tensors made at
        capture, and zero_grad(set_to_none=True) would put fresh ones in their place, so they are set aside"""
        params = [p for group in self.optimizer.param_groups for p in group["params"]]
        kept = [p.grad for p in params] if self._graphed is not None else None
        self.optimizer.zero_grad()
        pred = self._forward(args)
        loss = self.loss_fn(pred, rating)
        loss.backward()
        self.optimizer.step()
        if kept is not None:
            for p, g in zip(params, kept):
                p.grad = g
        return pred, loss

    def _check_groups(self, loader):
        size = getattr(self.loss_fn, "group_size", None)
        if size is None:
            return
        if not (getattr(loader, "grouped", False) or not loader.shuffle):
            raise ValueError("train_epoch: a group loss needs a loader built with grouped=True (or shuffle=False): a "
                             "shuffled epoch scatters a positive and its negatives over the batches")
        if getattr(loader, "negatives", 0) + 1 != size:
            raise ValueError(f"train_epoch: the loss reads groups of {size}, the loader draws "
                             f"{getattr(loader, 'negatives', 0)} negatives per positive")
        if loader.batch_size % size:
            raise ValueError(f"train_epoch: batch_size {loader.batch_size} is not a multiple of the group size {size}")

    def train_epoch(self, loader, epoch):
        """one optimizer step per batch of ``loader.epoch(epoch)``.  With ``graph=True`` the full-size batches replay
        ONE graph captured over the loader's static buffers (the loader launch runs eagerly in front of each replay);
        the tail batch has buffers of its own and runs eagerly, so it never replaces the captured graph.
        ``train_loss``: sample-weighted mean of the batch losses; predictions / rating: those of the last batch.
        A loss over groups (one that has ``group_size``: ``loss.BPRLoss``, ``loss.SampledSoftmaxLoss``) needs a loader
        that delivers whole groups of that size."""
        self._check_groups(loader)
        held = getattr(self.loss_fn, "log_q", None)
        if held is not None and not torch.is_tensor(held) and held is not loader:
            raise ValueError("train_epoch: the loss corrects with the log-q column of another loader than the one it is "
                             "given")
        self.model.train()
        static = loader.static_batch()
        total = torch.zeros((), dtype=torch.float64, device=loader.device)
        samples = 0
        pred = rating = None
        for args, rating in loader.epoch(epoch):
            if self._graph and static is not None and rating is static[1]:
                key = tuple(t.data_ptr() for t in args) + (rating.data_ptr(),)
                if self._graphed is None or key != self._graph_key:
                    from ..graph import GraphedStep
                    self._graphed = GraphedStep(self.model, self.loss_fn, args, rating)
                    self._graph_key = key
                loss, pred = self._graphed(), self._graphed.prob
                self.optimizer.step()
            else:
                pred, loss = self._eager_batch(args, rating)
            total.add_(loss.detach(), alpha=rating.shape[0])
            samples += rating.shape[0]
        if samples == 0:
            raise ValueError("train_epoch: the loader has no batch for this rank")
        self.train_loss = (total / samples).float()
        self.predictions_train, self.train_rating = pred, rating

    def _eval_epoch(self, loader):
        """unshuffled pass under no_grad -> (predictions (N, ...), ratings (N, ...), sample-weighted mean loss)"""
        self.model.eval()
        n = loader.num_rank_samples
        if n == 0:
            raise ValueError("the loader has no batch for this rank")
        total = torch.zeros((), dtype=torch.float64, device=loader.device)
        preds = ratings = None
        done = 0
        with torch.no_grad():
            for args, rating in loader.epoch(0, shuffle=False):
                pred = self._forward(args)
                if preds is None:
                    preds = torch.empty((n,) + tuple(pred.shape[1:]), dtype=pred.dtype, device=pred.device)
                    ratings = torch.empty((n,) + tuple(rating.shape[1:]), dtype=rating.dtype, device=rating.device)
                count = rating.shape[0]
                preds[done:done + count] = pred
                ratings[done:done + count] = rating
                total.add_(self.loss_fn(pred, rating), alpha=count)
                done += count
        return preds, ratings, (total / n).float()

    def valid_epoch(self, loader):
        self.predictions_valid, self.valid_rating, self.valid_loss = self._eval_epoch(loader)

    def test_epoch(self, loader):
        self.predictions_test, self.test_rating, self.test_loss = self._eval_epoch(loader)

    def rank_epoch(self, loader, negatives=None, cutoffs=(10,)):
        """sampled leave-one-out evaluation: an unshuffled pass over a loader whose samples lie in groups of
        1 + ``negatives``, the positive first (``data.LeaveOneOut``'s loaders, or a ``DeviceLoader`` that draws its own
        negatives, whose count is the default), then HR@c / NDCG@c / MRR@c for every c of ``cutoffs`` and MRR from
        the gathered predictions (``evaluator.sampled``).  Keeps and returns ``rank_metrics``; the predictions, ratings
        and loss of the pass are kept as ``predictions_rank`` / ``rank_rating`` / ``rank_loss``."""
        from ..evaluator.sampled import group_ranking_metrics
        if negatives is None:
            negatives = getattr(loader, "negatives", 0)
            if negatives < 1:
                raise ValueError("rank_epoch: the loader draws no negatives of its own; pass negatives=k")
        negatives = int(negatives)
        if negatives < 1:
            raise ValueError("rank_epoch: negatives must be positive")
        if loader.world != 1:
            raise ValueError("rank_epoch: the batches of a loader with world > 1 interleave across ranks and break the "
                             "groups; evaluate with a world=1 loader")
        if loader.num_samples % (1 + negatives):
            raise ValueError(f"rank_epoch: {loader.num_samples} samples are not groups of 1 + {negatives}")
        self.predictions_rank, self.rank_rating, self.rank_loss = self._eval_epoch(loader)
        self.rank_metrics = group_ranking_metrics(self.predictions_rank, negatives, cutoffs)
        return self.rank_metrics

    def score_epoch(self, loader, groups=None):
        """score-level evaluation: an unshuffled pass over ``loader``, then log-loss, the thresholded metrics,
        calibration, RMSE and AUC of the gathered predictions, and with ``groups`` -- the ``evaluator.UserGroups`` of
        ``loader.user_ids()``, built once per evaluation set -- GAUC (``evaluator.score``).  The log-loss is there
        whatever ``loss_fn`` is.  Keeps and returns ``score_metrics``; the predictions, ratings and loss of the pass are
        kept as ``predictions_score`` / ``score_rating`` / ``score_loss``."""
        from ..evaluator.score import score_metrics
        if groups is not None:
            if loader.world != 1:
                raise ValueError("score_epoch: a loader with world > 1 shows this rank a part of the samples, and the "
                                 "groups are those of all of them; evaluate with a world=1 loader")
            if groups.num_samples != loader.num_samples:
                raise ValueError(f"score_epoch: the groups hold {groups.num_samples} samples, the loader "
                                 f"{loader.num_samples}")
        self.predictions_score, self.score_rating, self.score_loss = self._eval_epoch(loader)
        self.score_metrics = score_metrics(self.score_rating, self.predictions_score, groups)
        return self.score_metrics

    def model_eval(self, epoch):
        """prints the reference's per-epoch report (trainer/trainer.py:116-146)"""
        # the report syncs on loss.item() anyway: the place to surface a bad id seen by any step since the
        # last report (the HIP modules flag it on the device instead of asserting like nn.Embedding)
        check = getattr(self.model, "check_bad_index", None)
        if check is not None:
            check()
        ev = Evaluator()
        tr = ev.eval(self.train_rating, self.predictions_train)
        va = ev.eval(self.valid_rating, self.predictions_valid)
        te = ev.eval(self.test_rating, self.predictions_test)
        names = ["Accuracy", "Precision", "Recall", "F1 Score", "ROC AUC Score"]
        lines = [f"        Epoch {epoch + 1}:",
                 f"          - Training Loss: {self.train_loss.item()}",
                 f"          - Valid Loss: {self.valid_loss.item()}",
                 f"          - Test Loss: {self.test_loss.item()}", ""]
        for k, n in enumerate(names):
            lines += [f"          - Training {n}: {tr[k]}", f"          - Valid {n}: {va[k]}",
                      f"          - Test {n}: {te[k]}", ""]
        print("\n" + "\n".join(lines))
        return tr, va, te
