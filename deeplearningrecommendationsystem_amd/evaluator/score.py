"""Score-level evaluation of a CTR model on the device: log-loss, the confusion-matrix metrics, calibration and RMSE
from one pass over ``(y, p)``, and GAUC -- the impression-weighted mean of every user's own AUC, the headline metric of
the DIN and DIEN papers (csrc/score_eval.hip).  The reference has neither: what its evaluator calls "ROC AUC" is the
balanced accuracy of the 0.5-thresholded predictions, kept here under that name.

A sample is positive iff ``y > 0.5`` and a prediction is hard iff ``p >= 0.5`` (``Evaluator.eval``'s rule).  Per user g,
with i over the user's positives and j over the user's negatives, the device counts integers only:

    pos[g], neg[g]          u2[g] = sum_i sum_j ( 2 [p_j < p_i] + [p_j == p_i] )

and the host finishes in float64 over the users that have both classes:

    auc_g = u2[g] / (2 pos[g] neg[g])          GAUC = sum_g (pos[g] + neg[g]) auc_g / sum_g (pos[g] + neg[g])

A NaN score on either side of a pair adds nothing, so it counts against the positive.  Which samples belong to which
user is a plan, ``UserGroups``, built once per evaluation set with torch ops (a stable sort by user and the work lists
of the two kernel arms); the kernels need no sort of the scores.  The global AUC stays ``Evaluator.score_auc``: an
exact one needs a full sort of the scores, which is ``torch.sort``'s job.

There is no CPU fallback for the kernels; ``UserGroups`` and ``gauc_from_counts`` are plumbing and work anywhere.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import _lib, ops
from .evaluator import Evaluator

__all__ = ["UserGroups", "GaucResult", "ScoreMetrics", "user_auc_counts", "gauc_from_counts", "score_metrics"]

SMALL, SLAB, CHUNK = _lib.CTR_GAUC_SMALL, _lib.CTR_GAUC_SLAB, _lib.CTR_SCORE_CHUNK


class UserGroups:
    """The plan of one evaluation set: ``users`` is the (N,) int64 user id of every sample in evaluation order (ids may
    be sparse, large and interleaved in any way).  Group g is one user, ``group_users[g]`` (ascending), and holds the
    samples ``order[offsets[g] : offsets[g + 1]]`` in sample order.  ``small_groups`` lists the groups of at most 64
    samples (one wave each); every larger group of s samples has ``ceil(s / 1024)`` slabs ``(slab_group, slab_first)``,
    ``slab_first`` = 0, 1024, ...  Tensors live on the device ``users`` is on."""

    def __init__(self, users: torch.Tensor):
        if not isinstance(users, torch.Tensor) or users.dtype != torch.int64 or users.dim() != 1:
            raise ValueError("UserGroups: users must be an (N,) int64 tensor")
        n = users.shape[0]
        if n >= 1 << 31:
            raise ValueError("UserGroups: N must be below 2^31 (sample indices are stored as int32)")
        dev = users.device
        ordered, order = torch.sort(users, stable=True)
        self.group_users, sizes = torch.unique_consecutive(ordered, return_counts=True)
        self.order = order.to(torch.int32)
        self.offsets = torch.zeros(sizes.shape[0] + 1, dtype=torch.int64, device=dev)
        torch.cumsum(sizes, 0, out=self.offsets[1:])
        small = sizes <= SMALL
        self.small_groups = torch.nonzero(small).reshape(-1).to(torch.int32)
        large = torch.nonzero(~small).reshape(-1)
        slabs = torch.div(sizes[large] + (SLAB - 1), SLAB, rounding_mode="floor")
        self.slab_group = torch.repeat_interleave(large, slabs).to(torch.int32)
        before = torch.repeat_interleave(torch.cumsum(slabs, 0) - slabs, slabs)     # slabs of the earlier groups
        self.slab_first = ((torch.arange(self.slab_group.shape[0], device=dev) - before) * SLAB).to(torch.int32)
        self.num_samples, self.num_groups = n, int(sizes.shape[0])
        self.max_group = int(sizes.max()) if self.num_groups else 0

    @property
    def device(self):
        return self.order.device

    def sizes(self) -> torch.Tensor:
        """(G,) int64 samples per group"""
        return self.offsets.diff()

    def pair_evaluations(self) -> int:
        """the kernels' cost model: sum over groups of size x (size rounded up to slabs; small groups: size)"""
        s = self.sizes()
        rounded = torch.where(s <= SMALL, s, torch.div(s + (SLAB - 1), SLAB, rounding_mode="floor") * SLAB)
        return int((s * rounded).sum())


GaucResult = namedtuple("GaucResult", "gauc user_auc_mean users_scored samples_scored")


class ScoreMetrics(namedtuple("ScoreMetrics", "samples positives logloss accuracy precision recall f1 balanced_accuracy "
                                              "auc calibration rmse bad gauc user_auc_mean users_scored samples_scored")):
    """``balanced_accuracy`` is what ``Evaluator.eval`` (and the reference) call AUC; ``auc`` is ``Evaluator.score_auc``;
    ``calibration`` = sum p / sum y; ``bad`` = predictions that are NaN or outside [0, 1]; the last four are None
    without ``groups``"""
    __slots__ = ()

    def report(self) -> str:
        lines = [f"        {self.samples} samples, {self.positives} positive:",
                 f"          - LogLoss: {self.logloss}",
                 f"          - AUC: {self.auc}"]
        if self.gauc is not None:
            lines.append(f"          - GAUC: {self.gauc} ({self.users_scored} users, {self.samples_scored} samples scored)")
            lines.append(f"          - Mean user AUC: {self.user_auc_mean}")
        lines += [f"          - Accuracy: {self.accuracy}", f"          - Precision: {self.precision}",
                  f"          - Recall: {self.recall}", f"          - F1 Score: {self.f1}",
                  f"          - Balanced accuracy: {self.balanced_accuracy}",
                  f"          - Calibration: {self.calibration}", f"          - RMSE: {self.rmse}"]
        if self.bad:
            lines.append(f"          - Predictions outside [0, 1] or NaN: {self.bad}")
        return "\n".join(lines)


def _flat_pair(y_true, y_pred):
    """the two contiguous (N,) float32 device vectors the kernels read"""
    out = []
    for name, t in (("y_true", y_true), ("y_pred", y_pred)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or \
                not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1)):
            raise ValueError(f"{name} must be an (N,) or (N, 1) float32 device tensor")
        if not t.is_cuda:
            raise _lib.CtrHipError("score evaluation runs on the HIP device (got a CPU tensor); there is no CPU fallback")
        out.append(t.detach().reshape(-1).contiguous())
    if out[0].shape != out[1].shape:
        raise ValueError(f"y_true holds {out[0].shape[0]} samples, y_pred {out[1].shape[0]}")
    return out


def user_auc_counts(groups: UserGroups, y_true: torch.Tensor, y_pred: torch.Tensor):
    """``(pos, neg, u2)``: (G,) int32, int32 and int64 device tensors of the module docstring, from one launch pair"""
    y, p = _flat_pair(y_true, y_pred)
    if not isinstance(groups, UserGroups) or groups.num_samples != p.shape[0]:
        raise ValueError(f"groups must be the UserGroups of these {p.shape[0]} samples")
    if groups.device != p.device:
        raise ValueError("groups and the predictions must live on one device")
    g, dev = groups.num_groups, p.device
    counts = torch.zeros((2, g), dtype=torch.int32, device=dev)
    u2 = torch.zeros(g, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.gauc_groups(p, y, groups.order, groups.offsets, groups.small_groups, groups.slab_group, groups.slab_first,
                       counts[0], counts[1], u2, err)
    return counts[0], counts[1], u2


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def gauc_from_counts(pos, neg, u2) -> GaucResult:
    """float64 host arithmetic of the module docstring over the groups that have both classes; GAUC and the
    unweighted ``user_auc_mean`` are nan when no group has"""
    pos, neg, u2 = (_host(t).astype(np.int64).reshape(-1) for t in (pos, neg, u2))
    if not pos.shape == neg.shape == u2.shape:
        raise ValueError("pos, neg and u2 must have one length")
    keep = (pos > 0) & (neg > 0)
    users = int(keep.sum())
    if users == 0:
        return GaucResult(float("nan"), float("nan"), 0, 0)
    p, q = pos[keep].astype(np.float64), neg[keep].astype(np.float64)
    auc = u2[keep].astype(np.float64) / (2.0 * p * q)
    weight = p + q
    return GaucResult(float(np.sum(weight * auc) / np.sum(weight)), float(np.mean(auc)), users,
                      int((pos[keep] + neg[keep]).sum()))


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def score_metrics(y_true: torch.Tensor, y_pred: torch.Tensor, groups: UserGroups = None) -> ScoreMetrics:
    """every score-level number of one evaluation set: labels and predictions are float32 device tensors of N elements,
    (N,) or (N, 1).  One ``ctr_score_counts`` launch and two small copies give the pointwise numbers, summed in float64;
    ``auc`` is ``Evaluator.score_auc``; with ``groups`` (the ``UserGroups`` of the samples' users) one
    ``ctr_gauc_groups`` launch pair adds GAUC."""
    y, p = _flat_pair(y_true, y_pred)
    n = p.shape[0]
    if n == 0:
        raise ValueError("score_metrics: no sample")
    if groups is not None and (not isinstance(groups, UserGroups) or groups.num_samples != n):
        raise ValueError(f"groups must be the UserGroups of these {n} samples")
    counts = torch.zeros(8, dtype=torch.int64, device=p.device)
    sums = torch.empty((-(-n // CHUNK), 4), dtype=torch.float64, device=p.device)
    ops.score_counts(p, y, counts, sums)
    gauc = gauc_from_counts(*user_auc_counts(groups, y, p)) if groups is not None else GaucResult(None, None, None, None)
    auc = Evaluator.score_auc(y, p)
    positives, negatives, tp, fp, fn, tn, bad, _ = (int(v) for v in counts.cpu().numpy())
    rows = sums.cpu().numpy()
    bce, sum_p, sum_sq, sum_y = (float(np.cumsum(rows[:, k])[-1]) for k in range(4))   # the rows in chunk order
    precision = tp / max(tp + fp, 1)
    recall = tp / max(tp + fn, 1)
    f1 = 2 * precision * recall / max(precision + recall, 1e-12)
    balanced = 0.5 * (_ratio(tp, tp + fn) + _ratio(tn, tn + fp))
    calibration = sum_p / sum_y if sum_y else float("nan")
    return ScoreMetrics(n, positives, bce / n, (tp + tn) / n, precision, recall, f1, balanced, auc, calibration,
                        float(np.sqrt(sum_sq / n)), bad, *gauc)
