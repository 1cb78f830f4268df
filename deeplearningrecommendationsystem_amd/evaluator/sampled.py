"""Sampled leave-one-out evaluation: every held-out positive ranked against k sampled negatives, the "1 positive + 99
negatives, HR@10 / NDCG@10" protocol of the NeuralCF paper (csrc/group_eval.hip).  The reference has no such stage; the
numbers are its ``Ranking``'s on one-item ground truths (Recall@c = HR@c, Mean NDCG@c, MAP@c = MRR@c, MRR).

Scores come in groups of 1 + k, slot 0 the positive -- the order of an unshuffled pass over a ``data.LeaveOneOut``
loader or over a ``DeviceLoader`` that draws its own negatives.  The device computes

    rank[g] = #{ j in 1..k : not (scores[g, j] < scores[g, 0]) }          hist[r] = #{ g : rank[g] == r }

with integers only: ties and NaN count against the positive, so a constant-output model ranks k and scores HR = 0
(saturated sigmoids tie often, and "lower slot first" would hand every tie to the positive).  Every metric follows on
the host in float64 from the k + 1 counts, w_r = hist[r] / N:

    HR@c = sum_{r<c} w_r     NDCG@c = sum_{r<c} w_r / log2(r + 2)     MRR@c = sum_{r<c} w_r / (r + 1)     MRR = MRR@(k+1)

There is no CPU fallback.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import ops

__all__ = ["GroupRankingMetrics", "group_ranks", "group_histogram", "group_ranking_metrics", "metrics_from_histogram"]


class GroupRankingMetrics(namedtuple("GroupRankingMetrics", "hr ndcg mrr_at mrr groups histogram")):
    """``hr`` / ``ndcg`` / ``mrr_at``: dicts by cutoff; ``mrr`` over the whole group; ``groups`` = N; ``histogram``:
    the (k + 1,) int64 numpy counts of the ranks"""
    __slots__ = ()

    def report(self) -> str:
        lines = [f"        {self.groups} groups of 1 + {len(self.histogram) - 1} candidates:"]
        for c in self.hr:
            lines.append(f"          - HR@{c}: {self.hr[c]}")
            lines.append(f"          - NDCG@{c}: {self.ndcg[c]}")
            lines.append(f"          - MRR@{c}: {self.mrr_at[c]}")
        lines.append(f"          - MRR: {self.mrr}")
        return "\n".join(lines)


def _groups(scores: torch.Tensor, negatives: int) -> torch.Tensor:
    """the (N, 1 + k) view the kernel reads"""
    k = int(negatives)
    if k < 1:
        raise ValueError(f"negatives = {negatives}: a group needs at least one negative")
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32:
        raise ValueError("scores must be a float32 device tensor")
    if not scores.is_cuda:
        raise RuntimeError("sampled ranking evaluation runs on the HIP device; there is no CPU fallback")
    if scores.dim() == 2 and scores.shape[1] == 1 + k and (scores.shape[0] == 0 or scores.stride(1) == 1) and \
            (scores.shape[0] < 2 or scores.stride(0) >= 1 + k):
        return scores
    if scores.numel() % (1 + k):
        raise ValueError(f"{scores.numel()} scores are not groups of 1 + {k}")
    return scores.contiguous().view(scores.numel() // (1 + k), 1 + k)


def _rank(scores, negatives, hist, want_ranks):
    rows = _groups(scores, negatives)
    k = int(negatives)
    if hist is None:
        hist = torch.zeros(k + 1, dtype=torch.int64, device=rows.device)
    ranks = torch.empty(rows.shape[0], dtype=torch.int32, device=rows.device) if want_ranks else None
    ops.group_rank(rows, k, hist, ranks)
    return ranks, hist


def group_ranks(scores: torch.Tensor, negatives: int) -> torch.Tensor:
    """(N,) int32: how many of its ``negatives`` candidates each positive fails to beat (0 = ranked first)"""
    return _rank(scores, negatives, None, True)[0]


def group_histogram(scores: torch.Tensor, negatives: int, out: torch.Tensor = None) -> torch.Tensor:
    """(k + 1,) int64 counts of the ranks, ADDED to ``out`` when given (an evaluation scored in chunks)"""
    return _rank(scores, negatives, out, False)[1]


def metrics_from_histogram(histogram, cutoffs=(10,)) -> GroupRankingMetrics:
    """the float64 host arithmetic of the module docstring on (k + 1,) counts"""
    hist = np.asarray(histogram.cpu() if isinstance(histogram, torch.Tensor) else histogram, dtype=np.int64)
    groups = int(hist.sum())
    if groups < 1:
        raise ValueError("the histogram holds no group")
    cutoffs = tuple(int(c) for c in cutoffs)
    if any(c < 1 for c in cutoffs):
        raise ValueError("cutoffs must be positive")
    w = hist.astype(np.float64) / groups
    r = np.arange(hist.shape[0], dtype=np.float64)
    gain, recip = w / np.log2(r + 2.0), w / (r + 1.0)
    hr = {c: float(np.sum(w[:c])) for c in cutoffs}
    ndcg = {c: float(np.sum(gain[:c])) for c in cutoffs}
    mrr_at = {c: float(np.sum(recip[:c])) for c in cutoffs}
    return GroupRankingMetrics(hr, ndcg, mrr_at, float(np.sum(recip)), groups, hist)


def group_ranking_metrics(scores: torch.Tensor, negatives: int, cutoffs=(10,)) -> GroupRankingMetrics:
    """HR@c / NDCG@c / MRR@c for every c of ``cutoffs`` and MRR, of scores in groups of 1 + ``negatives`` (any float32
    device tensor of N (1 + k) elements, or (N, 1 + k) with unit inner stride); one launch and one (k + 1)-count copy"""
    return metrics_from_histogram(group_histogram(scores, negatives), cutoffs)
