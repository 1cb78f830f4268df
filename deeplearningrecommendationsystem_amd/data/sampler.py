"""The distribution weighted negatives are drawn from: an alias table over the items, built once on the host
(``build_alias_table``, Vose's method in float64 numpy) and read by the device loader's weighted draw
(csrc/loader.hip, header comment: weighted negatives).

Item ``c`` owns column ``c`` of the table, one 64-bit word ``(thresh_c << 32) | alias_c``: a draw picks a column
uniformly, keeps it when a uniform 32-bit number is below ``thresh_c`` and takes ``alias_c`` otherwise.  A column that
always keeps itself is encoded as ``alias_c == c`` (2^32 does not fit the threshold).  An item of weight 0 is never
drawn: its column has ``thresh == 0`` and an alias of positive weight, and no column aliases to it.

``q`` is the distribution the TABLE implies, from its integers -- not the normalised weights, which the 32-bit
thresholds only approximate (within 2^-33 per item):
    q_i = (own kept mass + sum over c != i with alias_c == i of (2^32 - thresh_c)) / (I * 2^32)
with the own kept mass 2^32 for a column that keeps itself and ``thresh_i`` otherwise.  ``log_q`` is what the loader's
log-q column copies from and ``loss.SampledSoftmaxLoss(log_q=...)`` subtracts: the correction uses the distribution that
is actually drawn from.
"""
from __future__ import annotations

import numpy as np
import torch

_ONE = 1 << 32


def build_alias_table(weights):
    """``weights``: (I,) non-negative finite numbers, at least one positive, I < 2^31 -> ``(thresh, alias)``, (I,) uint32
    and (I,) int64.  Pure host code (float64 numpy)."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    n = w.shape[0]
    if n < 1 or n >= 1 << 31:
        raise ValueError("ItemSampler: need 1 <= number of items < 2^31")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("ItemSampler: the weights must be non-negative and finite")
    total = w.sum()
    if not total > 0 or not np.isfinite(total):
        raise ValueError("ItemSampler: at least one weight must be positive (and their sum finite)")
    p = w * (n / total)                                  # mean 1: a column holds mass 1
    keep = np.ones(n, dtype=np.float64)
    alias = np.arange(n, dtype=np.int64)
    # stacks; the zero-weight columns lie on top of `small`, so they are paired while `large` cannot be empty: the
    # columns left always hold their own count in mass, and the zero ones hold none of it
    positive_small = np.nonzero((p < 1.0) & (w > 0))[0]
    small = positive_small.tolist() + np.nonzero(w == 0)[0].tolist()
    large = np.nonzero(p >= 1.0)[0].tolist()
    p = p.tolist()
    while small and large:
        s, big = small.pop(), large.pop()
        keep[s], alias[s] = p[s], big
        p[big] = (p[big] + p[s]) - 1.0
        (small if p[big] < 1.0 else large).append(big)
    # what is left keeps itself (mass 1 up to rounding) -- except a zero-weight column, which rounding must not let
    # keep itself: it goes to the heaviest item
    heaviest = int(np.argmax(w))
    for s in small:
        if w[s] == 0:
            keep[s], alias[s] = 0.0, heaviest
    thresh = np.rint(np.clip(keep, 0.0, 1.0) * _ONE)
    full = thresh >= _ONE                                # always keeps itself: said by the alias
    alias[full] = np.nonzero(full)[0]
    thresh[full] = _ONE - 1
    thresh[w == 0] = 0
    return thresh.astype(np.uint32), alias


def table_words(thresh, alias):
    """the (I,) uint64 words ``(thresh << 32) | alias``"""
    return (thresh.astype(np.uint64) << np.uint64(32)) | alias.astype(np.uint64)


def implied_q(thresh, alias):
    """(I,) float64: the distribution a table draws from, exactly from its integers (module docstring)"""
    n = thresh.shape[0]
    own = np.arange(n, dtype=np.int64)
    kept = np.where(alias == own, _ONE, thresh.astype(np.int64))
    mass = kept.copy()
    away = alias != own
    np.add.at(mass, alias[away], _ONE - kept[away])      # int64: at most I * 2^32 < 2^63
    return mass.astype(np.float64) / (float(n) * float(_ONE))


class ItemSampler:
    """``ItemSampler(weights)``: draw items in proportion to ``weights`` ((I,) tensor or array, non-negative, finite, one
    positive entry at least; I < 2^31).  ``q`` (I,) float64 on the host and ``log_q`` (I,) float32 on the device are the
    table's own distribution (module docstring; ``-inf`` where ``q == 0``); ``table`` the (I,) words on the device, as
    int64 bits.  ``device``: where ``table`` / ``log_q`` live -- default: that of ``weights`` if it is a device tensor,
    else the current HIP device."""

    def __init__(self, weights, device=None):
        if torch.is_tensor(weights):
            if device is None and weights.is_cuda:
                device = weights.device
            weights = weights.detach().cpu().double().numpy()
        self.thresh, self.alias = build_alias_table(weights)
        self.num_items = int(self.thresh.shape[0])
        self.q = implied_q(self.thresh, self.alias)
        with np.errstate(divide="ignore"):
            self._log_q_host = np.log(self.q).astype(np.float32)
        self._device = device
        self._table = self._log_q = None

    @classmethod
    def popularity(cls, observed, alpha=0.75):
        """weights ``count_i ** alpha`` over the pairs of an ``ObservedPairs`` (``alpha = 0``: 1 for every item that
        occurs), 0 for an item that never occurs"""
        count = torch.bincount(observed.indices.long(), minlength=observed.num_items).cpu().double().numpy()
        weights = np.where(count > 0, np.power(np.maximum(count, 1.0), float(alpha)), 0.0)
        return cls(weights, device=observed.indices.device if observed.indices.is_cuda else None)

    def _to_device(self):
        if self._table is None:
            device = torch.device("cuda", torch.cuda.current_device()) if self._device is None else self._device
            words = table_words(self.thresh, self.alias).view(np.int64)
            self._table = torch.from_numpy(words).to(device)
            self._log_q = torch.from_numpy(self._log_q_host).to(device)

    @property
    def table(self) -> torch.Tensor:
        self._to_device()
        return self._table

    @property
    def log_q(self) -> torch.Tensor:
        self._to_device()
        return self._log_q
