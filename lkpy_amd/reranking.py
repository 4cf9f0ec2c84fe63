"""
FA*IR top-N reranking: ``lenskit.reranking.fair.FAIRReranker`` (src/lenskit/reranking/fair.py,
Zehlike et al. 2017, https://doi.org/10.1145/3132847.3132938) -- a ranked list and a binary
protected flag per item in, the top n out such that every prefix of i + 1 items holds at least
``m[i]`` protected ones where the list has them to give.

Training is host work (float64, ``scipy.stats.binom``, as the reference does it): the thresholds
``m`` of a binomial test at significance ``alpha_c``, and ``alpha_c`` itself by bisection so that
the test over all n prefixes together rejects a fair ranking with probability ``alpha``
(Algorithm 1 of the paper).  Reranking runs on the device, one list (``__call__``) or a batch of
lists in one launch (:meth:`FAIRReranker.rerank_batch`), through ``lk_fair_rerank``
(csrc/fair.hip).  There is no host path.

The protected flag is ``data.item_attrs[protected_attribute]``: a 1-D array-like with one value
per item number.  An item is protected iff ``np.equal(value, True)``.
"""

from __future__ import annotations

import logging

import numpy as np
from pydantic import BaseModel, Field, PositiveInt, field_validator
from scipy.stats import binom

from . import _native
from .data import ItemList
from .pipeline import Component
from .training import TrainingOptions

_log = logging.getLogger(__name__)

__all__ = ["FAIRReranker", "FAIRRerankerConfig"]


class FAIRRerankerConfig(BaseModel, extra="forbid"):
    "fair.py:29-58"

    n: PositiveInt  # the length of the reranked list (at most ``_native.FAIR_MAX_N``)
    p: float = Field(0.5, gt=0.0, lt=1.0)  # the target share of protected items
    alpha: float = Field(0.1, gt=0.0, lt=1.0)  # type-I error over all prefixes together
    protected_attribute: str = "protected"  # the item attribute holding the flag

    @field_validator("n")
    @classmethod
    def _n_within_kernel_limit(cls, n):
        if n > _native.FAIR_MAX_N:
            raise ValueError(f"n = {n} is over the reranking kernel's limit of "
                             f"{_native.FAIR_MAX_N} (LK_FAIR_MAX_N)")
        return n


def m_table(n: int, p: float, alpha: float) -> np.ndarray:
    "m[i]: the protected items a prefix of i + 1 needs at significance ``alpha`` (fair.py:85-91)"
    sizes = np.arange(1, n + 1)
    return np.clip(binom.ppf(alpha, sizes, p), 0, sizes).astype(int)


def block_sizes(m) -> np.ndarray:
    "the distances between the positions where m increases (fair.py:93-102)"
    m = np.asarray(m)
    if len(m) == 0 or int(m[-1]) == 0:
        return np.zeros(0, dtype=np.int64)
    steps = np.flatnonzero(np.diff(m, prepend=0)) + 1
    return np.diff(steps, prepend=0)


def rejection_probability(n: int, p: float, alpha_c: float, pmf_cache: dict | None = None):
    """
    The probability that a ranking drawn with protected share ``p`` fails the test at some prefix
    (fair.py:104-128): the distribution of the protected count is carried block by block
    (convolved with Bin(block, p)) and the entry j - 1 is struck after block j.
    """
    pmf_cache = {} if pmf_cache is None else pmf_cache
    dist = np.array([1.0], dtype=np.float64)
    for j, size in enumerate(block_sizes(m_table(n, p, alpha_c)), start=1):
        if size not in pmf_cache:
            pmf_cache[size] = binom.pmf(np.arange(size + 1), size, p)
        dist = np.convolve(pmf_cache[size], dist)
        dist[j - 1] = 0
    return float(1 - dist.sum())


def adjusted_alpha(n: int, p: float, alpha: float, tolerance: float = 1e-10,
                   max_iter: int = 100) -> float:
    "``alpha_c`` by bisection on [0, 1] (fair.py:130-145)"
    low, high = 0, 1
    cache: dict = {}
    for _ in range(max_iter):
        mid = (low + high) / 2
        prob = rejection_probability(n, p, mid, cache)
        if prob > alpha:
            high = mid
        else:
            low = mid
        if abs(prob - alpha) < tolerance or high - low < tolerance:
            break
    return (low + high) / 2


class FAIRReranker(Component):
    """
    FA*IR reranking (``FAIRReranker``, fair.py:61-248).  ``train`` computes ``alpha_c`` and
    ``m_list`` and reads the protected flags; ``__call__`` reranks one ordered list,
    :meth:`rerank_batch` a [B x L] batch of item numbers.
    """

    config: FAIRRerankerConfig

    alpha_c: float
    m_list: np.ndarray

    def is_trained(self):
        return hasattr(self, "alpha_c")

    def train(self, data, options: TrainingOptions = TrainingOptions()):
        cfg = self.config
        attrs = getattr(data, "item_attrs", {})
        if cfg.protected_attribute not in attrs:
            raise ValueError(f"Dataset is missing required '{cfg.protected_attribute}' attribute "
                             "for item entities")
        flags = np.asarray(attrs[cfg.protected_attribute])
        if flags.ndim != 1 or len(flags) != data.item_count:
            raise ValueError(f"item attribute '{cfg.protected_attribute}' must hold one value per "
                             f"item ({data.item_count}), got shape {flags.shape}")
        alpha_c = adjusted_alpha(cfg.n, cfg.p, cfg.alpha)
        self.m_list = m_table(cfg.n, cfg.p, alpha_c)
        self.protected_attributes = np.equal(flags, True).astype(np.bool_)
        self.vocab = data.items
        self.alpha_c = alpha_c
        _log.info("FA*IR thresholds for n=%d, p=%.2f, alpha=%.2f: alpha_c=%.8f", cfg.n, cfg.p,
                  cfg.alpha, alpha_c)

    # -- device state ---------------------------------------------------------------------------
    def _device_tables(self):
        "(flags uint8 [n_items], thresholds int32 [n]) in HBM"
        import torch

        from . import _device as D

        def build():
            dev = D.device()
            flags = np.ascontiguousarray(self.protected_attributes, dtype=np.uint8)
            m = np.ascontiguousarray(self.m_list, dtype=np.int32)
            return torch.from_numpy(flags).to(dev), torch.from_numpy(m).to(dev)

        return self._device_cache("fair", build, self.protected_attributes, self.m_list)

    def _length(self, n: int | None) -> int:
        limit = self.config.n
        if n is not None:
            if n > limit:
                raise ValueError(f"The requested rerank length n={n}, exceeds configured "
                                 f"n={limit}.")
            if n < limit:
                _log.warning("FA*IR: model trained for n=%d used on n=%d; fairness test might be "
                             "violated.", limit, n)
        return int(n or limit)

    # -- one list ---------------------------------------------------------------------------------
    def __call__(self, items: ItemList, n: int | None = None) -> ItemList:
        import torch

        from . import _device as D

        dev = D.device()
        n = min(self._length(n), len(items))
        if n == 0:
            return ItemList(items[np.zeros(0, dtype=np.int64)], ordered=True)
        nums = np.ascontiguousarray(items.numbers(vocabulary=self.vocab, missing="negative"),
                                    dtype=np.int32).reshape(1, -1)
        flags, m = self._device_tables()
        lengths = torch.full((1,), nums.shape[1], dtype=torch.int32, device=dev)
        _items, _scores, pos = D.fair_rerank(torch.from_numpy(nums).to(dev), flags, m, n,
                                             lengths=lengths, want_pos=True)
        positions = pos[0].cpu().numpy().astype(np.int64)
        return ItemList(items[positions], ordered=True)

    # -- batches ----------------------------------------------------------------------------------
    def rerank_batch(self, lists, scores=None, n: int | None = None, *, lengths=None,
                     device_output: bool = False):
        """
        Rerank every row of ``lists`` (int32 [B x L] item numbers of this reranker's vocabulary, a
        host array or a device tensor) in one launch.  ``lengths=None``: a row ends at its first
        negative entry (the trailing -1 padding of ``recommend_batch``); with ``lengths`` (int32
        [B]) a negative entry inside a row is an unknown item and counts as unprotected.
        ``scores``: float32 in the shape of ``lists``, carried along bit for bit.  Returns (items
        [B x n] with -1 padding, scores [B x n] with NaN padding or None), host arrays or
        (``device_output``) device tensors; a row shorter than n gives a list of its own length.
        """
        import torch

        from . import _device as D

        dev = D.device()
        n = self._length(n)

        def on_device(a, dtype):
            if a is None:
                return None
            if not isinstance(a, torch.Tensor):
                a = torch.from_numpy(np.ascontiguousarray(
                    a, dtype=np.float32 if dtype == torch.float32 else np.int32))
            a = a.to(device=dev, dtype=dtype)
            return a if a.dim() < 2 or a.shape[1] <= 1 or a.stride(1) == 1 else a.contiguous()

        d_lists = on_device(lists, torch.int32)
        if d_lists.dim() != 2:
            raise ValueError("lists must be a [B x L] array of item numbers")
        d_scores = on_device(scores, torch.float32)
        if d_scores is not None:
            if d_scores.shape != d_lists.shape:
                raise ValueError("scores must have the shape of lists")
            if d_scores.stride(0) != d_lists.stride(0):
                d_lists, d_scores = d_lists.contiguous(), d_scores.contiguous()
        d_len = on_device(lengths, torch.int32)
        if d_len is not None:
            d_len = d_len.contiguous()
            if d_len.shape != (d_lists.shape[0],):
                raise ValueError("lengths must hold one entry per row of lists")
        flags, m = self._device_tables()
        out, out_sc, _pos = D.fair_rerank(d_lists, flags, m, n, lengths=d_len, scores=d_scores)
        if device_output:
            return out, out_sc
        if out_sc is None:
            return D.to_host(out), None
        return D.lists_to_host(out, out_sc)
