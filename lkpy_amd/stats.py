"""``lenskit.stats``: the Gini coefficient (``stats.py:21-61``)."""

from __future__ import annotations

import warnings

import numpy as np

from .knn import DataWarning


def gini(xs) -> float:
    """
    The Gini coefficient of the non-negative values ``xs`` (``stats.py:44-61``): the sorted
    values against their centred ranks, without a zero adjustment; warns on negative values and
    on a total that is not positive.
    """
    xs = np.asarray(xs)
    if np.any(xs < 0):
        warnings.warn("Gini coefficient is not defined for negative values", DataWarning,
                      stacklevel=2)
    n = len(xs)
    xs = np.sort(xs)
    ranks = np.arange(1, n + 1, dtype=np.float64)
    ranks *= 2
    ranks -= n + 1
    num = np.sum(xs * ranks)
    denom = n * np.sum(xs, dtype=np.float64)
    if denom <= 0:
        warnings.warn("Gini coefficient is not defined for non-positive totals", DataWarning,
                      stacklevel=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return max(num / denom, 0)
