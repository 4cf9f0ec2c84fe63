"""
CPU restatement, in plain NumPy / float64, of the exposure, diversity, popularity and reranking
metrics of ``lenskit.metrics`` (``ranking/_gini.py``, ``_entropy.py``, ``_ils.py``, ``_pop.py``,
``reranking/_rbo.py``, ``_lip.py``, ``stats.gini``), list by list and in the order the reference
takes every step.  The yardstick of ``tests/test_diversity_host.py`` and
``tests/test_gpu_diversity.py``: the code under test is never its own reference.

A list is an array of item NUMBERS in rank order, already free of padding; a number that is
negative or ``>= n_items`` stands for an item the metric's vocabulary does not know.
"""
from __future__ import annotations

import numpy as np

NAN = float("nan")


def geometric_weight(ranks, patience=0.85):  # ranking/_weighting.py:79-84
    return np.exp(np.log(patience) * (np.asarray(ranks) - 1))


def truncate(recs, n):
    recs = np.asarray(recs)
    return recs[:n] if n is not None and len(recs) > n else recs


# ---- stats.gini, GiniAccumulator -----------------------------------------------------------


def gini(xs):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    n = len(xs)
    ranks = np.arange(1, n + 1, dtype=np.float64)
    ranks *= 2
    ranks -= n + 1
    num = np.sum(xs * ranks)
    denom = n * np.sum(xs, dtype=np.float64)
    return max(num / denom, 0)


def exposure_totals(lists, n_items, n=None, weight=None, totals=None):
    """``for list in lists: totals[items] += weights`` one addition after the other; ``weight``
    maps ranks to weights (None: every weight is 1.0, ListGini)."""
    totals = np.zeros(n_items) if totals is None else totals
    for recs in lists:
        recs = truncate(recs, n)
        w = np.ones(len(recs)) if weight is None else weight(np.arange(1, len(recs) + 1))
        for item, wi in zip(recs, w):
            if 0 <= item < n_items:
                totals[item] += wi
    return totals


def gini_of_totals(totals):  # GiniAccumulator.accumulate
    return gini(totals / totals.sum())


# ---- category matrices: normalize_matrix, ILS, entropy -------------------------------------


def normalize_rows(mat, mode):
    mat = np.asarray(mat, dtype=np.float64)
    if mode == "unit":
        stats = np.linalg.norm(mat, axis=1)
    else:
        stats = mat.sum(axis=1)
    stats[stats == 0] = 1.0
    return mat / stats[:, None]


def known(recs, n_items, n=None):
    recs = truncate(recs, n)
    return recs[(recs >= 0) & (recs < n_items)], recs


def ils(recs, vectors, n=None):
    "``vectors``: the unit-normalised dense item x category matrix"
    items, recs = known(recs, len(vectors), n)
    if len(recs) == 0 or len(items) == 0:
        return NAN
    k = len(items)
    if k <= 1:
        return 1.0
    v = vectors[items]
    sim = v @ v.T
    return float(np.sum(np.triu(sim, 1)) / (k * (k - 1) / 2))


def column_entropy(matrix, weights=None):
    if matrix.shape[0] == 0 or matrix.shape[1] == 0:
        return NAN
    if weights is not None:
        matrix = matrix * weights[:, np.newaxis]
    values = np.asarray(matrix.sum(axis=0)) + 1e-6
    probs = values / np.sum(values)
    return float(-np.sum(probs * np.log2(probs)))


def entropy(recs, dist, n=None, weight=None):
    """``dist``: the distribution-normalised dense matrix.  With ``weight`` (ranks -> weights)
    every known item keeps the weight of its own rank in the truncated list."""
    items, recs = known(recs, len(dist), n)
    if len(items) == 0:
        return NAN
    w = None
    if weight is not None:
        ok = (recs >= 0) & (recs < len(dist))
        w = weight(np.arange(1, len(recs) + 1))[ok]
    return column_entropy(dist[items], w)


# ---- MeanPopRank ---------------------------------------------------------------------------


def pop_table(counts):
    "average ranks (ties share the mean of their places) of the positive counts / their number"
    counts = np.asarray(counts, dtype=np.float64)
    table = np.zeros(len(counts))
    pos = np.flatnonzero(counts > 0)
    vals = counts[pos]
    for j, i in enumerate(pos):
        below = np.sum(vals < vals[j])
        same = np.sum(vals == vals[j])
        table[i] = (below + (same + 1) / 2) / len(pos)
    return table


def mean_pop_rank(recs, table, n=None):
    recs = truncate(recs, n)
    if len(recs) == 0:
        return NAN
    q = np.array([table[i] if 0 <= i < len(table) else 0.0 for i in recs])
    return float(q.mean())


# ---- reranking: RBO, LIP -------------------------------------------------------------------


def rbo_sum(reference, reranked, weights):
    "(the sum of agreement x weight over the depths, the sequentially summed total weight)"
    reference, reranked = np.asarray(reference), np.asarray(reranked)
    total_sum, total_weights = 0, 0
    for d, w in enumerate(weights, start=1):
        overlap = len(np.intersect1d(reference[:d], reranked[:d], assume_unique=True))
        agreement = overlap / d
        total_sum += agreement * w
        total_weights += w
    return total_sum, total_weights


def rbo(reference, reranked, n=10, weight=geometric_weight):
    s, t = rbo_sum(reference, reranked, weight(np.arange(1, n + 1)))
    return s / t


def lip(reference, reranked, n=10):
    reference = np.asarray(reference)
    if len(reference) == 0:
        return NAN
    lip_rank = n
    for item in np.asarray(reranked)[:n]:
        (at,) = np.where(reference == item)
        if at.size > 0:
            lip_rank = max(lip_rank, at[0])
    return lip_rank - n
