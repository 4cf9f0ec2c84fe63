"""
CPU restatement of ``lenskit.metrics`` **per list**, in plain NumPy on id arrays, following the
reference's ``measure_list`` bodies line by line; every float sum is taken with ``math.fsum``
(exact, then rounded once).  The yardstick of ``tests/test_metrics_host.py`` and
``tests/test_gpu_metrics.py``: the code under test is never its own reference.

A list is ``recs`` (item ids in rank order, already free of padding) and a test list is ``test``
(item ids) with optional ``gains`` / ``ratings`` (float32, aligned with ``test``).
"""
from __future__ import annotations

import math

import numpy as np

NAN = float("nan")


# ranking/_weighting.py:79-84 and 118-122
def geometric_weight(ranks, patience=0.85):
    return np.exp(np.log(patience) * (np.asarray(ranks) - 1))


def log_weight(ranks, base=2, offset=0):
    ranks = np.asarray(ranks)
    if offset > 0:
        return np.log(base) / np.log(ranks + offset)
    return np.log(base) / np.log(np.maximum(ranks, 2))


def truncate(recs, n):  # ranking/_base.py:63-73
    recs = np.asarray(recs)
    if n is not None and len(recs) > n:
        return recs[:n]
    return recs


def hit(recs, test, n=None):  # _hit.py:36-42
    if len(test) == 0:
        return NAN
    recs = truncate(recs, n)
    return 1 if np.any(np.isin(recs, test)) else 0


def recip_rank(recs, test, n=None):  # _recip.py:40-50
    if len(test) == 0:
        return NAN
    recs = truncate(recs, n)
    good = np.isin(recs, test)
    (npz,) = np.nonzero(good)
    if len(npz):
        return 1.0 / (npz[0] + 1.0)
    return 0.0


def precision(recs, test, n=None):  # _pr.py:38-45
    recs = truncate(recs, n)
    if len(recs) == 0:
        return NAN
    return int(np.isin(recs, test).sum()) / len(recs)


def recall(recs, test, n=None):  # _pr.py:64-71
    recs = truncate(recs, n)
    ngood = int(np.isin(recs, test).sum())
    nrel = len(test)
    if n is not None and n < nrel:
        nrel = n
    return ngood / nrel if nrel else NAN  # (numpy's 0 / 0)


def average_precision(recs, test, n=None):  # _map.py:30-44
    recs = truncate(recs, n)
    if len(recs) == 0:
        return NAN
    good = np.isin(recs, test)
    sum_good = np.cumsum(good)
    ranks = np.arange(1, len(recs) + 1)
    ap_sum = math.fsum(int(c) / int(r) for c, r in zip(sum_good[good], ranks[good]))
    denom = min(len(test), len(recs))
    if denom == 0:
        return NAN  # the reference raises ZeroDivisionError here (the one stated deviation)
    return ap_sum / denom


def _binary_dcg(recs, test, weight):  # _dcg.py:248-255
    good = np.isin(recs, test)
    ranks = np.arange(1, len(recs) + 1)
    return math.fsum(weight(ranks[good]))


def _graded_dcg(recs, test, gains, weight):  # _dcg.py:224-245
    gains = np.asarray(gains, dtype=np.float32)
    keep = ~np.isnan(gains)  # dropna
    if not keep.any():
        return NAN
    t_ids, g = np.asarray(test)[keep], np.maximum(gains[keep], np.float32(0))  # clip(lower=0)
    lookup = dict(zip(t_ids.tolist(), g.tolist()))  # (float32 values widened exactly)
    total = []
    for rank, item in enumerate(np.asarray(recs).tolist(), start=1):
        if item in lookup:  # ranks.align(gains, join="inner")
            total.append(lookup[item] * float(weight(np.array([rank]))[0]))
    return math.fsum(total)


def fixed_dcg(n, weight):  # _dcg.py:293-301
    return math.fsum(weight(np.arange(1, n + 1)))


def dcg(recs, test, n=None, weight=log_weight, gains=None):  # _dcg.py:211-221
    recs = truncate(recs, n)
    if len(test) == 0:
        return NAN
    if gains is not None:
        return _graded_dcg(recs, test, gains, weight)
    return _binary_dcg(recs, test, weight)


def ndcg(recs, test, n=None, weight=log_weight, gains=None):  # _dcg.py:108-145
    recs = truncate(recs, n)
    if len(test) == 0:
        return NAN
    if gains is not None:
        realized = _graded_dcg(recs, test, gains, weight)
        g = np.asarray(gains, dtype=np.float32)
        g = g[~np.isnan(g)]
        if len(g) == 0:
            return NAN
        g = np.maximum(g, np.float32(0))
        g = np.sort(g)[::-1]
        if n:
            g = g[:n]  # nlargest(n)
        iw = weight(np.arange(1, len(g) + 1))
        ideal = math.fsum(float(a) * float(b) for a, b in zip(g, iw))
        if ideal == 0:
            return 0.0
    else:
        realized = _binary_dcg(recs, test, weight)
        k = len(test)
        if n and n < k:
            k = n
        ideal = fixed_dcg(k, weight)
    return realized / ideal


def rbp(recs, test, n=None, weight=geometric_weight, series_sum=1 / (1 - 0.85),
        normalize=False):  # _rbp.py:130-162
    recs = truncate(recs, n)
    k = len(recs)
    nrel = len(test)
    if nrel == 0:
        return NAN
    good = np.isin(recs, test)
    weights = weight(np.arange(1, k + 1))
    if normalize:
        normalization = math.fsum(weights[: min(nrel, k)])
    elif series_sum is not None:
        normalization = series_sum
    else:
        normalization = math.fsum(weights)
    if normalization == 0:
        return NAN  # (ZeroDivisionError in the reference: an empty list)
    return math.fsum(weights[good]) / normalization


def int_stats(recs, test, n=None):
    "(n_recs, n_hits, first_hit) of a list inside cutoff n"
    recs = truncate(recs, n)
    good = np.isin(recs, test)
    (npz,) = np.nonzero(good)
    return len(recs), int(good.sum()), int(npz[0]) + 1 if len(npz) else 0


def predict_errors(p_ids, p_scores, t_ids, t_ratings):
    """
    predict.py:93-109 + 134-137 / 166-169: (sse, sae, n, n_missing_score, n_missing_truth); the
    elements are float32 operations as on two float32 series, summed exactly.
    """
    p_scores = np.asarray(p_scores, dtype=np.float32)
    t_ratings = np.asarray(t_ratings, dtype=np.float32)
    truth = dict(zip(np.asarray(t_ids).tolist(), range(len(t_ids))))
    sq, ab, n, seen = [], [], 0, set()
    miss_truth = 0
    for item, s in zip(np.asarray(p_ids).tolist(), p_scores):
        j = truth.get(item)
        r = t_ratings[j] if j is not None else np.float32(np.nan)
        if not np.isnan(s) and np.isnan(r):
            miss_truth += 1
        if np.isnan(s) or np.isnan(r):
            continue
        seen.add(item)
        with np.errstate(all="ignore"):
            e = np.float32(s - r)
            if np.isnan(e):
                continue
            sq.append(float(np.float32(e * e)))
            ab.append(float(np.float32(abs(e))))
        n += int(np.isfinite(e))
    rated = {i for i, r in zip(np.asarray(t_ids).tolist(), t_ratings) if not np.isnan(r)}
    return math.fsum(sq), math.fsum(ab), n, len(rated - seen), miss_truth


def value_stats(values):  # data/accum/_value.py:46-64
    v = np.asarray([x for x in values if x is not None and not np.isnan(x)], dtype=np.float64)
    return {"n": len(v), "mean": np.mean(v).item(), "median": np.median(v).item(),
            "std": np.std(v).item()}
