"""
NumPy restatement of the Popular baseline, for the tests: the shared order of a score vector, the
rule of the batch path (``lk_shared_order_topn``: the order with each row's history skipped) as a
plain loop, and the three training rules of ``PopScorer`` written without pandas.
"""

from __future__ import annotations

import numpy as np


def order(scores) -> np.ndarray:
    "item numbers with a non-NaN score by score descending, ties by lower number (int32)"
    scores = np.asarray(scores, np.float32)
    ok = np.flatnonzero(~np.isnan(scores))
    # (-x of -0.0 / +0.0 compare equal, +-inf order as they should; the sort is stable)
    return ok[np.argsort(-scores[ok], kind="stable")].astype(np.int32)


def lists(order_, scores, hist_rows, n: int):
    """
    Row b's list: the first ``n`` (``n < 0``: all) entries of ``order_`` that do not occur in
    ``hist_rows[b]`` (any iterable of item numbers; None: no history), in order.  Returns (item
    numbers int32 [B x width], scores float32 [B x width]) with -1 / NaN padding, width = ``n``
    or ``len(order_)``.
    """
    scores = np.asarray(scores, np.float32)
    width = len(order_) if n < 0 else n
    idx = np.full((len(hist_rows), width), -1, np.int32)
    out = np.full((len(hist_rows), width), np.nan, np.float32)
    for b, hist in enumerate(hist_rows):
        seen = set() if hist is None else {int(i) for i in hist}
        k = 0
        for item in order_:
            if k >= width:
                break
            if int(item) in seen:
                continue
            idx[b, k] = item
            out[b, k] = scores[item]
            k += 1
    return idx, out


def _blocks(counts):
    "(ascending distinct counts, per count the item numbers that have it)"
    counts = np.asarray(counts)
    values = np.unique(counts)
    return values, [np.flatnonzero(counts == v) for v in values]


def train(counts, mode: str):
    """
    ``count``: the counts as float32.  ``rank``: average ranks, float32 (1-based; a block of ``m``
    tied items after ``k`` smaller ones gets ``k + (m + 1) / 2``).  ``quantile``: which item of a
    block of tied counts gets which value is the sort's business, so the answer is per block the
    sorted array of values the block must receive: a list of (item numbers, float32 values
    ascending) -- the block's cumulative masses ``(before + c, before + 2 c, ...) / total``.
    """
    counts = np.asarray(counts)
    if mode == "count":
        return counts.astype(np.float32)
    values, members = _blocks(counts)
    if mode == "rank":
        out = np.zeros(len(counts), np.float64)
        below = 0
        for who in members:
            out[who] = below + (len(who) + 1) / 2.0
            below += len(who)
        return out.astype(np.float32)
    if mode == "quantile":
        total = int(counts.astype(np.int64).sum())
        before = 0
        blocks = []
        for v, who in zip(values.tolist(), members):
            mass = before + int(v) * np.arange(1, len(who) + 1, dtype=np.int64)
            with np.errstate(invalid="ignore", divide="ignore"):
                blocks.append((who, (mass / np.float64(total)).astype(np.float32)))
            before = int(mass[-1])
        return blocks
    raise ValueError(mode)
