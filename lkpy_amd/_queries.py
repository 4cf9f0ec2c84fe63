"""
Host side of the scorers' batched calls: a batch of queries -> the arrays the device calls take,
and a dense score row -> an ``ItemList``'s scores.  NumPy and the ``data`` types only (no Torch,
no device), so that what differs between the scorers -- are unknown history items dropped, are
rows sorted or de-duplicated, which values ride along -- is said in one call each.
"""

from __future__ import annotations

import numpy as np

from .basic import HistoryBatch
from .data import ItemList, RecQuery, Vocabulary


def resolve_queries(queries, items: Vocabulary):
    """
    The :class:`HistoryBatch` itself when its item numbers are ``items``' (the scorer then cuts
    the histories out of the HBM-resident training matrix), else a list of ``RecQuery``: a batch
    over another item vocabulary goes through the per-query mapping (``batch.queries()``).
    """
    if isinstance(queries, HistoryBatch):
        if queries.items is items or queries.items == items:
            return queries
        return queries.queries()
    return [RecQuery.create(q) for q in queries]


def pack_histories(queries: list[RecQuery], items: Vocabulary, *, unknown: str,
                   sort: bool = False, unique: bool = False, values=None):
    """
    The histories of a list of queries as CSR rows over ``items``: (offsets int64 [B + 1], item
    numbers int32, values float32 | None).  A query without history and an empty history give an
    empty row.

    ``unknown``: what becomes of a history item ``items`` does not have.  ``"drop"``: it is left
    out -- the reference's fold-in builds its ``ri_good`` mask for exactly that
    (src/lenskit/als/_implicit.py:82-90) although its ``numbers()`` call raises ``KeyError`` first
    (default ``missing="error"``, data/_items.py:617,654-655); a batch must not fail because one
    history mentions a new item.  ``"keep"``: it stays as -1, in
    its place, for kernels that step over it.
    ``sort``: rows in ascending item number (stable), values following; else in query order.
    ``unique``: sorted, and a repeated item counts ONCE -- the reference's EASE sets
    ``q_vec[q_good] = 1.0`` (src/lenskit/knn/ease.py), it does not add per occurrence.  No values.
    ``values``: the scorer's own ``f(history ItemList, item numbers, kept mask)`` -> one value per
    kept entry of a non-empty history, in history order; cast to float32 here.  It raises the
    scorer's own error when the history lacks what it needs.
    """
    if unknown not in ("keep", "drop") or (unique and values is not None):
        raise ValueError("pack_histories: unknown is 'keep' or 'drop'; unique rows carry no values")
    idx, val = [], []
    ptr = np.zeros(len(queries) + 1, dtype=np.int64)
    for i, q in enumerate(queries):
        hist = q.query_items
        if hist is not None and len(hist) > 0:
            nums = hist.numbers(vocabulary=items, missing="negative")
            kept = nums >= 0 if unknown == "drop" else np.ones(len(nums), dtype=bool)
            row = nums[kept]
            v = None if values is None else np.asarray(values(hist, nums, kept), dtype=np.float32)
            if unique:
                row = np.unique(row)
            elif sort:
                order = np.argsort(row, kind="stable")
                row = row[order]
                v = None if v is None else v[order]
            idx.append(row)
            val.append(v)
            ptr[i + 1] = len(row)
    np.cumsum(ptr, out=ptr)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return ptr, cat(idx, np.int32), None if values is None else cat(val, np.float32)


def pack_targets(item_lists: list[ItemList], items: Vocabulary):
    """
    The target lists of a batch as ragged rows over ``items``: (offsets int64 [B + 1], item
    numbers int32), list order kept, repeats kept, -1 for an item ``items`` does not have.  One
    vocabulary lookup over the concatenated ids; list ``i``'s numbers are
    ``nums[ptr[i]:ptr[i + 1]]``.
    """
    ptr = np.zeros(len(item_lists) + 1, dtype=np.int64)
    np.cumsum([len(il) for il in item_lists], out=ptr[1:])
    ids = [il.ids() for il in item_lists if len(il)]
    if not ids:
        return ptr, np.zeros(0, np.int32)
    return ptr, items.numbers(np.concatenate(ids), missing="negative")


def user_numbers(queries, users: Vocabulary | None) -> np.ndarray:
    """
    The queries' rows in ``users`` (int64, -1 = unknown user, no user id, or ``users`` is None).
    A :class:`HistoryBatch` over the same vocabulary already has them; over another one they come
    from one vectorised lookup; a list of ``RecQuery`` is looked up id by id.
    """
    if users is not None and isinstance(queries, HistoryBatch):
        if queries.users is users or queries.users == users:
            return queries.user_nums.astype(np.int64)
        return users.numbers(queries.user_ids, missing="negative").astype(np.int64)
    nums = np.full(len(queries), -1, dtype=np.int64)
    if users is not None:
        for i, q in enumerate(queries):
            num = None if q.user_id is None else users.number(q.user_id, missing=None)
            if num is not None:
                nums[i] = num
    return nums


def item_scores(items: ItemList, vocab: Vocabulary, dense_row: np.ndarray) -> np.ndarray:
    "``dense_row`` (a score per item of ``vocab``) at ``items``: float32, NaN for unknown items."
    nums = items.numbers(vocabulary=vocab, missing="negative")
    known = nums >= 0
    scores = np.full(len(items), np.nan, dtype=np.float32)
    scores[known] = dense_row[nums[known]]
    return scores
