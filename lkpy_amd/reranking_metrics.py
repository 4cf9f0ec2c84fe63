"""
``lenskit.metrics.reranking``: how far a reranked list moved from the ranking it was made from --
rank-biased overlap (``reranking/_rbo.py``) and least item promoted (``reranking/_lip.py``).

Both come from ONE device pass over all pairs (``lk_list_pair_stats``, csrc/diversity.hip): the
kernel adds RBO's weighted agreements sequentially in the depth, as the reference's loop does, and
finds the deepest reference position of a reranked top-``n`` item in one scan of the reference
list.  The functions on two :class:`ItemList` are the same path with a batch of one; the
``*_collection`` functions compare every list of a reranked collection -- the ``(user_id,
sample)`` lists of ``batch.recommend_samples``, say -- with the reference list its key projects
onto (the ``user_id`` lists of ``batch.recommend``).
"""

from __future__ import annotations

import numpy as np
import pandas as pd

from .data import ItemList, ItemListCollection
from .metrics import (GeometricRankWeight, RankWeight, _Packed, key_index, pack_collection,
                      project_rows)


def _common_numbers(ref: _Packed, rer: _Packed):
    """
    (offsets, item numbers) of both sides in ONE numbering: the item numbers the collections
    already carry when both are numbered by the same vocabulary (the array-backed results of
    ``batch.recommend`` / ``recommend_samples``), else the ids' positions among the sorted distinct
    ids of both sides.
    """
    a_ptr, a_ids, a_nums, a_vocab, _f = ref.as_ragged()
    b_ptr, b_ids, b_nums, b_vocab, _f = rer.as_ragged()
    if a_nums is not None and b_nums is not None and (a_vocab is b_vocab or a_vocab == b_vocab):
        a, b = a_nums, b_nums
    else:
        if a_ids is None:
            a_ids = a_vocab.ids(a_nums) if len(a_nums) else np.zeros(0, np.int64)
        if b_ids is None:
            b_ids = b_vocab.ids(b_nums) if len(b_nums) else np.zeros(0, np.int64)
        _u, inv = np.unique(np.concatenate([np.asarray(a_ids), np.asarray(b_ids)]),
                            return_inverse=True)
        a, b = inv[:len(a_ids)], inv[len(a_ids):]
    return (np.ascontiguousarray(a_ptr, dtype=np.int64), np.ascontiguousarray(a, dtype=np.int32),
            np.ascontiguousarray(b_ptr, dtype=np.int64), np.ascontiguousarray(b, dtype=np.int32))


def _pair_stats(ref: _Packed, rer: _Packed, rows, n: int, weight: RankWeight | None):
    """
    lk_list_pair_stats over the lists of ``rer`` against rows ``rows`` of ``ref``.  Returns
    (rbo float64 [P], lip float64 [P]) on the host, NaN where a pair has no reference list (and,
    for lip, where the reference list is empty).
    """
    import torch

    from . import _device as D

    n = int(n)
    if not 1 <= n <= D.PAIR_STATS_MAX_DEPTH:
        raise ValueError(f"n must be between 1 and {D.PAIR_STATS_MAX_DEPTH}")
    if weight is None:
        weight = GeometricRankWeight(0.85)
    weights = np.ascontiguousarray(weight.weight(np.arange(1, n + 1)), dtype=np.float64)
    total = 0  # _rbo.py:46-55: the weights summed one after the other
    for w in weights:
        total += w
    P = len(rer)
    if P == 0:
        return np.zeros(0), np.zeros(0)
    a_ptr, a_items, b_ptr, b_items = _common_numbers(ref, rer)
    dev = D.device()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    rows = np.ascontiguousarray(rows, dtype=np.int32)
    rbo, lip, flag = D.list_pair_stats(up(a_ptr), up(a_items), up(b_ptr), up(b_items), n,
                                       up(weights), up(rows))
    rbo, lip, flag = rbo.cpu().numpy(), lip.cpu().numpy(), flag.cpu().numpy()
    none = rows < 0
    rbo = rbo / total
    rbo[none] = np.nan
    lip = lip.astype(np.float64)
    lip[none | (flag != 0)] = np.nan
    return rbo, lip


def _one(il: ItemList) -> _Packed:
    coll = ItemListCollection(("list",))
    coll.add(il, 0)
    return pack_collection(coll)


def rank_biased_overlap(reference: ItemList, reranked: ItemList,
                        weight: RankWeight | None = None, n: int = 10) -> float:
    """
    Rank-biased overlap of two rankings down to depth ``n`` (``_rbo.py:15-58``): the weighted
    mean over the depths ``d`` of ``|reference[:d] & reranked[:d]| / d``; ``weight`` defaults to
    ``GeometricRankWeight(0.85)``.  The items of a list must be distinct.
    """
    rbo, _lip = _pair_stats(_one(reference), _one(reranked), np.zeros(1, np.int32), n, weight)
    return rbo[0].item()


def least_item_promoted(reference: ItemList, reranked: ItemList, n: int = 10) -> float:
    """
    Least item promoted (``_lip.py:14-48``): how far beyond ``n`` the deepest reference position
    of an item of ``reranked[:n]`` lies; NaN when the reference ranking is empty.
    """
    _rbo, lip = _pair_stats(_one(reference), _one(reranked), np.zeros(1, np.int32), n, None)
    return lip[0].item()


def _collection_stats(reference: ItemListCollection, reranked: ItemListCollection, n, weight):
    ref, rer = pack_collection(reference), pack_collection(reranked)
    cols = rer.key_columns()
    rows = project_rows(key_index(ref.key_fields, ref.key_columns()), ref.key_fields, cols,
                        len(rer), "reference")
    fields = list(rer.key_fields)
    index = pd.Index(cols[fields[0]], name=fields[0]) if len(fields) == 1 else \
        pd.MultiIndex.from_arrays([cols[f] for f in fields], names=fields)
    return _pair_stats(ref, rer, rows, n, weight), index


def rank_biased_overlap_collection(reference: ItemListCollection, reranked: ItemListCollection,
                                   weight: RankWeight | None = None, n: int = 10) -> pd.Series:
    """
    :func:`rank_biased_overlap` of every list of ``reranked`` against the list of ``reference``
    its key projects onto, as a series indexed by the reranked keys; NaN without such a list.
    """
    (rbo, _lip), index = _collection_stats(reference, reranked, n, weight)
    return pd.Series(rbo, index=index, name="RBO")


def least_item_promoted_collection(reference: ItemListCollection, reranked: ItemListCollection,
                                   n: int = 10) -> pd.Series:
    ":func:`least_item_promoted` per list of ``reranked``, as :func:`rank_biased_overlap_collection`"
    (_rbo, lip), index = _collection_stats(reference, reranked, n, None)
    return pd.Series(lip, index=index, name="LIP")
