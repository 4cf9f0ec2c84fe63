"""
Batch inference that routes whole query batches to the fused kernels (SURVEY.md section 8f,
rank 1): the reference's ``batch.recommend`` / ``batch.predict`` loop queries in Python
(src/lenskit/batch/_runner.py:259-345); results here are keyed by user like its
``ItemListCollection``.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

from .data import ItemList, ItemListCollection, RecQuery
from .pipeline import Pipeline


def recommend(pipe: Pipeline, users, n: int, *, batch_size: int = 16384,
              rerank_depth: int | None = None) -> ItemListCollection:
    """Ordered lists of ``n`` recommendations as an ``ItemListCollection`` keyed by ``user_id``
    (what ``BatchResults.output("recommendations")`` is in the reference,
    src/lenskit/batch/_runner.py:157-191): ``out.lookup(user)`` / ``out.lookup(user_id=user)``,
    iteration over ``(key, list)``, ``out.to_df()``.  A pipeline whose ranker is a
    ``StochasticTopNRanker`` gets sampled rankings (``_sample_panels``), any other the scorer's
    own top-N.  A pipeline whose ranker is a ``RandomSelector`` over the candidates, with an empty
    scorer slot (``random_pipeline``), is drawn by panels of one constant (``_recommend_random``);
    its lists carry no score.

    A pipeline with a ``reranker`` node (``Pipeline.add_reranker``) has the [B x n] arrays of
    every branch passed through the component's ``rerank_batch`` before the lists are built -- on
    the device where the scorer's ``recommend_batch`` has ``device_output`` --; a reranker
    without ``rerank_batch``, or one over another item vocabulary than the scorer's, runs through
    ``pipe.run`` user by user.  ``rerank_depth`` (>= n):
    the scorer's lists are taken at that depth and reranked down to ``n``.  That departs from the
    reference's wiring, where the reranker sees the ranker's ``n`` items and can only reorder
    them (``pipe.run`` keeps that); it gives a fairness reranker items to promote.  Not with a
    stochastic ranker."""
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    reranker = _reranker(pipe)
    if scorer is None and _random_selector(pipe) is not None:
        if reranker is not None or rerank_depth is not None or not _random_by_panels(pipe):
            if rerank_depth is not None:
                raise ValueError("rerank_depth does not apply to a random selection")
            return _recommend_loop(pipe, users, n)
        return _recommend_random(pipe, users, n, batch_size)
    batched = _reranks_batches(reranker, scorer)
    if rerank_depth is not None:
        if not batched:
            raise ValueError("rerank_depth needs a pipeline whose reranker has rerank_batch")
        if _stochastic_ranker(pipe) is not None:
            raise ValueError("rerank_depth does not apply to a stochastic ranker")
        if rerank_depth < n:
            raise ValueError(f"rerank_depth = {rerank_depth} is below n = {n}")
    if reranker is not None and not batched:
        return _recommend_loop(pipe, users, n)
    depth = n if rerank_depth is None else int(rerank_depth)
    if _stochastic_ranker(pipe) is not None:
        # a sampled ranking is not the scorer's own top-N: the lists come from the ranker, by
        # panels where the scorer has them, else through the pipeline user by user
        if not _has_panels(scorer, lookup):
            return _recommend_loop(pipe, users, n)
        ids, idx, keys = _sample_panels(pipe, users, n, 1, batch_size)
        i0, k0 = idx[:, 0], keys[:, 0]
        if batched:
            i0, k0 = reranker.rerank_batch(i0, k0, _rerank_length(n))
        return ItemListCollection.from_arrays(ids, i0, k0, scorer.items, key=("user_id",))
    if hasattr(scorer, "recommend_batch") and _takes_history_batches(scorer, lookup):
        # the whole batch by user number: the histories are rows of the HBM-resident training
        # matrix, no per-query host work (an id ARRAY stays an array); the lists are built when
        # somebody looks at them
        ids = users if isinstance(users, np.ndarray) else np.asarray(list(users))
        on_device = batched and getattr(scorer, "returns_device_lists", False)
        idx, sc = [], []
        for s in range(0, len(ids), batch_size):
            if on_device:  # (the lists meet the reranker where they are)
                i, v = scorer.recommend_batch(lookup.batch(ids[s:s + batch_size]), depth,
                                              device_output=True)
            else:
                i, v = scorer.recommend_batch(lookup.batch(ids[s:s + batch_size]), depth)
            if batched:
                i, v = reranker.rerank_batch(i, v, n)
            idx.append(i)
            sc.append(v)
        if not idx:
            return ItemListCollection(("user_id",))
        one = len(idx) == 1
        return ItemListCollection.from_arrays(ids, idx[0] if one else np.concatenate(idx),
                                              sc[0] if one else np.concatenate(sc),
                                              scorer.items, key=("user_id",))
    users = list(users)
    if not hasattr(scorer, "recommend_batch"):
        return _recommend_loop(pipe, users, n)
    out = {}
    for s in range(0, len(users), batch_size):
        chunk = users[s:s + batch_size]
        queries = [lookup(RecQuery.create(u)) for u in chunk]
        idx, sc = scorer.recommend_batch(queries, depth)
        if batched:
            idx, sc = reranker.rerank_batch(idx, sc, n)
        for u, i, v in zip(chunk, idx, sc):
            keep = i >= 0
            out[u] = ItemList(item_nums=i[keep], vocabulary=scorer.items, scores=v[keep],
                              ordered=True)
    return ItemListCollection.from_dict(out, key=("user_id",))


def _recommend_loop(pipe: Pipeline, users, n) -> ItemListCollection:
    "``recommend`` through ``pipe.run``, one user at a time"
    return ItemListCollection.from_dict(
        {u: pipe.run("recommender", query=u, n=n) for u in users}, key=("user_id",))


def _takes_history_batches(scorer, lookup) -> bool:
    "the lookup hands out ``HistoryBatch`` es and the scorer's batch calls take them"
    return hasattr(lookup, "batch") and getattr(scorer, "accepts_history_batch", False)


def _reranker(pipe: Pipeline):
    "the component of the pipeline's ``reranker`` node, or None"
    node = pipe.nodes.get("reranker")
    return None if node is None else node.component


def _reranks_batches(reranker, scorer) -> bool:
    "``rerank_batch`` takes the scorer's item NUMBERS: it must exist and mean the same items"
    if reranker is None or not hasattr(reranker, "rerank_batch"):
        return False
    mine, theirs = getattr(reranker, "vocab", None), getattr(scorer, "items", None)
    return mine is None or mine is theirs or mine == theirs


def _rerank_length(n):
    "a ranker's length as a reranker takes it: None where the ranker's means `every item`"
    return None if n is None or n < 0 else int(n)


# what the score panel and the key panel of one chunk of a stochastic batch may take together
STOCHASTIC_PANEL_BYTES = 4 << 30


def _stochastic_ranker(pipe: Pipeline):
    "the pipeline's ranker when it is a ``StochasticTopNRanker``, else None"
    from .stochastic import StochasticTopNRanker

    node = pipe.nodes.get(pipe.aliases.get("ranker", "ranker"))
    comp = None if node is None else node.component
    return comp if isinstance(comp, StochasticTopNRanker) else None


def _random_selector(pipe: Pipeline):
    "the pipeline's ranker when it is a ``RandomSelector``, else None"
    from .basic import RandomSelector

    node = pipe.nodes.get(pipe.aliases.get("ranker", "ranker"))
    comp = None if node is None else node.component
    return comp if isinstance(comp, RandomSelector) else None


def _random_by_panels(pipe: Pipeline) -> bool:
    """the selector picks from the standard candidates -- every training item but the query's
    history -- and the lookup hands out ``HistoryBatch`` es over those items"""
    from .basic import TrainingItemsCandidateSelector

    ranker = pipe.nodes[pipe.aliases.get("ranker", "ranker")]
    lookup = pipe.node("history-lookup").component
    cand = pipe.nodes.get("candidate-selector")
    cand = None if cand is None else cand.component
    if ranker.wiring.get("items") != "candidates" or not hasattr(lookup, "batch") or \
            getattr(lookup, "interactions", None) is None or \
            not isinstance(cand, TrainingItemsCandidateSelector) or not cand.is_trained() or \
            cand.config.exclude not in ("query", "all"):
        return False
    items = lookup.interactions._ds.items
    return cand.items_ is items or cand.items_ == items


def _recommend_random(pipe: Pipeline, users, n, batch_size: int) -> ItemListCollection:
    """
    ``recommend`` for a ``random_pipeline``: per chunk of ``STOCHASTIC_PANEL_BYTES / (8 n_items)``
    rows a panel of one constant, the users' training rows as the exclusion (an unknown user has
    none: every item is a candidate) and the selector's ``rank_panel`` -- the stochastic ranker's
    keys with no transform.  The lists hold item numbers only.
    """
    import torch

    from . import _device as D

    selector = _random_selector(pipe)
    lookup = pipe.node("history-lookup").component
    ids = users if isinstance(users, np.ndarray) else np.asarray(list(users))
    if len(ids) == 0:
        return ItemListCollection(("user_id",))
    hb = lookup.batch(ids)
    n_items = len(hb.items)
    n = selector._length(n)
    width = n_items if n < 0 else n
    rows = max(1, min(batch_size, len(ids), STOCHASTIC_PANEL_BYTES // (8 * max(1, n_items))))
    streams = selector.streams(hb.user_ids)  # (the ids as the lookup types them, like a query's)
    idx = np.full((len(ids), width), -1, np.int32)
    panel = torch.ones((rows, n_items), dtype=torch.float32, device=D.device())
    for s in range(0, len(ids), rows):
        sub = hb.subset(slice(s, s + rows))
        i, _keys = selector.rank_panel(panel[:len(sub)], streams[s:s + rows], n,
                                       excl=sub.csr(with_values=False))
        idx[s:s + rows, :i.shape[2]] = i[:, 0]
    return ItemListCollection.from_arrays(ids, idx, None, hb.items, key=("user_id",))


def _has_panels(scorer, lookup) -> bool:
    return hasattr(scorer, "dense_scores_batch") and _takes_history_batches(scorer, lookup)


def _sample_panels(pipe: Pipeline, users, n: int, samples: int, batch_size: int):
    """
    ``samples`` sampled rankings per user, whole batches at a time: the scorer's
    ``dense_scores_batch`` panel -> the stochastic ranker's ``rank_panel``, in chunks of
    ``STOCHASTIC_PANEL_BYTES / (8 n_items)`` rows (a float32 score and a float32 key per item).
    Returns (user ids, item numbers [B x S x n], keys [B x S x n]).
    """
    ranker = _stochastic_ranker(pipe)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    ids = users if isinstance(users, np.ndarray) else np.asarray(list(users))
    n = ranker._length(n)
    width = len(scorer.items) if n < 0 else n
    rows = max(1, min(batch_size, STOCHASTIC_PANEL_BYTES // (8 * max(1, len(scorer.items)))))
    hb = lookup.batch(ids)
    streams = ranker.streams(hb.user_ids)  # (the ids as the lookup types them, like a query's)
    idx = np.full((len(ids), samples, width), -1, np.int32)
    keys = np.full((len(ids), samples, width), np.nan, np.float32)
    for s in range(0, len(ids), rows):
        panel, _valid, hist = scorer.dense_scores_batch(hb.subset(slice(s, s + rows)))
        i, k = ranker.rank_panel(panel, streams[s:s + rows], n, excl=hist, samples=samples)
        idx[s:s + rows, :, :i.shape[2]] = i
        keys[s:s + rows, :, :i.shape[2]] = k
    return ids, idx, keys


def recommend_samples(pipe: Pipeline, users, n: int, samples: int, *,
                      batch_size: int = 16384) -> ItemListCollection:
    """
    ``samples`` sampled rankings of ``n`` items per user from a pipeline whose ranker is a
    :class:`lkpy_amd.stochastic.StochasticTopNRanker`, keyed by ``(user_id, sample)``; sample 0 is
    what ``recommend`` draws.  A scorer without ``dense_scores_batch`` is scored through the
    pipeline user by user and ranked ``samples`` times.  A pipeline's ``reranker`` is applied to
    every sampled list, as ``recommend`` applies it.
    """
    ranker = _stochastic_ranker(pipe)
    if ranker is None:
        raise TypeError("recommend_samples needs a pipeline whose ranker is a StochasticTopNRanker")
    samples = int(samples)
    scorer = pipe.node("scorer").component
    reranker = _reranker(pipe)
    if reranker is not None and not _reranks_batches(reranker, scorer) and \
            _has_panels(scorer, pipe.node("history-lookup").component):
        ids, idx, keys = _sample_panels(pipe, users, n, samples, batch_size)
        out = {}
        for b, u in enumerate(ids.tolist()):
            for s in range(samples):
                keep = idx[b, s] >= 0
                il = ItemList(item_nums=idx[b, s][keep], vocabulary=scorer.items,
                              scores=keys[b, s][keep], ordered=True)
                out[(u, s)] = reranker(items=il, n=_rerank_length(n))
        return ItemListCollection.from_dict(out, key=("user_id", "sample"))
    if not _has_panels(scorer, pipe.node("history-lookup").component):
        out = {}
        for u in users:
            got = pipe.run_all("history-lookup", "scorer", query=u)
            lists = ranker.sample(got["scorer"], got["history-lookup"], n, samples=samples)
            if reranker is not None:
                lists = [reranker(items=il, n=_rerank_length(n)) for il in lists]
            out.update({(u, s): il for s, il in enumerate(lists)})
        return ItemListCollection.from_dict(out, key=("user_id", "sample"))
    ids, idx, keys = _sample_panels(pipe, users, n, samples, batch_size)
    pairs = [(u, s) for u in ids.tolist() for s in range(samples)]
    flat = idx.shape[0] * idx.shape[1]
    idx, keys = idx.reshape(flat, -1), keys.reshape(flat, -1)
    if reranker is not None:
        idx, keys = reranker.rerank_batch(idx, keys, _rerank_length(n))
    return ItemListCollection.from_arrays(pairs, idx, keys, scorer.items,
                                          key=("user_id", "sample"))


def predict(pipe: Pipeline, pairs, *, batch_size: int = 16384) -> ItemListCollection:
    """
    Scores for each user's items (``rating-predictor`` semantics) as an ``ItemListCollection``
    keyed by ``user_id`` (``BatchResults.output("predictions")``).  ``pairs``: a dict of user ->
    ``ItemList`` (or item-id array), an ``ItemListCollection`` keyed by ``user_id`` (the
    reference's ``predict(pipeline, test)``), or a ``DataFrame`` with ``user_id`` and ``item_id``
    columns (users in order of first appearance, rows in order within a user; the other columns
    become fields of the lists).

    An item-kNN, a user-kNN or a biased-MF (``BiasedMFScorer``) pipeline (``std:topn-predict``
    with its ``BiasScorer`` fallback, or without a fallback) whose vocabularies agree is run as
    whole batches by user number (:func:`_predict_batched`): the lists are the per-query
    composition's bit for bit (float32 of it where the biased-MF scorer alone hands out float64).
    Every other pipeline runs query by query.
    """
    keys, offsets, item_ids, fields, lists = _ragged_pairs(pairs)
    parts = _batched_predict_parts(pipe)
    if parts is not None and fields is not None and not (
            set(fields) & {"score", "nbr_counts", "is_fallback"}):
        return _predict_batched(parts, keys, offsets, item_ids, fields, batch_size)
    if isinstance(pairs, dict):
        return _predict_loop(pipe, pairs)
    if lists is None:
        lists = [ItemList(item_ids=item_ids[offsets[i]:offsets[i + 1]],
                          **{f: v[offsets[i]:offsets[i + 1]] for f, v in fields.items()})
                 for i in range(len(keys))]
    return _predict_loop(pipe, dict(zip(_key_list(keys), lists)))


def _key_list(keys) -> list:
    return [k.item() if isinstance(k, np.generic) else k for k in keys]


def _ragged_pairs(pairs):
    """
    The query lists of a ``predict`` input as ragged arrays: (user keys, int64 offsets, the
    concatenated item ids, {field: concatenated values} -- None when the lists do not all carry
    the same fields --, the ``ItemList`` objects or None for a frame).
    """
    if isinstance(pairs, pd.DataFrame):
        codes, uniq = pd.factorize(pairs["user_id"], sort=False)  # order of first appearance
        order = np.argsort(codes, kind="stable")
        counts = np.bincount(codes[codes >= 0], minlength=len(uniq))
        offsets = np.zeros(len(uniq) + 1, np.int64)
        np.cumsum(counts, out=offsets[1:])
        order = order[len(order) - int(offsets[-1]):]  # (rows without a user id dropped)
        item_ids = pairs["item_id"].to_numpy()[order]
        fields = {c: pairs[c].to_numpy()[order] for c in pairs.columns
                  if c not in ("user_id", "item_id")}
        return np.asarray(uniq), offsets, item_ids, fields, None
    if isinstance(pairs, ItemListCollection):
        keys, lists = [], []
        for k, il in pairs:
            keys.append(getattr(k, "user_id") if "user_id" in k._fields else k[0])
            lists.append(il)
    else:
        keys = list(pairs)
        lists = [pairs[u] if isinstance(pairs[u], ItemList) else ItemList(np.asarray(pairs[u]))
                 for u in keys]
    offsets = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(il) for il in lists], out=offsets[1:])
    ids = [il.ids() for il in lists]
    item_ids = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    names = {tuple(il._fields) for il in lists}
    fields = None
    if len(names) <= 1:
        fields = {f: np.concatenate([il._fields[f] for il in lists]) for f in
                  (names.pop() if names else ())}
    return keys, offsets, item_ids, fields, lists


def _batched_predict_parts(pipe: Pipeline):
    """(scorer, lookup, BiasScorer or None) when ``rating-predictor`` can run by user number:
    an ``ItemKNNScorer``, a ``UserKNNScorer`` or a ``BiasedMFScorer``, a lookup with ``batch``, no
    merger or a ``FallbackScorer`` over a ``BiasScorer``, and one item (and user) vocabulary
    throughout; None otherwise.  A ``UserKNNScorer`` must share the lookup's USER vocabulary too
    (a known user is then always scored from the looked-up history, never from the stored
    vector), and with explicit feedback the dataset must have ratings (without, the per-query
    path answers NaN, and goes on doing so through the loop)."""
    from .als import BiasedMFScorer
    from .basic import BiasScorer, FallbackScorer
    from .knn import ItemKNNScorer, UserKNNScorer

    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    if not isinstance(scorer, (ItemKNNScorer, UserKNNScorer, BiasedMFScorer)) \
            or not hasattr(lookup, "batch") \
            or getattr(lookup, "interactions", None) is None:
        return None
    ds = lookup.interactions._ds
    same = lambda a, b: a is b or a == b  # noqa: E731
    rating = ds._attrs.get("rating")
    if isinstance(scorer, BiasedMFScorer):
        # trained, a bias model with both terms, ratings to fold in (the per-query path raises
        # without), and the lookup's users where stored rows are taken by user number
        if getattr(scorer, "item_embeddings", None) is None or \
                getattr(scorer, "bias", None) is None or not scorer._batch_ready() or \
                rating is None or not same(scorer.items, ds.items) or \
                (scorer.users is not None and not same(scorer.users, ds.users)):
            return None
    elif isinstance(scorer, UserKNNScorer):
        if not scorer.is_trained() or not same(scorer.items, ds.items) or \
                not same(scorer.users, ds.users):
            return None
        if scorer.config.explicit and rating is None:
            return None  # (the per-query path answers NaN)
    else:
        if not scorer.is_trained() or not same(scorer.items, ds.items):
            return None
        if scorer.config.explicit and rating is None:
            return None  # (the per-query path raises)
    bias = None
    merger = pipe.nodes.get("rating-merger")
    if merger is not None:
        fb = pipe.nodes.get("fallback-predictor")
        if not isinstance(merger.component, FallbackScorer) or fb is None or \
                not isinstance(fb.component, BiasScorer) or not fb.component.is_trained():
            return None
        bias = fb.component
        model = bias.model
        if model.items is not None and not same(model.items, ds.items):
            return None
        if model.users is not None and (not same(model.users, ds.users) or rating is None or
                                        rating.dtype != np.float32):
            return None  # (the host sums the history's own ratings: float32 in HBM)
    return scorer, lookup, bias


def _predict_batched(parts, keys, offsets, item_ids, fields, batch_size: int):
    """
    ``rating-predictor`` for whole batches by user number: one vectorised vocabulary lookup of
    every target, and per batch the histories cut out of the HBM-resident training matrix,
    one ``lk_iknn_score_batch`` call (``ItemKNNScorer.score_history_batch``), the user biases of
    the ``BiasScorer`` fallback (``lk_bias_user_offsets``), the item means and the fallback merge
    (``lk_predict_merge``) and one download of scores, counts and flags.  The lists carry the
    caller's item ids and fields; a query without history has no ``nbr_counts``
    (item.py:238-245), ``is_fallback`` exists with a fallback only.

    A ``BiasedMFScorer`` scores by ``predict_history_batch`` (fold-in, ``lk_score_dense``,
    ``lk_bmf_finish_pairs``), has no item means to add back and no ``nbr_counts``; its fallback
    is the same merge.  So does a ``UserKNNScorer`` (``lk_uknn_query_panel``,
    ``lk_uknn_sims_panel``, ``lk_uknn_score_pairs``): its scores carry the history's centre
    already, the per-query lists have no ``nbr_counts``, and without a fallback there is no merge
    call.
    """
    import torch

    from . import _device as D

    scorer, lookup, bias = parts
    B = len(keys)
    if B == 0:
        return ItemListCollection(("user_id",))
    key_arr = keys if isinstance(keys, np.ndarray) else np.asarray(_key_list(keys))
    n_items = len(scorer.items)
    nums = scorer.items.numbers(item_ids, missing="negative") if len(item_ids) else \
        np.zeros(0, np.int32)
    total = int(offsets[-1])
    knn = hasattr(scorer, "score_history_batch")  # (else: BiasedMFScorer, UserKNNScorer)
    scores = np.empty(total, np.float32)
    counts = np.empty(total, np.int32) if knn else None
    fb = np.empty(total, np.bool_) if bias is not None else None
    nohist = np.empty(B, np.bool_)
    d = scorer._device_sims()["device"] if knn else scorer._device_state()["device"]
    means = scorer._device_means() if knn else None
    item_biases = bias._device_item_biases() if bias is not None else None
    for s0 in range(0, B, batch_size):
        s1 = min(B, s0 + batch_size)
        nb = s1 - s0
        lo, hi = int(offsets[s0]), int(offsets[s1])
        n = hi - lo
        hb = lookup.batch(key_arr[s0:s1])
        nohist[s0:s1] = hb.lengths == 0
        if n == 0:
            continue  # (empty target lists only: nothing to score)
        # one upload: target offsets (int64) and item numbers (int32)
        packed = np.empty(2 * (nb + 1) + n + (n & 1), np.int32)
        packed[:2 * (nb + 1)] = (offsets[s0:s1 + 1] - lo).view(np.int32)
        packed[2 * (nb + 1):2 * (nb + 1) + n] = nums[lo:hi]
        d_packed = torch.from_numpy(packed).to(d)
        d_ptr = d_packed[:2 * (nb + 1)].view(torch.int64)
        d_nums = d_packed[2 * (nb + 1):2 * (nb + 1) + n]
        if knn:
            s_dev, c_dev = scorer.score_history_batch(hb, d_ptr, d_nums)
        else:
            s_dev = scorer.predict_history_batch(hb, d_ptr, d_nums,
                                                 h_tgt_ptr=offsets[s0:s1 + 1] - lo)
        out = torch.empty(9 * n, dtype=torch.uint8, device=d)  # scores | counts | flags
        if bias is not None:
            ub, add = bias.user_offsets_batch(hb)
            D.predict_merge(d_ptr, d_nums, n_items, s_dev, means, fallback=True,
                            global_bias=bias.model.global_bias, item_biases=item_biases,
                            user_bias=ub, user_add=add, out_is_fallback=out[8 * n:])
        elif knn:
            D.predict_merge(d_ptr, d_nums, n_items, s_dev, means)
        out[:4 * n] = s_dev.view(torch.uint8)
        if knn:
            out[4 * n:8 * n] = c_dev.view(torch.uint8)
        host = out.cpu().numpy()
        scores[lo:hi] = host[:4 * n].view(np.float32)
        if knn:
            counts[lo:hi] = host[4 * n:8 * n].view(np.int32)
        if fb is not None:
            fb[lo:hi] = host[8 * n:].view(np.bool_)
    out_fields = dict(fields)
    if knn:
        out_fields["nbr_counts"] = counts
    out_fields["score"] = scores
    if fb is not None:
        out_fields["is_fallback"] = fb
    return ItemListCollection.from_ragged(keys, offsets, item_ids, out_fields, key=("user_id",),
                                          absent={"nbr_counts": nohist} if knn else None)


def _predict_loop(pipe: Pipeline, pairs: dict) -> ItemListCollection:
    "``predict`` one query at a time (the path of every pipeline without a batched one)."
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    users = list(pairs)
    lists = [pairs[u] if isinstance(pairs[u], ItemList) else ItemList(np.asarray(pairs[u]))
             for u in users]
    if hasattr(scorer, "score_batch"):
        queries = [lookup(RecQuery.create(u)) for u in users]
        scored = scorer.score_batch(queries, lists)
        merger = pipe.nodes.get("rating-merger")
        if merger is not None:
            fb = pipe.node("fallback-predictor").component
            scored = [merger.component(primary=s, backup=fb(q, il))
                      for s, q, il in zip(scored, queries, lists)]
        return ItemListCollection.from_dict(dict(zip(users, scored)), key=("user_id",))
    return ItemListCollection.from_dict(
        {u: pipe.run("rating-predictor", query=u, items=il) for u, il in zip(users, lists)},
        key=("user_id",))
