"""
Batch inference that routes whole query batches to the fused kernels (SURVEY.md section 8f,
rank 1): the reference's ``batch.recommend`` / ``batch.predict`` loop queries in Python
(src/lenskit/batch/_runner.py:259-345); results here are keyed by user like its
``ItemListCollection``.
"""

from __future__ import annotations

from itertools import repeat

import numpy as np
import pandas as pd

from .basic import RandomSelector, TopNRanker
from .data import ItemList, ItemListCollection, RecQuery
from .pipeline import Pipeline
from .stochastic import StochasticTopNRanker


def recommend(pipe: Pipeline, users, n: int, *, candidates=None, batch_size: int = 16384,
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
    stochastic ranker.

    ``candidates`` (a dict of user -> ``ItemList`` or item ids, an ``ItemListCollection`` keyed by
    ``user_id``, or a frame with ``user_id`` and ``item_id``): every user's OWN items are ranked
    instead of the catalogue -- ``pipe.run("recommender", query=u, items=candidates[u], n=n)``,
    the reference's ``BatchRecRequest.candidates`` -- see :func:`_recommend_candidates`.
    ``users=None`` then means the candidates' keys in their order.  Whole batches on the device
    for every scorer :func:`_candidate_route` has a route for -- the factor models, the k-NN
    scorers, EASE, SLIM, association rules and popularity; only ``BiasedMFScorer`` goes query by
    query --, under a plain ``TopNRanker``, a ``StochasticTopNRanker`` (the sampled rankings of
    the lists, ``lk_ragged_stochastic_keys``) and the ``RandomSelector`` of a
    ``random_pipeline``."""
    if candidates is not None:
        return _recommend_candidates(pipe, users, n, candidates, batch_size, rerank_depth)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    reranker = _slot(pipe, "reranker")
    if scorer is None and _ranker(pipe, RandomSelector) is not None:
        if reranker is not None or rerank_depth is not None or not _random_by_panels(pipe):
            if rerank_depth is not None:
                raise ValueError("rerank_depth does not apply to a random selection")
            return _recommend_loop(pipe, users, n)
        return _recommend_random(pipe, users, n, batch_size)
    batched = _check_rerank_depth(pipe, reranker, scorer, n, rerank_depth)
    if reranker is not None and not batched:
        return _recommend_loop(pipe, users, n)
    depth = n if rerank_depth is None else int(rerank_depth)
    if _ranker(pipe, StochasticTopNRanker) is not None:
        # a sampled ranking is not the scorer's own top-N: the lists come from the ranker, by
        # panels where the scorer has them, else through the pipeline user by user
        drawn = _draw_samples(pipe, users, n, 1, batch_size)
        if drawn is None:
            return _recommend_loop(pipe, users, n)
        return _sampled_lists(drawn, scorer.items, reranker, n, key=("user_id",))
    if hasattr(scorer, "recommend_batch") and _takes_history_batches(scorer, lookup):
        # the whole batch by user number: the histories are rows of the HBM-resident training
        # matrix, no per-query host work (an id ARRAY stays an array); the lists are built when
        # somebody looks at them
        ids = _as_array(users)
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


def _check_rerank_depth(pipe: Pipeline, reranker, scorer, n, rerank_depth) -> bool:
    """Does the reranker take whole batches (``_reranks_batches``)?  Raises ``ValueError`` for a
    ``rerank_depth`` the pipeline cannot honour -- before anything is computed."""
    batched = _reranks_batches(reranker, scorer)
    if rerank_depth is not None:
        if not batched:
            raise ValueError("rerank_depth needs a pipeline whose reranker has rerank_batch")
        if _ranker(pipe, StochasticTopNRanker) is not None:
            raise ValueError("rerank_depth does not apply to a stochastic ranker")
        if rerank_depth < n:
            raise ValueError(f"rerank_depth = {rerank_depth} is below n = {n}")
    return batched


def _recommend_loop(pipe: Pipeline, users, n) -> ItemListCollection:
    "``recommend`` through ``pipe.run``, one user at a time"
    return ItemListCollection.from_dict(
        {u: pipe.run("recommender", query=u, n=n) for u in users}, key=("user_id",))


def _takes_history_batches(scorer, lookup) -> bool:
    """the lookup hands out ``HistoryBatch`` es and the scorer's batch calls take them -- those
    of THIS lookup, where the scorer has a say in it (``takes_batches_of``: ``BiasScorer``)"""
    if not (hasattr(lookup, "batch") and getattr(scorer, "accepts_history_batch", False)):
        return False
    return _takes_batches_of(scorer, lookup)


def _takes_batches_of(scorer, lookup) -> bool:
    "``scorer.takes_batches_of(lookup)`` where the scorer has such a rule; True without one"
    rule = getattr(scorer, "takes_batches_of", None)
    return rule is None or bool(rule(lookup))


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


def _slot(pipe: Pipeline, name: str):
    "the component of the node that ``name`` names or is an alias of; None without one"
    node = pipe.nodes.get(pipe.aliases.get(name, name))
    return None if node is None else node.component


def _ranker(pipe: Pipeline, cls, *, exact: bool = False, over_scorer: bool = False):
    """The pipeline's ranker when it is a ``cls`` (``exact``: of that very class, no subclass) and
    -- ``over_scorer`` -- ranks the scorer's output; else None."""
    comp = _slot(pipe, "ranker")
    if not (type(comp) is cls if exact else isinstance(comp, cls)):
        return None
    if not over_scorer:
        return comp
    wired_to = pipe.node("ranker").wiring.get("items")
    return comp if wired_to == pipe.aliases.get("scorer", "scorer") else None


def _as_array(users) -> np.ndarray:
    "user keys as an array (an id ARRAY stays the array it is, a list is not copied first)"
    return np.asarray(users if isinstance(users, (np.ndarray, list)) else list(users))


def _random_by_panels(pipe: Pipeline) -> bool:
    """the selector picks from the standard candidates -- every training item but the query's
    history -- and the lookup hands out ``HistoryBatch`` es over those items"""
    from .basic import TrainingItemsCandidateSelector

    ranker = pipe.node("ranker")
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

    selector = _ranker(pipe, RandomSelector)
    lookup = pipe.node("history-lookup").component
    ids = _as_array(users)
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
    ranker = _ranker(pipe, StochasticTopNRanker)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    ids = _as_array(users)
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


def recommend_samples(pipe: Pipeline, users, n: int, samples: int, *, candidates=None,
                      batch_size: int = 16384) -> ItemListCollection:
    """
    ``samples`` sampled rankings of ``n`` items per user from a pipeline whose ranker is a
    :class:`lkpy_amd.stochastic.StochasticTopNRanker`, keyed by ``(user_id, sample)``; sample 0 is
    what ``recommend`` draws.  A scorer without ``dense_scores_batch`` is scored through the
    pipeline user by user and ranked ``samples`` times.  A pipeline's ``reranker`` is applied to
    every sampled list, as ``recommend`` applies it.

    ``candidates``: as in ``recommend(candidates=)`` -- every user's OWN items are ranked
    ``samples`` times, ``users=None`` means the candidates' keys in their order, sample 0 is
    what ``recommend(candidates=)`` draws; whole batches on the device where that call has them
    (:func:`_sample_candidates`: one statistics pass serves every sample of a list).
    """
    ranker = _ranker(pipe, StochasticTopNRanker)
    if ranker is None:
        raise TypeError("recommend_samples needs a pipeline whose ranker is a StochasticTopNRanker")
    samples = int(samples)
    scorer, reranker = _slot(pipe, "scorer"), _slot(pipe, "reranker")
    lists = None if candidates is None else _candidate_lists(users, candidates)
    if lists is None:
        drawn = _draw_samples(pipe, users, n, samples, batch_size)
    else:
        users = lists[0]
        drawn = _draw_samples(pipe, users, n, samples, batch_size, lists,
                              _candidate_mode(pipe, lists[3], len(users)))
    if drawn is None:
        out = {}
        for u, il in zip(users, repeat(None) if lists is None else _query_lists(lists)):
            got = pipe.run_all("history-lookup", "scorer", query=u, items=il)
            drew = ranker.sample(got["scorer"], got["history-lookup"], n, samples=samples)
            if reranker is not None:
                drew = [reranker(items=d, n=_rerank_length(n)) for d in drew]
            out.update({(u, s): d for s, d in enumerate(drew)})
        return ItemListCollection.from_dict(out, key=("user_id", "sample"))
    if reranker is not None and not _reranks_batches(reranker, scorer):  # (panels only)
        ids, idx, keys = drawn
        out = {}
        for b, u in enumerate(ids.tolist()):
            for s in range(samples):
                keep = idx[b, s] >= 0
                il = ItemList(item_nums=idx[b, s][keep], vocabulary=scorer.items,
                              scores=keys[b, s][keep], ordered=True)
                out[(u, s)] = reranker(items=il, n=_rerank_length(n))
        return ItemListCollection.from_dict(out, key=("user_id", "sample"))
    return _sampled_lists(drawn, scorer.items, reranker, n, key=("user_id", "sample"))


def _draw_samples(pipe: Pipeline, users, n, samples: int, batch_size: int, cand=None, mode=None):
    """
    ``samples`` sampled rankings per user as (user keys, item numbers [B x S x w], keys
    [B x S x w]): off the scorer's panels (:func:`_sample_panels`), or -- ``cand``: what
    :func:`_candidate_lists` returned, ``mode``: what :func:`_candidate_mode` says of it -- of
    every user's own list (:func:`_sample_candidates`).  None where the caller has to go query by
    query: a scorer without panels, candidates in another mode than ``"sample"``, lists that
    cannot be addressed.
    """
    if cand is None:
        if not _has_panels(pipe.node("scorer").component, pipe.node("history-lookup").component):
            return None
        return _sample_panels(pipe, users, n, samples, batch_size)
    keys, offsets, item_ids, _fields, lists = cand
    kind, ranker, plan = mode
    if kind != "sample":
        return None
    return _sample_candidates(plan, ranker, keys, offsets, item_ids, lists, n, samples, batch_size)


def _sampled_lists(drawn, vocab, reranker, n, *, key) -> ItemListCollection:
    """The collection of what :func:`_draw_samples` drew: the [B·S x w] lists, through the
    ``rerank_batch`` of a reranker (one that has it: the caller's matter), under ``key`` --
    ``("user_id",)``, of one sample per user, or ``("user_id", "sample")``."""
    ids, idx, kk = drawn
    B, S, w = idx.shape
    idx, kk = idx.reshape(B * S, w), kk.reshape(B * S, w)
    if reranker is not None:
        idx, kk = reranker.rerank_batch(idx, kk, _rerank_length(n))
    if "sample" in key:
        ids = [(u, s) for u in ids.tolist() for s in range(S)]
    return ItemListCollection.from_arrays(ids, idx, kk, vocab, key=key)


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
    So is a pipeline whose scorer is a trained ``BiasScorer`` (:func:`_predict_bias`).  Every
    other pipeline runs query by query.
    """
    ragged = _ragged_pairs(pairs)
    keys, offsets, item_ids, fields, _lists = ragged
    parts = _batched_predict_parts(pipe)
    if parts is not None and fields is not None and not (
            set(fields) & {"score", "nbr_counts", "is_fallback"}):
        return _predict_batched(parts, keys, offsets, item_ids, fields, batch_size)
    parts = _bias_predict_parts(pipe)
    if parts is not None and fields is not None and not (set(fields) & {"score", "is_fallback"}):
        return _predict_bias(parts, keys, offsets, item_ids, fields, batch_size)
    if isinstance(pairs, dict):
        return _predict_loop(pipe, pairs)
    return _predict_loop(pipe, dict(zip(_key_list(keys), _query_lists(ragged))))


def _key_list(keys) -> list:
    return [k.item() if isinstance(k, np.generic) else k for k in keys]


def _query_lists(ragged) -> list:
    """One ``ItemList`` per query of what :func:`_ragged_pairs` / :func:`_candidate_lists`
    returned, for the per-query loops: the caller's own lists where there are any, else (a frame)
    cut out of the ragged arrays with their fields."""
    keys, offsets, item_ids, fields, lists = ragged
    if lists is not None:
        return lists
    return [ItemList(item_ids=item_ids[offsets[i]:offsets[i + 1]],
                     **{f: v[offsets[i]:offsets[i + 1]] for f, v in fields.items()})
            for i in range(len(keys))]


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


def _same(a, b) -> bool:
    return a is b or a == b


def _numbered_dataset(scorer, lookup):
    """The dataset behind ``lookup`` when a batch can go by ITS numbers: the lookup hands out
    ``HistoryBatch`` es over a training matrix and the scorer's item vocabulary is that matrix's;
    None otherwise (an untrained scorer has no vocabulary)."""
    if not hasattr(lookup, "batch") or getattr(lookup, "interactions", None) is None:
        return None
    ds = lookup.interactions._ds
    items = getattr(scorer, "items", None)
    if items is None or not _same(items, ds.items):
        return None
    return ds


def _users_agree(scorer, ds, *, required: bool) -> bool:
    "the scorer's user vocabulary is the dataset's (``required``: and it has one)"
    users = getattr(scorer, "users", None)
    if users is None:
        return not required
    return _same(users, ds.users)


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
    if not isinstance(scorer, (ItemKNNScorer, UserKNNScorer, BiasedMFScorer)):
        return None
    ds = _numbered_dataset(scorer, lookup)
    if ds is None:
        return None
    rating = ds._attrs.get("rating")
    if isinstance(scorer, BiasedMFScorer):
        # trained, a bias model with both terms, ratings to fold in (the per-query path raises
        # without), and the lookup's users where stored rows are taken by user number
        if getattr(scorer, "item_embeddings", None) is None or \
                getattr(scorer, "bias", None) is None or not scorer._batch_ready() or \
                rating is None or not _users_agree(scorer, ds, required=False):
            return None
    elif isinstance(scorer, UserKNNScorer):
        if not scorer.is_trained() or not _users_agree(scorer, ds, required=True):
            return None
        if scorer.config.explicit and rating is None:
            return None  # (the per-query path answers NaN)
    else:
        if not scorer.is_trained():
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
        if model.items is not None and not _same(model.items, ds.items):
            return None
        if model.users is not None and (not _same(model.users, ds.users) or rating is None or
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
    key_arr = _as_array(keys)
    n_items = len(scorer.items)
    nums = _item_numbers(scorer.items, item_ids)
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
        lo, hi = int(offsets[s0]), int(offsets[s1])
        n = hi - lo
        hb = lookup.batch(key_arr[s0:s1])
        nohist[s0:s1] = hb.lengths == 0
        if n == 0:
            continue  # (empty target lists only: nothing to score)
        h_ptr = offsets[s0:s1 + 1] - lo
        d_ptr, d_nums = D.upload_targets(h_ptr, nums[lo:hi], d)
        if knn:
            s_dev, c_dev = scorer.score_history_batch(hb, d_ptr, d_nums)
        else:
            s_dev = scorer.predict_history_batch(hb, d_ptr, d_nums, h_tgt_ptr=h_ptr)
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
    return _scored_lists(keys, offsets, item_ids, fields, scores, counts, nohist, fb)


def _bias_predict_parts(pipe: Pipeline):
    """(BiasScorer, lookup, with_fallback) when ``rating-predictor`` is a trained ``BiasScorer`` that
    takes the lookup's batches (``takes_batches_of``: an item vocabulary, the lookup's
    vocabularies, float32 ratings under a user term), alone or under the ``FallbackScorer`` of
    ``std:topn-predict`` over a trained ``BiasScorer``; None otherwise."""
    from .basic import BiasScorer, FallbackScorer

    scorer = _slot(pipe, "scorer")
    lookup_node = pipe.nodes.get("history-lookup")
    if not isinstance(scorer, BiasScorer) or lookup_node is None or not scorer.is_trained():
        return None
    lookup = lookup_node.component
    if _numbered_dataset(scorer, lookup) is None or not _takes_history_batches(scorer, lookup):
        return None
    target = pipe.aliases.get("rating-predictor")
    if target == pipe.aliases.get("scorer", "scorer"):
        return scorer, lookup, False
    merger = pipe.nodes.get("rating-merger")
    if target != "rating-merger" or merger is None:
        return None  # (``std:topn`` has no rating predictor: the loop raises, as before)
    fb = pipe.nodes.get("fallback-predictor")
    if not isinstance(merger.component, FallbackScorer) or fb is None or \
            not isinstance(fb.component, BiasScorer) or not fb.component.is_trained():
        return None
    return scorer, lookup, True


def _predict_bias(parts, keys, offsets, item_ids, fields, batch_size: int):
    """
    ``rating-predictor`` of a Bias pipeline for whole batches: per batch the user terms
    (``lk_bias_user_offsets``), the cells at the targets (``lk_bias_score_ragged``) and one
    download.  A ``BiasScorer`` scores every target -- an unknown item, an unknown user -- so the
    fallback of ``std:topn-predict`` is never taken: ``is_fallback`` is there, and all False.
    """
    scorer, lookup, with_fallback = parts
    B = len(keys)
    if B == 0:
        return ItemListCollection(("user_id",))
    key_arr = _as_array(keys)
    nums = _item_numbers(scorer.items, item_ids)
    total = int(offsets[-1])
    scores = np.empty(total, np.float32)
    for _s0, _s1, lo, hi, _hb, _h_ptr, _d_ptr, _d_nums, s_dev, _c in _scored_batches(
            (scorer, lookup, "own"), key_arr, offsets, nums, batch_size):
        if s_dev is not None:
            scores[lo:hi] = s_dev.cpu().numpy()
    return _scored_lists(keys, offsets, item_ids, fields, scores,
                         is_fallback=np.zeros(total, np.bool_) if with_fallback else None)


def _scored_lists(keys, offsets, item_ids, fields, scores, counts=None, nohist=None,
                  is_fallback=None) -> ItemListCollection:
    """The result of ``predict`` / ``score``: the caller's ids and fields, then ``nbr_counts``
    (where there are ``counts``; absent from the lists of the queries ``nohist`` flags, those
    without history), ``score``, and ``is_fallback`` last (where there are flags)."""
    out_fields = dict(fields)
    if counts is not None:
        out_fields["nbr_counts"] = counts
    out_fields["score"] = scores
    if is_fallback is not None:
        out_fields["is_fallback"] = is_fallback
    return ItemListCollection.from_ragged(
        keys, offsets, item_ids, out_fields, key=("user_id",),
        absent=None if counts is None else {"nbr_counts": nohist})


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


# ---- per-query candidate lists: recommend(candidates=...) and score ---------------------------
def _candidate_route(pipe: Pipeline):
    """
    (scorer, lookup, route) when the scorer's output for each query's OWN items can be computed
    for whole batches by user number, None when it takes the per-query loop.  ``route``:
    ``"own"`` -- the scorer has ``score_candidates_batch`` (``ImplicitMFScorer``, the
    ``BiasedFactorScoring`` family: ``FlexMFImplicitScorer``, ``HPFScorer``, ``LightGCNScorer``;
    ``GlobalBiasPairScoring``: ``FlexMFExplicitScorer``, ``BiasedSVDScorer``; ``ItemKNNScorer``;
    ``SLIMScorer`` and ``AssociationScorer``: the chain of their panel cell at the targets only,
    ``lk_sparse_score_candidates``; ``PopScorer`` / ``TimeBoundedPopScore``: the score row read at
    the targets; ``BiasScorer``: its cell at the targets, ``lk_bias_score_ragged``);
    ``"panel"`` -- ``dense_scores_batch`` read at the targets by ``lk_panel_take_ragged``
    (``EASEScorer``, ``UserKNNScorer``: the two whose panel is shown bit-equal to ``__call__``).
    The pipeline must be wired as ``std:topn`` wires it (the scorer scores ``items`` when given;
    a scorer that declares ``ignores_query`` may have no ``query`` input at all),
    the lookup must hand out ``HistoryBatch`` es and every vocabulary must agree
    (``_numbered_dataset``, ``_users_agree``: the checks of ``_batched_predict_parts``).

    Follow-up work, today through the loop: ``BiasedMFScorer`` (its ``__call__`` is float64 on the
    host; ``lk_bmf_finish_ragged`` is the finish its route will take).  Which RANKERS run batched
    over a route is :func:`_candidate_mode`'s matter.
    """
    from .knn import EASEScorer, ItemKNNScorer, UserKNNScorer

    scorer = _slot(pipe, "scorer")
    lookup_node = pipe.nodes.get("history-lookup")
    if scorer is None or lookup_node is None:
        return None
    node = pipe.node("scorer")
    cand =pipe.nodes.get(node.wiring.get("items"))
    unwired = "query" not in node.wiring and getattr(scorer, "ignores_query", False)
    if (node.wiring.get("query") != "history-lookup" and not unwired) or cand is None or \
            cand.kind != "first-of" or cand.wiring["sources"][:1] != ["items"]:
        return None
    lookup = lookup_node.component
    ds = _numbered_dataset(scorer, lookup)
    if ds is None or not _users_agree(scorer, ds, required=False):
        return None
    if hasattr(scorer, "is_trained") and not scorer.is_trained():
        return None
    if not _takes_batches_of(scorer, lookup):
        return None  # (``BiasScorer``: a user term over ratings that are not float32)
    if isinstance(scorer, (ItemKNNScorer, UserKNNScorer)) and scorer.config.explicit and \
            ds._attrs.get("rating") is None:
        return None  # (the per-query path raises / answers NaN: it goes on doing so)
    if hasattr(scorer, "score_candidates_batch"):
        return scorer, lookup, "own"
    if isinstance(scorer, (EASEScorer, UserKNNScorer)) and hasattr(scorer, "dense_scores_batch"):
        return scorer, lookup, "panel"
    return None


def _scored_batches(plan, key_arr, offsets, nums, batch_size: int, *, with_counts: bool = False):
    """
    The batches of a candidate call, scored: per batch of at most ``batch_size`` queries (a panel
    scorer: at most its ``_panel_rows()``, 2048 without one) the histories by user number, ONE
    packed upload of the target offsets and item numbers, and the scorer's scores of the targets
    left on the device.  Yields (s0, s1, lo, hi, HistoryBatch, host offsets from 0, device
    offsets, device item numbers, device scores, device neighbour counts | None); a batch without
    targets is yielded with ``None`` s for the device values.
    """
    from . import _device as D

    scorer, lookup, route = plan
    B = len(key_arr)
    if route == "panel":
        rows = scorer._panel_rows() if hasattr(scorer, "_panel_rows") else 2048
        batch_size = max(1, min(batch_size, rows))
    dev = D.device()
    for s0 in range(0, B, batch_size):
        s1 = min(B, s0 + batch_size)
        lo, hi = int(offsets[s0]), int(offsets[s1])
        hb = lookup.batch(key_arr[s0:s1])
        h_ptr = offsets[s0:s1 + 1] - lo
        if hi == lo:
            yield s0, s1, lo, hi, hb, h_ptr, None, None, None, None
            continue
        d_ptr, d_nums = D.upload_targets(h_ptr, nums[lo:hi], dev)
        counts = None
        if route == "panel":
            panel, _valid, _hist = scorer.dense_scores_batch(hb)  # (the history is not struck)
            s_dev = D.panel_take_ragged(panel, len(scorer.items), d_ptr, d_nums, h_ptr)
            del panel
        elif with_counts:
            s_dev, counts = scorer.score_candidates_batch(hb, h_ptr, nums[lo:hi],
                                                          d_targets=(d_ptr, d_nums),
                                                          with_counts=True)
        else:
            s_dev = scorer.score_candidates_batch(hb, h_ptr, nums[lo:hi],
                                                  d_targets=(d_ptr, d_nums))
        yield s0, s1, lo, hi, hb, h_ptr, d_ptr, d_nums, s_dev, counts


def _ranks_unknown_items(scorer, item_ids=None, *, nums=None) -> bool:
    """Does a ranking of these candidates (``item_ids``, or their numbers ``nums``) hold items the
    scorer's vocabulary does not?  Every scorer but ``BiasScorer`` answers NaN for such an item and
    the rankers drop it -- for them the answer is False, unlooked --; ``BiasScorer`` scores it
    (``scores_unknown_items``) and ``pipe.run`` lists it under its id, which a list of item NUMBERS
    cannot say: such a call goes query by query."""
    if not getattr(scorer, "scores_unknown_items", False):
        return False
    if nums is None:
        nums = _item_numbers(scorer.items, item_ids)
    return bool((nums < 0).any())


def _item_numbers(vocab, item_ids) -> np.ndarray:
    "the ids' numbers in ``vocab`` as int32, negative for an id it does not hold"
    if len(item_ids) == 0:
        return np.zeros(0, np.int32)
    return np.ascontiguousarray(vocab.numbers(item_ids, missing="negative"), np.int32)


def _candidate_lists(users, candidates):
    """
    The candidate lists of a call as :func:`_ragged_pairs` gives them, in the order of the
    output: ``users=None`` -- the candidates' keys in their order; otherwise the lists of
    ``users`` in that order (``ValueError`` naming the first user without an entry).
    """
    keys, offsets, item_ids, fields, lists = _ragged_pairs(candidates)
    keys = _key_list(keys)
    if users is not None:
        users = _key_list(users)
        pos = {k: i for i, k in enumerate(keys)}
        for u in users:
            if u not in pos:
                raise ValueError(f"recommend: no candidates for user {u!r}")
        sel = np.fromiter((pos[u] for u in users), np.int64, len(users))
        lens = np.diff(offsets)[sel]
        new_off = np.zeros(len(sel) + 1, np.int64)
        np.cumsum(lens, out=new_off[1:])
        take = np.repeat(offsets[:-1][sel] - new_off[:-1], lens) + np.arange(int(new_off[-1]))
        item_ids = item_ids[take]
        if fields is not None:
            fields = {f: v[take] for f, v in fields.items()}
        if lists is not None:
            lists = [lists[i] for i in sel]
        keys, offsets = users, new_off
    return keys, offsets, item_ids, fields, lists


def _candidate_mode(pipe: Pipeline, fields, n_lists: int):
    """
    How a call over candidate lists runs, as (mode, ranker, route): ``fields`` is the lists' own
    fields (None: they differ from list to list), ``n_lists`` how many lists there are.

    - ``"random"``: an empty scorer slot, a ``RandomSelector`` and no reranker, lists with the
      same fields, at least one -- :func:`_random_candidates` is tried;
    - ``"topn"``: a route (:func:`_candidate_route`), lists without fields, no reranker or one that
      takes batches (``_reranks_batches``), and a ranker that is exactly a ``TopNRanker`` over the
      scorer's output (a subclass may rank otherwise) -- also with no list at all;
    - ``"sample"``: the same under a ``StochasticTopNRanker`` over the scorer's output, at least
      one list -- :func:`_sample_candidates` is tried;
    - ``"loop"``: everything else, query by query (``ranker`` and ``route`` are None).

    ``"random"`` and ``"sample"`` may still end in the loop: for another wiring than
    ``random_pipeline``'s, or lists :func:`_candidate_addresses` cannot pack.
    """
    scorer = _slot(pipe, "scorer")
    reranker = _slot(pipe, "reranker")
    if scorer is None:
        selector = _ranker(pipe, RandomSelector)
        if selector is not None and reranker is None and fields is not None and n_lists:
            return "random", selector, None
        return "loop", None, None
    plan = _candidate_route(pipe)
    if plan is not None and fields == {} and \
            (reranker is None or _reranks_batches(reranker, scorer)):
        ranker = _ranker(pipe, TopNRanker, exact=True, over_scorer=True)
        if ranker is not None:
            return "topn", ranker, plan
        ranker = _ranker(pipe, StochasticTopNRanker, over_scorer=True)
        if ranker is not None and n_lists:
            return "sample", ranker, plan
    return "loop", None, None


def _candidate_addresses(lists, offsets, numbers, vocab):
    """
    How the draws of a ragged batch of candidate lists are addressed -- exactly as
    ``StochasticTopNRanker.sample`` / ``RandomSelector.__call__`` address one list:

    - lists without a vocabulary (``lists`` None: a frame; ids; dicts of arrays): by POSITION, the
      row is as wide as the list;
    - lists that all carry ``vocab``: by item NUMBER (``numbers``: each entry's number in
      ``vocab``), the row is as wide as the vocabulary, and the entries of a list are sorted by
      number (``lk_ragged_stochastic_keys`` wants ascending addresses).

    Returns (addresses int32 [total], widths int32 [B], order): ``order`` is None by position,
    else the int64 permutation with ``sorted = original[order]`` -- the entries stay inside their
    list.  None when the batch has to go query by query: a list with another vocabulary, lists of
    both kinds, or a list in which an item repeats (``numbers`` equal and not negative: the
    per-query row keeps the last one).  Empty lists are of either kind.
    """
    offsets = np.asarray(offsets, np.int64)
    numbers = np.asarray(numbers)
    lens = np.diff(offsets)
    B, total = len(lens), int(offsets[-1])
    by_number = False
    if lists is not None:
        kinds = set()
        for il in lists:
            if len(il) == 0:
                continue
            v = il.vocabulary
            if v is None:
                kinds.add(0)
            elif vocab is not None and _same(v, vocab):
                kinds.add(1)
            else:
                return None
        if len(kinds) > 1:
            return None
        by_number = kinds == {1}
    # one int64 key per entry, (list, number + 1): a sort of it brings a list's repeats together
    # (an unknown item, negative, is 0 in the low word and never counts) -- ten times cheaper than
    # a lexsort at a million entries
    seg = np.repeat(np.arange(B, dtype=np.int64), lens)
    key = (seg << 32) | (np.maximum(numbers, -1).astype(np.int64) + 1)
    if not by_number:
        srt = np.sort(key)
        if total > 1 and ((srt[1:] == srt[:-1]) & ((srt[1:] & 0xFFFFFFFF) != 0)).any():
            return None
        addr = (np.arange(total, dtype=np.int64) - np.repeat(offsets[:-1], lens)).astype(np.int32)
        return addr, lens.astype(np.int32), None
    order = np.argsort(key, kind="stable")  # (the lists stay apart: the list is the high word)
    srt = key[order]
    if total and ((srt & 0xFFFFFFFF) == 0).any():
        return None  # (a list that carries the vocabulary holds its items only)
    if total > 1 and (srt[1:] == srt[:-1]).any():
        return None
    return (np.ascontiguousarray((srt & 0xFFFFFFFF) - 1, np.int32),
            np.full(B, len(vocab), np.int32), order.astype(np.int64))


def _sample_candidates(plan, ranker, keys, offsets, item_ids, lists, n, samples: int,
                       batch_size: int):
    """
    ``samples`` sampled rankings of every user's own candidate list, whole batches at a time:
    :func:`_scored_batches` -> the ranker's ``rank_ragged`` -> one download per batch; no
    [B x items] panel.  Streams as :func:`_sample_panels` takes them: ONE ``streams`` call over
    the users as the lookup types them.  Returns (user ids, item numbers [B x S x width], keys
    [B x S x width]), or None where :func:`_candidate_addresses` sends the batch to the loop
    (nothing has been drawn then).
    """
    from . import _device as D

    scorer, lookup, _route = plan
    B = len(keys)
    key_arr = _as_array(keys)
    nums = _item_numbers(scorer.items, item_ids)
    if _ranks_unknown_items(scorer, nums=nums):
        return None
    packed = _candidate_addresses(lists, offsets, nums, scorer.items)
    if packed is None:
        return None
    addr, widths, order = packed
    if order is not None:
        nums = nums[order]  # (scored in address order; the lists hold item numbers either way)
    samples = int(samples)
    n = ranker._length(n)
    width = int(np.diff(offsets).max()) if n < 0 else n
    idx = np.full((B, samples, width), -1, np.int32)
    kk = np.full((B, samples, width), np.nan, np.float32)
    if width == 0 or samples == 0:
        return key_arr, idx, kk
    streams = ranker.streams(lookup.batch(key_arr).user_ids)
    for s0, s1, lo, hi, _hb, h_ptr, _d_ptr, d_nums, s_dev, _c in _scored_batches(
            plan, key_arr, offsets, nums, batch_size):
        if s_dev is None:
            continue
        i_dev, k_dev = ranker.rank_ragged(h_ptr, addr[lo:hi], d_nums, s_dev, widths[s0:s1],
                                          streams[s0:s1], n, samples=samples, device_output=True)
        w = i_dev.shape[2]
        if w:
            i, k = D.lists_to_host(i_dev.view(-1, w), k_dev.view(-1, w))
            idx[s0:s1, :, :w] = i.reshape(s1 - s0, samples, w)
            kk[s0:s1, :, :w] = k.reshape(s1 - s0, samples, w)
    return key_arr, idx, kk


def _item_codes(item_ids) -> np.ndarray:
    "a non-negative number below 2^31 - 1 per entry, equal for equal ids (no vocabulary needed)"
    ids = np.asarray(item_ids)
    if len(ids) and ids.dtype.kind in "iu":
        lo = int(ids.min())
        if int(ids.max()) - lo < 2 ** 31 - 1:
            return (ids - lo).astype(np.int64)
    return pd.factorize(ids)[0]


def _random_candidates(pipe: Pipeline, selector, keys, offsets, item_ids, fields, lists, n,
                       batch_size: int):
    """
    ``recommend(candidates=)`` for a ``random_pipeline``: there is no scorer, the selector's
    ``rank_ragged`` draws from the candidate lists directly (a constant score, no transform),
    and the result carries the caller's ids and fields and no score, as
    ``RandomSelector.__call__`` returns it.  Unknown items are ordinary candidates; an unknown
    user has a stream like any other.  None where the batch has to go query by query: another
    wiring than ``random_pipeline``'s, a lookup without ``batch``, or addresses
    (:func:`_candidate_addresses`: by the vocabulary the lists carry, else by position) that
    cannot be packed.
    """
    node = pipe.node("ranker")
    cand = pipe.nodes.get(node.wiring.get("items"))
    lookup_node = pipe.nodes.get("history-lookup")
    if cand is None or cand.kind != "first-of" or cand.wiring["sources"][:1] != ["items"] or \
            node.wiring.get("query") != "history-lookup" or lookup_node is None or \
            not hasattr(lookup_node.component, "batch"):
        return None
    vocab = None
    if lists is not None:
        vocab = next((il.vocabulary for il in lists if len(il)), None)
    numbers = _item_codes(item_ids) if vocab is None else _item_numbers(vocab, item_ids)
    packed = _candidate_addresses(lists, offsets, numbers, vocab)
    if packed is None:
        return None
    addr, widths, order = packed
    B, total = len(keys), int(offsets[-1])
    n = selector._length(n)
    key_arr = _as_array(keys)
    streams = selector.streams(lookup_node.component.batch(key_arr).user_ids)
    # the result carries each picked entry's position in the caller's arrays
    where = np.arange(total, dtype=np.int32) if order is None else order.astype(np.int32)
    picked, counts = [], np.zeros(B, np.int64)
    for s0 in range(0, B, batch_size):
        s1 = min(B, s0 + batch_size)
        lo, hi = int(offsets[s0]), int(offsets[s1])
        if hi == lo or n == 0:
            continue
        idx = selector.rank_ragged(offsets[s0:s1 + 1] - lo, addr[lo:hi], where[lo:hi],
                                   widths[s0:s1], streams[s0:s1], n)[:, 0]
        keep = idx >= 0
        counts[s0:s1] = keep.sum(axis=1)
        picked.append(idx[keep])  # (row-major: list by list, in rank order)
    take = np.concatenate(picked) if picked else np.zeros(0, np.int32)
    out_off = np.zeros(B + 1, np.int64)
    np.cumsum(counts, out=out_off[1:])
    return ItemListCollection.from_ragged(keys, out_off, item_ids[take],
                                          {f: v[take] for f, v in fields.items()},
                                          key=("user_id",))


def _recommend_candidates(pipe: Pipeline, users, n, candidates, batch_size: int,
                          rerank_depth) -> ItemListCollection:
    """
    ``recommend`` over each user's own candidate list: user ``u``'s result is
    ``pipe.run("recommender", query=u, items=candidates[u], n=n)``.  The candidate selector is
    bypassed exactly as in the reference pipeline, so the user's history is NOT excluded; items
    the scorer does not know never appear; an unknown user and an empty candidate list give an
    empty list that is present in the output.  ``users=None``: the candidates' keys in their
    order; otherwise every user must have an entry (``ValueError`` naming the first without) and
    the output follows ``users``.  ``n`` None or negative ranks every candidate.

    Whole batches on the device where :func:`_candidate_route` has a route and the ranker is a
    plain ``TopNRanker``: per batch one packed upload, the scorer's scores of the targets,
    ``lk_ragged_topn`` (the order of ``lk_argtopn`` per list), one download; a reranker with
    ``rerank_batch`` and ``rerank_depth`` then apply to the [B x n] arrays as in ``recommend``.
    A ``StochasticTopNRanker`` over the scorer's output takes the same scores through its
    ``rank_ragged`` (:func:`_sample_candidates`: the keys of ``lk_ragged_stochastic_keys`` as the
    lists' scores, as ``sample()`` returns them; ``rerank_depth`` raises), and a
    ``random_pipeline`` -- no scorer -- draws from the lists directly
    (:func:`_random_candidates`).  The lists are the per-query ones bit for bit.  Through
    ``pipe.run`` query by query instead: candidate lists that carry fields of their own under a
    scorer (a ``score`` among them: the per-query lists keep them), a reranker without
    ``rerank_batch``, a scorer without a route, vocabularies that disagree, and under the two
    drawing rankers the lists :func:`_candidate_addresses` cannot pack -- a repeated item,
    another vocabulary than the scorer's, lists with and without a vocabulary.  So does a call
    whose lists hold an item outside the vocabulary of a scorer that scores such items
    (``BiasScorer``: ``_ranks_unknown_items``); with ``rerank_depth``, which the loop cannot
    honour, that call raises ``ValueError``.
    """
    ragged = _candidate_lists(users, candidates)
    keys, offsets, item_ids, fields, lists = ragged
    scorer = _slot(pipe, "scorer")
    reranker = _slot(pipe, "reranker")
    if scorer is None and rerank_depth is not None:
        raise ValueError("rerank_depth does not apply to a random selection")
    _check_rerank_depth(pipe, reranker, scorer, n, rerank_depth)
    mode, ranker, plan = _candidate_mode(pipe, fields, len(keys))
    if mode == "topn" and _ranks_unknown_items(scorer, item_ids):
        if rerank_depth is not None:  # (the loop reranks the ranker's n items: it has no depth)
            raise ValueError("rerank_depth needs candidate lists of items the scorer knows: "
                             "an item outside its vocabulary sends the call through pipe.run")
        mode = "loop"
    out = None  # (in every mode but "loop" the reranker, if there is one, takes batches)
    if mode == "random":
        out = _random_candidates(pipe, ranker, keys, offsets, item_ids, fields, lists, n,
                                 batch_size)
    elif mode == "sample":
        drawn = _draw_samples(pipe, keys, n, 1, batch_size, ragged, (mode, ranker, plan))
        if drawn is not None:
            out = _sampled_lists(drawn, scorer.items, reranker, n, key=("user_id",))
    if out is not None:
        return out
    if mode != "topn":
        return ItemListCollection.from_dict(
            {u: pipe.run("recommender", query=u, items=il, n=n)
             for u, il in zip(keys, _query_lists(ragged))}, key=("user_id",))

    from . import _device as D

    B = len(keys)
    if B == 0:
        return ItemListCollection(("user_id",))
    length = n if n is not None else (ranker.config.n or -1)  # (``TopNRanker.__call__``)
    length = -1 if length < 0 else int(length)
    depth = length if rerank_depth is None else int(rerank_depth)
    width = int(np.diff(offsets).max()) if depth < 0 else depth
    key_arr = _as_array(keys)
    nums = _item_numbers(scorer.items, item_ids)
    idx = np.full((B, width), -1, np.int32)
    sc = np.full((B, width), np.nan, np.float32)
    if width:
        for s0, s1, _lo, _hi, _hb, h_ptr, d_ptr, d_nums, s_dev, _c in _scored_batches(
                plan, key_arr, offsets, nums, batch_size):
            if s_dev is None:
                continue
            i_dev, v_dev = D.ragged_topn(d_ptr, d_nums, s_dev, depth, h_ptr)
            if i_dev.shape[1]:
                i, v = D.lists_to_host(i_dev, v_dev)
                idx[s0:s1, :i.shape[1]] = i
                sc[s0:s1, :i.shape[1]] = v
    if reranker is not None:
        idx, sc = reranker.rerank_batch(idx, sc, _rerank_length(n))
    return ItemListCollection.from_arrays(key_arr, idx, sc, scorer.items, key=("user_id",))


def score(pipe: Pipeline, test, *, batch_size: int = 16384) -> ItemListCollection:
    """
    The scorer's scores for each query's own items -- ``pipe.run("scorer", query=u, items=il)`` for
    every list of ``test`` -- as an ``ItemListCollection`` keyed by ``user_id``
    (``BatchPipelineRunner.score``, src/lenskit/batch/_runner.py:114-124).  ``test``: what
    :func:`predict` takes.  No fallback is merged in and there is no ``is_fallback``: an item the
    scorer cannot score is NaN.

    Where :func:`_candidate_route` has a route the batch runs on the device like
    :func:`_predict_batched`: one packed upload and one download per batch, the lists carry the
    caller's ids and fields plus ``score`` (an ``ItemKNNScorer``: ``nbr_counts`` before it, absent
    for a query without history), bit for bit the per-query lists.  ``SLIMScorer`` and
    ``AssociationScorer`` score the targets alone (``lk_sparse_score_candidates``: no [1 x items]
    panel per query), ``PopScorer`` reads its score row at them.  Lists that already carry a
    ``score`` or ``nbr_counts``, lists with differing fields, a scorer without a route and
    vocabularies that disagree go through ``pipe.run`` query by query.
    """
    ragged = _ragged_pairs(test)
    keys, offsets, item_ids, fields, _lists = ragged
    plan = _candidate_route(pipe)
    if plan is None or fields is None or set(fields) & {"score", "nbr_counts"}:
        return ItemListCollection.from_dict(
            {u: pipe.run("scorer", query=u, items=il)
             for u, il in zip(_key_list(keys), _query_lists(ragged))}, key=("user_id",))

    import torch

    from .knn import ItemKNNScorer

    scorer = plan[0]
    B = len(keys)
    if B == 0:
        return ItemListCollection(("user_id",))
    key_arr = _as_array(keys)
    nums = _item_numbers(scorer.items, item_ids)
    total = int(offsets[-1])
    knn = isinstance(scorer, ItemKNNScorer)
    scores = np.empty(total, np.float32)
    counts = np.empty(total, np.int32) if knn else None
    nohist = np.empty(B, np.bool_)
    for s0, s1, lo, hi, hb, _h_ptr, _d_ptr, _d_nums, s_dev, c_dev in _scored_batches(
            plan, key_arr, offsets, nums, batch_size, with_counts=knn):
        nohist[s0:s1] = hb.lengths == 0
        if s_dev is None:
            continue
        if knn:  # one download: scores | counts
            host = torch.cat([s_dev.view(torch.int32), c_dev]).cpu().numpy()
            scores[lo:hi] = host[:hi - lo].view(np.float32)
            counts[lo:hi] = host[hi - lo:]
        else:
            scores[lo:hi] = s_dev.cpu().numpy()
    return _scored_lists(keys, offsets, item_ids, fields, scores, counts, nohist)
