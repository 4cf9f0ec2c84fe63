"""
Plumbing components of the standard pipelines -- mirror of ``lenskit.basic`` as far as the
two target TOMLs need it (host NumPy; not on the accelerated path except ``TopNRanker``):

``UserTrainingHistoryLookup``       src/lenskit/basic/history.py:37-95
``TrainingItemsCandidateSelector``  src/lenskit/basic/candidates.py:50-94
``TopNRanker``                      src/lenskit/basic/topn.py:32-69 (-> ItemList.top_n ->
                                    the GPU top-N kernel)
``BiasScorer`` / ``FallbackScorer`` src/lenskit/basic/bias.py, composite.py (std:topn-predict;
                                    the fit and the batch paths are csrc/bias.hip)
``PopScorer`` / ``TimeBoundedPopScore``  src/lenskit/basic/popularity.py (host training; the batch
                                    path is one walk over a shared order, csrc/popular.hip)
``RandomSelector``                  src/lenskit/basic/random.py (the stochastic ranker's draws
                                    over equal weights)
"""

from __future__ import annotations

import logging
from datetime import datetime, timezone
from typing import Any, Literal

import numpy as np
import pandas as pd
from pydantic import BaseModel

from ._streams import RowStreams
from .data import Dataset, ItemList, RecQuery, Vocabulary
from .pipeline import Component
from .training import Trainable, TrainingOptions

_log = logging.getLogger(__name__)


class LookupConfig(BaseModel):
    interaction_class: str | None = None


class UserTrainingHistoryLookup(Component):
    config: LookupConfig

    def is_trained(self):
        return hasattr(self, "interactions")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        # a retrain drops the HBM copy of the previous training matrix (and what was learned
        # about it, ``ratings_finite``): batch() must never cut rows out of the old one
        self.__dict__.pop("_dev", None)
        self.interactions = data.interactions(self.config.interaction_class).matrix()

    def __call__(self, query) -> RecQuery:
        query = RecQuery.create(query)
        if query.user_id is None or self.interactions is None:
            return query
        id_type = self.interactions.row_vocabulary.ids().dtype
        if isinstance(query.user_id, str) and issubclass(id_type.type, np.number):
            query.user_id = id_type.type(query.user_id)
        if query.history_items is None:
            query.history_items = self.interactions.row_items(query.user_id)
        return query


    # -- whole batches of queries --------------------------------
    def _device_matrix(self):
        "The training matrix resident in HBM (uploaded once per training): offsets, items, ratings."
        def upload():
            from . import _device as D

            ds = self.interactions._ds
            dev = D.device()
            rat = ds._attrs.get("rating")
            return {"device": dev,
                    "csr": D.DeviceCSR.from_arrays(ds._indptr, ds._cols, rat,
                                                   (ds.user_count, ds.item_count), dev),
                    "has_ratings": rat is not None}

        return self._device_cache("matrix", upload, self.interactions)

    def ratings_finite(self) -> bool:
        """
        Is every rating of the HBM-resident training matrix finite (and float32 on the host, so
        that the device copy is the host's values)?  Scanned once per uploaded matrix and kept
        with it: the scorers that subtract a bias model from whole rows on the device
        (``BiasedMFScorer``) take the per-query rule -- non-finite ratings are dropped -- only
        through the host.
        """
        st = self._device_matrix()
        if "ratings_finite" not in st:
            import torch

            rat = self.interactions._ds._attrs.get("rating")
            vals = st["csr"].values
            st["ratings_finite"] = bool(
                rat is not None and rat.dtype == np.float32 and vals is not None
                and (vals.numel() == 0 or bool(torch.isfinite(vals).all().item())))
        return st["ratings_finite"]

    def batch(self, user_ids) -> "HistoryBatch":
        """
        The training histories of MANY users at once: what ``__call__`` does per query
        (src/lenskit/basic/history.py:77-95: attach ``interactions.row_items(user_id)`` as the
        query's history) for a whole batch, without building an ``ItemList`` per user -- the user
        numbers come from one vectorised vocabulary lookup and the rows are cut out of the
        HBM-resident training matrix by one kernel when a scorer asks for them
        (:meth:`HistoryBatch.csr`).  Unknown users get empty histories, like the reference.
        """
        ids = np.asarray(list(user_ids) if not isinstance(user_ids, np.ndarray) else user_ids)
        vocab = self.interactions.row_vocabulary
        id_type = vocab.ids().dtype
        if ids.dtype.kind in "US" and issubclass(id_type.type, np.number):
            ids = ids.astype(id_type)  # (history.py:85-87: string ids for a numeric vocabulary)
        nums = vocab.numbers(ids, missing="negative") if len(ids) else np.zeros(0, np.int32)
        return HistoryBatch(self, ids, nums)


class HistoryBatch:
    """
    The histories of a batch of queries as rows of the training matrix (user numbers), not as
    one ``ItemList`` per user: ``len``, ``user_ids``, ``user_nums`` (-1 = unknown user),
    ``lengths`` (host), ``items`` (the vocabulary the item numbers refer to), and :meth:`csr` --
    the histories' CSR in HBM, cut out by ``lk_csr_gather_rows``.  ``queries()`` gives the plain
    per-query objects for scorers without a batched path.
    """

    def __init__(self, lookup: "UserTrainingHistoryLookup", user_ids: np.ndarray,
                 user_nums: np.ndarray):
        self.lookup = lookup
        self.user_ids = user_ids
        self.user_nums = np.ascontiguousarray(user_nums, dtype=np.int32)
        ds = lookup.interactions._ds
        self.items: Vocabulary = ds.items
        self.users: Vocabulary = ds.users
        hp = ds._indptr
        safe = np.maximum(self.user_nums, 0)
        self.lengths = np.where(self.user_nums >= 0, hp[safe + 1] - hp[safe], 0).astype(np.int64)
        self._cache: dict = {}

    def __len__(self):
        return len(self.user_nums)

    @property
    def has_ratings(self) -> bool:
        return "rating" in self.lookup.interactions._ds._attrs

    def csr(self, *, use_ratings: bool = False, scale: float = 1.0, with_values: bool = True,
            col_bias=None):
        """Device CSR (queries x items, int64 offsets; ``h_indptr`` = the host copy) of the
        histories; values = ``rating * scale`` (``use_ratings``) or the constant ``scale``, with
        ``col_bias`` (device f32 per item) subtracted from the rating first."""
        from . import _device as D

        key = (bool(use_ratings), float(scale), bool(with_values),
               None if col_bias is None else int(col_bias.data_ptr()))
        hit = self._cache.get(key)
        if hit is not None:
            return hit
        st = self.lookup._device_matrix()
        src = st["csr"]
        if use_ratings and not st["has_ratings"]:
            raise ValueError("no ratings in user items")  # (_implicit.py:85-86)
        if not use_ratings and src.values is not None:
            src = D.DeviceCSR(src.indptr, src.indices, None, src.shape, src.h_indptr)
        out = D.gather_rows(src, self.user_nums, scale=scale, with_values=with_values,
                            col_bias=col_bias)
        self._cache[key] = out
        return out

    def matrix_rows(self):
        """(the HBM-resident training matrix itself as a structure-only device CSR with int64
        offsets, device int32 row numbers [B] into it, -1 = unknown user): the histories by user
        number for the kernels that take row numbers -- no row gather.  Row ``r`` holds
        ``ds._cols[s:e]``, the items ``row_items`` attaches per query, in that order.  The int64
        offsets are made once per uploaded matrix and kept with it."""
        import torch

        from . import _device as D

        st = self.lookup._device_matrix()
        if "rows_csr" not in st:
            src = st["csr"]
            st["rows_csr"] = D.DeviceCSR(src.indptr.long(), src.indices, None, src.shape,
                                         src.h_indptr)
        return st["rows_csr"], torch.from_numpy(self.user_nums).to(st["device"])

    def subset(self, mask: np.ndarray) -> "HistoryBatch":
        return HistoryBatch(self.lookup, self.user_ids[mask], self.user_nums[mask])

    def queries(self) -> list:
        return [self.lookup(RecQuery.create(u.item() if isinstance(u, np.generic) else u))
                for u in self.user_ids]


class TrainingItemsCandidateConfig(BaseModel):
    exclude: str | None = "query"


class TrainingItemsCandidateSelector(Component):
    config: TrainingItemsCandidateConfig

    def is_trained(self):
        return hasattr(self, "items_")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        self.items_ = data.items

    def __call__(self, query) -> ItemList:
        query = RecQuery.create(query)
        items = ItemList.from_vocabulary(self.items_)
        exclude = query.query_items if self.config.exclude in ("query", "all") else None
        if exclude is not None and len(exclude) > 0:
            nums = exclude.numbers(vocabulary=self.items_, missing="negative")
            items = items.remove(numbers=nums[nums >= 0])
        return items


class TopNConfig(BaseModel):
    n: int | None = None


class TopNRanker(Component):
    config: TopNConfig

    def __call__(self, *, items: ItemList, n: int | None = None) -> ItemList:
        if n is None:
            n = self.config.n or -1
        return items.top_n(n)


class BiasConfig(BaseModel):
    damping: float | tuple[float, float] | dict[str, float] = 0.0
    entities: list[str] = ["user", "item"]


def _damping(d, which):
    if isinstance(d, dict):
        return float(d.get(which, 0.0))
    if isinstance(d, (tuple, list)):
        return float(d[0] if which == "user" else d[1])
    return float(d)


class BiasModel:
    """
    User-item bias model  b_ui = b_g + b_i + b_u  with Bayesian damping
    (``BiasModel``, src/lenskit/basic/bias.py:35-275): reusable by components that normalise
    ratings (the biased-MF ALS) as well as by :class:`BiasScorer`.
    """

    def __init__(self, damping=0.0, global_bias: float = 0.0):
        self.damping = damping
        self.global_bias = float(global_bias)
        self.items = self.users = None
        self.item_biases = self.user_biases = None
        # (item, user) biases left in HBM by a device fit (``learn(device=...)``); never pickled
        self.device_biases = None

    def __getstate__(self):
        st = dict(self.__dict__)
        st["device_biases"] = None
        return st

    @classmethod
    def learn(cls, data: Dataset, damping=0.0, *, entities=("user", "item"), device=None,
              csr=None, csr_t=None) -> "BiasModel":
        """
        bias.py:83-150, call for call (float64 sums, float32 biases).  ``device`` (a HIP device):
        the two passes run there (``lk_bias_fit_pass``, csrc/bias.hip) and give the bits of the
        host arithmetic below; ``csr`` / ``csr_t`` are the ratings in HBM (users x items with the
        float32 values, entries in the dataset's order) and their stable transpose with values
        where the caller holds them already -- they are built here otherwise.  The fitted
        vectors stay on the device too (``device_biases``).  Ratings that are not float32 are
        fitted on the host.
        """
        ratings = data.interaction_matrix(format="scipy", layout="coo", field="rating")
        nrows, ncols = ratings.shape
        model = cls(damping, float(np.mean(ratings.data)))
        if device is not None and ratings.data.dtype == np.float32:
            from . import _device as D

            dev = D.device(device)
            if csr is None:
                csr = D.DeviceCSR.from_arrays(data._indptr, data._cols, ratings.data,
                                              (nrows, ncols), dev)
            if csr_t is None and "item" in entities:
                csr_t = D.csr_transpose(csr, with_values=True)
            ib, ub = D.bias_fit(csr, csr_t, model.global_bias, _damping(damping, "item"),
                                _damping(damping, "user"), items="item" in entities,
                                users="user" in entities)
            if ib is not None:
                model.items, model.item_biases = data.items, ib.cpu().numpy()
            if ub is not None:
                model.users, model.user_biases = data.users, ub.cpu().numpy()
            model.device_biases = (ib, ub)
            return model
        centered = ratings.data - model.global_bias
        if "item" in entities:
            counts = np.full(ncols, _damping(damping, "item"))
            sums = np.zeros(ncols)
            np.add.at(counts, ratings.col, 1)
            np.add.at(sums, ratings.col, centered)
            i_bias = np.zeros(ncols, dtype=np.float32)
            np.divide(sums, counts, out=i_bias, where=counts > 0)
            model.items, model.item_biases = data.items, i_bias
            centered = centered - i_bias[ratings.col]
        if "user" in entities:
            counts = np.full(nrows, _damping(damping, "user"))
            sums = np.zeros(nrows)
            np.add.at(counts, ratings.row, 1)
            np.add.at(sums, ratings.row, centered)
            u_bias = np.zeros(nrows, dtype=np.float32)
            np.divide(sums, counts, out=u_bias, where=counts > 0)
            model.users, model.user_biases = data.users, u_bias
        return model

    def compute_for_items(self, items: ItemList, user_id=None, user_items: ItemList | None = None,
                          *, bias: float | None = None):
        """
        bias.py:166-241: composite biases of ``items``; with ``bias`` (a known user bias) only
        the scores are returned, otherwise (scores, user_bias) with the user bias taken from
        ``user_items``' ratings when present, else from the stored value of ``user_id``.
        """
        scores = np.full(len(items), self.global_bias, dtype=np.float32)
        if self.item_biases is not None:
            idx = items.numbers(vocabulary=self.items, missing="negative")
            m = idx >= 0
            scores[m] += self.item_biases[idx[m]]
        if bias is not None:
            return scores + bias
        ratings = user_items.field("rating") if user_items is not None else None
        user_bias = 0.0
        if self.users is not None:
            if ratings is not None:
                uoff = np.asarray(ratings, dtype=np.float64) - self.global_bias
                if self.item_biases is not None:
                    r_idx = user_items.numbers(vocabulary=self.items, missing="negative")
                    rm = r_idx >= 0
                    uoff[rm] -= self.item_biases[r_idx[rm]]
                user_bias = np.sum(uoff) / (np.sum(np.isfinite(uoff)) +
                                            _damping(self.damping, "user"))
                if np.isnan(user_bias):
                    user_bias = 0
                scores += np.float32(user_bias)
            elif user_id is not None:
                uno = self.users.number(user_id, missing=None)
                if uno is not None:
                    user_bias = self.user_biases[uno]
                    scores += user_bias
        return scores, user_bias

    def transform_matrix(self, matrix):
        "bias.py:246-275: subtract the biases from a COO ratings matrix."
        import scipy.sparse as sps

        values = matrix.data - self.global_bias
        if self.item_biases is not None:
            values -= self.item_biases[matrix.col]
        if self.user_biases is not None:
            values -= self.user_biases[matrix.row]
        return sps.coo_array((values, (matrix.row, matrix.col)), shape=matrix.shape)


class BiasScorer(Component):
    """``BiasScorer`` (src/lenskit/basic/bias.py:278-360) over :class:`BiasModel`:
    score = mu + b_i + b_u.

    Trained on the device where there is one (``lk_bias_fit_pass``; the host arithmetic of
    ``BiasModel.learn`` without -- the model has the same bits either way).  A whole batch of
    queries is scored by csrc/bias.hip: :meth:`recommend_batch` and :meth:`dense_scores_batch`
    through [rows x items] panels of at most ``PANEL_BYTES``, :meth:`score_candidates_batch` at
    the ragged targets alone.  A cell is ``(float32(mu) + b_i) + ub_q`` with the user term of
    :meth:`user_offsets_batch`; an item the model does not know scores ``float32(mu) (+ ub_q)``,
    not NaN (``scores_unknown_items``).
    """

    config: BiasConfig

    PANEL_BYTES = 1 << 30  # score panel of one recommend step
    accepts_history_batch = True  # the batch calls take a HistoryBatch
    returns_device_lists = True  # recommend_batch has ``device_output``
    scores_unknown_items = True  # a candidate outside the vocabulary keeps a finite score

    def is_trained(self):
        return hasattr(self, "model")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        from . import _native

        device = None
        name = options.configured_device()
        if name != "cpu":
            try:
                from . import _device as D

                device = D.device(None if name == "cuda" else name)
            except _native.BackendUnavailable:
                device = None  # (no HIP device: the host arithmetic, the same bits)
        self.model = BiasModel.learn(data, self.config.damping, entities=self.config.entities,
                                     device=device)

    # the learned parameters, under the names the reference's scorer exposes
    global_bias = property(lambda self: self.model.global_bias)
    item_biases = property(lambda self: self.model.item_biases)
    user_biases = property(lambda self: self.model.user_biases)
    items = property(lambda self: self.model.items)
    users = property(lambda self: self.model.users)

    def __call__(self, query, items: ItemList) -> ItemList:
        query = RecQuery.create(query)
        scores, _ = self.model.compute_for_items(items, query.user_id, query.history_items)
        return ItemList(items, scores=scores)

    # -- whole batches of queries (batch.predict) ---------------------------------------------
    def _device_item_biases(self):
        "The item biases in HBM (f32; None without an item term), uploaded once per model."
        def upload():
            import torch

            from . import _device as D

            ib = self.model.item_biases
            if ib is None:
                return None
            kept = getattr(self.model, "device_biases", None)
            if kept is not None and kept[0] is not None and kept[0].device == D.device():
                return kept[0]  # (a device fit left them there)
            return torch.from_numpy(np.ascontiguousarray(ib, dtype=np.float32)).to(D.device())

        return self._device_cache("item_biases", upload, self.model)

    def takes_batches_of(self, lookup) -> bool:
        """Can a batch go by the numbers of ``lookup``'s training matrix?  The model has an item
        vocabulary and it is that matrix's; with a user term the users are its users and its
        ratings are float32 (the host sums the history's own ratings: float32 in HBM).  Answered
        once per (model, training matrix): comparing vocabularies that are not one object is a
        full comparison."""
        model = getattr(self, "model", None)
        inter = getattr(lookup, "interactions", None)
        if model is None or model.items is None or inter is None or not hasattr(lookup, "batch"):
            return False
        return self._device_cache("takes_batches_of", lambda: self._matches(model, inter._ds),
                                  model, inter)

    @staticmethod
    def _matches(model, ds) -> bool:
        if not (model.items is ds.items or model.items == ds.items):
            return False
        if model.users is not None:
            rating = ds._attrs.get("rating")
            if not (model.users is ds.users or model.users == ds.users) or rating is None or \
                    rating.dtype != np.float32:
                return False
        return True

    def _panel_rows(self) -> int:
        return max(1, self.PANEL_BYTES // (4 * max(len(self.model.items), 1)))

    def _panel(self, batch: "HistoryBatch", *, strike_history: bool):
        "One ``lk_bias_score_panel`` call: the device panel of the queries of ``batch``."
        import torch

        from . import _device as D

        if not isinstance(batch, HistoryBatch) or not self.takes_batches_of(batch.lookup):
            raise TypeError("BiasScorer's batch calls take a HistoryBatch over the training "
                            "matrix the model was fitted on")
        ub, add = self.user_offsets_batch(batch)
        strike = nums = None
        if strike_history:
            strike = batch.lookup._device_matrix()["csr"]
            nums = torch.from_numpy(batch.user_nums).to(ub.device)
        return D.bias_score_panel(len(self.model.items), self.model.global_bias,
                                  self._device_item_biases(), ub, add, strike=strike,
                                  user_nums=nums)

    def dense_scores_batch(self, queries):
        """(panel f32 [B x items] on the device, valid -- all True: an unknown user is scored
        without a user term --, history CSR): nothing is struck, the history is for the caller
        to exclude."""
        return (self._panel(queries, strike_history=False), np.ones(len(queries), dtype=bool),
                queries.csr(with_values=False))

    def recommend_batch(self, queries, n: int | None, *, exclude_history: bool = True,
                        device_output: bool = False):
        """
        The top ``n`` (None or negative: every candidate) of many queries at once -- what the
        ``recommender`` pipeline computes per query: every training item but the query's own,
        scored, ``TopNRanker``.  ``queries``: a :class:`HistoryBatch`.  Panels of at most
        ``PANEL_BYTES``, each selected from by ``lk_argtopn`` (score descending, then item number
        ascending: the per-query order).  Returns (item numbers [B x n] with -1 padding, scores
        [B x n] with NaN padding), on the device with ``device_output``.
        """
        import torch

        from . import _device as D

        B = len(queries)
        n_items = len(self.model.items)
        n = -1 if n is None else int(n)
        cols = n_items if n < 0 else n
        d = D.device()
        oi = torch.full((B, cols), -1, dtype=torch.int32, device=d)
        osc = torch.full((B, cols), float("nan"), dtype=torch.float32, device=d)
        step = self._panel_rows()
        for lo in range(0, B, step):
            sub = queries if lo == 0 and B <= step else queries.subset(slice(lo, lo + step))
            panel = self._panel(sub, strike_history=exclude_history)
            idx = D.argtopn(panel, n)
            oi[lo:lo + step, :idx.shape[1]] = idx
            osc[lo:lo + step, :idx.shape[1]] = D.take_scores(panel, idx)
            del panel
        if device_output:
            return oi, osc
        return D.lists_to_host(oi, osc)

    def score_candidates_batch(self, queries, tgt_ptr, item_nums, *, d_targets=None):
        """
        The scores of each query's OWN items, left on the device: f32 [total], entry t of query q
        is ``(float32(mu) + b_i) + ub_q``, the bits ``__call__`` gives (``lk_bias_score_ragged``:
        one pass, no panel).  An unknown item is NOT NaN: it has no item term.  ``tgt_ptr`` int64
        [B + 1] and ``item_nums`` int32 are host arrays, ``d_targets`` their device copies.
        """
        from . import _device as D

        if not isinstance(queries, HistoryBatch) or not self.takes_batches_of(queries.lookup):
            raise TypeError("BiasScorer's batch calls take a HistoryBatch over the training "
                            "matrix the model was fitted on")
        ub, add = self.user_offsets_batch(queries)
        d_ptr, d_nums = d_targets or D.upload_targets(tgt_ptr, item_nums, ub.device)
        return D.bias_score_ragged(d_ptr, d_nums, len(self.model.items), self.model.global_bias,
                                   self._device_item_biases(), ub, add)

    def user_offsets_batch(self, batch: "HistoryBatch"):
        """
        The user-bias part of ``__call__`` for a whole :class:`HistoryBatch`: what
        ``BiasModel.compute_for_items`` computes from each query's training ratings
        (src/lenskit/basic/bias.py:166-240), by one ``lk_bias_user_offsets`` call that reads the
        rows straight from the lookup's HBM-resident training matrix.  Returns device
        (ub f32 [B], add uint8 [B]): ``add`` is 1 where the host path adds ub to the scores (the
        model has user biases and the query has a training row).
        """
        import torch

        from . import _device as D

        mat = batch.lookup._device_matrix()
        dev = mat["device"]
        B = len(batch)
        if self.model.users is None:  # no user term: nothing is added
            return (torch.zeros(B, dtype=torch.float32, device=dev),
                    torch.zeros(B, dtype=torch.uint8, device=dev))
        if not mat["has_ratings"]:
            raise ValueError("user biases from the history need ratings")
        nums = torch.from_numpy(np.ascontiguousarray(batch.user_nums, dtype=np.int32)).to(dev)
        return D.bias_user_offsets(mat["csr"], nums, self.model.global_bias,
                                   self._device_item_biases(),
                                   _damping(self.model.damping, "user"))


class FallbackScorer(Component):
    "Primary scores, back-filled from the backup where missing (basic/composite.py)."

    def __call__(self, primary: ItemList, backup: ItemList) -> ItemList:
        ps = np.array(primary.scores(), dtype=np.float32, copy=True)
        missing = np.isnan(ps)
        if np.any(missing):
            b = backup.scores()
            if np.array_equal(primary.ids(), backup.ids()):
                ps[missing] = b[missing]
            else:
                lookup = dict(zip(backup.ids().tolist(), b.tolist()))
                for i in np.flatnonzero(missing):
                    ps[i] = lookup.get(primary.ids()[i], np.nan)
        return ItemList(primary, scores=ps, is_fallback=missing)


class PopConfig(BaseModel):
    "src/lenskit/basic/popularity.py:24-33"

    score: Literal["quantile", "rank", "count"] = "quantile"


class PopScorer(Component, Trainable):
    """
    Score items by their popularity (``PopScorer``, src/lenskit/basic/popularity.py:36-91):
    ``items`` and ``item_scores`` (float32, one per item number), trained on the host from
    ``data.item_stats()["count"]`` with the reference's own pandas calls -- ``quantile`` depends on
    the tie order of pandas' unstable sort, which only the same call reproduces.

    Every user's top-N over these scores is one globally sorted list with the user's own items
    skipped: :meth:`recommend_batch` walks that shared order (``lk_shared_order_topn``) instead of
    scoring and selecting per user.  The scorer never looks at the user, so an unknown user gets
    the plain top ``n`` -- in ``pipe.run`` and here.
    """

    config: PopConfig
    items: Vocabulary
    item_scores: np.ndarray

    accepts_history_batch = True  # recommend_batch takes a HistoryBatch
    returns_device_lists = True  # ... and has ``device_output``: the lists left on the device

    def is_trained(self):
        return hasattr(self, "item_scores")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        self.items = data.items
        self.item_scores = np.require(self._train_internal(data.item_stats()["count"]).values,
                                      np.float32)

    def _train_internal(self, scores: pd.Series) -> pd.Series:
        "popularity.py:68-82, call for call"
        if self.config.score == "rank":
            return scores.rank()
        elif self.config.score == "quantile":
            cmass = scores.sort_values()
            cmass = cmass.cumsum()
            cdens = cmass / scores.sum()
            return cdens.reindex(scores.index)
        elif self.config.score == "count":
            return scores
        raise ValueError("invalid scoring method " + repr(self.config.score))

    def __call__(self, items: ItemList) -> ItemList:
        inums = items.numbers(vocabulary=self.items, missing="negative")
        mask = inums >= 0
        scores = np.full(len(items), np.nan, np.float32)
        scores[mask] = self.item_scores[inums[mask]]
        return ItemList(items, scores=scores)

    # -- whole batches of queries ---------------------------------------------------------------
    def _device_order(self):
        """
        The model in HBM, built once per training: ``scores`` f32 [items], ``order`` int32 [L] --
        the items with a non-NaN score by score descending, then item number ascending -- and
        ``order_scores`` f32 [L].  The order is ``lk_argtopn``'s over the whole score row, the
        call ``ItemList.top_n`` makes per query: the tie rule is the per-query one by construction.
        """
        def build():
            import torch

            from . import _device as D

            d = D.device()
            sc = torch.from_numpy(np.ascontiguousarray(self.item_scores, dtype=np.float32)).to(d)
            if sc.numel() == 0:
                order, osc = torch.zeros(0, dtype=torch.int32, device=d), sc
            else:
                full = D.argtopn(sc[None], -1)
                vals = D.take_scores(sc[None], full)
                keep = full[0] >= 0
                order, osc = full[0][keep].contiguous(), vals[0][keep].contiguous()
            return {"device": d, "scores": sc, "order": order, "order_scores": osc}

        return self._device_cache("order", build, self.item_scores)

    def _history_rows(self, queries):
        "(queries resolved, the CSR to skip, device row numbers into it | None: row b)"
        import torch

        from . import _device as D
        from ._queries import pack_histories, resolve_queries

        queries = resolve_queries(queries, self.items)
        dev = self._device_order()["device"]
        if isinstance(queries, HistoryBatch):
            # the training matrix itself, by user number: no row gather
            return queries, queries.lookup._device_matrix()["csr"], \
                torch.from_numpy(queries.user_nums).to(dev)
        ptr, idx, _ = pack_histories(queries, self.items, unknown="drop", sort=True)
        return queries, D.DeviceCSR.from_arrays(ptr, idx, None, (len(queries), len(self.items)),
                                                dev), None

    def recommend_batch(self, queries, n: int | None, *, exclude_history: bool = True,
                        device_output: bool = False):
        """
        The top ``n`` (None or negative: all) of many queries at once: (item numbers [B x n] with
        -1 padding, scores [B x n] with NaN padding), each row the shared order with the query's
        history skipped.  ``queries``: a list of queries or a :class:`HistoryBatch`, whose rows
        are read from the HBM-resident training matrix by user number.
        """
        from . import _device as D

        st = self._device_order()
        n = -1 if n is None else int(n)
        if exclude_history:
            queries, hist, rows = self._history_rows(queries)
        else:
            hist = rows = None
        idx, sc = D.shared_order_topn(st["order"], st["order_scores"], n, len(queries),
                                      hist=hist, rows=rows)
        if device_output:
            return idx, sc
        return D.lists_to_host(idx, sc)

    ignores_query = True  # ``__call__`` takes no query: the scorer node need not be wired to one

    def score_candidates_batch(self, queries, tgt_ptr, item_nums, *, d_targets=None):
        """
        The scores of each query's OWN items, left on the device: f32 [total], entry t is
        ``item_scores[item_nums[t]]`` (the bits ``__call__`` gives), NaN for an unknown item --
        the cached device score row read at the targets as a one-row panel
        (``lk_panel_take_ragged`` with the offsets ``[0, total]``).  ``queries`` is not looked at:
        an unknown user is scored like any other, as in ``pipe.run``.  ``tgt_ptr`` int64 [B + 1]
        and ``item_nums`` int32 are host arrays, ``d_targets`` their device copies.
        """
        import torch

        from . import _device as D

        st = self._device_order()
        _d_ptr, d_nums = d_targets or D.upload_targets(tgt_ptr, item_nums, st["device"])
        ends = np.array([0, d_nums.numel()], np.int64)
        return D.panel_take_ragged(st["scores"][None], len(self.items),
                                   torch.from_numpy(ends).to(st["device"]), d_nums, ends)

    def dense_scores_batch(self, queries):
        """
        (panel f32 [B x items], valid -- all True --, history CSR): ``item_scores`` repeated per
        row, contiguous as the stochastic kernels take it; the history is for the caller to
        exclude.
        """
        from . import _device as D
        from ._queries import pack_histories, resolve_queries

        st = self._device_order()
        queries = resolve_queries(queries, self.items)
        B = len(queries)
        if isinstance(queries, HistoryBatch):
            hist = queries.csr(with_values=False)
        else:
            ptr, idx, _ = pack_histories(queries, self.items, unknown="drop", sort=True)
            hist = D.DeviceCSR.from_arrays(ptr, idx, None, (B, len(self.items)), st["device"])
        panel = st["scores"][None].expand(B, -1).contiguous()
        return panel, np.ones(B, dtype=bool), hist


class TimeBoundedPopConfig(PopConfig):
    # required by the reference's config (popularity.py:94-98); here every component can be
    # built from its defaults, so a missing cutoff is refused by ``train`` instead
    cutoff: datetime | None = None


class TimeBoundedPopScore(PopScorer):
    """
    Popularity among the interactions whose ``timestamp`` is later than ``config.cutoff``
    (``TimeBoundedPopScore``, popularity.py:101-134); without a ``timestamp`` attribute it trains
    as :class:`PopScorer` and logs a warning.  ``timestamp`` may be ``datetime64`` or numeric
    seconds since the epoch; a cutoff without a time zone is taken as UTC.

    The reference skips a retrain on ``hasattr(self, "item_scores_")``, an attribute it never
    sets; here ``train`` follows the ordinary rule of a ``Trainable``: it returns at once when
    ``is_trained()`` and ``options.retrain`` is off.  Where no interaction passes the cutoff,
    ``quantile`` is 0 / 0: every score is NaN and every list is empty, as in the reference.
    """

    config: TimeBoundedPopConfig

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        if self.is_trained() and not options.retrain:
            return
        if self.config.cutoff is None:
            raise ValueError("TimeBoundedPopScore needs a cutoff")
        stamps = data._attrs.get("timestamp")
        if stamps is None:
            _log.warning("no timestamps in interaction log; falling back to PopScorer")
            super().train(data, options)
            return
        cutoff = self.config.cutoff
        if cutoff.tzinfo is not None:
            cutoff = cutoff.astimezone(timezone.utc).replace(tzinfo=None)
        stamps = np.asarray(stamps)
        if stamps.dtype.kind == "M":
            late = stamps > np.datetime64(cutoff)
        else:
            late = stamps > cutoff.replace(tzinfo=timezone.utc).timestamp()
        counts = np.bincount(data._cols[late], minlength=data.item_count)
        series = pd.Series(counts, index=pd.Index(data.items.ids(), name="item_id"))
        with np.errstate(invalid="ignore", divide="ignore"):
            scores = self._train_internal(series)
        self.items = data.items
        self.item_scores = np.require(scores.values, np.float32)


class RandomConfig(BaseModel, arbitrary_types_allowed=True):
    "src/lenskit/basic/random.py:15-24"

    n: int | None = None  # how many items to select; -1 or None: all of them, permuted
    rng: Any = None  # DerivableSeed: a seed, "user", or (seed, "user")


class RandomSelector(RowStreams, Component):
    """
    Pick items uniformly at random without replacement (``RandomSelector``,
    src/lenskit/basic/random.py:27-78).  The reference draws ``rng.choice`` from a NumPy
    generator; a device cannot reproduce that stream, so the draws are this package's (DESIGN.md
    section 4.18): a uniform ordered sample without replacement is the Plackett-Luce ranking over
    equal weights, i.e. the stochastic ranker's keys over a constant score with no transform.
    ``seed``, ``by_user``, ``streams()`` and the call counter are ``StochasticTopNRanker``'s; an
    item's draw is addressed by its item number, so one list and the same list inside a batch
    agree.  The result keeps the input's fields and carries no score of its own.
    """

    config: RandomConfig

    def __init__(self, config=None, **kwargs):
        if isinstance(config, dict) and isinstance(config.get("rng"), list):
            config = {**config, "rng": tuple(config["rng"])}  # (a TOML / JSON [seed, "user"])
        super().__init__(config, **kwargs)
        self._init_streams(self.config.rng)

    def _length(self, n: int | None) -> int:
        if n is None:
            n = self.config.n or -1  # (random.py:63-64)
        return int(n)

    def rank_panel(self, panel, streams, n: int | None, *, excl=None, samples: int = 1,
                   first_sample: int = 0, device_output: bool = False):
        "``stochastic.rank_panel`` with no transform over a panel of one constant"
        from .stochastic import rank_panel

        return rank_panel(panel, streams, self._length(n), transform=None, scale=1.0,
                          seed=self.seed, excl=excl, samples=samples, first_sample=first_sample,
                          device_output=device_output)

    def rank_ragged(self, ptr, addr, payload, widths, streams, n: int | None, *,
                    samples: int = 1, first_sample: int = 0, device_output: bool = False):
        """
        ``stochastic.rank_ragged`` with no transform over a constant score of 1.0: the selection
        ``__call__`` makes from each list of a ragged batch, as the ``payload`` numbers of the
        picked entries ([B x S x n] int32, -1 padding).  The keys are not returned.
        """
        import torch

        from . import _device as D
        from .stochastic import rank_ragged

        total = int(np.asarray(ptr).reshape(-1)[-1])
        ones = torch.ones(total, dtype=torch.float32, device=D.device())
        idx, _keys = rank_ragged(ptr, addr, payload, ones, widths, streams, self._length(n),
                                 transform=None, scale=1.0, seed=self.seed, samples=samples,
                                 first_sample=first_sample, device_output=device_output)
        return idx

    def __call__(self, items: ItemList, query=None, n: int | None = None) -> ItemList:
        import torch

        from . import _device as D

        n = self._length(n)
        query = RecQuery.create(query)
        stream = self.streams(None if query.user_id is None else [query.user_id], 1)
        n = len(items) if n < 0 else min(n, len(items))  # (random.py:69-72)
        if n == 0:
            return items[np.zeros(0, dtype=np.int32)]
        # a one-row panel over the item numbers: the kernels, and the draws, of a batch row
        if items.vocabulary is not None:
            nums, width = items.numbers(), len(items.vocabulary)
        else:
            nums, width = np.arange(len(items)), len(items)
        row = np.full((1, width), np.nan, dtype=np.float32)
        row[0, nums] = 1.0
        position = np.full(width, -1, dtype=np.int64)
        position[nums] = np.arange(len(items))
        idx, _keys = self.rank_panel(torch.from_numpy(row).to(D.device()), stream, n)
        picked = idx[0, 0]
        return items[position[picked[picked >= 0]]]
