"""
Component seam for neighbourhood models -- item-based k-NN and user-based
k-NN (mirror of ``lenskit.knn.UserKNNScorer``, src/lenskit/knn/user.py:25-316), EASE (mirror of
``lenskit.knn.EASEScorer``, src/lenskit/knn/ease.py), SLIM / fsSLIM (mirror of
``lenskit.knn.SLIMScorer``, src/lenskit/knn/slim.py) and association rules (end of the file, mirror
of ``lenskit.knn.AssociationScorer``, src/lenskit/knn/association.py).

Item-based k-NN: mirror of ``lenskit.knn.ItemKNNScorer`` /
``ItemKNNConfig`` (src/lenskit/knn/item.py:41-295).  Matrix preparation is the reference's
own SciPy code path (item-mean centring, L2 normalisation); the similarity build and the
scoring run in the HIP kernels.

User-based k-NN scores candidate lists through ``lk_csr_rows_dot`` + ``lk_uknn_score_batch``
(``score_batch``) and EVERY item for panels of queries through csrc/uknn_recommend.hip
(``recommend_batch`` / ``dense_scores_batch``, the loops of :class:`_PanelScorer`): the query
vectors built on the device, the neighbour similarities user-major, and each (query, item) cell a
gather from the transposed ratings into the reference's accumulator.
``batch.predict`` scores its ragged (query, target) cells by the same gather
(``predict_history_batch``, csrc/uknn_predict.hip).
``batch.recommend`` takes that path, as it takes item-kNN's, SLIM's, the association rules' and
EASE's (``lk_ease_score_panel``; EASE's training can invert its Gramian with this package's blocked
Cholesky, ``lk_spd_inverse_blocked``: DESIGN.md section 4.25).
"""

from __future__ import annotations

import warnings
from functools import partial
from typing import Literal

import numpy as np
import scipy.sparse as sps
import torch
from pydantic import (AliasChoices, BaseModel, Field, NonNegativeFloat, PositiveFloat, PositiveInt,
                      field_validator)

from . import _device as D
from ._queries import item_scores, pack_histories, pack_targets, resolve_queries
from .basic import HistoryBatch
from .data import Dataset, ItemList, RecQuery, SparseRowArray, Vocabulary
from .pipeline import Component
from .training import TrainingOptions


class DataWarning(UserWarning):
    "``lenskit.diagnostics.DataWarning``"


class ItemKNNConfig(BaseModel, extra="forbid"):
    "src/lenskit/knn/item.py:41-84"

    max_nbrs: PositiveInt = Field(20, validation_alias=AliasChoices("max_nbrs", "nnbrs", "k"))
    min_nbrs: PositiveInt = 1
    min_sim: PositiveFloat = 1.0e-6
    save_nbrs: PositiveInt | None = None
    feedback: Literal["explicit", "implicit"] = "explicit"
    block_size: int = 250

    @field_validator("min_sim", mode="after")
    @staticmethod
    def clamp_min_sim(sim) -> float:
        return max(sim, float(np.finfo(np.float64).smallest_normal))

    @property
    def explicit(self) -> bool:
        return self.feedback == "explicit"


class ItemKNNScorer(Component):
    config: ItemKNNConfig

    items: Vocabulary
    item_means: np.ndarray | None
    item_counts: np.ndarray
    sim_matrix: SparseRowArray

    def is_trained(self):
        return hasattr(self, "sim_matrix")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        field = "rating" if self.config.explicit else None
        rmat = data.interactions().matrix().scipy(field, layout="coo").astype(np.float32)
        n_rows, n_items = rmat.shape
        dev = D.device()
        # centring + normalisation (item.py:142-156,202-228) on the device, bit-identical to
        # the SciPy calls of the reference (see _device.iknn_prepare)
        dui, diu, means, all_zero = D.iknn_prepare(rmat, self.config.explicit, dev)
        if all_zero:
            warnings.warn("Ratings seem to have the same value, centering is not recommended.",
                          DataWarning)
        out = D.iknn_build(dui, diu, self.config.min_sim, self.config.save_nbrs)
        self.items = data.items
        self.item_means = None if means is None else np.asarray(means)
        offsets = out.indptr.cpu().numpy()
        self.item_counts = np.diff(offsets)
        # Arrow extension array, int64 offsets (item.py:176-177: LargeList -> from_array); an
        # unbounded ML-25M model is 9.2 GB: D.to_host moves it at PCIe speed (lk_download)
        self.sim_matrix = SparseRowArray.from_arrays(
            offsets, D.to_host(out.indices, index_bound=out.shape[1]), D.to_host(out.values),
            shape=(n_items, n_items))
        import pyarrow as pa

        assert pa.types.is_large_list(self.sim_matrix.type.storage_type)
        # the build's output IS the device copy of the new matrix: not uploaded again
        self._device_cache("sims", lambda: {"sims": out, "device": dev}, self.sim_matrix)

    def _device_sims(self):
        "The similarity matrix in HBM (int64 offsets), uploaded once per model."
        def upload():
            d = D.device()
            from .matrix import csr_arrays

            return {"device": d, "sims": D.DeviceCSR.from_host(*csr_arrays(self.sim_matrix), d)}

        return self._device_cache("sims", upload, self.sim_matrix)

    def _device_means(self):
        "The explicit model's item means in HBM (f32), uploaded once per model; None if implicit."
        if not self.config.explicit or self.item_means is None:
            return None
        return self._device_cache(
            "means", lambda: torch.from_numpy(np.asarray(self.item_means, dtype=np.float32)).to(
                self._device_sims()["device"]), self.item_means)

    def _row_hits(self, csr: D.DeviceCSR) -> np.ndarray:
        """
        Per row of a device CSR of item numbers (-1 = unknown): the similarity-row lengths of its
        items, summed -- a query's hit count, which ``lk_iknn_recommend`` sizes its lists and
        balances its launch by.  Host int64.
        """
        d = csr.indices.device
        cnt = torch.from_numpy(np.asarray(self.item_counts, dtype=np.int64)).to(d)
        idx = csr.indices.long()
        csum = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=d)
        torch.cumsum(torch.where(idx >= 0, cnt[idx.clamp(min=0)], 0), 0, out=csum[1:])
        ptr = csr.indptr.long()
        return (csum[ptr[1:]] - csum[ptr[:-1]]).cpu().numpy()

    def _user_hits(self, lookup) -> np.ndarray:
        """
        The hit count of every training user of ``lookup``, computed on the device once per
        training of either component.  The entry is tied to the host matrix the lookup's device
        matrix is built from, so it does not keep that device matrix alive after a retrain.
        """
        return self._device_cache("user_hits",
                                  lambda: self._row_hits(lookup._device_matrix()["csr"]),
                                  lookup.interactions, self.sim_matrix)

    # -- the two front-ends: histories as a device CSR in query order -------------------------
    def _centred_ratings(self, hist: ItemList, nums: np.ndarray, kept: np.ndarray) -> np.ndarray:
        "One history's float32 ratings minus the float32 item means; unknown items not centred."
        rv = hist.field("rating")
        if rv is None:
            raise RuntimeError("explicit-feedback scorer must have ratings")
        rv = np.asarray(rv).astype(np.float32, copy=True)
        m = nums >= 0
        rv[m] -= self.item_means[nums[m]]  # mean-centre (item.py:268-271)
        return rv

    def _query_csr(self, queries: list[RecQuery]) -> D.DeviceCSR:
        "The histories of a list of queries, uploaded: -1 = unknown item; explicit: with values."
        values = self._centred_ratings if self.config.explicit else None
        ptr, idx, val = pack_histories(queries, self.items, unknown="keep", values=values)
        return D.DeviceCSR.from_arrays(ptr, idx, val, (len(queries), len(self.items)),
                                       self._device_sims()["device"])

    def _batch_csr(self, batch) -> D.DeviceCSR:
        """
        The histories of a :class:`lkpy_amd.basic.HistoryBatch`, in the training rows' order
        (what the reference's lookup hands the scorer, basic/history.py:77-95): cut out of the
        HBM-resident training matrix with the ratings mean-centred on the way
        (``lk_csr_gather_rows`` with the item means as column bias: item.py:268-271).
        """
        if self.config.explicit and not batch.has_ratings:
            raise RuntimeError("explicit-feedback scorer must have ratings")
        return batch.csr(use_ratings=self.config.explicit, scale=1.0,
                         col_bias=self._device_means(), with_values=self.config.explicit)

    # -- scoring ------------------------------------------------------------------------------
    def _score(self, hist: D.DeviceCSR, tgt_ptr, tgt_nums):
        "One ``lk_iknn_score_batch`` call: device (scores f32, counts int32), item means not added."
        return D.iknn_score_batch(self._device_sims()["sims"], hist.indptr, hist.indices,
                                  hist.values if self.config.explicit else None, tgt_ptr,
                                  tgt_nums, self.config.max_nbrs, self.config.min_nbrs)

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "Score many (query, items) pairs in one kernel launch (item.py:231-295 per pair)."
        hist = self._query_csr([RecQuery.create(q) for q in queries])
        d = hist.indices.device
        t_ptr, tgt = pack_targets(item_lists, self.items)
        s, c = self._score(hist, torch.from_numpy(t_ptr).to(d), torch.from_numpy(tgt).to(d))
        s, c = s.cpu().numpy(), c.cpu().numpy()
        out = []
        for qi, items in enumerate(item_lists):
            if hist.h_indptr[qi] == hist.h_indptr[qi + 1]:
                out.append(ItemList(items, scores=np.nan))  # no history: item.py:238-245
                continue
            sc = s[t_ptr[qi]:t_ptr[qi + 1]].copy()
            ti = tgt[t_ptr[qi]:t_ptr[qi + 1]]
            if self.config.explicit:
                m = ti >= 0
                sc[m] += self.item_means[ti[m]]  # item.py:282
            out.append(ItemList(items, scores=sc, nbr_counts=c[t_ptr[qi]:t_ptr[qi + 1]]))
        return out

    def __call__(self, query, items: ItemList) -> ItemList:
        return self.score_batch([query], [items])[0]

    def score_history_batch(self, batch, tgt_ptr, tgt_nums):
        """
        ``score_batch`` for training histories by user number (``UserTrainingHistoryLookup.batch``):
        the histories are cut out of the HBM-resident training matrix (:meth:`_batch_csr`), the
        targets -- int64 offsets ``tgt_ptr`` [B + 1] and this scorer's item numbers ``tgt_nums``
        (-1 = unknown), host arrays or device tensors -- are uploaded once, and one
        ``lk_iknn_score_batch`` call scores everything.  Returns device (scores f32, counts
        int32) over the targets: the kernel's output, item means NOT yet added back
        (``lk_predict_merge`` does that).
        """
        d = self._device_sims()["device"]
        if not isinstance(tgt_ptr, torch.Tensor):
            tgt_ptr = torch.from_numpy(np.ascontiguousarray(tgt_ptr, dtype=np.int64)).to(d)
        if not isinstance(tgt_nums, torch.Tensor):
            tgt_nums = torch.from_numpy(np.ascontiguousarray(tgt_nums, dtype=np.int32)).to(d)
        return self._score(self._batch_csr(batch), tgt_ptr, tgt_nums)

    def score_candidates_batch(self, queries, tgt_ptr, item_nums, *, d_targets=None,
                               with_counts: bool = False):
        """
        The scores of each query's OWN items, left on the device: f32 [total], entry t the score
        ``__call__`` gives item ``item_nums[t]`` for the query q with ``tgt_ptr[q] <= t <
        tgt_ptr[q + 1]`` -- the same bits: one ``lk_iknn_score_batch`` call and the item means
        added back by ``lk_predict_merge`` (item.py:282).  ``queries``: a list of queries or a
        :class:`lkpy_amd.basic.HistoryBatch`; ``tgt_ptr`` int64 [B + 1] and ``item_nums`` int32
        (-1: unknown item) are host arrays, ``d_targets`` their device copies ``(offsets,
        numbers)`` where the caller has uploaded them already.  NaN for an unknown item, for an
        item with fewer than ``min_nbrs`` neighbours and for a query without history.
        ``with_counts``: (scores, neighbour counts int32) -- ``__call__``'s ``nbr_counts``.
        """
        queries = resolve_queries(queries, self.items)
        d = self._device_sims()["device"]
        d_ptr, d_nums = d_targets or D.upload_targets(tgt_ptr, item_nums, d)
        if isinstance(queries, HistoryBatch):
            hist = self._batch_csr(queries)
        else:
            hist = self._query_csr(queries)
        scores, counts = self._score(hist, d_ptr, d_nums)
        means = self._device_means()
        if means is not None and d_nums.numel():
            D.predict_merge(d_ptr, d_nums, len(self.items), scores, means)
        return (scores, counts) if with_counts else scores

    # -- top-n --------------------------------------------------------------------------------
    accepts_history_batch = True  # recommend_batch takes a lkpy_amd.basic.HistoryBatch

    def recommend_batch(self, queries, n: int, *, exclude_history: bool = True):
        """
        Top-``n`` lists for many queries at once -- what the ``recommender`` pipeline computes one
        query at a time (src/lenskit/batch/_runner.py:283-308): candidates = every training item
        minus the query's own (src/lenskit/basic/candidates.py:77-94), this scorer over them
        (item.py:231-295, means added back: 282), ``TopNRanker`` (basic/topn.py:45-69).  One
        ``lk_iknn_recommend`` call: scores bit-identical to the reference accumulator's, items
        with fewer than ``min_nbrs`` neighbours never listed, queries without history get empty
        lists (item.py:238-245: all-NaN scores).  ``queries``: a list of queries, or a
        :class:`lkpy_amd.basic.HistoryBatch` (training histories by user number: nothing is done
        per query on the host, and a query's hit count is a property of the USER, computed once
        for every training user on the device).  Returns (item numbers [B x n] with -1 padding,
        scores [B x n] with NaN padding), like ``ImplicitMFScorer.recommend_batch``.
        """
        queries = resolve_queries(queries, self.items)
        if isinstance(queries, HistoryBatch):
            batch = queries
            nums = batch.user_nums
            hits = np.where(nums >= 0, self._user_hits(batch.lookup)[np.maximum(nums, 0)], 0)
            return self._recommend(lambda order: self._batch_csr(batch.subset(order)),
                                   hits.astype(np.int64), n, exclude_history)
        hist = self._query_csr(queries)
        return self._recommend(
            lambda order: D.gather_rows(hist, order, with_values=self.config.explicit),
            self._row_hits(hist), n, exclude_history)

    def _recommend(self, cut, hits: np.ndarray, n: int, exclude_history: bool):
        """
        The tail of both ``recommend_batch`` front-ends: ``cut(order)`` gives the histories as a
        device CSR with the heaviest query first (the launch is as long as its longest task
        chain), one ``lk_iknn_recommend`` call scores them, and the lists are put back in the
        caller's order on the device and downloaded at once.
        """
        order = np.argsort(-hits, kind="stable")
        hist = cut(order)
        oi, osc = D.iknn_recommend(self._device_sims()["sims"], hist.indptr, hist.indices,
                                   hist.values if self.config.explicit else None,
                                   self._device_means(), self.config.max_nbrs,
                                   self.config.min_nbrs, n, hits[order], exclude_history)
        inv = np.empty_like(order)
        inv[order] = np.arange(len(order))  # (the inverse permutation: O(n), no second sort)
        return D.lists_to_host(oi, osc, torch.from_numpy(inv).to(oi.device))


# ---------------------------------------------------------------------------------------
# Panel scorers: a sparse model in HBM, every item scored for a panel of queries at a time
# ---------------------------------------------------------------------------------------


class _PanelScorer:
    """
    What ``SLIMScorer``, ``AssociationScorer``, ``UserKNNScorer`` and ``EASEScorer`` share, beside
    :class:`Component`: the model is a matrix in HBM (a sparse item-item one; user-kNN: the
    transposed ratings; EASE: the dense weights), a kernel call scores every item for a range of
    queries (a [rows x items] float32 panel), and a batch goes through in panels of at most
    ``PANEL_BYTES``.  A subclass supplies ``items``, :meth:`_device_matrix` and
    :meth:`_score_panel` (and :meth:`_panel_device` if its matrix is no ``DeviceCSR``).
    """

    PANEL_BYTES = 1 << 30  # score panel of one recommend / score step
    accepts_history_batch = True  # recommend_batch takes a lkpy_amd.basic.HistoryBatch

    def _device_matrix(self) -> D.DeviceCSR:
        "The model matrix in HBM (int64 offsets), uploaded once per model."
        raise NotImplementedError

    def _score_panel(self, hist: D.DeviceCSR, rows, *, strike_history: bool, nan_empty: bool):
        "One kernel call: the device panel of the queries ``rows = (lo, hi)`` of ``hist``."
        raise NotImplementedError

    def _panel_device(self):
        "The device the model lives on (a subclass whose matrix is no CSR overrides this)."
        return self._device_matrix().indices.device

    def _panel_rows(self) -> int:
        return max(1, self.PANEL_BYTES // (4 * max(len(self.items), 1)))

    def _query_csr(self, queries: list[RecQuery]) -> D.DeviceCSR:
        "The histories of a list of queries in query order, uploaded: item numbers, -1 = unknown."
        ptr, idx, _ = pack_histories(queries, self.items, unknown="keep")
        return D.DeviceCSR.from_arrays(ptr, idx, None, (len(queries), len(self.items)),
                                       self._panel_device())

    def _batch_csr(self, queries) -> D.DeviceCSR:
        "The histories of a batch as a device CSR: a HistoryBatch's training rows, or a list's."
        queries = resolve_queries(queries, self.items)
        if isinstance(queries, HistoryBatch):
            return queries.csr(with_values=False)
        return self._query_csr(queries)

    def _score_lists(self, hist: D.DeviceCSR, item_lists, *, nan_empty: bool, score_panel=None):
        """
        The loop of ``score_batch``: each panel of ``hist`` scored (by ``score_panel``, called
        like :meth:`_score_panel`, which it defaults to) and downloaded, each list's scores read
        out of its query's row.  ``nan_empty``: the kernel makes the row of a query without a
        known history item NaN; else an empty row of ``hist`` (a query CSR: the host has its
        offsets) is told here.
        """
        score_panel = score_panel or self._score_panel
        out = []
        step = self._panel_rows()
        for lo in range(0, len(item_lists), step):
            hi = min(len(item_lists), lo + step)
            panel = D.to_host(score_panel(hist, (lo, hi), strike_history=False,
                                          nan_empty=nan_empty))
            for i in range(lo, hi):
                items = item_lists[i]
                if not nan_empty and hist.h_indptr[i] == hist.h_indptr[i + 1]:
                    out.append(ItemList(items, scores=np.nan))
                    continue
                out.append(ItemList(items, scores=item_scores(items, self.items, panel[i - lo])))
        return out

    def __call__(self, query, items: ItemList) -> ItemList:
        return self.score_batch([query], [items])[0]

    def _sparse_candidates(self, queries, model: D.DeviceCSR, reduce: str, tgt_ptr, item_nums,
                           d_targets):
        """
        ``score_candidates_batch`` of the scorers whose model is a sparse item-item matrix
        (``model``: columns ascending inside a row): the panel's cells at the targets by
        ``lk_sparse_score_candidates``, no panel formed.  A :class:`HistoryBatch` is read out of
        the HBM-resident training matrix by user number (no row gather); a list of queries is
        packed like ``score_batch`` packs it (:meth:`_query_csr`).
        """
        queries = resolve_queries(queries, self.items)
        d = model.indices.device
        d_ptr, d_nums = d_targets or D.upload_targets(tgt_ptr, item_nums, d)
        if isinstance(queries, HistoryBatch):
            hist, rows = queries.matrix_rows()
        else:
            hist, rows = self._query_csr(queries), None
        return D.sparse_score_candidates(hist, model, reduce, d_ptr, d_nums, tgt_ptr, rows=rows)

    def recommend_batch(self, queries, n: int | None, *, exclude_history: bool = True):
        """
        Top-``n`` lists for many queries at once -- what the ``recommender`` pipeline computes one
        query at a time: candidates = every training item minus the query's own
        (src/lenskit/basic/candidates.py:77-94), this scorer over them, ``TopNRanker``
        (basic/topn.py:45-69).  Items no history item points at score 0.0 and are listed when
        fewer than ``n`` score above it; a query without a known history item gets an empty list.
        ``queries``: a list of queries, or a :class:`lkpy_amd.basic.HistoryBatch` (training
        histories by user number, cut out of the HBM-resident training matrix).  The batch goes
        through in panels of at most ``PANEL_BYTES``, each selected from by ``lk_argtopn``.
        ``n`` negative or None: every candidate, ranked.  Returns (item numbers [B x n] with -1
        padding, scores [B x n] with NaN padding), like ``ItemKNNScorer.recommend_batch``.
        """
        hist = self._batch_csr(queries)
        d = self._panel_device()
        B = hist.shape[0]
        n = -1 if n is None else int(n)
        cols = len(self.items) if n < 0 else n
        oi = torch.full((B, cols), -1, dtype=torch.int32, device=d)
        osc = torch.full((B, cols), float("nan"), dtype=torch.float32, device=d)
        step = self._panel_rows()
        for lo in range(0, B, step):
            hi = min(B, lo + step)
            panel = self._score_panel(hist, (lo, hi), strike_history=exclude_history,
                                      nan_empty=True)
            idx = D.argtopn(panel, n)
            oi[lo:hi, :idx.shape[1]] = idx
            osc[lo:hi, :idx.shape[1]] = D.take_scores(panel, idx)
        return D.lists_to_host(oi, osc)


# ---------------------------------------------------------------------------------------
# User-based k-NN
# ---------------------------------------------------------------------------------------


class UserKNNConfig(BaseModel, extra="forbid"):
    "src/lenskit/knn/user.py:39-71"

    max_nbrs: PositiveInt = Field(20, validation_alias=AliasChoices("max_nbrs", "nnbrs", "k"))
    min_nbrs: PositiveInt = 1
    min_sim: PositiveFloat = 1.0e-6
    feedback: Literal["explicit", "implicit"] = "explicit"

    @field_validator("min_sim", mode="after")
    @staticmethod
    def clamp_min_sim(sim) -> float:
        return max(sim, float(np.finfo(np.float64).smallest_normal))

    @property
    def explicit(self) -> bool:
        return self.feedback == "explicit"


class UserKNNScorer(_PanelScorer, Component):
    """
    User-user nearest-neighbour collaborative filtering (``UserKNNScorer``,
    src/lenskit/knn/user.py:74-316).  "Training" memorises the mean-centred and the
    row-normalised rating matrices with the reference's own SciPy calls; scoring runs on the
    device for whole batches of queries: neighbour similarities = normalised matrix x query
    vector (``lk_csr_rows_dot``), neighbours with sim >= min_sim in ascending user order,
    per-item accumulation of the ``max_nbrs`` most similar raters (``lk_uknn_score_batch``).

    ``recommend_batch`` / ``dense_scores_batch`` score EVERY item for panels of queries
    (:class:`_PanelScorer`; csrc/uknn_recommend.hip): the query vectors are built on the device
    (``lk_uknn_query_panel``), the similarities come user-major (``lk_uknn_sims_panel``), and
    each (query, item) cell gathers the item's raters from the transposed ratings into its own
    accumulator (``lk_uknn_score_panel``) -- the bits ``score_batch`` gives the same query.
    ``predict_history_batch`` scores the ragged targets of ``batch.predict`` the same way, only
    the (query, target) cells that are asked for (``lk_uknn_score_pairs``, csrc/uknn_predict.hip).
    """

    PANEL_BYTES = 1 << 30  # the query, similarity and score panels of one step, together

    config: UserKNNConfig

    users: Vocabulary
    items: Vocabulary
    user_means: np.ndarray | None
    user_vectors: sps.csr_array
    user_ratings: SparseRowArray

    def is_trained(self):
        return hasattr(self, "user_ratings")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        "user.py:122-168: centre by user mean (explicit), normalise rows, keep both matrices"
        import scipy.sparse.linalg as spla

        rmat = data.interactions().matrix().scipy(
            attribute="rating" if self.config.explicit else None).astype(np.float32)
        means = None
        if self.config.explicit:
            counts = np.diff(rmat.indptr)
            sums = rmat.sum(axis=1)
            means = np.zeros(sums.shape, dtype=np.float32)
            np.divide(sums, counts, out=means, where=counts > 0)
            rmat.data = rmat.data - np.repeat(means, counts)
            if np.allclose(rmat.data, 0.0):
                warnings.warn("Ratings seem to have the same value, centering is not "
                              "recommended.", DataWarning)
        norms = spla.norm(rmat, 2, axis=1)
        cmat = rmat / np.maximum(norms, np.finfo("f4").smallest_normal).reshape(-1, 1)
        self.user_vectors = sps.csr_array(cmat.tocsr())
        self.user_ratings = SparseRowArray.from_scipy(rmat, values=self.config.explicit)
        self.users = data.users
        self.user_means = means
        self.items = data.items

    def _device_state(self):
        def upload():
            from .matrix import csr_arrays

            d = D.device()
            uv = self.user_vectors
            uv.sort_indices()
            return {
                "device": d,
                "vectors": D.DeviceCSR.from_arrays(uv.indptr, uv.indices, uv.data, uv.shape, d),
                "ratings": D.DeviceCSR.from_host(*csr_arrays(self.user_ratings), d),
            }

        return self._device_cache("model", upload, self.user_vectors, self.user_ratings)

    def _user_data(self, query: RecQuery):
        "``_get_user_data`` (user.py:264-307): (user number | None, dense item vector, mean)"
        index = self.users.number(query.user_id, missing=None) \
            if query.user_id is not None else None
        hist = query.query_items
        n_items = len(self.items)
        if hist is None:
            if index is None:
                return None
            uv = self.user_vectors
            row = np.zeros(n_items, dtype=np.float32)
            s, e = uv.indptr[index], uv.indptr[index + 1]
            row[uv.indices[s:e]] = uv.data[s:e]
            umean = float(self.user_means[index]) if self.config.explicit else 0.0
            return index, row, umean
        if len(hist) == 0:
            return None
        ratings = np.zeros(n_items, dtype=np.float32)
        nos = hist.numbers(missing="negative", vocabulary=self.items)
        ok = nos >= 0
        if self.config.explicit:
            urv = hist.field("rating")
            if urv is None:
                return None
            urv = np.require(urv, dtype=np.float32)
            umean = float(urv.mean())
            ratings[nos[ok]] = urv[ok] - umean
        else:
            umean = 0.0
            ratings[nos[ok]] = 1.0
        return index, ratings, umean

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "Many (query, items) pairs through two kernel launches (user.py:171-262 per pair)."
        st = self._device_state()
        d = st["device"]
        queries = [RecQuery.create(q) for q in queries]
        data = [self._user_data(q) if len(il) > 0 else None
                for q, il in zip(queries, item_lists)]
        live = [i for i, u in enumerate(data) if u is not None]
        out: list[ItemList | None] = [None] * len(queries)
        for i, il in enumerate(item_lists):
            if data[i] is None:
                out[i] = ItemList(il, scores=np.nan)
        if not live:
            return out  # type: ignore[return-value]
        # neighbour similarities for the whole batch: [B x users]
        X = np.stack([data[i][1] for i in live], axis=1)  # [items x B]
        sims = D.csr_rows_dot(st["vectors"], torch.from_numpy(np.ascontiguousarray(X)).to(d))
        for b, i in enumerate(live):
            if data[i][0] is not None:
                sims[b, data[i][0]] = 0.0  # zero out the self-similarity (user.py:199-201)
        mask = sims >= float(np.float32(self.config.min_sim))  # user.py:206 (f32 comparison)
        counts = mask.sum(dim=1)
        nbr_ptr = torch.zeros(len(live) + 1, dtype=torch.int64, device=d)
        nbr_ptr[1:] = torch.cumsum(counts, 0)
        nbr_rows = mask.nonzero()[:, 1].to(torch.int32)  # per query, ascending user number
        nbr_sims = sims[mask]
        t_ptr, tgt = pack_targets([item_lists[i] for i in live], self.items)
        s, _c = D.uknn_score_batch(st["ratings"], nbr_ptr, nbr_rows.contiguous(),
                                   nbr_sims.contiguous(), torch.from_numpy(t_ptr).to(d),
                                   torch.from_numpy(tgt).to(d), self.config.max_nbrs,
                                   self.config.min_nbrs)
        s = s.cpu().numpy()
        has_nbrs = counts.cpu().numpy() > 0
        for b, i in enumerate(live):
            sc = s[t_ptr[b]:t_ptr[b + 1]].copy()
            if not has_nbrs[b]:
                sc[:] = np.nan  # no candidate neighbours (user.py:217-219)
            out[i] = ItemList(item_lists[i], scores=sc + np.float32(data[i][2]))
        return out  # type: ignore[return-value]

    def __call__(self, query, items: ItemList) -> ItemList:
        return self.score_batch([query], [items])[0]

    # -- every item for panels of queries (csrc/uknn_recommend.hip) ---------------------------
    def _panel_rows(self) -> int:
        "Queries per panel: X [items x P], sims [users x P] and scores [P x items] live at once."
        per = 4 * (2 * len(self.items) + len(self.users))
        return max(64, self.PANEL_BYTES // max(per, 1) // 64 * 64)

    def _device_transposed(self):
        """
        The centred ratings transposed in HBM (items x users, users ascending: ``lk_csr_transpose``
        is stable), once per model, with the items ordered by falling rater count (the order in
        which ``lk_uknn_score_panel`` starts its columns) and the longest column.
        """
        def build():
            from .matrix import csr_arrays

            rt = D.csr_transpose(self._device_state()["ratings"], with_values=self.config.explicit)
            rt.perm = None  # (the permutation is as large as the values: not kept)
            counts = np.bincount(csr_arrays(self.user_ratings)[1], minlength=len(self.items))
            order = np.argsort(-counts, kind="stable").astype(np.int32)
            return {"ratings_t": rt, "order": torch.from_numpy(order).to(rt.indices.device),
                    "max_col": int(counts.max()) if len(counts) else 0}

        return self._device_cache("ratings_t", build, self.user_ratings)

    def _device_matrix(self) -> D.DeviceCSR:
        return self._device_transposed()["ratings_t"]

    def _history_centres(self, lookup) -> np.ndarray:
        """
        What the reference centres a PROVIDED history by (user.py:281-304): ``urv.mean()`` of the
        history's float32 ratings -- NumPy's pairwise float32 sum, not the training mean -- for
        every training row of ``lookup``, by the same NumPy call.  Host float32 per user, computed
        once per (lookup matrix, scorer); a user without ratings gets 0.
        """
        def build():
            ds = lookup.interactions._ds
            rat, hp = ds._attrs["rating"], ds._indptr
            out = np.zeros(len(hp) - 1, dtype=np.float32)
            for u in range(len(out)):
                if hp[u + 1] > hp[u]:
                    out[u] = np.require(rat[hp[u]:hp[u + 1]], dtype=np.float32).mean()
            return out

        return self._device_cache("centres", build, lookup.interactions, self.user_ratings)

    def _device_centres(self, lookup) -> torch.Tensor:
        "``_history_centres`` in HBM, one upload per (lookup matrix, scorer)."
        return self._device_cache(
            "centres_dev", lambda: torch.from_numpy(self._history_centres(lookup)).to(
                self._device_state()["device"]), lookup.interactions, self.user_ratings)

    def _batch_csr(self, queries) -> D.DeviceCSR:
        """
        The queries of a batch as :meth:`_score_panel` takes them: the device CSR of their
        histories (item numbers, -1 = unknown: what is struck) carrying ``self_user`` (device
        int32, this scorer's number of the query's user or -1), ``centre`` (device f32, the mean
        the history is centred by = the offset of the scores; None if implicit), ``valid`` (host
        bool: the query has data to score from) and ``x_rows``.  A :class:`HistoryBatch` is cut
        out of the HBM-resident training matrix with its ratings (``x_rows`` None: the query
        vectors are built on the device); a list of queries goes through :meth:`_user_data` per
        query, stored-vector branch included, and ``x_rows`` holds the dense host rows.
        """
        from ._queries import user_numbers

        queries = resolve_queries(queries, self.items)
        d = self._device_state()["device"]
        explicit = self.config.explicit
        if isinstance(queries, HistoryBatch):
            if explicit and not queries.has_ratings:
                raise RuntimeError("explicit-feedback scorer must have ratings")
            hist = queries.csr(use_ratings=explicit, with_values=explicit)
            hist = D.DeviceCSR(hist.indptr, hist.indices, hist.values, hist.shape, hist.h_indptr)
            hist.x_rows = None
            hist.valid = queries.lengths > 0
            hist.centre = None
            if explicit:
                nums = torch.from_numpy(np.maximum(queries.user_nums, 0).astype(np.int64)).to(d)
                hist.centre = self._device_centres(queries.lookup)[nums].contiguous()
            selves = user_numbers(queries, self.users)
        else:
            data = [self._user_data(q) for q in queries]
            ptr, idx, _ = pack_histories(queries, self.items, unknown="keep")
            hist = D.DeviceCSR.from_arrays(ptr, idx, None, (len(queries), len(self.items)), d)
            hist.x_rows = [None if u is None else u[1] for u in data]
            hist.valid = np.array([u is not None for u in data], dtype=bool)
            hist.centre = None
            if explicit:
                hist.centre = torch.from_numpy(np.array(
                    [0.0 if u is None else u[2] for u in data], dtype=np.float32)).to(d)
            selves = [-1 if u is None or u[0] is None else u[0] for u in data]
        hist.self_user = torch.from_numpy(np.asarray(selves, dtype=np.int32)).to(d)
        return hist

    def _score_panel(self, hist, rows, *, strike_history: bool, nan_empty: bool = False):
        """
        The device panel of the queries ``rows = (lo, hi)`` of ``hist`` (:meth:`_batch_csr`): query
        panel -> similarities -> scores.  ``nan_empty`` is not passed on: a known user without a
        history is scored from the stored vector, and the row of a query without neighbours --
        an unknown user, an empty history -- is NaN cell by cell (fewer than ``min_nbrs``).
        """
        st, tr = self._device_state(), self._device_transposed()
        lo, hi = (0, hist.shape[0]) if rows is None else (int(rows[0]), int(rows[1]))
        if hist.x_rows is None:
            x = D.uknn_query_panel(hist, hist.centre, rows=(lo, hi))
        else:
            X = np.zeros((len(self.items), hi - lo), dtype=np.float32)
            for j, row in enumerate(hist.x_rows[lo:hi]):
                if row is not None:
                    X[:, j] = row
            x = torch.from_numpy(X).to(st["device"])
        sims = D.uknn_sims_panel(st["vectors"], x, hist.self_user[lo:hi])
        del x
        return D.uknn_score_panel(
            tr["ratings_t"], sims, hi - lo, float(np.float32(self.config.min_sim)),
            self.config.max_nbrs, self.config.min_nbrs,
            None if hist.centre is None else hist.centre[lo:hi], hist=hist, rows=(lo, hi),
            strike_history=strike_history, item_order=tr["order"], max_col=tr["max_col"])

    def recommend_batch(self, queries, n: int | None, *, exclude_history: bool = True):
        """
        Top-``n`` lists for many queries at once -- what the ``recommender`` pipeline computes one
        query at a time: candidates = every training item minus the query's own
        (src/lenskit/basic/candidates.py:77-94), this scorer over them (user.py:171-262, the
        query's mean added back), ``TopNRanker`` (basic/topn.py:45-69).  Items with fewer than
        ``min_nbrs`` passing raters are never listed; an unknown user without history, an empty
        history and a query without neighbours get an empty list.  ``queries``: a list of queries,
        or a :class:`lkpy_amd.basic.HistoryBatch` (training histories by user number, nothing done
        per query on the host).  The batch goes through in panels (:meth:`_panel_rows`), each
        selected from by ``lk_argtopn``.  ``n`` negative or None: every scorable candidate,
        ranked.  Returns (item numbers [B x n] with -1 padding, scores [B x n] with NaN padding).
        """
        return super().recommend_batch(queries, n, exclude_history=exclude_history)

    def predict_history_batch(self, hb, d_tgt_ptr, d_tgt_items, *, h_tgt_ptr=None):
        """
        Scores for the ragged targets of a :class:`lkpy_amd.basic.HistoryBatch` -- what
        ``batch.predict`` asks for -- left on the device: float32, one per entry of
        ``d_tgt_items`` (device int32 item numbers, -1 = unknown; ``d_tgt_ptr`` device int64
        offsets per query), the history's centre added back for explicit feedback, NaN where
        :meth:`__call__` answers NaN (unknown item, fewer than ``min_nbrs`` passing raters, a
        query without history).  Nothing is done per query on the host: the query vectors are
        built on the device (``lk_uknn_query_panel``), the similarities as a user-major panel
        (``lk_uknn_sims_panel``) and ``lk_uknn_score_pairs`` gathers each (query, target) cell from
        the transposed ratings -- the cell ``lk_uknn_score_panel`` would write, only those asked
        for.  The batch goes through in steps of :meth:`_panel_rows` queries.  ``h_tgt_ptr``: the
        host copy of the offsets, if the caller has one (it sizes each step's launch).
        """
        st, tr = self._device_state(), self._device_transposed()
        hist = self._batch_csr(hb)
        B = hist.shape[0]
        out = torch.empty(int(d_tgt_items.shape[0]), dtype=torch.float32, device=st["device"])
        thr = float(np.float32(self.config.min_sim))
        step = self._panel_rows()
        for lo in range(0, B, step):
            hi = min(B, lo + step)
            x = D.uknn_query_panel(hist, hist.centre, rows=(lo, hi))
            sims = D.uknn_sims_panel(st["vectors"], x, hist.self_user[lo:hi])
            del x
            D.uknn_score_pairs(
                tr["ratings_t"], sims, d_tgt_ptr[lo:hi + 1], d_tgt_items, thr,
                self.config.max_nbrs, self.config.min_nbrs,
                None if hist.centre is None else hist.centre[lo:hi],
                self_user=hist.self_user[lo:hi], user_major=True, max_col=tr["max_col"], out=out,
                entries=None if h_tgt_ptr is None else (int(h_tgt_ptr[lo]), int(h_tgt_ptr[hi])))
        return out

    def dense_scores_batch(self, queries):
        """
        Every item's score for many queries at once, left on the device: (panel f32 [B x items],
        valid, history CSR), the contract of ``AssociationScorer.dense_scores_batch``.  The row of
        a query that cannot be scored is NaN (``valid`` False: no data to score from); the history
        CSR (known items, ascending) is for the caller to exclude.  The caller bounds the batch.
        """
        queries = resolve_queries(queries, self.items)
        hist = self._batch_csr(queries)
        if isinstance(queries, HistoryBatch):
            excl = queries.csr(with_values=False)  # training rows: known items, ascending
        else:
            ptr, idx, _ = pack_histories(queries, self.items, unknown="drop", sort=True)
            excl = D.DeviceCSR.from_arrays(ptr, idx, None, hist.shape, hist.indices.device)
        return self._score_panel(hist, None, strike_history=False), hist.valid, excl


def _binary_cooccurrence(data: Dataset):
    """
    The item-item co-occurrence counts of the training matrix, (user, item) pairs counted once:
    the similarity-build kernel on unit values.  Returns (device CSR of the counts, the host
    user-item and item-user matrices it was built from, the device).
    """
    ui = data.interactions().matrix().scipy(attribute=None).astype(np.float32)
    ui = sps.csr_array(ui)
    ui.sum_duplicates()
    ui.data[:] = 1.0  # co-occurrences count (user, item) pairs once
    ui.sort_indices()
    iu = sps.csr_array(ui.T)
    iu.sort_indices()
    d = D.device()
    cooc = D.iknn_build(D.DeviceCSR.from_scipy(ui, d), D.DeviceCSR.from_scipy(iu, d), 0.5)
    return cooc, ui, iu, d


class EASEConfig(BaseModel, extra="forbid"):
    "``EASEConfig`` (src/lenskit/knn/ease.py:36-44)."

    regularization: PositiveFloat = 1
    "Regularization term for EASE."


class EASEScorer(_PanelScorer, Component):
    """
    Embarrassingly shallow autoencoder (``EASEScorer``, src/lenskit/knn/ease.py:47-170;
    SURVEY.md section 8f rank 4).  Training: the dense item-item co-occurrence Gramian
    ``X^T X + reg I`` is built on the device (the similarity-build kernel on unit values +
    ``lk_ease_gram``), inverted there, and turned into the weight matrix ``B = inv / -diag(inv)``
    with a zero diagonal.  The inverse is, by ``LK_EASE_SOLVER``: unset or ``torch``, the very
    PyTorch calls of the reference's ``_chol_invert_torch`` (``torch.linalg.cholesky_ex`` +
    ``torch.cholesky_inverse``, ease.py:190-208 -- a library factorisation, as in the reference);
    ``native``, this package's blocked Cholesky inverse (``lk_spd_inverse_blocked``,
    csrc/spd_blocked.hip: f32 MFMA GEMMs, float64 diagonal blocks).
    Scoring = sum of the history items' weight rows, whole batches of queries at a time:
    ``score_batch`` through ``lk_ease_score_batch``; ``recommend_batch`` / ``dense_scores_batch``
    from bounded device panels (:class:`_PanelScorer`, ``lk_ease_score_panel``: the same bits).
    A repeated history item counts once (``q_vec[q_good] = 1.0``): a list of queries is packed
    that way; the rows of a :class:`lkpy_amd.basic.HistoryBatch` are training rows, whose items
    are distinct.
    """

    config: EASEConfig

    items: Vocabulary
    weights: np.ndarray

    def is_trained(self):
        return hasattr(self, "weights")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        solver = options.env_var("LK_EASE_SOLVER", None)
        if solver and solver not in ("torch", "scipy", "native"):
            raise ValueError(f"unsupported option: LK_EASE_SOLVER={solver}")  # ease.py:96-97
        if solver == "scipy":
            raise ValueError("LK_EASE_SOLVER=scipy: the device backend has no host solver")
        n_items = data.item_count
        cooc, _ui, iu, d = _binary_cooccurrence(data)
        counts = torch.from_numpy(np.diff(iu.indptr).astype(np.int32)).to(d)
        gram = D.ease_gram(cooc, counts, float(self.config.regularization))
        del cooc
        with torch.inference_mode():
            if solver == "native":
                inv, flag = D.spd_inverse_blocked(gram)
                if flag.item():  # the one read of the flag: everything above was only queued
                    raise RuntimeError(f"matrix block {flag.item()} is not positive-definite.")
            else:
                decomp, info = torch.linalg.cholesky_ex(gram)
                if info.item():
                    # ease.py:202-203
                    raise RuntimeError(f"matrix minor {info.item()} is not positive-definite.")
                inv = torch.cholesky_inverse(decomp, out=gram)
                del decomp
            # divide cells by the column's diagonal entry, zero the diagonal (ease.py:140-142)
            inv /= -torch.diagonal(inv).reshape(1, -1).clone()
            inv.fill_diagonal_(0.0)
            mat = inv.cpu().numpy()
        self.items = data.items
        self.weights = mat
        assert self.weights.shape == (n_items, n_items)
        # the matrix in HBM IS the device copy of the new weights: not uploaded again
        self._device_cache("weights", lambda: inv, self.weights)

    def _device_weights(self):
        return self._device_cache(
            "weights", lambda: torch.from_numpy(
                np.ascontiguousarray(self.weights, dtype=np.float32)).to(D.device()), self.weights)

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "Scores for a batch of (query, items) pairs; one device call for all of them."
        w = self._device_weights()
        ptr, idx, _ = pack_histories([RecQuery.create(q) for q in queries], self.items,
                                     unknown="drop", unique=True)
        scores = D.ease_score_batch(torch.from_numpy(ptr).to(w.device),
                                    torch.from_numpy(idx).to(w.device), w).cpu().numpy()
        # ease.py:150-158: no usable history => all NaN
        return [ItemList(items, scores=item_scores(items, self.items, scores[i])
                         if ptr[i] < ptr[i + 1] else np.nan)
                for i, items in enumerate(item_lists)]

    def __call__(self, query, items: ItemList) -> ItemList:
        return self.score_batch([query], [items])[0]

    # -- every item for panels of queries (lk_ease_score_panel) -------------------------------
    def _device_matrix(self) -> torch.Tensor:
        "The dense weight matrix in HBM (f32 [items x items]), uploaded once per model."
        return self._device_weights()

    def _panel_device(self):
        return self._device_weights().device

    def _query_csr(self, queries: list[RecQuery]) -> D.DeviceCSR:
        "The histories of a list of queries as ``score_batch`` packs them: known, ascending, once."
        ptr, idx, _ = pack_histories(queries, self.items, unknown="drop", unique=True)
        return D.DeviceCSR.from_arrays(ptr, idx, None, (len(queries), len(self.items)),
                                       self._panel_device())

    def _score_panel(self, hist, rows, *, strike_history, nan_empty):
        return D.ease_score_panel(hist.indptr, hist.indices, self._device_weights(), rows=rows,
                                  strike_history=strike_history, nan_empty=nan_empty)

    def dense_scores_batch(self, queries):
        """
        Every item's score for many queries at once, left on the device: (panel f32 [B x items],
        valid, history CSR), the contract of ``AssociationScorer.dense_scores_batch``.  The row of a
        query without a known history item is NaN (``valid`` False; ease.py:150-158); the history
        CSR (known items, ascending) is for the caller to exclude.  The caller bounds the batch.
        """
        queries = resolve_queries(queries, self.items)
        if isinstance(queries, HistoryBatch):
            hist = queries.csr(with_values=False)  # training rows: known items, ascending
            valid = queries.lengths > 0
        else:
            hist = self._query_csr(queries)  # (known items, ascending: the exclusion CSR as well)
            valid = np.diff(hist.h_indptr) > 0
        return self._score_panel(hist, None, strike_history=False, nan_empty=True), valid, hist


# ---------------------------------------------------------------------------------------
# SLIM / fsSLIM
# ---------------------------------------------------------------------------------------


class SLIMConfig(BaseModel, extra="forbid"):
    "``SLIMConfig`` (src/lenskit/knn/slim.py:29-50)."

    l1_reg: PositiveFloat = 1.0
    "L1 regularization strength."
    l2_reg: PositiveFloat = 1.0
    "L2 regularization strength."
    max_iters: PositiveInt = 100
    "Maximum coordinate-descent rounds per column."
    max_nbrs: PositiveInt | None = None
    "Maximum neighbours (features) per item; a positive integer enables fsSLIM (cosine selection)."


class SLIMScorer(_PanelScorer, Component):
    """
    Sparse linear methods (``SLIMScorer``, src/lenskit/knn/slim.py:53-152): one elastic-net
    regression per item, learned by coordinate descent with soft thresholding.  Training runs on
    the device, a wave per column, and learns the reference's sparse matrix bit for bit
    (``lk_slim_train_count`` / ``_fill``, csrc/slim.hip); scoring adds the history items' weight
    rows in history order (``lk_slim_score_batch``), whole batches of queries at a time, and
    ``recommend_batch`` selects the lists from bounded panels (:class:`_PanelScorer`).  The
    learned state stays on the host: ``weights`` (SciPy CSR, feature rows) and ``items``.
    """

    config: SLIMConfig

    weights: sps.csr_array
    "The TRANSPOSED weight matrix: ``weights[i, j]`` is the weight of item i in predicting item j."
    items: Vocabulary

    def is_trained(self) -> bool:
        return hasattr(self, "weights")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        "slim.py:93-119, line for line."
        import pyarrow as pa

        from ._accel import slim as _slim_accel
        from .parallel import run_accel_task

        ui_matrix = data.interactions().matrix().csr_structure(format="arrow")
        iu_matrix = ui_matrix.transpose()
        weights = run_accel_task(
            _slim_accel.train_slim(
                ui_matrix,
                iu_matrix,
                self.config.l1_reg,
                self.config.l2_reg,
                self.config.max_iters,
                self.config.max_nbrs,
            )
        )
        weights = pa.chunked_array(weights).combine_chunks()
        weights = SparseRowArray.from_array(weights)
        self.weights = weights.to_scipy().T.tocsr()
        self.items = data.items

    def _device_weights(self) -> D.DeviceCSR:
        def upload():
            w = self.weights
            return D.DeviceCSR.from_host(w.indptr, w.indices, w.data, w.shape, D.device())

        return self._device_cache("weights", upload, self.weights)

    def _device_matrix(self) -> D.DeviceCSR:
        return self._device_weights()

    def _score_panel(self, hist, rows, *, strike_history, nan_empty):
        return D.slim_score_batch(hist.indptr, hist.indices, self._device_matrix(), rows=rows,
                                  strike_history=strike_history, nan_empty=nan_empty)

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "Scores for a batch of (query, items) pairs (slim.py:121-152 per pair)."
        hist = self._query_csr([RecQuery.create(q) for q in queries])
        # no / empty history: every score NaN, told by the row's length (slim.py:125-130)
        return self._score_lists(hist, item_lists, nan_empty=False)

    def _device_weights_ascending(self) -> D.DeviceCSR:
        "``_device_weights`` with ascending columns inside a row: a sorted COPY where they are not."
        w = self.weights
        if w.has_sorted_indices:
            return self._device_weights()

        def upload():
            s = w.copy()
            s.sort_indices()
            return D.DeviceCSR.from_host(s.indptr, s.indices, s.data, s.shape, D.device())

        return self._device_cache("weights_ascending", upload, self.weights)

    def score_candidates_batch(self, queries, tgt_ptr, item_nums, *, d_targets=None):
        """
        The scores of each query's OWN items, left on the device: f32 [total], entry t the score
        ``__call__`` gives item ``item_nums[t]`` for the query q with ``tgt_ptr[q] <= t <
        tgt_ptr[q + 1]`` -- the same bits, without the [1 x items] panel ``__call__`` forms:
        ``lk_sparse_score_candidates`` adds, per target, the weights of the history items whose
        row holds the target, in history order, which is the panel cell's own chain
        (``lk_slim_score_batch``: ``row[c] += v`` once per history item).  The arguments are those
        of ``ItemKNNScorer.score_candidates_batch``.  NaN for an unknown item and for a query
        without history (an unknown user); 0.0 where no history item reaches the target.

        The equality rests on the history order: a :class:`HistoryBatch` row is the training
        matrix's row ``ds._cols[s:e]``, which is what the per-query lookup attaches
        (``row_items``, data.py) and ``pack_histories`` hands on in that order
        (``unknown="keep"``, no sort) -- the fact ``recommend_batch``'s equality rests on too.
        The weight rows are assumed to name a column once, as the trainer leaves them.
        """
        return self._sparse_candidates(queries, self._device_weights_ascending(), "sum", tgt_ptr,
                                       item_nums, d_targets)


# ---------------------------------------------------------------------------------------
# Association rules: conditional probability, lift, biased lift
# ---------------------------------------------------------------------------------------


class AssociationConfig(BaseModel, extra="forbid"):
    "``AssociationConfig`` (src/lenskit/knn/association.py:32-56)."

    method: Literal["probability", "lift"] = "probability"
    "The formula for the item association level."
    damping: NonNegativeFloat = 0.0
    "Damping factor (kappa) of biased lift."
    max_nbrs: PositiveInt | None = None
    "``None``: the mean over the reference items; 1: the maximum.  Other values are not offered."


class AssociationScorer(_PanelScorer, Component):
    """
    Association rules between items (``AssociationScorer``, src/lenskit/knn/association.py:59-163):
    conditional probability ``P[c|r]``, lift, and -- with ``damping`` -- biased lift, from the
    co-occurrence counts of the training matrix.  Training counts co-occurrences with the
    similarity-build kernel on unit values (as ``EASEScorer`` does), scales them in place
    (``lk_assoc_scale``, NumPy's float64 divisions and float32 multiply bit for bit) and downloads
    the matrix; scoring reduces the reference items' rows by mean or max for whole batches of
    queries (``lk_assoc_score_batch``: a cell's additions in reference-item order, as ``np.mean``
    over the reference's dense rows), and ``recommend_batch`` selects the lists from bounded panels
    (:class:`_PanelScorer`).  The learned state stays on the host: ``items``, ``item_freqs`` and
    ``assoc_scores`` (SciPy CSR, reference items on rows, target items on columns).
    """

    config: AssociationConfig

    items: Vocabulary
    item_freqs: np.ndarray
    assoc_scores: sps.csr_array

    def is_trained(self) -> bool:
        return hasattr(self, "assoc_scores")

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        "association.py:91-130"
        n_items = data.item_count
        cooc, ui, _iu, d = _binary_cooccurrence(data)
        n_groups = ui.shape[0]  # the matrix's rows, not user_count: there might be sessions (99)
        # the marginals count interaction RECORDS (item_stats, association.py:113)
        item_counts = np.ascontiguousarray(data.item_stats()["count"].values, dtype=np.int32)
        D.assoc_scale(cooc, torch.from_numpy(item_counts).to(d), n_groups, self.config.method,
                      float(self.config.damping))
        # handed back like ItemKNNScorer's sim_matrix: D.to_host moves it at PCIe speed
        scores = sps.csr_array(
            (D.to_host(cooc.values), D.to_host(cooc.indices, index_bound=n_items),
             cooc.indptr.cpu().numpy()), shape=(n_items, n_items))
        scores.has_sorted_indices = True  # (the build's rows ascend)
        self.items = data.items
        self.item_freqs = item_counts
        self.assoc_scores = scores
        # the scaled build output IS the device copy of the new matrix: not uploaded again
        self._device_cache("assoc_scores", lambda: cooc, self.assoc_scores)

    def _device_scores(self) -> D.DeviceCSR:
        "The association matrix in HBM (int64 offsets), uploaded once per model."
        def upload():
            s = self.assoc_scores
            s.sort_indices()
            return D.DeviceCSR.from_host(s.indptr, s.indices, s.data, s.shape, D.device())

        return self._device_cache("assoc_scores", upload, self.assoc_scores)

    def _device_matrix(self) -> D.DeviceCSR:
        return self._device_scores()

    def _reduction(self) -> str:
        if self.config.max_nbrs is None:
            return "mean"
        if self.config.max_nbrs == 1:
            return "max"
        raise NotImplementedError("limited reference items not yet implemented")  # 155

    def _score_panel(self, hist, rows, *, strike_history, nan_empty, reduce=None):
        return D.assoc_score_batch(hist.indptr, hist.indices, self._device_matrix(),
                                   reduce or self._reduction(), rows=rows,
                                   strike_history=strike_history, nan_empty=nan_empty)

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "Scores for a batch of (query, items) pairs (association.py:132-163 per pair)."
        hist = self._query_csr([RecQuery.create(q) for q in queries])
        if hist.nnz and bool((hist.indices >= 0).any()):
            reduce = self._reduction()  # (the reference raises once it has reference items)
        else:
            reduce = "mean"
        # a query without a known reference item: every score NaN (association.py:144-146)
        return self._score_lists(hist, item_lists, nan_empty=True,
                                 score_panel=partial(self._score_panel, reduce=reduce))

    def recommend_batch(self, queries, n: int | None, *, exclude_history: bool = True):
        "``_PanelScorer.recommend_batch`` (the pipeline of ``biased-lift.toml``) by mean or max."
        self._reduction()  # (an unsupported max_nbrs is refused before anything is uploaded)
        return super().recommend_batch(queries, n, exclude_history=exclude_history)

    def score_candidates_batch(self, queries, tgt_ptr, item_nums, *, d_targets=None):
        """
        The scores of each query's OWN items, left on the device: f32 [total], entry t the score
        ``__call__`` gives item ``item_nums[t]`` for the query q with ``tgt_ptr[q] <= t <
        tgt_ptr[q + 1]`` -- the same bits, without the [1 x items] panel ``__call__`` forms:
        ``lk_sparse_score_candidates`` folds, per target, the cells of the reference items' rows
        in reference-item order and ends as ``lk_assoc_score_batch`` does
        (``float32(double(sum) / double(m))``, or the maximum over 0).  The arguments are those of
        ``ItemKNNScorer.score_candidates_batch``.  NaN for an unknown item and for a query
        without a known reference item (an unknown user).

        The equality rests on the history order, as ``SLIMScorer.score_candidates_batch`` says:
        a :class:`HistoryBatch` row is the training row the per-query lookup attaches, and
        ``pack_histories`` keeps its order.
        """
        reduce = self._reduction()  # (as in recommend_batch: refused before anything is uploaded)
        return self._sparse_candidates(queries, self._device_matrix(), reduce, tgt_ptr, item_nums,
                                       d_targets)

    def dense_scores_batch(self, queries):
        """
        Every item's score for many queries at once, left on the device: (panel f32 [B x items],
        valid, history CSR), the contract of ``FlexMFScorerBase.dense_scores_batch``.  The row of a
        query without a known reference item is NaN (``valid`` False); the history CSR (known
        items, ascending) is for the caller to exclude.  The caller bounds the batch.
        """
        self._reduction()  # (as in recommend_batch)
        queries = resolve_queries(queries, self.items)
        if isinstance(queries, HistoryBatch):
            hist = excl = queries.csr(with_values=False)  # training rows: known items, ascending
            valid = queries.lengths > 0
        else:
            hist = self._query_csr(queries)
            ptr, idx, _ = pack_histories(queries, self.items, unknown="drop", sort=True)
            excl = D.DeviceCSR.from_arrays(ptr, idx, None, hist.shape, hist.indices.device)
            valid = np.diff(ptr) > 0
        return self._score_panel(hist, None, strike_history=False, nan_empty=True), valid, excl
