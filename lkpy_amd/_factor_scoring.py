"""
Device scoring of factor models with bias terms, shared by the FlexMF scorers
(``lkpy_amd.flexmf``), the SVD scorer (``lkpy_amd.sklearn.svd``) and the FunkSVD scorer
(``lkpy_amd.funksvd``): the biases are extra columns
of the two operand matrices, so that a score is one inner product on ``lk_score_topk``,
``lk_score_dense`` or ``lk_mf_score_pairs``.

A scorer mixing these in has ``config.embedding_size``, ``users``, ``items``, ``user_embeddings``
[users x k], ``item_embeddings`` [items x k], ``user_bias`` [users] | None, ``item_bias`` [items]
| None (with :class:`GlobalBiasPairScoring` also ``global_bias``) and ``Component``'s
``_device_cache``.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _device as D
from ._queries import pack_histories, pack_targets, resolve_queries, user_numbers
from .basic import HistoryBatch, _damping
from .data import ItemList, RecQuery


class BiasedFactorScoring:
    "Batched recommendation and dense scoring from ``[p_u, 1, b_u] . [q_i, b_i, 1]``."

    accepts_history_batch = True  # recommend_batch takes a lkpy_amd.basic.HistoryBatch
    returns_device_lists = True  # ... and has ``device_output``: the lists left on the device

    # -- device state: the biases folded in as extra columns ----------------------------
    def _bias_columns(self, one_u, bu, one_i, bi):
        "(user columns, item columns) behind the embeddings: [p_u, 1, b_u] . [q_i, b_i, 1]"
        return [one_u, bu], [bi, one_i]

    def _device_state(self):
        def upload():
            d = D.device()
            P, Q = self.user_embeddings, self.item_embeddings
            one_u, one_i = np.ones((len(P), 1), np.float32), np.ones((len(Q), 1), np.float32)
            bu = np.zeros_like(one_u) if self.user_bias is None else \
                np.asarray(self.user_bias, np.float32).reshape(-1, 1)
            bi = np.zeros_like(one_i) if self.item_bias is None else \
                np.asarray(self.item_bias, np.float32).reshape(-1, 1)
            ucols, icols = self._bias_columns(one_u, bu, one_i, bi)
            return {"device": d, "U": D.to_device_padded(np.hstack([P, *ucols]), d),
                    "Q": D.to_device_padded(np.hstack([Q, *icols]), d)}

        return self._device_cache("model", upload, self.user_embeddings, self.item_embeddings,
                                  self.user_bias, self.item_bias)

    @property
    def _score_k(self) -> int:
        return self.config.embedding_size + 2

    def _user_rows(self, nums: np.ndarray):
        "device [B x KP] operand rows of the users ``nums`` (-1: unknown -> a zero row) + validity"
        st = self._device_state()
        nums = np.asarray(nums, dtype=np.int64)
        valid = nums >= 0
        idx = torch.from_numpy(np.where(valid, nums, 0)).to(st["device"])
        return st["U"][idx].contiguous(), valid

    def _query_rows(self, queries):
        "``_user_rows`` of a batch of queries (a list of ``RecQuery`` or a ``HistoryBatch``)"
        return self._user_rows(user_numbers(queries, self.users))

    def recommend_batch(self, queries, n: int, *, exclude_history: bool = True,
                        device_output: bool = False):
        """
        Dense scoring + top-N for many queries at once on ``lk_score_topk``, from the operands
        ``__call__`` scores with.  ``queries``: a list of queries or a
        :class:`lkpy_amd.basic.HistoryBatch`.  Returns (item numbers [B x n] with -1 padding,
        scores [B x n] with NaN padding); an unknown user's row is all padding.
        """
        u, valid, hist = self._batch_operands(queries, exclude_history)
        st = self._device_state()
        if hist is not None:
            idx, sc = D.score_topk(u, st["Q"], self._score_k, n, hist.indptr, hist.indices)
        else:
            idx, sc = D.score_topk(u, st["Q"], self._score_k, n)
        D.blank_rows(idx, sc, valid)
        if device_output:
            return idx, sc
        return D.lists_to_host(idx, sc)

    def _batch_operands(self, queries, exclude_history: bool = True):
        "(device [B x KP] user rows, valid, the CSR of items to strike | None) of a batch"
        queries = resolve_queries(queries, self.items)
        st = self._device_state()
        hist = None
        if exclude_history and isinstance(queries, HistoryBatch):
            hist = queries.csr(with_values=False)
        elif exclude_history:  # the items to strike: known ones, sorted, no values
            ptr, idx, _ = pack_histories(queries, self.items, unknown="drop", sort=True)
            hist = D.DeviceCSR.from_arrays(ptr, idx, None, (len(queries), len(self.items)),
                                           st["device"])
        u, valid = self._query_rows(queries)
        return u, valid, hist

    def dense_scores_batch(self, queries):
        """
        Every item's score for many queries at once, left on the device: (panel f32 [B x items],
        valid, history CSR) -- ``recommend_batch``'s operands scored by ``lk_score_dense``.  An
        unknown user's row is NaN; the history is for the caller to exclude.
        """
        u, valid, hist = self._batch_operands(queries)
        panel = D.score_dense(u, self._device_state()["Q"], self._score_k)
        D.blank_panel_rows(panel, valid)
        return panel, valid, hist

    def score_candidates_batch(self, queries, tgt_ptr, item_nums, *, d_targets=None):
        """
        The scores of each query's OWN items, left on the device: f32 [total], entry t the score
        ``__call__`` gives item ``item_nums[t]`` for the query q with ``tgt_ptr[q] <= t <
        tgt_ptr[q + 1]`` -- the same bits, from :meth:`_query_rows` and the dense chain evaluated
        at the targets only (``lk_score_candidates``): no panel is formed.  ``queries``: a list of
        queries or a :class:`lkpy_amd.basic.HistoryBatch`; ``tgt_ptr`` int64 [B + 1] and
        ``item_nums`` int32 (-1: unknown item) are host arrays, ``d_targets`` their device copies
        ``(offsets, numbers)`` where the caller has uploaded them already.  NaN for an unknown
        item and for an unknown user.
        """
        u, valid = self._query_rows(resolve_queries(queries, self.items))
        st = self._device_state()
        d_ptr, d_nums = d_targets or D.upload_targets(tgt_ptr, item_nums, st["device"])
        rows = np.where(valid, np.arange(len(valid)), -1).astype(np.int32)
        return D.score_candidates(u, st["Q"], self._score_k,
                                  torch.from_numpy(rows).to(st["device"]), d_ptr, d_nums, tgt_ptr)


class GlobalBiasPairScoring(BiasedFactorScoring):
    """
    ``score = g + b_u + b_i + p_u . q_i`` with a global bias ``g``, and the ratings of ragged
    (user, item) lists by ``lk_mf_score_pairs``: ``__call__`` is ``score_batch`` with one query,
    so the two agree bit for bit.
    """

    def _bias_columns(self, one_u, bu, one_i, bi):
        # [p_u, 1, b_u, 1] . [q_i, b_i, 1, g]: g is a float32 value (the mean's), carried exactly
        g = np.full_like(one_i, np.float32(self.global_bias))
        return [one_u, bu, one_u], [bi, one_i, g]

    @property
    def _score_k(self) -> int:
        return self.config.embedding_size + 3

    def _score_rows(self, users: torch.Tensor, user_rows, tgt_ptr, item_nums,
                    device_output: bool):
        """
        Query q is row ``user_rows[q]`` of the device operand ``users`` against the items
        ``item_nums[tgt_ptr[q]:tgt_ptr[q + 1]]`` (-1: unknown -> NaN).  One upload, one
        ``lk_mf_score_pairs`` launch, one download (none with ``device_output``).
        """
        st = self._device_state()
        user_rows = np.ascontiguousarray(user_rows, dtype=np.int32).reshape(-1)
        tgt_ptr = np.ascontiguousarray(tgt_ptr, dtype=np.int64).reshape(-1)
        item_nums = np.ascontiguousarray(item_nums, dtype=np.int32).reshape(-1)
        nq, total = len(user_rows), len(item_nums)
        if len(tgt_ptr) != nq + 1 or tgt_ptr[0] != 0 or tgt_ptr[-1] != total or \
                (np.diff(tgt_ptr) < 0).any():
            raise ValueError("tgt_ptr must ascend from 0 to len(item_nums), one entry per query "
                             "and one more")
        if total == 0:
            empty = np.zeros(0, np.float32)
            return torch.from_numpy(empty).to(st["device"]) if device_output else empty
        # one upload: offsets (int64) | user rows | item numbers (int32)
        packed = np.empty(2 * (nq + 1) + nq + total, np.int32)
        packed[:2 * (nq + 1)] = tgt_ptr.view(np.int32)
        packed[2 * (nq + 1):2 * (nq + 1) + nq] = user_rows
        packed[2 * (nq + 1) + nq:] = item_nums
        d_packed = torch.from_numpy(packed).to(st["device"])
        out = self._pair_scores(users, st["Q"], d_packed[2 * (nq + 1):2 * (nq + 1) + nq],
                                d_packed[:2 * (nq + 1)].view(torch.int64),
                                d_packed[2 * (nq + 1) + nq:], tgt_ptr)
        return out if device_output else out.cpu().numpy()

    def _pair_scores(self, users, items, d_rows, d_ptr, d_nums, tgt_ptr):
        "the kernel behind ``_score_rows`` (``tgt_ptr``: the host copy of the offsets ``d_ptr``)"
        return D.mf_score_pairs(users, items, self._score_k, d_rows, d_ptr, d_nums)

    def score_candidates_batch(self, queries, tgt_ptr, item_nums, *, d_targets=None):
        """
        The scores of each query's OWN items, left on the device (f32 [total]; the contract of
        ``BiasedFactorScoring.score_candidates_batch``).  ``__call__`` is defined by
        ``lk_mf_score_pairs`` here, so this is ``_score_rows(device_output=True)`` on the operand
        rows ``__call__`` takes (:meth:`_query_rows`): a candidate ranking made from these scores
        carries the bits of ``__call__``, which are NOT those of ``lk_score_topk`` (the whole-
        catalogue ``recommend_batch``: the k-ordered chain, not per-lane partial sums).
        ``_score_rows`` packs and uploads the targets itself; ``d_targets`` is not used.
        """
        u, valid = self._query_rows(resolve_queries(queries, self.items))
        return self._score_rows(u, np.where(valid, np.arange(len(valid)), -1), tgt_ptr, item_nums,
                                True)

    def score_pairs(self, user_nums, tgt_ptr, item_nums, *, device_output: bool = False):
        "Scores by number: ``_score_rows`` with the users' stored operand rows."
        return self._score_rows(self._device_state()["U"], user_nums, tgt_ptr, item_nums,
                                device_output)

    def _pair_operand(self, queries: list[RecQuery]):
        "(device user operand, the queries' rows in it; -1: unknown user) for ``score_batch``"
        return self._device_state()["U"], user_numbers(queries, self.users)

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "``__call__`` for many queries: one vocabulary pass, one launch, the same bits."
        qs = [RecQuery.create(q) for q in queries]
        ptr, nums = pack_targets(item_lists, self.items)
        users, rows = self._pair_operand(qs)
        scores = self._score_rows(users, rows, ptr, nums, False)
        return [ItemList(il, scores=scores[ptr[i]:ptr[i + 1]])
                for i, il in enumerate(item_lists)]

    def __call__(self, query, items: ItemList) -> ItemList:
        return self.score_batch([query], [items])[0]


class QueryUserBias:
    """
    For a :class:`GlobalBiasPairScoring` scorer whose biases are a ``BiasModel`` (``self.bias``):
    the user bias of a query follows ``BiasModel.compute_for_items`` -- recomputed from the
    query's rated history where it has one, the stored bias otherwise -- so the user operand's
    bias column is set per query.  Mixed in before the scoring class (``BiasedSVDScorer``,
    ``FunkSVDScorer``).
    """

    user_bias = property(lambda self: self.bias.user_biases)
    item_bias = property(lambda self: self.bias.item_biases)
    global_bias = property(lambda self: self.bias.global_bias)

    def _device_item_bias(self):
        def upload():
            ib = self.bias.item_biases
            return None if ib is None else torch.from_numpy(
                np.ascontiguousarray(ib, dtype=np.float32)).to(D.device())

        return self._device_cache("item_bias", upload, self.bias)

    def _history_user_bias(self, query: RecQuery):
        """The user bias ``BiasModel.compute_for_items`` computes from the query's rated history
        (bias.py:211-229), or None where it takes the stored one."""
        hist = query.query_items
        ratings = hist.field("rating") if hist is not None else None
        if ratings is None:
            return None
        b = self.bias
        uoff = np.asarray(ratings, dtype=np.float64) - b.global_bias
        if b.item_biases is not None:
            nums = hist.numbers(vocabulary=b.items, missing="negative")
            known = nums >= 0
            uoff[known] -= b.item_biases[nums[known]]
        ub = np.sum(uoff) / (np.sum(np.isfinite(uoff)) + _damping(b.damping, "user"))
        return np.float32(0.0 if np.isnan(ub) else ub)

    def _query_rows(self, queries):
        """The users' operand rows with the bias column as ``compute_for_items`` sets it: from
        the query's ratings where it has some (a ``HistoryBatch``: ``lk_bias_user_offsets`` on
        the training matrix in HBM), else the stored bias the row already carries."""
        u, valid = self._user_rows(user_numbers(queries, self.users))
        if self.bias.user_biases is None or len(valid) == 0:
            return u, valid
        col = self.config.embedding_size + 1  # [x_u, 1, b_u, 1]
        dev = u.device
        if isinstance(queries, HistoryBatch):
            mat = queries.lookup._device_matrix()
            if not mat["has_ratings"]:
                return u, valid
            nums = torch.from_numpy(np.ascontiguousarray(queries.user_nums, np.int32)).to(dev)
            ub, add = D.bias_user_offsets(mat["csr"], nums, self.bias.global_bias,
                                          self._device_item_bias(),
                                          _damping(self.bias.damping, "user"))
            u[:, col] = torch.where(add.bool(), ub, u[:, col])
            return u, valid
        own = [self._history_user_bias(q) for q in queries]
        rows = [i for i, b in enumerate(own) if b is not None]
        if rows:
            vals = np.asarray([own[i] for i in rows], dtype=np.float32)
            u[torch.from_numpy(np.asarray(rows)).to(dev), col] = torch.from_numpy(vals).to(dev)
        return u, valid

    def _pair_operand(self, queries: list[RecQuery]):
        u, valid = self._query_rows(queries)
        return u, np.where(valid, np.arange(len(valid)), -1)
