"""
Component seam for ALS matrix factorisation (implicit feedback; the explicit / biased-MF model
is at the end of the file): mirror of ``lenskit.als.ImplicitMFScorer`` /
``ImplicitMFTrainer`` / ``ALSBase`` / ``ALSTrainerBase`` / ``ALSConfig``
(src/lenskit/als/_common.py:36-356, src/lenskit/als/_implicit.py:24-184), with the same
config fields, attributes after training (``users``, ``items``, ``user_embeddings``,
``item_embeddings``, ``_OtOr``, ``trained_epochs``) and scoring semantics, but with the
epoch loop resident on the GPU (:class:`lkpy_amd._als_engine.ImplicitALSEngine`).
Learned state is kept as host NumPy arrays so pickling / ``get_parameters`` keep working
(SURVEY.md section 5 "Checkpoint / resume"); device state is rebuilt lazily.
"""

from __future__ import annotations

from typing import Literal

import numpy as np
import scipy.sparse as sps
import torch
from pydantic import AliasChoices, BaseModel, Field, PositiveFloat, PositiveInt

from . import _device as D
from . import _native
from ._als_engine import HipBackend, ImplicitALSEngine
from ._queries import (item_scores, pack_histories, pack_targets, resolve_queries,
                       user_numbers)
from .basic import BiasModel, HistoryBatch, _damping
from .data import Dataset, ItemList, RecQuery, Vocabulary
from .pipeline import Component
from .training import ModelTrainer, TrainingOptions, UsesTrainer


class _DeviceBacked:
    """
    A learned array attribute (``user_embeddings``, ``item_embeddings``, ``_OtOr``) that lives on
    the host -- so that pickling / ``get_parameters`` work as in the reference -- but is only
    REFRESHED FROM HBM WHEN SOMEBODY READS IT: while a trainer is live the factors stay on the
    device across epochs (one PCIe crossing in, one out) and ``train_epoch`` merely marks the
    host copies stale.  The ``ModelTrainer`` contract "the model is usable after every epoch"
    (src/lenskit/training.py:336-378) holds: the first read after an epoch downloads.
    """

    def __set_name__(self, owner, name):
        self.slot = "_h_" + name

    def __get__(self, obj, cls=None):
        if obj is None:
            return self
        pend = obj.__dict__.get("_pending_sync")
        if pend is not None:
            pend()
        return obj.__dict__.get(self.slot)

    def __set__(self, obj, value):
        obj.__dict__[self.slot] = value


def _scorer_state(obj) -> dict:
    "``__getstate__`` of the ALS scorers: host arrays only (synchronised first), no device state."
    pend = obj.__dict__.get("_pending_sync")
    if pend is not None:
        pend()
    st = Component.__getstate__(obj)
    st.pop("_pending_sync", None)
    return st


def _restore_scorer_state(obj, state: dict):
    """
    ``__setstate__`` of the ALS scorers.  Pickles written before the learned arrays became
    lazily-synchronised descriptors hold them under their plain names (``user_embeddings``,
    ``item_embeddings``, ``_OtOr``); they are moved to the descriptors' ``_h_`` slots so that an
    old model file scores as before instead of failing later inside ``_device_state``.
    """
    state = dict(state)
    for name in ("user_embeddings", "item_embeddings", "_OtOr"):
        if name in state and isinstance(getattr(type(obj), name, None), _DeviceBacked):
            state.setdefault("_h_" + name, state.pop(name))
    state.pop("_dev", None)
    state.pop("_pending_sync", None)
    obj.__dict__.update(state)


def _reference_order(options: TrainingOptions) -> str | None:
    """``LK_ALS_RHS_ORDER`` through ``TrainingOptions.environment`` (or the process environment):
    ``auto`` (default: rows of more than 2048 entries summed exactly as the reference sums them),
    ``reference`` (strict: every row of more than 256 entries), ``accurate`` (the tuned kernels'
    own order everywhere) -- INTEGRATION.md, environment knobs; None = not said here, the backend
    reads the process environment."""
    order = options.env_var("LK_ALS_RHS_ORDER", None) if options is not None else None
    return None if not order else order.lower()


class UIPair(BaseModel):
    user: PositiveFloat
    item: PositiveFloat


class ALSConfig(BaseModel):
    "src/lenskit/als/_common.py:36-78 (+ EmbeddingSizeMixin's ``embedding_size_exp``)."

    embedding_size: PositiveInt = Field(
        default=64, validation_alias=AliasChoices("embedding_size", "features"))
    embedding_size_exp: PositiveInt | None = None
    epochs: PositiveInt = 10
    regularization: PositiveFloat | UIPair | dict = 0.1
    user_embeddings: bool | Literal["prefer"] = True

    def model_post_init(self, _ctx):
        if self.embedding_size_exp is not None:
            object.__setattr__(self, "embedding_size", 2 ** int(self.embedding_size_exp))
        if self.embedding_size > 1024:
            # fail at configuration time, not in the middle of training (lk_padded_dim).  Up to
            # 256 the normal matrix stays in registers; 257 .. 1024 take the HBM-tile solver
            # (csrc/als_big.hip: exact, slower)
            raise ValueError(
                f"embedding_size {self.embedding_size} exceeds the device kernels' limit of 1024")
        if isinstance(self.regularization, dict):
            object.__setattr__(self, "regularization", UIPair(**self.regularization))

    @property
    def user_reg(self) -> float:
        r = self.regularization
        return r.user if isinstance(r, UIPair) else float(r)

    @property
    def item_reg(self) -> float:
        r = self.regularization
        return r.item if isinstance(r, UIPair) else float(r)


class ImplicitMFConfig(ALSConfig):
    "src/lenskit/als/_implicit.py:24-32"

    weight: float = 40
    use_ratings: bool = False
    solver: Literal["auto", "cholesky", "cg"] = "auto"
    """Backend knob (also ``LK_ALS_SOLVER``): ``auto`` = ``cholesky`` = the exact solve the
    reference performs (LAPACK sposv), at every supported embedding size (k <= 1024); ``cg`` =
    tolerance-terminated conjugate gradient (64 <= padded k <= 256), on request only."""


_SOLVERS = {"auto": _native.SOLVER_AUTO, "cholesky": _native.SOLVER_CHOLESKY,
            "chol": _native.SOLVER_CHOLESKY, "cg": _native.SOLVER_CG}


class ImplicitMFScorer(UsesTrainer, Component):
    """
    Implicit-feedback matrix factorisation trained with ALS (Hu, Koren, Volinsky); the
    reference solves every row exactly with LAPACK ``sposv`` (class docstring,
    src/lenskit/als/_implicit.py:52-54) and so does the default GPU solver.
    """

    config: ImplicitMFConfig
    accepts_history_batch = True  # recommend_batch takes a lkpy_amd.basic.HistoryBatch
    returns_device_lists = True  # ... and has ``device_output``: the lists left on the device

    users: Vocabulary | None = None
    items: Vocabulary
    user_embeddings = _DeviceBacked()  # np.ndarray [users x k] f32 | None
    item_embeddings = _DeviceBacked()  # np.ndarray [items x k] f32
    _OtOr = _DeviceBacked()  # np.ndarray [k x k] f32: Q^T Q + user_reg I

    def create_trainer(self, data, options):
        return ImplicitMFTrainer(self, data, options)

    # -- device-side caches (never pickled) ---------------------------------------
    def __getstate__(self):
        return _scorer_state(self)

    def __setstate__(self, state):
        _restore_scorer_state(self, state)

    def _device_state(self):
        def upload():
            d = D.device()
            return {"device": d, "Q": D.to_device_padded(self.item_embeddings, d),
                    "OtOr": torch.from_numpy(np.ascontiguousarray(self._OtOr)).to(d)}

        return self._device_cache("model", upload, self.item_embeddings, self._OtOr)

    def _solver(self, options: TrainingOptions | None = None) -> int:
        name = self.config.solver
        if options is not None:
            name = options.env_var("LK_ALS_SOLVER", name) or name
        return _SOLVERS[name.lower()]

    # -- fold-in --------------------------------------------------------------------
    def _confidence(self, hist: ItemList, nums: np.ndarray, kept: np.ndarray) -> np.ndarray:
        """
        The confidence values of one history's kept items (_implicit.py:83-92): ``rating *
        weight`` in the ratings' own dtype (the caller casts to float32), or the constant
        ``weight``.
        """
        if not self.config.use_ratings:
            return np.full(int(kept.sum()), self.config.weight)
        ratings = hist.field("rating")
        if ratings is None:
            raise ValueError("no ratings in user items")  # (_implicit.py:85-86)
        return np.asarray(ratings)[kept] * self.config.weight

    def _history_rows(self, queries: list[RecQuery]):
        """
        histories -> CSR (queries x items) of confidence values (_implicit.py:77-99), rows sorted
        by item number, history items the model does not know DROPPED.
        """
        return pack_histories(queries, self.items, unknown="drop", sort=True,
                              values=self._confidence)

    def _query_csr(self, queries: list[RecQuery]) -> D.DeviceCSR:
        "``_history_rows`` uploaded: the list front-end's histories as a device CSR."
        ptr, idx, val = self._history_rows(queries)
        return D.DeviceCSR.from_arrays(ptr, idx, val, (len(queries), len(self.items)),
                                       self._device_state()["device"])

    def _fold_in(self, hist: D.DeviceCSR, pending: list | None = None) -> torch.Tensor:
        "One fold-in per row of ``hist`` (_implicit.py:77-130 per query): one half-epoch launch."
        st = self._device_state()
        return D.fold_in(hist, st["Q"], st["OtOr"], self.config.embedding_size, self._solver(),
                         pending)

    def new_user_embedding(self, user_num, user_items: ItemList):
        "One fold-in (_implicit.py:77-99); returns (vector, None)."
        u = self._fold_in(self._query_csr([RecQuery(user_items=user_items)]))
        return D.to_host_unpadded(u, self.config.embedding_size)[0], None

    def _embeddings(self, hist: D.DeviceCSR, has_hist: np.ndarray, stored: np.ndarray,
                    pending: list | None = None) -> tuple[torch.Tensor, np.ndarray]:
        """
        Device [B x KP] embedding per query + validity mask, with ``ALSBase.__call__``'s
        precedence (_common.py:139-157): history present and user_embeddings != "prefer" ->
        fold-in; else the stored row; else invalid.  ``hist``: the queries' histories (device
        CSR of confidence values); ``has_hist``, ``stored`` (the user's row of
        ``user_embeddings``, -1 = none): host arrays over the queries.
        """
        d = self._device_state()["device"]
        B = len(has_hist)
        fold = has_hist & (self.config.user_embeddings != "prefer")
        if B and fold.all():
            u = self._fold_in(hist, pending)
        else:
            u = torch.zeros((B, D.padded_dim(self.config.embedding_size)), dtype=torch.float32,
                            device=d)
            if fold.any():
                rows = np.flatnonzero(fold)
                u[torch.from_numpy(rows).to(d)] = self._fold_in(D.gather_rows(hist, rows), pending)
        take = ~fold & (stored >= 0)
        if take.any():
            rows = np.ascontiguousarray(self.user_embeddings[stored[take]], dtype=np.float32)
            u[torch.from_numpy(np.flatnonzero(take)).to(d)] = D.to_device_padded(rows, d)
        return u, fold | take

    def _query_embeddings(self, queries: list[RecQuery], pending: list | None = None):
        """
        :meth:`_embeddings` for a list of queries: histories by :meth:`_history_rows`, stored
        rows by user id.  Returns (device [B x KP], valid, history CSR).
        """
        hist = self._query_csr(queries)
        has_hist = np.array([q.query_items is not None and len(q.query_items) > 0
                             for q in queries], dtype=bool)
        return (*self._embeddings(hist, has_hist, self._stored_rows(queries), pending), hist)

    def _stored_rows(self, queries) -> np.ndarray:
        "per query: the user's row of ``user_embeddings``, -1 = none"
        return user_numbers(queries, None if self.user_embeddings is None else self.users)

    def _history_batch_embeddings(self, batch, pending: list | None = None):
        """
        :meth:`_embeddings` for a :class:`lkpy_amd.basic.HistoryBatch`: the histories' CSR is cut
        out of the HBM-resident training matrix by one kernel (no per-query Python), the stored
        rows are found by user number.  Returns (device [B x KP], valid, history CSR).
        """
        cfg = self.config
        hist = batch.csr(use_ratings=cfg.use_ratings, scale=cfg.weight)
        return (*self._embeddings(hist, batch.lengths > 0, self._stored_rows(batch), pending),
                hist)

    # -- scoring (src/lenskit/als/_common.py:133-175) -----------------------------------
    def __call__(self, query, items: ItemList) -> ItemList:
        query = RecQuery.create(query)
        u, valid, _ = self._query_embeddings([query])
        if not valid[0]:
            return ItemList(items, scores=np.nan)
        st = self._device_state()
        all_scores = D.score_dense(u, st["Q"], self.config.embedding_size)[0].cpu().numpy()
        return ItemList(items, scores=item_scores(items, self.items, all_scores))

    def recommend_batch(self, queries, n: int, *, exclude_history: bool = True,
                        device_output: bool = False):
        """
        Batched fold-in + dense scoring + top-N for many queries at once (the reference
        loops queries in Python, src/lenskit/batch/_runner.py:283-308).  ``queries``: a list of
        queries, or a :class:`lkpy_amd.basic.HistoryBatch` (training histories by user number: the
        whole call then has no per-query host work).  Returns (item numbers [B x n] with -1
        padding, scores [B x n] with NaN padding) as host arrays (``device_output``: as device
        tensors, nothing downloaded).
        """
        u, valid, hist, pending = self._batch_operands(queries)
        st = self._device_state()
        if exclude_history:
            idx, sc = D.score_topk(u, st["Q"], self.config.embedding_size, n, hist.indptr,
                                   hist.indices)
        else:
            idx, sc = D.score_topk(u, st["Q"], self.config.embedding_size, n)
        for plan in pending:
            plan.check_status()  # RuntimeError("ALS solve error: ...") like the fold-in alone
        D.blank_rows(idx, sc, valid)
        if device_output:
            return idx, sc
        return D.lists_to_host(idx, sc)

    def _batch_operands(self, queries):
        """
        What scoring a batch starts from: (device [B x KP] embeddings, valid, history CSR, the
        fold-in plans whose status is read once the scoring is queued behind them).
        """
        queries = resolve_queries(queries, self.items)
        pending: list = []
        if isinstance(queries, HistoryBatch):
            return (*self._history_batch_embeddings(queries, pending), pending)
        return (*self._query_embeddings(queries, pending), pending)

    def dense_scores_batch(self, queries):
        """
        Every item's score for many queries at once, left on the device: (panel f32 [B x items],
        valid, history CSR) -- ``recommend_batch``'s operands scored by ``lk_score_dense``.  The
        row of a query that cannot be scored is NaN; the history is for the caller to exclude.
        """
        u, valid, hist, pending = self._batch_operands(queries)
        panel = D.score_dense(u, self._device_state()["Q"], self.config.embedding_size)
        for plan in pending:
            plan.check_status()
        D.blank_panel_rows(panel, valid)
        return panel, valid, hist

    def score_candidates_batch(self, queries, tgt_ptr, item_nums, *, d_targets=None):
        """
        The scores of each query's OWN items, left on the device: f32 [total], entry t the score
        ``__call__`` gives item ``item_nums[t]`` for the query q with ``tgt_ptr[q] <= t <
        tgt_ptr[q + 1]`` -- the same bits, from ``recommend_batch``'s operands and the dense
        chain evaluated at the targets only (``lk_score_candidates``): no panel is formed.
        ``queries``: a list of queries or a :class:`lkpy_amd.basic.HistoryBatch`; ``tgt_ptr`` int64
        [B + 1] and ``item_nums`` int32 (-1: unknown item) are host arrays, ``d_targets`` their
        device copies ``(offsets, numbers)`` where the caller has uploaded them already.  NaN for
        an unknown item and for a query that cannot be scored.
        """
        u, valid, _hist, pending = self._batch_operands(queries)
        st = self._device_state()
        d_ptr, d_nums = d_targets or D.upload_targets(tgt_ptr, item_nums, st["device"])
        rows = np.where(valid, np.arange(len(valid)), -1).astype(np.int32)
        out = D.score_candidates(u, st["Q"], self.config.embedding_size,
                                 torch.from_numpy(rows).to(st["device"]), d_ptr, d_nums, tgt_ptr)
        for plan in pending:
            plan.check_status()  # RuntimeError("ALS solve error: ...") like the fold-in alone
        return out


class ImplicitMFTrainer(ModelTrainer):
    "``ALSTrainerBase`` + ``ImplicitMFTrainer`` (_common.py:195-356, _implicit.py:133-175)."

    def __init__(self, scorer: ImplicitMFScorer, data: Dataset, options: TrainingOptions):
        self.scorer = scorer
        cfg = scorer.config
        scorer.users, scorer.items = data.users, data.items
        self.rng = options.random_generator()
        import threading

        k = cfg.embedding_size
        init = {}

        def draw():
            # item matrix FIRST, then users, same generator (_common.py:287-301).  NumPy draws
            # outside the GIL: the 14 M normals of an ML-25M model (0.1 s) are drawn while the
            # main thread uploads the matrix and builds both orientations and the plans in HBM
            init["Q"] = self.initial_params(data.item_count, k)
            init["P"] = self.initial_params(data.user_count, k)

        th = threading.Thread(target=draw)
        th.start()
        try:
            ui = self.prepare_matrix(data)
            dev = D.device(None if options.configured_device() in ("cuda", "cpu") else
                           options.configured_device())
            backend = HipBackend(k, dev, scorer._solver(options), _reference_order(options))
            self.engine = ImplicitALSEngine(sps.csr_array(ui), k, cfg.user_reg, cfg.item_reg,
                                            None, None, backend, defer_init=True)
        finally:
            th.join()
        scorer.item_embeddings, scorer.user_embeddings = init["Q"], init["P"]
        self.engine.set_initial(scorer.user_embeddings, scorer.item_embeddings)
        self.epochs_trained = 0

    def prepare_matrix(self, data: Dataset) -> sps.csr_array:
        """
        _implicit.py:141-149 + the ``from_scipy(ui_rates)`` of _common.py:218: confidence values
        ``weight`` (or ``weight * rating``) in CSR.  The reference goes through COO and lets
        SciPy convert; the dataset already holds (user, item)-sorted interactions, so the CSR
        arrays are taken as they are -- same matrix, no host sort -- unless the dataset reports
        repeated pairs, which are summed as SciPy's conversion would.
        """
        ints = data.interactions().matrix()
        rmat = ints.scipy(attribute="rating", layout="csr") if self.scorer.config.use_ratings \
            else ints.scipy(layout="csr")
        vals = np.require(rmat.data, dtype=np.float32) * np.float32(self.scorer.config.weight)
        if getattr(data, "has_duplicates", True):
            # repeated (user, item) pairs: ONE entry with the summed confidence, exactly what
            # the reference's COO -> CSR conversion produces (y gets (2v + 1) once, not (v + 1)
            # twice).  ``scipy()`` hands out the Dataset's OWN index arrays without a copy and
            # ``sum_duplicates`` rewrites indices / indptr in place: canonicalise private copies,
            # never the dataset (tests/test_host_logic.py::test_prepare_matrix_leaves_dataset_alone)
            out = sps.csr_array((vals, rmat.indices.copy(), rmat.indptr.copy()), shape=rmat.shape)
            out.sum_duplicates()
            return out
        return sps.csr_array((vals, rmat.indices, rmat.indptr), shape=rmat.shape)

    def initial_params(self, nrows: int, ncols: int) -> np.ndarray:
        "_implicit.py:152-155"
        mat = self.rng.standard_normal((nrows, ncols), dtype=np.float32) * 0.01
        mat *= mat
        return mat

    def train_epoch(self):
        du, di = self.engine.train_epoch()
        self.engine.check()  # RuntimeError("ALS solve error: ...") like implicit.rs:79
        self.epochs_trained += 1
        # the factors stay in HBM; the host copies are refreshed on first read (_DeviceBacked)
        self.scorer.__dict__["_pending_sync"] = self._sync
        return {"deltaP": float(du.item()), "deltaQ": float(di.item())}

    def _sync(self):
        "download the current factors (called lazily through the scorer's attributes)"
        s = self.scorer
        s.__dict__.pop("_pending_sync", None)
        s.user_embeddings = self.engine.user_embeddings()
        s.item_embeddings = self.engine.item_embeddings()
        s._OtOr = self.engine.otor()  # _save_user_otor (_implicit.py:171-175)

    def finalize(self):
        self._sync()
        if not self.scorer.config.user_embeddings:  # _common.py:318-325
            self.scorer.user_embeddings = None
            self.scorer.users = None

    def get_parameters(self):
        return {"user_embeddings": self.scorer.user_embeddings,
                "item_embeddings": self.scorer.item_embeddings}


# ---------------------------------------------------------------------------------------
# Explicit feedback: biased matrix factorisation
# ---------------------------------------------------------------------------------------


class BiasedMFConfig(ALSConfig):
    "src/lenskit/als/_explicit.py:25-29"

    damping: float | tuple[float, float] | dict[str, float] = 5.0


class BiasedMFScorer(UsesTrainer, Component):
    """
    Biased matrix factorisation trained with ALS on bias-normalised ratings
    (``BiasedMFScorer``, src/lenskit/als/_explicit.py:32-90): the bias model stays on the
    host, the row solves (training and fold-in) run in the explicit mode of the HIP kernel.
    Scoring follows ``ALSBase.__call__`` (src/lenskit/als/_common.py:133-175) +
    ``finalize_scores`` (adds b_g + b_i + b_u back).  Whole batches -- ``recommend_batch``,
    ``dense_scores_batch``, ``score_batch``, ``predict_history_batch`` -- do the same arithmetic on
    the device (csrc/bmf_batch.hip) and hold float32(the per-query score) bit for bit.
    """

    config: BiasedMFConfig
    accepts_history_batch = True  # recommend_batch takes a lkpy_amd.basic.HistoryBatch
    returns_device_lists = True  # ... and has ``device_output``: the lists left on the device
    PANEL_BYTES = 1 << 30  # score panel of one recommend / score step

    users: Vocabulary | None = None
    items: Vocabulary
    user_embeddings = _DeviceBacked()
    item_embeddings = _DeviceBacked()
    bias: BiasModel

    def create_trainer(self, data, options):
        return BiasedMFTrainer(self, data, options)

    def __getstate__(self):
        return _scorer_state(self)

    def __setstate__(self, state):
        _restore_scorer_state(self, state)

    def _device_state(self):
        def upload():
            d = D.device()
            f32 = lambda a: None if a is None else torch.from_numpy(  # noqa: E731
                np.ascontiguousarray(a, dtype=np.float32)).to(d)
            kept = self.user_embeddings is not None
            return {"device": d, "Q": D.to_device_padded(self.item_embeddings, d),
                    "item_biases": f32(self.bias.item_biases),
                    "user_biases": f32(self.bias.user_biases) if kept else None}

        return self._device_cache("model", upload, self.item_embeddings, self.bias,
                                  self.bias.item_biases, self.bias.user_biases)

    def _device_users(self) -> torch.Tensor:
        "The stored user embeddings in HBM ([users x KP]), uploaded when a batch first takes one."
        return self._device_cache(
            "users", lambda: D.to_device_padded(self.user_embeddings, D.device()),
            self.user_embeddings)

    def _residual_row(self, user_items: ItemList):
        """
        The host part of a fold-in (_explicit.py:56-70): the history's known items with a finite
        rating in ascending item number, their ratings minus the bias model (float32), and the
        user bias ``BiasModel.compute_for_items`` derives from the history.
        """
        inums = user_items.numbers(vocabulary=self.items, missing="negative")
        ratings = user_items.field("rating")
        assert ratings is not None
        ratings = np.asarray(ratings, dtype=np.float32)
        mask = (inums >= 0) & np.isfinite(ratings)
        biases, u_bias = self.bias.compute_for_items(user_items, None, user_items)
        resid = (ratings - biases)[mask]
        order = np.argsort(inums[mask], kind="stable")
        return inums[mask][order].astype(np.int32), resid[order].astype(np.float32), u_bias

    def new_user_embedding(self, user_num, user_items: ItemList):
        "_explicit.py:56-74: normalise the ratings with the bias model, one explicit row solve."
        nums, resid, u_bias = self._residual_row(user_items)
        st = self._device_state()
        hist = D.DeviceCSR.from_arrays(
            np.array([0, len(nums)], dtype=np.int64), nums, resid, (1, len(self.items)),
            st["device"])
        u = D.fold_in_explicit(hist, st["Q"], self.config.user_reg, self.config.embedding_size)
        return D.to_host_unpadded(u, self.config.embedding_size)[0], u_bias

    def finalize_scores(self, user_num, items: ItemList, user_bias) -> ItemList:
        "_explicit.py:76-93"
        scores = items.scores()
        if user_bias is None:
            if user_num is not None and self.bias.user_biases is not None:
                user_bias = self.bias.user_biases[user_num]
            else:
                user_bias = 0.0
        biases = self.bias.compute_for_items(items, bias=user_bias)
        return ItemList(items, scores=scores + biases)

    def __call__(self, query, items: ItemList) -> ItemList:
        query = RecQuery.create(query)
        user_num = None
        if query.user_id is not None and self.users is not None:
            user_num = self.users.number(query.user_id, missing=None)
        u_feat, u_off = None, None
        hist = query.query_items
        if hist is not None and len(hist) > 0 and self.config.user_embeddings != "prefer":
            u_feat, u_off = self.new_user_embedding(user_num, hist)
        if u_feat is None:
            if user_num is None or self.user_embeddings is None:
                return ItemList(items, scores=np.nan)
            u_feat = self.user_embeddings[user_num, :]
        st = self._device_state()
        k = self.config.embedding_size
        u = D.to_device_padded(np.ascontiguousarray(u_feat, dtype=np.float32)[None, :],
                               st["device"])
        all_scores = D.score_dense(u, st["Q"], k)[0].cpu().numpy()
        scores = item_scores(items, self.items, all_scores)
        return self.finalize_scores(user_num, ItemList(items, scores=scores), u_off)

    # -- whole batches of queries ---------------------------------------------------------------
    # ``__call__`` adds in float64 on a fold-in row (the user bias derived from the history is a
    # NumPy float64 scalar: NEP 50) and in float32 on a stored row; a batched list holds
    # float32(the per-query score), formed in the branch's own precision by lk_bmf_finish_*.

    def _batch_ready(self) -> bool:
        "the bias model has both terms (``BiasedMFTrainer`` always learns both): the kernels' case"
        return self.bias.item_biases is not None and self.bias.user_biases is not None

    def _panel_rows(self) -> int:
        return max(1, self.PANEL_BYTES // (4 * max(len(self.items), 1)))

    def _batch_operands(self, queries):
        """
        What scoring a batch starts from, with the precedence of ``__call__``: history present
        and user_embeddings != "prefer" -> fold-in; else the stored row of a known user; else
        invalid.  Returns (device [B x KP] embeddings, host modes uint8 [B] (``_native.BMF_*``),
        the same on the device, device float64 [B] user biases -- the history's on a fold-in row,
        the model's on a stored one --, the histories' CSR (structure: the items to strike), the
        fold-in plans whose status is read once the scoring is queued behind them).

        A :class:`HistoryBatch` over a float32 training matrix of finite ratings does no
        per-query host work: ``lk_bmf_residual_rows`` reads the rows by user number, one explicit
        half-epoch solves every fold-in row, stored rows are gathered by number.  Any other batch
        computes the residuals per query on the host (``_residual_row``) and uploads one CSR.
        """
        queries = resolve_queries(queries, self.items)
        if isinstance(queries, HistoryBatch) and not queries.lookup.ratings_finite():
            queries = queries.queries()
        st = self._device_state()
        d, cfg = st["device"], self.config
        B = len(queries)
        pending: list = []
        prefer = cfg.user_embeddings == "prefer"
        if isinstance(queries, HistoryBatch):
            fold = (queries.lengths > 0) & (not prefer)
            resid, ub = D.bmf_residual_rows(
                queries.lookup._device_matrix()["csr"], np.where(fold, queries.user_nums, -1),
                self.bias.global_bias, st["item_biases"], _damping(self.bias.damping, "user"))
            # the fold-in rows ARE the histories unless stored rows are preferred
            hist = queries.csr(with_values=False) if prefer else resid
        else:
            fold = np.zeros(B, dtype=bool)
            ptr = np.zeros(B + 1, dtype=np.int64)
            idx, val, h_ub = [], [], np.zeros(B, dtype=np.float64)
            for i, q in enumerate(queries):
                h = q.query_items
                if h is not None and len(h) > 0 and not prefer:
                    nums, res, u_bias = self._residual_row(h)
                    fold[i] = True
                    ptr[i + 1] = len(nums)
                    idx.append(nums)
                    val.append(res)
                    h_ub[i] = u_bias  # (a NaN bias came back as 0: the same sum in either type)
            np.cumsum(ptr, out=ptr)
            cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)  # noqa: E731
            resid = D.DeviceCSR.from_arrays(ptr, cat(idx, np.int32), cat(val, np.float32),
                                            (B, len(self.items)), d)
            ub = torch.from_numpy(h_ub).to(d)
            hp, hi, _ = pack_histories(queries, self.items, unknown="drop", sort=True)
            hist = D.DeviceCSR.from_arrays(hp, hi, None, (B, len(self.items)), d)
        if fold.any():
            u = D.fold_in_explicit(resid, st["Q"], cfg.user_reg, cfg.embedding_size, pending)
        else:
            u = torch.zeros((B, D.padded_dim(cfg.embedding_size)), dtype=torch.float32, device=d)
        stored = self._stored_rows(queries)
        take = ~fold & (stored >= 0)
        if take.any():
            at = torch.from_numpy(np.flatnonzero(take)).to(d)
            rows = torch.from_numpy(stored[take]).to(d)
            u[at] = self._device_users()[rows]
            ub[at] = st["user_biases"][rows].to(torch.float64)
        mode = np.where(fold, _native.BMF_FOLD,
                        np.where(take, _native.BMF_STORED, _native.BMF_INVALID)).astype(np.uint8)
        return u, mode, torch.from_numpy(mode).to(d), ub, hist, pending

    def _stored_rows(self, queries) -> np.ndarray:
        "per query: the user's row of ``user_embeddings``, -1 = none"
        return user_numbers(queries, None if self.user_embeddings is None else self.users)

    def _query_list(self, queries) -> list[RecQuery]:
        if isinstance(queries, HistoryBatch):
            return queries.queries()
        return [RecQuery.create(q) for q in queries]

    def recommend_batch(self, queries, n: int | None, *, exclude_history: bool = True,
                        device_output: bool = False):
        """
        Top-``n`` lists for many queries at once -- what the ``recommender`` pipeline computes one
        query at a time: fold-in or stored row, every item scored, the query's own items struck,
        ``TopNRanker``.  ``queries``: a list of queries, or a :class:`lkpy_amd.basic.HistoryBatch`
        (training histories by user number: no per-query host work).  The batch goes through in
        panels of at most ``PANEL_BYTES``: ``lk_score_dense``, ``lk_bmf_finish_panel`` (biases
        added as ``__call__`` adds them, history struck), ``lk_argtopn``, ``lk_take_scores``.
        ``n`` negative or None: every candidate, ranked.  Returns (item numbers [B x n] with -1
        padding, scores [B x n] float32 with NaN padding) as host arrays (``device_output``:
        device tensors); a query with nothing to score is all padding.
        """
        n = -1 if n is None else int(n)
        if not self._batch_ready():
            return self._recommend_per_query(queries, n, exclude_history, device_output)
        u, _mode, d_mode, ub, hist, pending = self._batch_operands(queries)
        st = self._device_state()
        B = u.shape[0]
        cols = len(self.items) if n < 0 else n
        oi = torch.full((B, cols), -1, dtype=torch.int32, device=st["device"])
        osc = torch.full((B, cols), float("nan"), dtype=torch.float32, device=st["device"])
        step = self._panel_rows()
        for lo in range(0, B, step):
            hi = min(B, lo + step)
            panel = D.score_dense(u[lo:hi], st["Q"], self.config.embedding_size)
            D.bmf_finish_panel(panel, d_mode[lo:hi], ub[lo:hi], self.bias.global_bias,
                               st["item_biases"],
                               hist.indptr[lo:hi + 1] if exclude_history else None,
                               hist.indices if exclude_history else None)
            idx = D.argtopn(panel, n)
            oi[lo:hi, :idx.shape[1]] = idx
            osc[lo:hi, :idx.shape[1]] = D.take_scores(panel, idx)
        for plan in pending:
            plan.check_status()  # RuntimeError("ALS solve error: ...") like the fold-in alone
        if device_output:
            return oi, osc
        return D.lists_to_host(oi, osc)

    def _recommend_per_query(self, queries, n: int, exclude_history: bool, device_output: bool):
        "``recommend_batch`` through ``__call__``: a bias model set by hand without both terms"
        qs = self._query_list(queries)
        cols = len(self.items) if n < 0 else n
        oi = np.full((len(qs), cols), -1, dtype=np.int32)
        osc = np.full((len(qs), cols), np.nan, dtype=np.float32)
        for i, q in enumerate(qs):
            cand = ItemList.from_vocabulary(self.items)
            h = q.query_items
            if exclude_history and h is not None and len(h) > 0:
                nums = h.numbers(vocabulary=self.items, missing="negative")
                cand = cand.remove(numbers=nums[nums >= 0])
            top = self(q, cand).top_n(n)
            oi[i, :len(top)] = top.numbers(vocabulary=self.items)
            osc[i, :len(top)] = top.scores()
        if device_output:
            d = self._device_state()["device"]
            return torch.from_numpy(oi).to(d), torch.from_numpy(osc).to(d)
        return oi, osc

    def dense_scores_batch(self, queries):
        """
        Every item's score for many queries at once, left on the device: (panel f32 [B x items],
        valid, history CSR) -- ``recommend_batch``'s operands scored by ``lk_score_dense`` and
        finished by ``lk_bmf_finish_panel``.  The row of a query that cannot be scored is NaN; the
        history is for the caller to exclude.
        """
        if not self._batch_ready():
            qs = self._query_list(queries)
            every = ItemList.from_vocabulary(self.items)
            rows = np.stack([np.asarray(self(q, every).scores(), dtype=np.float32) for q in qs]) \
                if qs else np.zeros((0, len(self.items)), np.float32)
            d = self._device_state()["device"]
            hp, hi, _ = pack_histories(qs, self.items, unknown="drop", sort=True)
            return (torch.from_numpy(rows).to(d), ~np.isnan(rows).all(axis=1),
                    D.DeviceCSR.from_arrays(hp, hi, None, rows.shape, d))
        u, mode, d_mode, ub, hist, pending = self._batch_operands(queries)
        st = self._device_state()
        panel = D.score_dense(u, st["Q"], self.config.embedding_size)
        D.bmf_finish_panel(panel, d_mode, ub, self.bias.global_bias, st["item_biases"])
        for plan in pending:
            plan.check_status()
        return panel, mode != _native.BMF_INVALID, hist

    def _score_pairs(self, queries, tgt_ptr: np.ndarray, d_ptr: torch.Tensor,
                     d_nums: torch.Tensor) -> torch.Tensor:
        """
        The scores of ragged target lists (host int64 offsets ``tgt_ptr`` [B + 1], the same and
        this scorer's item numbers on the device; -1 = unknown -> NaN), device f32 [entries]: per
        panel of at most ``PANEL_BYTES`` one ``lk_score_dense`` and one ``lk_bmf_finish_pairs``,
        which reads each dot product out of the panel -- the entry ``__call__`` reads.
        """
        u, _mode, d_mode, ub, _hist, pending = self._batch_operands(queries)
        st = self._device_state()
        B = u.shape[0]
        out = torch.empty(int(tgt_ptr[-1]), dtype=torch.float32, device=st["device"])
        step = self._panel_rows()
        for lo in range(0, B, step):
            hi = min(B, lo + step)
            first, count = int(tgt_ptr[lo]), int(tgt_ptr[hi] - tgt_ptr[lo])
            if count == 0:
                continue
            panel = D.score_dense(u[lo:hi], st["Q"], self.config.embedding_size)
            D.bmf_finish_pairs(panel, d_mode[lo:hi], ub[lo:hi], self.bias.global_bias,
                               st["item_biases"], d_ptr[lo:hi + 1], d_nums, first, count, out)
        for plan in pending:
            plan.check_status()
        return out

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "``__call__`` for many queries: the scores are float32(the per-query score), bit for bit."
        qs = [RecQuery.create(q) for q in queries]
        if not self._batch_ready():
            return [self(q, il) for q, il in zip(qs, item_lists)]
        ptr, nums = pack_targets(item_lists, self.items)
        d = self._device_state()["device"]
        if int(ptr[-1]) == 0:
            return [ItemList(il, scores=np.zeros(0, np.float32)) for il in item_lists]
        scores = self._score_pairs(
            qs, ptr, torch.from_numpy(ptr).to(d),
            torch.from_numpy(np.ascontiguousarray(nums, dtype=np.int32)).to(d)).cpu().numpy()
        return [ItemList(il, scores=scores[ptr[i]:ptr[i + 1]])
                for i, il in enumerate(item_lists)]

    def predict_history_batch(self, batch, tgt_ptr, tgt_items, *, h_tgt_ptr=None):
        """
        ``score_batch`` for training histories by user number (``UserTrainingHistoryLookup.batch``)
        and targets already on the device: ``tgt_ptr`` int64 [B + 1], ``tgt_items`` int32 (this
        scorer's item numbers, -1 = unknown); ``h_tgt_ptr``: the offsets' host copy when the
        caller has one.  Returns device f32 [entries].
        """
        if not self._batch_ready():
            raise RuntimeError("predict_history_batch needs a bias model with both terms")
        if h_tgt_ptr is None:
            h_tgt_ptr = tgt_ptr.cpu().numpy()
        return self._score_pairs(batch, np.asarray(h_tgt_ptr, dtype=np.int64), tgt_ptr, tgt_items)


class BiasedMFTrainer(ModelTrainer):
    "``ALSTrainerBase`` + ``BiasedMFTrainer`` (_common.py:195-356, _explicit.py:93-118)."

    def __init__(self, scorer: BiasedMFScorer, data: Dataset, options: TrainingOptions):
        self.scorer = scorer
        cfg = scorer.config
        scorer.users, scorer.items = data.users, data.items
        self.rng = options.random_generator()
        dev = self.device = D.device(None if options.configured_device() in ("cuda", "cpu") else
                                     options.configured_device())
        ui = self.prepare_matrix(data)
        k = cfg.embedding_size
        # item matrix FIRST, then users, same generator (_common.py:287-301)
        scorer.item_embeddings = self.initial_params(data.item_count, k)
        scorer.user_embeddings = self.initial_params(data.user_count, k)
        backend = HipBackend(k, dev, _native.SOLVER_CHOLESKY, _reference_order(options))
        self.engine = ImplicitALSEngine(sps.csr_array(ui), k, cfg.user_reg, cfg.item_reg,
                                        scorer.user_embeddings, scorer.item_embeddings, backend,
                                        explicit=True)
        self.epochs_trained = 0

    def prepare_matrix(self, data: Dataset) -> sps.coo_array:
        "_explicit.py:95-102: ratings minus the learned biases, float32"
        rmat = data.interactions().matrix().scipy(attribute="rating", layout="coo")
        self.scorer.bias = BiasModel.learn(data, damping=self.scorer.config.damping,
                                           device=self.device)
        return self.scorer.bias.transform_matrix(rmat).astype(np.float32)

    def initial_params(self, nrows: int, ncols: int) -> np.ndarray:
        "_explicit.py:104-108: N(0,1) rows scaled to unit length"
        mat = self.rng.standard_normal((nrows, ncols), dtype=np.float32)
        mat /= np.linalg.norm(mat, axis=1).reshape((nrows, 1))
        return mat

    def train_epoch(self):
        du, di = self.engine.train_epoch()
        self.engine.check()  # RuntimeError("ALS solve error: ...") like explicit.rs:72
        self.epochs_trained += 1
        self.scorer.__dict__["_pending_sync"] = self._sync  # lazy download (_DeviceBacked)
        return {"deltaP": float(du.item()), "deltaQ": float(di.item())}

    def _sync(self):
        s = self.scorer
        s.__dict__.pop("_pending_sync", None)
        s.user_embeddings = self.engine.user_embeddings()
        s.item_embeddings = self.engine.item_embeddings()

    def finalize(self):
        self._sync()
        if not self.scorer.config.user_embeddings:  # _common.py:318-325
            self.scorer.user_embeddings = None
            self.scorer.users = None

    def get_parameters(self):
        return {"user_embeddings": self.scorer.user_embeddings,
                "item_embeddings": self.scorer.item_embeddings}
