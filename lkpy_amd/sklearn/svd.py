"""
Singular value decomposition for explicit feedback: mirror of
``lenskit.sklearn.svd.BiasedSVDScorer`` / ``BiasedSVDConfig`` (src/lenskit/sklearn/svd.py:33-139)
-- the bias model, then a truncated SVD of the bias residuals,
``score = user_components[u] . components_[:, i] + g + b_i + b_u``.

The reference hands the residuals to ``sklearn.decomposition.TruncatedSVD``; here the randomized
algorithm runs on the device (:func:`lkpy_amd._device.randomized_svd`: ``lk_csr_spmm``,
``lk_gramian``, ``lk_chol_upper_inverse``, ``lk_score_dense``) from the same Gaussian start panel
the reference's call would draw.  ``algorithm="arpack"`` validates, and ``train`` raises
``NotImplementedError``: there is no device Lanczos and no CPU fallback in this package.

The trained model is a factor model with biases, so it scores through
:class:`lkpy_amd._factor_scoring.GlobalBiasPairScoring` like ``FlexMFExplicitScorer``.  One thing
differs: the user bias of a query follows ``BiasModel.compute_for_items`` -- recomputed from the
query's rated history where it has one, the stored bias otherwise -- so the user operand's bias
column is set per query.
"""

from __future__ import annotations

from typing import Literal

import numpy as np
import torch
from pydantic import AliasChoices, BaseModel, Field

from .. import _device as D
from .._factor_scoring import GlobalBiasPairScoring
from .._queries import user_numbers
from ..als import _scorer_state
from ..basic import BiasModel, HistoryBatch, _damping
from ..data import Dataset, RecQuery, Vocabulary
from ..pipeline import Component
from ..training import Trainable, TrainingOptions


class BiasedSVDConfig(BaseModel):
    "``BiasedSVDConfig`` (svd.py:33-44; ``embedding_size_exp`` is ``EmbeddingSizeMixin``'s)."

    embedding_size: int = Field(default=64,
                                validation_alias=AliasChoices("embedding_size", "features"))
    embedding_size_exp: int | None = None
    damping: float | tuple[float, float] | dict[str, float] = 5
    algorithm: Literal["arpack", "randomized"] = "randomized"
    n_iter: int = 5

    def model_post_init(self, _ctx):
        if self.embedding_size_exp is not None:
            object.__setattr__(self, "embedding_size", 2 ** int(self.embedding_size_exp))


class Factorization:
    """
    What the scorer keeps of ``TruncatedSVD`` after ``fit_transform``: ``components_``
    [k x items] (a view of ``item_factors`` [items x k], the layout the device operand is built
    from), ``singular_values_``, ``n_components``, ``n_iter`` and ``inverse_transform``.
    """

    def __init__(self, item_factors: np.ndarray, singular_values: np.ndarray, n_iter: int):
        self.item_factors = np.ascontiguousarray(item_factors, dtype=np.float32)
        self.singular_values_ = np.asarray(singular_values, dtype=np.float64)
        self.n_iter = int(n_iter)
        self.algorithm = "randomized"

    @property
    def components_(self) -> np.ndarray:
        return self.item_factors.T

    @property
    def n_components(self) -> int:
        return self.item_factors.shape[1]

    def inverse_transform(self, X) -> np.ndarray:
        "``X @ components_`` (``TruncatedSVD.inverse_transform``), on the host"
        return np.asarray(X) @ self.components_


class BiasedSVDScorer(GlobalBiasPairScoring, Component, Trainable):
    """
    Biased matrix factorisation by truncated SVD of the bias residuals.  Learned state: ``bias``
    (:class:`BiasModel`), ``users``, ``items``, ``user_components`` [users x k] float32 (sklearn's
    ``X_transformed``) and ``factorization`` (:class:`Factorization`).
    """

    config: BiasedSVDConfig

    bias: BiasModel
    factorization: Factorization
    users: Vocabulary
    items: Vocabulary
    user_components: np.ndarray

    _start_panel = None  # a test hook: the Gaussian start panel to use instead of drawing one

    def is_trained(self):
        return hasattr(self, "factorization")

    def __getstate__(self):
        return _scorer_state(self)

    def __setstate__(self, state):
        state = dict(state)
        state.pop("_dev", None)
        self.__dict__.update(state)

    # -- training (svd.py:74-104) ----------------------------------------------------------
    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        if self.is_trained() and not options.retrain:
            return
        cfg = self.config
        if cfg.algorithm != "randomized":
            raise NotImplementedError(
                f"algorithm={cfg.algorithm!r}: lkpy_amd trains the randomized SVD on the device "
                "and has neither a device Lanczos nor a CPU fallback")
        dev_name = options.configured_device()
        dev = D.device(None if dev_name in ("cuda", "cpu") else dev_name)
        k, l = cfg.embedding_size, cfg.embedding_size + D.SVD_OVERSAMPLES
        if k < 1 or l > min(data.user_count, data.item_count):
            raise ValueError(f"embedding_size + {D.SVD_OVERSAMPLES} = {l} sketch columns need at "
                             f"least that many users and items, got {data.user_count} x "
                             f"{data.item_count}")
        bias = BiasModel.learn(data, cfg.damping, device=dev)
        resid = bias.transform_matrix(
            data.interaction_matrix(format="scipy", layout="coo", field="rating")).tocsr()
        resid.sort_indices()
        csr = D.DeviceCSR.from_arrays(resid.indptr, resid.indices,
                                      resid.data.astype(np.float32), resid.shape, dev)
        csr_t = D.csr_transpose(csr)
        omega = self._start_panel
        if omega is None:
            # ``randomized_range_finder``'s own draw: normal(size=(A.shape[1], l)) of the matrix
            # sklearn operates on, whose column count is the smaller dimension
            omega = options.random_generator().normal(size=(min(resid.shape), l))
        sv, components, xt = D.randomized_svd(csr, csr_t, k, cfg.n_iter, omega)
        self.bias = bias
        self.users, self.items = data.users, data.items
        self.user_components = xt
        self.factorization = Factorization(components.T, sv, cfg.n_iter)

    # -- what the shared scoring reads -------------------------------------------------------
    user_embeddings = property(lambda self: self.user_components)
    item_embeddings = property(lambda self: self.factorization.item_factors)
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
