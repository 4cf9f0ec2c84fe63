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
column is set per query (:class:`lkpy_amd._factor_scoring.QueryUserBias`).
"""

from __future__ import annotations

from typing import Literal

import numpy as np
from pydantic import AliasChoices, BaseModel, Field

from .. import _device as D
from .._factor_scoring import GlobalBiasPairScoring, QueryUserBias
from ..als import _scorer_state
from ..basic import BiasModel
from ..data import Dataset, Vocabulary
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


class BiasedSVDScorer(QueryUserBias, GlobalBiasPairScoring, Component, Trainable):
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
