"""
FunkSVD (biased matrix factorisation by featurewise stochastic gradient descent): mirror of
``lenskit.funksvd.FunkSVDScorer`` / ``FunkSVDConfig`` (src/lenskit/funksvd.py:34-222),
``score = g + b_i + b_u + user_embeddings[u] . item_embeddings[i]``.

The reference trains one feature after the other, each by ``epochs`` sequential passes over the
shuffled ratings (``FunkSVDTrainer.feature_epoch``, src/accel/funksvd.rs).  A sample touches only
its user's and its item's entry of the feature, so the pass is a DAG and runs level by level on
the device (:func:`lkpy_amd._device.funksvd_fit`: ``lk_funksvd_plan_levels``,
``lk_funksvd_plan_order``, ``lk_funksvd_train_feature``) with the bits of the sequential pass:
the same seed and the same rating order give the reference's embeddings exactly.  Only the logged
training RMSE is summed in another order.

The trained model is a factor model with the biases of a ``BiasModel``, so it scores through
:class:`lkpy_amd._factor_scoring.GlobalBiasPairScoring` with the per-query user bias of
:class:`lkpy_amd._factor_scoring.QueryUserBias`, as ``BiasedSVDScorer`` does.  Scores are not
clamped to ``range``, as in the reference.
"""

from __future__ import annotations

import logging

import numpy as np
from pydantic import AliasChoices, BaseModel, Field, NonNegativeFloat, PositiveFloat, PositiveInt

from . import _device as D
from ._factor_scoring import GlobalBiasPairScoring, QueryUserBias
from .als import _scorer_state
from .basic import BiasModel
from .data import Dataset, Vocabulary
from .pipeline import Component
from .training import Trainable, TrainingOptions

_log = logging.getLogger(__name__)

INITIAL_VALUE = 0.1


class FunkSVDConfig(BaseModel):
    """``FunkSVDConfig`` (funksvd.py:34-62; ``embedding_size_exp`` is ``EmbeddingSizeMixin``'s).
    Keys it does not know are ignored, as the reference's model ignores them."""

    embedding_size: PositiveInt = Field(
        default=64, validation_alias=AliasChoices("embedding_size", "features"))
    embedding_size_exp: int | None = None
    epochs: PositiveInt = 100
    learning_rate: PositiveFloat = 0.001
    regularization: NonNegativeFloat = 0.015
    damping: float | tuple[float, float] | dict[str, float] = 5.0
    range: tuple[float, float] | None = None

    def model_post_init(self, _ctx):
        if self.embedding_size_exp is not None:
            object.__setattr__(self, "embedding_size", 2 ** int(self.embedding_size_exp))


class FunkSVDScorer(QueryUserBias, GlobalBiasPairScoring, Component, Trainable):
    """
    FunkSVD explicit-feedback matrix factorisation.  Learned state: ``bias``
    (:class:`BiasModel`), ``users``, ``items``, ``user_embeddings`` [users x k] and
    ``item_embeddings`` [items x k] (float32) and ``training_rmse_`` [k x epochs] (float64: the
    training RMSE the reference logs after every epoch of every feature).
    """

    config: FunkSVDConfig

    bias: BiasModel
    users: Vocabulary
    items: Vocabulary
    user_embeddings: np.ndarray
    item_embeddings: np.ndarray
    training_rmse_: np.ndarray

    # test hooks: the sample order to use instead of shuffling, the feature columns kept in
    # global memory at any size, and the sample-steps one launch may hold
    _order = None
    _global_columns = False
    _step_budget = None

    def is_trained(self):
        return hasattr(self, "item_embeddings")

    def __getstate__(self):
        return _scorer_state(self)

    def __setstate__(self, state):
        state = dict(state)
        state.pop("_dev", None)
        self.__dict__.update(state)

    # -- training (funksvd.py:111-197) -----------------------------------------------------------
    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        if self.is_trained() and not options.retrain:
            return
        cfg = self.config
        dev_name = options.configured_device()
        dev = D.device(None if dev_name in ("cuda", "cpu") else dev_name)
        rmat = data.interaction_matrix(format="scipy", layout="coo", field="rating")
        n_users, n_items = rmat.shape
        n_ratings = rmat.nnz
        bias = BiasModel.learn(data, cfg.damping, device=dev)

        shuf = self._order
        if shuf is None:
            shuf = np.arange(n_ratings, dtype=np.int_)
            options.random_generator().shuffle(shuf)
        users = np.asarray(rmat.row[shuf], dtype=np.int32)
        items = np.asarray(rmat.col[shuf], dtype=np.int32)
        ratings = np.asarray(rmat.data[shuf], dtype=np.float32)

        est = np.full(n_ratings, bias.global_bias, dtype=np.float32)
        if bias.item_biases is not None:
            est += bias.item_biases[items]
        if bias.user_biases is not None:
            est += bias.user_biases[users]

        rmin, rmax = cfg.range if cfg.range is not None else (-np.inf, np.inf)
        _log.info("training FunkSVD: %d features, %d epochs each, %d ratings", cfg.embedding_size,
                  cfg.epochs, n_ratings)
        uemb, iemb, rmse = D.funksvd_fit(
            users, items, ratings, est, n_users, n_items, cfg.embedding_size, cfg.epochs,
            cfg.learning_rate, cfg.regularization, rmin, rmax, initial=INITIAL_VALUE, dev=dev,
            global_columns=self._global_columns, step_budget=self._step_budget)
        for f in range(cfg.embedding_size):
            _log.info("finished feature %d (RMSE=%f)", f, rmse[f, -1])

        self.bias = bias
        self.users, self.items = data.users, data.items
        self.user_embeddings = uemb
        self.item_embeddings = iemb
        self.training_rmse_ = rmse

    # -- scoring (funksvd.py:199-222) ------------------------------------------------------------
    def _pair_scores(self, users, items, d_rows, d_ptr, d_nums, tgt_ptr):
        """``__call__`` and every ragged route score by the k-ordered chain of ``lk_score_dense``
        evaluated at the targets (``lk_score_candidates``), which is also the chain of
        ``lk_score_topk``: a list of ``batch.recommend`` has the bits ``pipe.run`` gives the same
        user, over the whole catalogue as over candidate lists."""
        return D.score_candidates(users, items, self._score_k, d_rows, d_ptr, d_nums, tgt_ptr)
