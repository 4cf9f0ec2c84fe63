"""
FlexMF: mirror of ``lenskit.flexmf.FlexMFImplicitScorer`` / ``FlexMFImplicitConfig`` /
``FlexMFImplicitTrainer`` / ``FlexMFWARPTrainer`` (src/lenskit/flexmf/_base.py:34-164,
_implicit.py:32-415, _model.py, _training.py:39-358) -- matrix factorisation with biases,
``score = b_u + b_i + p_u . q_i``, trained by minibatch Adam on logistic, pairwise (BPR) or WARP
loss with sampled negatives.

The reference runs a batch as a few dozen small Torch launches with two host round trips (the
negative sampler is a host function, the WARP search copies its mask to the host in the loop).
Here a whole epoch is queued on the device: the permutation is uploaded once, negatives are drawn
by a counter-based generator in a kernel, forward / loss gradient / per-row gradient sums /
optimiser update are the kernels of ``csrc/flexmf.hip``, the loss is accumulated on the device and
read once per epoch.  The parameter initialisation is the reference's own (a CPU
``torch.Generator`` seeded the same way), so the same seed starts from the same bits.

FlexMF explicit -- ``FlexMFExplicitScorer`` / ``FlexMFExplicitConfig`` / ``FlexMFExplicitTrainer``
(_explicit.py:25-125) -- is the same model with both biases and a global one,
``score = g + b_u + b_i + p_u . q_i``, trained on squared error against the centred ratings
(``lk_flexmf_step_explicit``); it predicts the ratings of ragged (user, item) lists through
``lk_mf_score_pairs`` instead of forming a row of scores per user.

Not here: the ``lightgcn`` preset (``convolution_layers > 0`` validates, and ``create_trainer``
raises ``NotImplementedError``); the model itself is :class:`lkpy_amd.graphs.lightgcn.LightGCNScorer`.
"""

from __future__ import annotations

from typing import Literal

import numpy as np
import torch
from pydantic import BaseModel, NonNegativeInt, PositiveFloat, PositiveInt, model_validator

from . import _device as D
from . import _native
from ._factor_scoring import BiasedFactorScoring, GlobalBiasPairScoring
from ._queries import item_scores
from .als import _DeviceBacked, _scorer_state
from .data import Dataset, ItemList, RecQuery, Vocabulary
from .pipeline import Component
from .training import ModelTrainer, TrainingOptions, UsesTrainer

WARP_MAX_TRIES = 200  # MAX_TRIES, _implicit.py:26

# What a preset stands for: the values it supplies for keys the caller leaves out.  "logistic"
# is not in the reference's table (_implicit.py:32-46), but its pipelines/flexmf-logistic.toml
# names it; it supplies nothing, because logistic loss is what the defaults already are.
_BIAS_FREE = {"user_bias": False, "item_bias": False}
PRESETS = {
    "logistic": {},
    "bpr": {"loss": "pairwise", **_BIAS_FREE},
    "warp": {"loss": "warp", "negative_strategy": "misranked", **_BIAS_FREE},
    "lightgcn": {"loss": "pairwise", "convolution_layers": 3, **_BIAS_FREE},
}


class FlexMFConfigBase(BaseModel):
    "``FlexMFConfigBase`` (_base.py:34-95): what the implicit and the explicit model share."

    embedding_size: PositiveInt = 64
    embedding_size_exp: PositiveInt | None = None
    batch_size: int = 8 * 1024
    learning_rate: float = 0.01
    epochs: int = 10
    regularization: float = 0.01
    reg_method: Literal["AdamW", "L2"] | None = "AdamW"

    def model_post_init(self, _ctx):
        if self.embedding_size_exp is not None:
            object.__setattr__(self, "embedding_size", 2 ** int(self.embedding_size_exp))
        if self.embedding_size > _native.FLEXMF_MAX_K:
            # fail at configuration time: the training kernels keep a row in at most four
            # registers per lane (scoring, with its bias columns, takes far wider operands)
            raise ValueError(f"embedding_size {self.embedding_size} exceeds the device kernels' "
                             f"limit of {_native.FLEXMF_MAX_K}")
        if self.batch_size < 1:
            raise ValueError("batch_size must be positive")


class FlexMFExplicitConfig(FlexMFConfigBase):
    "``FlexMFExplicitConfig`` (_explicit.py:25-35): stronger regularisation, as an explicit L2 term."

    regularization: float = 0.1
    reg_method: Literal["AdamW", "L2"] | None = "L2"


class FlexMFImplicitConfig(FlexMFConfigBase):
    """
    The fields and defaults of the reference's configuration (_base.py:34-95,
    _implicit.py:49-138), which pipeline files and callers address by name.
    """

    preset: Literal["bpr", "warp", "lightgcn", "logistic"] | None = None
    loss: Literal["logistic", "pairwise", "warp"] = "logistic"
    negative_strategy: Literal["uniform", "popular", "misranked"] | None = None
    negative_count: PositiveInt = 1
    positive_weight: PositiveFloat = 1.0
    user_bias: bool | None = None
    item_bias: bool = True
    convolution_layers: NonNegativeInt = 0

    def selected_negative_strategy(self) -> str:
        "the strategy in force: the configured one, else what the loss implies"
        implied = "misranked" if self.loss == "warp" else "uniform"
        return self.negative_strategy or implied

    def selected_user_bias(self) -> bool:
        "a user bias left unspecified is learned under logistic loss only (_implicit.py:223-228)"
        return self.loss == "logistic" if self.user_bias is None else bool(self.user_bias)

    @model_validator(mode="before")
    @classmethod
    def _fill_from_preset(cls, values):
        if not isinstance(values, dict) or not values.get("preset"):
            return values
        name = values["preset"]
        supplied = PRESETS.get(name)
        if supplied is None:
            raise ValueError(f"preset {name!r} is not one of {sorted(PRESETS)}")
        filled = dict(values)
        for key, default in supplied.items():
            filled.setdefault(key, default)  # a key the caller gave is kept
        return filled

    @model_validator(mode="after")
    def _check_negative_sampling(self):
        strategy = self.selected_negative_strategy()
        if self.loss == "warp" and strategy != "misranked":
            raise ValueError(f"loss 'warp' weights each sample by the search for a misranked "
                             f"negative; negative_strategy={strategy!r} cannot provide that")
        if strategy == "misranked" and self.negative_count != 1:
            raise ValueError(f"the misranked search yields one negative per positive; "
                             f"negative_count={self.negative_count} is not available with it")
        return self


class FlexMFScorerBase(BiasedFactorScoring, UsesTrainer, Component):
    """
    What the FlexMF scorers share (``FlexMFScorerBase``, _base.py:98-164).  Learned state (host
    arrays, refreshed lazily from the device while a trainer is live): ``user_embeddings``
    [users x k], ``item_embeddings`` [items x k], ``user_bias`` [users] | None, ``item_bias``
    [items] | None, ``users``, ``items``.  On the device the biases are extra columns of the two
    operand matrices, so that a score is one inner product: the batched scoring is
    :class:`lkpy_amd._factor_scoring.BiasedFactorScoring`.
    """

    users: Vocabulary
    items: Vocabulary
    user_embeddings = _DeviceBacked()
    item_embeddings = _DeviceBacked()
    user_bias = _DeviceBacked()
    item_bias = _DeviceBacked()

    def __getstate__(self):
        return _scorer_state(self)

    def __setstate__(self, state):
        state = dict(state)
        state.pop("_dev", None)
        state.pop("_pending_sync", None)
        self.__dict__.update(state)


class FlexMFImplicitScorer(FlexMFScorerBase):
    "Implicit-feedback FlexMF: ``score = b_u + b_i + p_u . q_i``, either bias optional."

    config: FlexMFImplicitConfig

    def create_trainer(self, data, options):
        if self.config.convolution_layers > 0:
            raise NotImplementedError(
                "LightGCN (convolution_layers > 0) has no device trainer in lkpy_amd")
        if self.config.selected_negative_strategy() == "misranked":
            return FlexMFWARPTrainer(self, data, options)
        return FlexMFImplicitTrainer(self, data, options)

    # -- scoring (_base.py:116-164) -------------------------------------------------------
    def __call__(self, query, items: ItemList) -> ItemList:
        query = RecQuery.create(query)
        u_row = None if query.user_id is None else self.users.number(query.user_id, missing=None)
        if u_row is None:  # no fold-in from a history: an unknown user cannot be scored
            return ItemList(items, scores=np.nan)
        st = self._device_state()
        u, _ = self._user_rows(np.array([u_row]))
        all_scores = D.score_dense(u, st["Q"], self._score_k)[0].cpu().numpy()
        return ItemList(items, scores=item_scores(items, self.items, all_scores))


class FlexMFExplicitScorer(GlobalBiasPairScoring, FlexMFScorerBase):
    """
    Explicit-feedback FlexMF (_explicit.py:38-55): ``score = g + b_u + b_i + p_u . q_i`` with the
    global bias ``g`` = the float32 mean of the training ratings.  Ratings are predicted for
    ragged (user, item) lists by ``lk_mf_score_pairs``
    (:class:`lkpy_amd._factor_scoring.GlobalBiasPairScoring`): ``__call__`` is ``score_batch``
    with one query, so the two agree bit for bit.
    """

    config: FlexMFExplicitConfig
    global_bias: float

    def create_trainer(self, data, options):
        return FlexMFExplicitTrainer(self, data, options)


def initial_tables(n_users: int, n_items: int, k: int, gen: torch.Generator, *, user_bias: bool,
                   item_bias: bool, user_counts=None, item_counts=None) -> dict:
    """
    ``FlexMFModel.__init__`` + ``zero_users`` / ``zero_items`` (_model.py:73-120,
    _training.py:108-112) on the host: ``normal_(std=0.1)`` from the CPU generator into u_bias,
    i_bias, u_embed, i_embed in that order (present tables only), then the rows of users and
    items without a training interaction zeroed.  Keys are Torch's ``state_dict`` names.
    """
    shapes = [("u_bias.weight", (n_users, 1), user_bias), ("i_bias.weight", (n_items, 1), item_bias),
              ("u_embed.weight", (n_users, k), True), ("i_embed.weight", (n_items, k), True)]
    out = {}
    for name, shape, present in shapes:
        out[name] = torch.empty(shape, dtype=torch.float32).normal_(0.0, 0.1, generator=gen) \
            .numpy() if present else None
    for names, counts in ((("u_bias.weight", "u_embed.weight"), user_counts),
                          (("i_bias.weight", "i_embed.weight"), item_counts)):
        if counts is not None:
            for name in names:
                if out[name] is not None:
                    out[name][np.asarray(counts) == 0] = 0.0
    return out


class FlexMFTrainerBase(ModelTrainer):
    """
    ``FlexMFTrainerBase`` (_training.py:39-258): seeding, initialisation and the epoch loop on the
    device.  A subclass says which biases the model has, builds its ``FlexMFState``, uploads what
    its samples carry (``prepare_data``) and queues one batch (``train_batch``).
    """

    def __init__(self, scorer, data: Dataset, options: TrainingOptions):
        self.scorer = scorer
        self.config = scorer.config
        self.check_data(data)
        # the NumPy generator first, then Torch's (_training.py:102-103): with a Generator as the
        # seed the Torch seed is that generator's next draw
        self.rng = options.random_generator()
        self.torch_rng = options.random_generator(type="torch")
        dev_name = options.configured_device()
        self.dev = dev = D.device(None if dev_name in ("cuda", "cpu") else dev_name)

        scorer.users, scorer.items = data.users, data.items
        self.matrix = data.interactions().matrix()
        ds = self.matrix._ds
        self.n_users, self.n_items = data.user_count, data.item_count
        self.n_samples = ds.interaction_count  # repeated pairs stay separate samples
        tabs = self.initial_parameters(ds)
        self.state = self.create_state(tabs)
        self.d_users = torch.from_numpy(ds._rows).to(dev)
        self.d_items = torch.from_numpy(ds._cols).to(dev)
        self.prepare_data(ds)
        self.epochs_trained = 0
        self._set_host(tabs)

    def check_data(self, data: Dataset) -> None:
        "what the model needs of the data, said before any device work"

    def initial_parameters(self, ds):
        "the model's parameters as drawn from ``torch_rng``: what ``create_state`` uploads"
        user_bias, item_bias = self.model_biases()
        return initial_tables(
            self.n_users, self.n_items, self.config.embedding_size, self.torch_rng,
            user_bias=user_bias, item_bias=item_bias,
            user_counts=np.diff(ds._indptr), item_counts=np.bincount(ds._cols,
                                                                     minlength=self.n_items))

    def _set_host(self, tabs: dict):
        s = self.scorer
        s.__dict__.pop("_pending_sync", None)
        s.user_embeddings, s.item_embeddings = tabs["u_embed.weight"], tabs["i_embed.weight"]
        ub, ib = tabs["u_bias.weight"], tabs["i_bias.weight"]
        s.user_bias = None if ub is None else ub.reshape(-1)
        s.item_bias = None if ib is None else ib.reshape(-1)

    def train_epoch(self) -> dict[str, float]:
        bs = self.config.batch_size
        perm = np.require(self.rng.permutation(self.n_samples), dtype=np.int32)
        d_perm = torch.from_numpy(perm).to(self.dev)  # one upload per epoch
        loss_sum = torch.zeros(1, dtype=torch.float32, device=self.dev)
        batches = 0
        for start in range(0, self.n_samples, bs):
            self.train_batch(d_perm[start:start + bs], batches, loss_sum)
            batches += 1
        self.epochs_trained += 1
        # the tables stay in HBM; the host copies are refreshed on first read (_DeviceBacked)
        self.scorer.__dict__["_pending_sync"] = self._sync
        avg = float(loss_sum.item()) / max(batches, 1)  # the epoch's one synchronisation
        return {"loss": avg}

    def _sync(self):
        self._set_host(self.state.host_tables())

    def finalize(self):
        self._sync()

    def get_parameters(self):
        return {k: v for k, v in self.state.host_tables().items() if v is not None}

    def load_parameters(self, state) -> None:
        self.state.load_tables(state)
        self.scorer.__dict__["_pending_sync"] = self._sync


class FlexMFImplicitTrainer(FlexMFTrainerBase):
    "``FlexMFImplicitTrainer`` (_implicit.py:164-290)."

    def model_biases(self):
        return self.config.selected_user_bias(), self.config.item_bias

    def create_state(self, tabs: dict):
        cfg = self.config
        return D.FlexMFState(
            tabs["u_embed.weight"], tabs["i_embed.weight"], tabs["u_bias.weight"],
            tabs["i_bias.weight"], loss=cfg.loss, reg_method=cfg.reg_method,
            regularization=cfg.regularization, learning_rate=cfg.learning_rate,
            negative_count=cfg.negative_count, positive_weight=cfg.positive_weight, dev=self.dev)

    def prepare_data(self, ds) -> None:
        self.d_indptr, self.d_cols = self.matrix._device_csr(self.dev)
        # the key of the negative sampler's counter-based stream
        self.sample_key = int(self.rng.bit_generator.random_raw())

    def negatives(self, users: torch.Tensor, positives: torch.Tensor, counter: int):
        "``scored_negatives`` (_implicit.py:276-290): (negatives [B x n], no weights)."
        cfg = self.config
        neg = D.flexmf_sample_negatives(self.d_indptr, self.d_cols, self.n_items, users,
                                        cfg.negative_count, cfg.selected_negative_strategy(),
                                        self.sample_key, counter)
        return neg, None

    def train_batch(self, d_sel: torch.Tensor, batch: int, loss_sum: torch.Tensor) -> None:
        users, items = D.flexmf_gather_batch(d_sel, self.d_users, self.d_items)
        neg, weights = self.negatives(users, items, (self.epochs_trained << 32) | batch)
        self.state.step(users, items, neg, weights, loss_sum=loss_sum, check_indices=False)


def centred_ratings(data: Dataset):
    """
    (global bias, ratings minus it) as the reference's ``prepare_data`` computes them
    (_explicit.py:65-79): the float32 mean by Torch's CPU reduction, as a Python float, and the
    float32 differences, in the order of the interactions (row-major COO).
    """
    ratings = data.interactions().matrix()._ds._attrs.get("rating")
    if ratings is None:
        raise ValueError("FlexMF explicit trains on the interactions' 'rating' field, which this "
                         "dataset does not have")
    values = torch.from_numpy(np.ascontiguousarray(ratings, dtype=np.float32))
    mean = values.mean()
    return mean.item(), (values - mean).numpy()


class FlexMFExplicitTrainer(FlexMFTrainerBase):
    """
    ``FlexMFExplicitTrainer`` (_explicit.py:58-125): every interaction with its centred rating is
    a sample, both biases are learned, a batch is one ``lk_flexmf_step_explicit``; the epoch's
    reported loss is the mean of the batches' mean squared errors.
    """

    def check_data(self, data: Dataset) -> None:
        self.scorer.global_bias, self._centred = centred_ratings(data)

    def model_biases(self):
        return True, True

    def create_state(self, tabs: dict):
        cfg = self.config
        return D.FlexMFState(
            tabs["u_embed.weight"], tabs["i_embed.weight"], tabs["u_bias.weight"],
            tabs["i_bias.weight"], loss="mse", reg_method=cfg.reg_method,
            regularization=cfg.regularization, learning_rate=cfg.learning_rate, dev=self.dev)

    def prepare_data(self, ds) -> None:
        self.d_ratings = torch.from_numpy(self._centred).to(self.dev)
        del self._centred

    def train_batch(self, d_sel: torch.Tensor, batch: int, loss_sum: torch.Tensor) -> None:
        users, items = D.flexmf_gather_batch(d_sel, self.d_users, self.d_items)
        ratings = D.flexmf_gather_values(d_sel, self.d_ratings)
        self.state.step_explicit(users, items, ratings, loss_sum=loss_sum, check_indices=False)


class FlexMFWARPTrainer(FlexMFImplicitTrainer):
    """
    ``FlexMFWARPTrainer`` (_implicit.py:293-396).  The reference draws candidates ten at a time
    for the rows still searching; candidates are independent draws, so the table of all
    ``WARP_MAX_TRIES`` per sample drawn up front has the same distribution, and the search is a
    deterministic function of it that scores only up to the stopping try.
    """

    def negatives(self, users, positives, counter):
        cand = D.flexmf_sample_negatives(self.d_indptr, self.d_cols, self.n_items, users,
                                         WARP_MAX_TRIES, "uniform", self.sample_key, counter)
        neg, _count, weights = self.state.warp_search(users, positives, cand,
                                                      check_indices=False)
        # the losses that ignore the weights but ask for misranked negatives take them here too
        return neg, (weights if self.config.loss == "warp" else None)
