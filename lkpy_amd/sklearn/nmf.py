"""
Non-negative matrix factorization for implicit feedback: mirror of
``lenskit.sklearn.nmf.NMFScorer`` / ``NMFConfig`` (src/lenskit/sklearn/nmf.py:32-135) -- the
user x item indicator matrix X factored as ``W H`` with no negative entry,
``score = user_components[u] . item_components[i]``.

The reference hands X to ``sklearn.decomposition.non_negative_factorization``, which with the
reference's options is the NNDSVDA start (from a randomized SVD) followed by Frobenius coordinate
descent, all in float32 because X arrives as float32.  Here the SVD runs on the device
(:func:`lkpy_amd._device.randomized_svd`), NNDSVDA -- once per fit, O((users + items) k) -- on the
host in float32 NumPy, line for line with sklearn's ``_initialize_nmf``, and the descent on the
device (:func:`lkpy_amd._device.nmf_fit`: ``lk_gramian``, ``lk_csr_spmm``, ``lk_nmf_cd_sweep``),
whose sweep has the bits of sklearn's.  ``method="minibatch"`` validates, and ``train`` raises
``NotImplementedError``; a ``beta_loss`` other than ``"frobenius"`` is a ``ValueError``, as it is
for sklearn's ``cd`` solver.

The trained model is a factor model without biases, so it scores through
:class:`lkpy_amd._factor_scoring.BiasedFactorScoring` like ``HPFScorer``.
"""

from __future__ import annotations

import logging
from math import sqrt
from typing import Literal

import numpy as np
from pydantic import AliasChoices, BaseModel, Field, PositiveInt

from .. import _device as D
from .._factor_scoring import BiasedFactorScoring
from .._queries import item_scores, pack_targets, user_numbers
from ..als import _scorer_state
from ..data import Dataset, ItemList, RecQuery, Vocabulary
from ..pipeline import Component
from ..training import Trainable, TrainingOptions

_log = logging.getLogger(__name__)

TOL = 1e-4  # sklearn's default ``tol``, which the reference does not expose
EPS = 1e-6  # ``_initialize_nmf``'s ``eps``


class NMFConfig(BaseModel, extra="forbid"):
    "``NMFConfig`` (nmf.py:32-48; ``embedding_size_exp`` is ``EmbeddingSizeMixin``'s)."

    beta_loss: Literal["frobenius", "kullback-leibler", "itakura-saito"] = "frobenius"
    max_iter: PositiveInt = Field(default=200, validation_alias=AliasChoices("max_iter", "epochs"))
    embedding_size: PositiveInt | None = Field(
        default=64, validation_alias=AliasChoices("embedding_size", "n_components"))
    embedding_size_exp: int | None = None
    alpha_W: float = 0.0
    alpha_H: float | Literal["same"] = "same"
    l1_ratio: float = 0.0
    method: Literal["full", "minibatch"] = "full"

    def model_post_init(self, _ctx):
        if self.embedding_size_exp is not None:
            object.__setattr__(self, "embedding_size", 2 ** int(self.embedding_size_exp))

    def regularization(self, n_users: int, n_items: int):
        "sklearn's ``_compute_regularization``: (l1_W, l1_H, l2_W, l2_H)"
        alpha_h = self.alpha_W if self.alpha_H == "same" else self.alpha_H
        return (n_items * self.alpha_W * self.l1_ratio, n_users * alpha_h * self.l1_ratio,
                n_items * self.alpha_W * (1.0 - self.l1_ratio),
                n_users * alpha_h * (1.0 - self.l1_ratio))


def _norm(x) -> float:
    "sklearn's ``norm``: ``math.sqrt`` of the dot product in the vector's dtype"
    return sqrt(np.dot(x, x))


def nndsvda(U: np.ndarray, S: np.ndarray, V: np.ndarray, avg):
    """
    sklearn's NNDSVDA start (``_initialize_nmf``, ``_nmf.py:318-361``) from the truncated SVD
    ``U`` [n x k], ``S`` [k], ``V`` [k x m] and ``avg = X.mean()``, in their dtype: (W [n x k],
    H [k x m]).  The signs of a component's two vectors do not matter to it.
    """
    W = np.zeros_like(U)
    H = np.zeros_like(V)
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(V[0, :])
    for j in range(1, len(S)):
        x, y = U[:, j], V[j, :]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm = _norm(x_p), _norm(y_p)
        x_n_nrm, y_n_nrm = _norm(x_n), _norm(y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        if m_p > m_n:
            u = x_p / x_p_nrm
            v = y_p / y_p_nrm
            sigma = m_p
        else:
            u = x_n / x_n_nrm
            v = y_n / y_n_nrm
            sigma = m_n
        lbd = np.sqrt(S[j] * sigma)
        W[:, j] = lbd * u
        H[j, :] = lbd * v
    W[W < EPS] = 0
    H[H < EPS] = 0
    W[W == 0] = avg
    H[H == 0] = avg
    return W, H


class NMFScorer(BiasedFactorScoring, Component, Trainable):
    """
    Non-negative matrix factorization of the indicator matrix.  Learned state: ``users``,
    ``items``, ``user_components`` [users x k] and ``item_components`` [items x k] (float32,
    never negative) and ``n_iter_`` (iterations run).

    The start's randomized SVD draws its Gaussian panel from the training options' generator (as
    ``BiasedSVDScorer`` does), so a seeded fit repeats bit for bit; the reference's own call
    passes no ``random_state`` and is not repeatable.
    """

    config: NMFConfig

    users: Vocabulary
    items: Vocabulary
    user_components: np.ndarray
    item_components: np.ndarray
    n_iter_: int

    # test hooks: the stopping tolerance, the Gaussian start panel of the SVD to use instead of
    # drawing one, and the start (W0 [users x k], H0 [k x items]) to use instead of NNDSVDA
    _tol = TOL
    _start_panel = None
    _start_factors = None

    def is_trained(self):
        return hasattr(self, "item_components")

    def __getstate__(self):
        return _scorer_state(self)

    def __setstate__(self, state):
        state = dict(state)
        state.pop("_dev", None)
        self.__dict__.update(state)

    # -- training (nmf.py:72-110) --------------------------------------------------------------
    def _start(self, mat, csr, csr_t, options: TrainingOptions):
        "sklearn's ``_initialize_nmf(init='nndsvda')``: (W0 [users x k], H0 [k x items]) float32"
        k = self.config.embedding_size
        omega = self._start_panel
        if omega is None:
            # ``randomized_range_finder``'s own draw, as BiasedSVDScorer.train makes it
            omega = options.random_generator().normal(
                size=(min(mat.shape), k + D.SVD_OVERSAMPLES))
        n_iter = 7 if k < 0.1 * min(mat.shape) else 4  # sklearn's ``n_iter="auto"``
        sv, components, transformed = D.randomized_svd(csr, csr_t, k, n_iter, omega)
        S = sv.astype(np.float32)
        U = (transformed / S).astype(np.float32)
        return nndsvda(U, S, np.ascontiguousarray(components, dtype=np.float32), mat.mean())

    def train(self, data: Dataset, options: TrainingOptions = TrainingOptions()):
        if self.is_trained() and not options.retrain:
            return
        cfg = self.config
        if cfg.method != "full":
            raise NotImplementedError(
                f"method={cfg.method!r}: lkpy_amd trains NMF by coordinate descent on the device "
                "and has neither a device minibatch solver nor a CPU fallback")
        if cfg.beta_loss != "frobenius":
            raise ValueError(f"beta_loss={cfg.beta_loss!r}: the coordinate descent solver "
                             "minimises the Frobenius loss only")
        k = cfg.embedding_size
        if k is None or k > D.nmf_max_k():
            raise ValueError(f"embedding_size {k} outside 1..lk_nmf_max_k() = {D.nmf_max_k()}")
        dev_name = options.configured_device()
        dev = D.device(None if dev_name in ("cuda", "cpu") else dev_name)
        mat = data.interactions().matrix().scipy(layout="csr").astype(np.float32)
        mat.sort_indices()
        csr = D.DeviceCSR.from_arrays(mat.indptr, mat.indices, mat.data, mat.shape, dev)
        csr_t = D.csr_transpose(csr)
        start = self._start_factors
        if start is None:
            start = self._start(mat, csr, csr_t, options)
        l1_w, l1_h, l2_w, l2_h = cfg.regularization(*mat.shape)
        _log.info("fitting NMF model with %d features", k)
        w, h, n_iter, _ = D.nmf_fit(csr, csr_t, start[0], start[1], cfg.max_iter, self._tol,
                                    l1_w, l1_h, l2_w, l2_h)
        _log.info("trained NMF in %d iterations", n_iter)
        self.users, self.items = data.users, data.items
        self.user_components = w
        self.item_components = np.ascontiguousarray(h.T)
        self.n_iter_ = n_iter

    # -- what the shared scoring reads ---------------------------------------------------------
    user_embeddings = property(lambda self: self.user_components)
    item_embeddings = property(lambda self: self.item_components)
    user_bias = None
    item_bias = None

    # -- scoring (nmf.py:112-135) ------------------------------------------------------------
    def __call__(self, query, items: ItemList) -> ItemList:
        query = RecQuery.create(query)
        u_row = None if query.user_id is None else self.users.number(query.user_id, missing=None)
        if u_row is None:  # nmf.py:120-121: an unknown user cannot be scored
            return ItemList(items, scores=np.nan)
        st = self._device_state()
        u, _ = self._user_rows(np.array([u_row]))
        all_scores = D.score_dense(u, st["Q"], self._score_k)[0].cpu().numpy()
        return ItemList(items, scores=item_scores(items, self.items, all_scores))

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "``__call__`` for many queries: one ``lk_score_dense`` panel, the same rows, the same bits"
        qs = [RecQuery.create(q) for q in queries]
        ptr, nums = pack_targets(item_lists, self.items)
        u, valid = self._user_rows(user_numbers(qs, self.users))
        panel = D.score_dense(u, self._device_state()["Q"], self._score_k).cpu().numpy()
        out = []
        for i, il in enumerate(item_lists):
            tgt = nums[ptr[i]:ptr[i + 1]]
            sc = np.full(len(tgt), np.nan, dtype=np.float32)
            if valid[i]:
                sc[tgt >= 0] = panel[i, tgt[tgt >= 0]]
            out.append(ItemList(il, scores=sc))
        return out
