"""
LightGCN: mirror of ``lenskit.graphs.lightgcn.LightGCNScorer`` / ``LightGCNConfig`` /
``LightGCNTrainer`` (src/lenskit/graphs/lightgcn.py:42-324) -- collaborative filtering by light
graph convolution over the bipartite interaction graph.

The reference delegates the model's arithmetic to an external graph library; the reference tree
states the same model in ``FlexMFModel.update_convolution`` / ``forward``
(src/lenskit/flexmf/_model.py:122-198), and that statement is what runs here:

* n_i items and n_u users are N = n_i + n_u nodes, items first (the reference's
  ``user_base = item_count``); M is the symmetric N x N adjacency of the training matrix's
  structure with unit values; d = deg^-1/2 (0 for a node without entries); M^ = diag(d) M diag(d).
* One float32 table X [N x k]; x~ = sum_{l=0..L} alpha_l M^^l X with L = ``layer_count``;
  ``score(u, i) = x~_u . x~_i``, no biases.
* ``layer_blend=None``: alpha_l = 1 / (L + 1); a scalar ``a``: alpha_l = a for every l.  A list
  validates as the reference validates it (length ``layer_count``), and ``create_trainer`` then
  raises ``NotImplementedError``: L + 1 terms are blended, so a list of L weights does not say
  what the blend is.
* Losses over one uniform negative per positive, redrawn while it is a training item:
  ``pairwise`` = mean -log sigmoid(s+ - s-), ``logistic`` = (sum -log sigmoid(s+) +
  sum -log sigmoid(-s-)) / 2B.  Whatever further terms the external library's loss methods add
  are not reproduced; the regulariser is AdamW's decoupled weight decay = ``regularization``
  (``None``: no decay, which is Adam).
* Every row of X is updated every step, as ``torch.optim.AdamW`` does with a dense gradient.

A step runs on the device (``csrc/lightgcn.hip`` through :class:`lkpy_amd._device.LightGCNState`);
the epoch loop is FlexMF's: the permutation uploaded once per epoch, batches gathered and
negatives drawn by kernels, the loss accumulated on the device and read once per epoch.  The
trained scorer keeps the propagated embeddings x~, split into ``item_embeddings`` and
``user_embeddings``, and scores with them like a bias-free FlexMF.
"""

from __future__ import annotations

from typing import Literal

import numpy as np
import torch
from pydantic import BaseModel, PositiveFloat, PositiveInt, model_validator

from .. import _device as D
from .. import _native
from .._queries import item_scores, user_numbers
from ..data import Dataset, ItemList, RecQuery
from ..flexmf import FlexMFScorerBase, FlexMFTrainerBase


class LightGCNConfig(BaseModel):
    "``LightGCNConfig`` (lightgcn.py:42-105; ``embedding_size_exp`` is ``EmbeddingSizeMixin``'s)."

    embedding_size: PositiveInt = 16
    embedding_size_exp: PositiveInt | None = None
    layer_count: PositiveInt = 2
    layer_blend: PositiveFloat | list[PositiveFloat] | None = None
    batch_size: PositiveInt = 4 * 1024
    learning_rate: PositiveFloat = 0.01
    epochs: PositiveInt = 10
    regularization: PositiveFloat | None = 0.01
    loss: Literal["logistic", "pairwise"] = "pairwise"

    def model_post_init(self, _ctx):
        if self.embedding_size_exp is not None:
            object.__setattr__(self, "embedding_size", 2 ** int(self.embedding_size_exp))
        if self.embedding_size > _native.FLEXMF_MAX_K:
            # fail at configuration time: the training kernels keep a row in at most four
            # registers per lane
            raise ValueError(f"embedding_size {self.embedding_size} exceeds the device kernels' "
                             f"limit of {_native.FLEXMF_MAX_K}")

    @model_validator(mode="after")
    def check_layer_blending(self):
        if isinstance(self.layer_blend, list) and len(self.layer_blend) != self.layer_count:
            raise ValueError(f"layer_blend has length {len(self.layer_blend)}, expected "
                             f"{self.layer_count}")
        return self

    def blend_weights(self) -> list[float]:
        "alpha_0 .. alpha_L (a list of L weights has no defined meaning: ``NotImplementedError``)"
        L = self.layer_count
        if isinstance(self.layer_blend, list):
            raise NotImplementedError(
                f"layer_blend given as a list of {L} weights: {L + 1} terms (the embeddings and "
                f"{L} layers) are blended, so the list does not say what the blend is; give "
                "layer_blend as one number or leave it out")
        a = 1.0 / (L + 1) if self.layer_blend is None else float(self.layer_blend)
        return [a] * (L + 1)


def graph_adjacency(indptr, cols, n_users: int, n_items: int, transpose=None):
    """
    The interaction graph of a training matrix (users x items CSR ``indptr`` / ``cols``):
    (offsets int64 [N + 1], columns int32 [2 nnz], d float32 [N]) of the symmetric adjacency M
    over N = n_items + n_users nodes, items first.  An item's row lists its users' nodes in
    ascending user order, a user's row its items in the matrix's entry order; d = deg^-1/2 with
    deg the stored entries of the node's row, 0 where there are none.  ``transpose``: the
    (offsets, rows) of the items x users transpose when the caller has it (``lk_csr_transpose``);
    otherwise it is formed here by a stable sort.
    """
    indptr = np.asarray(indptr, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int32)
    if transpose is None:
        rows = np.repeat(np.arange(n_users, dtype=np.int32), np.diff(indptr))
        order = np.argsort(cols, kind="stable")
        t_rows = rows[order]
        t_ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n_items))])
    else:
        t_ptr, t_rows = (np.asarray(a) for a in transpose)
    t_ptr = t_ptr.astype(np.int64)
    m_ptr = np.concatenate([t_ptr, t_ptr[-1] + indptr[1:]])
    m_cols = np.concatenate([t_rows.astype(np.int32) + np.int32(n_items), cols])
    deg = np.diff(m_ptr)
    d = np.zeros(len(deg), dtype=np.float32)
    d[deg > 0] = (1.0 / np.sqrt(deg[deg > 0].astype(np.float64))).astype(np.float32)
    return m_ptr, m_cols, d


def initial_table(n_users: int, n_items: int, k: int, gen: torch.Generator, degrees=None):
    """
    X [N x k]: ``normal_(std=0.1)`` from the CPU generator, the item rows drawn first, then the
    user rows (as ``lkpy_amd.flexmf.initial_tables`` draws a table); the rows of nodes without an
    entry (``degrees`` [N] == 0) zeroed.
    """
    parts = [torch.empty((n, k), dtype=torch.float32).normal_(0.0, 0.1, generator=gen).numpy()
             for n in (n_items, n_users)]
    table = np.concatenate(parts)
    if degrees is not None:
        table[np.asarray(degrees) == 0] = 0.0
    return table


class LightGCNScorer(FlexMFScorerBase):
    """
    LightGCN scorer.  Learned state (host arrays, refreshed lazily from the device while a
    trainer is live, from its construction on): ``user_embeddings`` [users x k] and
    ``item_embeddings`` [items x k] -- the PROPAGATED, blended embeddings x~, so that a score is
    one inner product -- ``users``, ``items``; ``user_bias`` and ``item_bias`` stay ``None``.
    State handling and scoring are :class:`lkpy_amd.flexmf.FlexMFScorerBase`'s
    (:class:`lkpy_amd._factor_scoring.BiasedFactorScoring` without biases); ``__call__`` is
    ``score_batch`` with one query, so the two agree bit for bit, and both read rows of the dense
    panel ``recommend_batch`` ranks.
    """

    config: LightGCNConfig

    def create_trainer(self, data, options):
        return LightGCNTrainer(self, data, options)

    def score_batch(self, queries, item_lists) -> list[ItemList]:
        "``__call__`` for many queries: one dense panel, NaN for unknown users and items."
        qs = [RecQuery.create(q) for q in queries]
        if not qs:
            return []
        u, valid = self._user_rows(user_numbers(qs, self.users))
        panel = D.score_dense(u, self._device_state()["Q"], self._score_k)
        D.blank_panel_rows(panel, valid)
        host = D.to_host(panel)
        return [ItemList(il, scores=item_scores(il, self.items, host[i]))
                for i, il in enumerate(item_lists)]

    def __call__(self, query, items: ItemList) -> ItemList:
        return self.score_batch([query], [items])[0]


class LightGCNTrainer(FlexMFTrainerBase):
    """
    ``LightGCNTrainer`` (lightgcn.py:186-324) on :class:`lkpy_amd.flexmf.FlexMFTrainerBase`: its
    seeding, device set-up and epoch loop, with the graph, the one embedding table and the
    LightGCN step as the model's own parts.  The step is not captured into a graph.
    """

    def __init__(self, scorer, data: Dataset, options):
        super().__init__(scorer, data, options)
        # what the base stored is the raw table X: the scorer's arrays are the propagated x~,
        # formed on the device when they are first read
        scorer.__dict__["_pending_sync"] = self._sync

    def check_data(self, data: Dataset) -> None:
        self.blend = self.config.blend_weights()  # (a list of weights: NotImplementedError)

    def initial_parameters(self, ds):
        "the graph (once per fit: the transpose is the device's) and the table X [N x k]"
        d_indptr, d_cols = self.matrix._device_csr(self.dev)
        csr = D.DeviceCSR(d_indptr, d_cols, None, (self.n_users, self.n_items), None)
        csr_t = D.csr_transpose(csr, with_values=False)
        self.graph = graph_adjacency(
            ds._indptr, ds._cols, self.n_users, self.n_items,
            transpose=(csr_t.indptr.cpu().numpy(), csr_t.indices.cpu().numpy()))
        return initial_table(self.n_users, self.n_items, self.config.embedding_size,
                             self.torch_rng, degrees=np.diff(self.graph[0]))

    def create_state(self, table):
        cfg = self.config
        m_ptr, m_cols, scale = self.graph
        del self.graph
        return D.LightGCNState(table, m_ptr, m_cols, scale, self.blend, loss=cfg.loss,
                               regularization=cfg.regularization,
                               learning_rate=cfg.learning_rate, dev=self.dev)

    def prepare_data(self, ds) -> None:
        # samples as node numbers (``d_users`` is overwritten: the base's holds user numbers);
        # the sampler's CSR addressed by node: the items' rows in front are empty
        dev = self.dev
        self.d_users = torch.from_numpy(ds._rows.astype(np.int32) + np.int32(self.n_items)).to(dev)
        d_indptr, self.d_cols = self.matrix._device_csr(dev)
        self.d_node_indptr = torch.cat([torch.zeros(self.n_items, dtype=torch.int64, device=dev),
                                        d_indptr.to(torch.int64)])
        self.sample_key = int(self.rng.bit_generator.random_raw())

    def _set_host(self, embeddings: np.ndarray):
        s = self.scorer
        s.__dict__.pop("_pending_sync", None)
        s.item_embeddings = np.ascontiguousarray(embeddings[:self.n_items])
        s.user_embeddings = np.ascontiguousarray(embeddings[self.n_items:])

    def batch_nodes(self, d_sel: torch.Tensor, batch: int):
        "(users, positives, negatives) of one batch as node numbers, on the device"
        users, items = D.flexmf_gather_batch(d_sel, self.d_users, self.d_items)
        neg = D.flexmf_sample_negatives(self.d_node_indptr, self.d_cols, self.n_items, users, 1,
                                        "uniform", self.sample_key,
                                        (self.epochs_trained << 32) | batch)
        return users, items, neg.reshape(-1)

    def train_batch(self, d_sel: torch.Tensor, batch: int, loss_sum: torch.Tensor) -> None:
        users, items, neg = self.batch_nodes(d_sel, batch)
        self.state.step(users, items, neg, loss_sum=loss_sum, check_indices=False)

    def _sync(self):
        self._set_host(self.state.final_embeddings())

    def get_parameters(self):
        return {"embedding.weight": self.state.host_table()}

    def load_parameters(self, state) -> None:
        self.state.load_table(state["embedding.weight"])
        self.scorer.__dict__["_pending_sync"] = self._sync
