"""
CPU restatement of FlexMF explicit (src/lenskit/flexmf/_explicit.py:58-125, _model.py:145-198,
_training.py:238-252), the yardstick of ``tests/test_flexmf_explicit_host.py`` and
``tests/test_gpu_flexmf_explicit.py``:

* :class:`TorchExplicitTrainer` -- one training step from ``nn.Embedding``, autograd and the
  REAL ``torch.optim.AdamW`` / ``torch.optim.SparseAdam``, in float32 or float64 on request:
  ``mse_loss(pred, r) + reg * mean(b_u^2 + b_i^2 + |p_u| + |q_i|)`` under ``reg_method = "L2"``;
  the step reports the squared error alone;
* :func:`numpy_explicit_gradients` -- the hand-derived gradients in NumPy float64, the formulas
  the kernels of ``csrc/flexmf.hip`` follow;
* :func:`train_explicit_restatement` -- the whole trainer on the CPU, the reference's generator
  order; :func:`predict_rmse` -- the RMSE of tables on held-out ratings.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.nn import functional as F

from flexmf_restatement import TABLES, Model, table_distance  # noqa: F401 (re-exported)


class TorchExplicitTrainer:
    "``FlexMFExplicitTrainer.train_batch`` + ``opt.step()`` on explicit (users, items, ratings)"

    def __init__(self, tabs: dict, *, reg_method="L2", regularization=0.1, learning_rate=0.01,
                 dtype=torch.float32):
        self.reg_method, self.reg, self.dtype = reg_method, regularization, dtype
        self.model = Model(tabs, dtype, sparse=reg_method != "AdamW")
        if reg_method == "AdamW":
            self.opt = torch.optim.AdamW(self.model.parameters(), lr=learning_rate,
                                         weight_decay=regularization)
        else:
            self.opt = torch.optim.SparseAdam(self.model.parameters(), lr=learning_rate)
        # the power check's two deliberate errors
        self.item_weight = 1.0          # 0.5: the implicit step's weight of the item side
        self.report_with_norm = False   # True: the reported loss includes the norm term

    def _parts(self, users, items, ratings):
        "(squared error, norm term) of the batch"
        users = torch.as_tensor(np.asarray(users), dtype=torch.int64)
        items = torch.as_tensor(np.asarray(items), dtype=torch.int64)
        r = torch.as_tensor(np.asarray(ratings)).to(self.dtype)
        l2 = self.reg_method == "L2"
        pred, factor = self.model(users, items, l2)
        mse = F.mse_loss(pred, r)
        if not l2:
            return mse, 0.0
        if self.item_weight != 1.0:
            m = self.model
            bu, bi = m._bias(m.u_bias, users), m._bias(m.i_bias, items)
            factor = bu * bu + m.u_embed(users).norm(dim=-1) + \
                self.item_weight * (bi * bi + m.i_embed(items).norm(dim=-1))
        return mse, self.reg * factor.mean()

    def loss_of(self, users, items, ratings):
        mse, norm = self._parts(users, items, ratings)
        return mse + norm

    def step(self, users, items, ratings) -> float:
        mse, norm = self._parts(users, items, ratings)
        total = mse + norm
        total.backward()
        self.opt.step()
        self.opt.zero_grad()
        return float((total if self.report_with_norm else mse).detach())

    def tables(self) -> dict:
        return {name: getattr(self.model, name.split(".")[0]).weight.detach().numpy().copy()
                for name in TABLES}

    def dense_gradients(self, users, items, ratings) -> dict:
        "autograd's gradient of every table as a dense float64 array (no optimiser step)"
        self.loss_of(users, items, ratings).backward()
        out = {}
        for name in TABLES:
            emb = getattr(self.model, name.split(".")[0])
            g = emb.weight.grad
            out[name] = (g.to_dense() if g.is_sparse else g).double().numpy().copy()
            emb.weight.grad = None
        return out


def numpy_explicit_gradients(tabs: dict, users, items, ratings, *, l2=False, reg=0.1):
    """
    (squared error, objective, {table: dense gradient}).  With pred = b_u + b_i + p_u . q_i and
    g_s = 2 (pred_s - r_s) / B per sample s:  dP[u_s] += g_s q_s,  dQ[i_s] += g_s p_s,
    db_u[u_s] += g_s,  db_i[i_s] += g_s.  The L2 term reg * mean(b_u^2 + b_i^2 + |p_u| + |q_i|)
    adds, per occurrence, reg x / (B |x|) to an embedding row (0 where |x| = 0) and 2 reg b / B
    to a bias -- the same on both sides.
    """
    P = np.asarray(tabs["u_embed.weight"], np.float64)
    Q = np.asarray(tabs["i_embed.weight"], np.float64)
    bu = np.asarray(tabs["u_bias.weight"], np.float64).reshape(-1)
    bi = np.asarray(tabs["i_bias.weight"], np.float64).reshape(-1)
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    r = np.asarray(ratings, np.float64)
    B = len(users)
    diff = bu[users] + bi[items] + np.einsum("bk,bk->b", P[users], Q[items]) - r
    mse = float((diff ** 2).mean())
    g = 2.0 * diff / B
    dP, dQ, dbu, dbi = np.zeros_like(P), np.zeros_like(Q), np.zeros_like(bu), np.zeros_like(bi)
    np.add.at(dP, users, g[:, None] * Q[items])
    np.add.at(dQ, items, g[:, None] * P[users])
    np.add.at(dbu, users, g)
    np.add.at(dbi, items, g)
    total = mse
    if l2:
        pn, qn = np.linalg.norm(P[users], axis=1), np.linalg.norm(Q[items], axis=1)
        total += reg * float((bu[users] ** 2 + bi[items] ** 2 + pn + qn).mean())

        def unit(x, nrm):
            return np.divide(x, nrm[:, None], out=np.zeros_like(x), where=nrm[:, None] > 0)

        np.add.at(dP, users, reg / B * unit(P[users], pn))
        np.add.at(dQ, items, reg / B * unit(Q[items], qn))
        np.add.at(dbu, users, 2.0 * reg / B * bu[users])
        np.add.at(dbi, items, 2.0 * reg / B * bi[items])
    grads = {"u_embed.weight": dP, "i_embed.weight": dQ, "u_bias.weight": dbu.reshape(-1, 1),
             "i_bias.weight": dbi.reshape(-1, 1)}
    return mse, total, grads


def train_explicit_restatement(ds, config, seed: int, dtype=torch.float32,
                               batch_losses: list | None = None):
    """``FlexMFExplicitScorer.train`` on the CPU: the reference's seeding (NumPy generator, then
    Torch's), its initialisation, the float32 mean and centred ratings, a permutation per epoch,
    the Torch step.  Returns (tables, global bias); ``batch_losses`` collects one list of batch
    losses per epoch."""
    from lkpy_amd.flexmf import initial_tables
    from lkpy_amd.training import TrainingOptions

    opts = TrainingOptions(rng=seed)
    rng = opts.random_generator()
    gen = opts.random_generator(type="torch")
    values = torch.from_numpy(np.ascontiguousarray(ds._attrs["rating"], dtype=np.float32))
    mean = values.mean()
    centred = (values - mean).numpy()
    tabs = initial_tables(ds.user_count, ds.item_count, config.embedding_size, gen,
                          user_bias=True, item_bias=True, user_counts=np.diff(ds._indptr),
                          item_counts=np.bincount(ds._cols, minlength=ds.item_count))
    tr = TorchExplicitTrainer(tabs, reg_method=config.reg_method,
                              regularization=config.regularization,
                              learning_rate=config.learning_rate, dtype=dtype)
    for _ in range(config.epochs):
        perm = rng.permutation(len(ds._rows))
        losses = []
        for start in range(0, len(perm), config.batch_size):
            sel = perm[start:start + config.batch_size]
            losses.append(tr.step(ds._rows[sel], ds._cols[sel], centred[sel]))
        if batch_losses is not None:
            batch_losses.append(losses)
    return tr.tables(), mean.item()


def predict_rmse(tabs: dict, global_bias: float, train, test) -> float:
    """Root of the mean squared error over every held-out (user, item, rating) of ``test`` (an
    ``ItemListCollection`` keyed by user) whose user and item the training set knows."""
    P, Q = tabs["u_embed.weight"].astype(np.float64), tabs["i_embed.weight"].astype(np.float64)
    bu, bi = tabs["u_bias.weight"].reshape(-1), tabs["i_bias.weight"].reshape(-1)
    errs = []
    for key, truth in test:
        u = train.users.number(key.user_id, missing=None)
        nums = truth.numbers(vocabulary=train.items, missing="negative")
        ok = nums >= 0
        if u is None or not ok.any():
            continue
        pred = global_bias + bu[u] + bi[nums[ok]] + Q[nums[ok]] @ P[u]
        errs.append(pred - np.asarray(truth.field("rating"), np.float64)[ok])
    return float(np.sqrt(np.mean(np.concatenate(errs) ** 2)))
