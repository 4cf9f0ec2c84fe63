"""
CPU restatement of LightGCN as ``lkpy_amd.graphs.lightgcn`` states it (the model of
``FlexMFModel.update_convolution`` / ``forward``, src/lenskit/flexmf/_model.py:122-198, with the
symmetric normalisation of the LightGCN paper), the yardstick of ``tests/test_lightgcn_host.py``
and ``tests/test_gpu_lightgcn.py``:

* :func:`propagate_f64` -- one ``out = a x + b diag(d) M diag(d) t`` in NumPy float64, with the
  absolute-value companion the rounding bound of the device kernel is built from;
* :func:`blend_layer_sum` / :func:`blend_horner` -- x~ = sum_l alpha_l M^^l X in both forms;
* :class:`TorchTrainer` -- the model as a Torch module (autograd through the products with M^, in
  float32 or float64 on request), the two losses and the REAL ``torch.optim.AdamW``;
* :func:`train_restatement` -- the whole trainer end to end on the CPU.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.nn import functional as F


# ---------------------------------------------------------------------------------------
# NumPy float64
# ---------------------------------------------------------------------------------------
def row_sums(indptr, cols, weights, t):
    "out[r] = sum over the entries e of CSR row r of weights[col_e] t[col_e], float64"
    indptr = np.asarray(indptr, np.int64)
    cols = np.asarray(cols, np.int64)
    t = np.asarray(t, np.float64)
    contrib = np.asarray(weights, np.float64)[cols, None] * t[cols]
    out = np.zeros((len(indptr) - 1, t.shape[1]))
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    np.add.at(out, rows, contrib)
    return out


def propagate_f64(indptr, cols, d, a, x, b, t):
    """(out, size): out = a x + b d_r sum_e d_c t_c in float64 (``x`` None: no a x term) and
    size = |a x| + |b| d_r sum_e d_c |t_c|, what a rounding bound multiplies."""
    d = np.asarray(d, np.float64)
    s = row_sums(indptr, cols, d, t)
    sa = row_sums(indptr, cols, d, np.abs(np.asarray(t, np.float64)))
    out = b * d[:, None] * s
    size = abs(b) * d[:, None] * sa
    if x is not None:
        out = out + a * np.asarray(x, np.float64)
        size = size + np.abs(a * np.asarray(x, np.float64))
    return out, size


def dense_operator(indptr, cols, d, dtype=np.float64):
    "M^ = diag(d) M diag(d) as a dense [N x N] array (test sizes only)"
    n = len(indptr) - 1
    m = np.zeros((n, n), dtype=np.float64)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    np.add.at(m, (rows, np.asarray(cols, np.int64)), 1.0)
    d = np.asarray(d, np.float64)
    return (d[:, None] * m * d[None, :]).astype(dtype)


def blend_layer_sum(mhat, x, alphas):
    "sum_l alpha_l M^^l x, each power formed in turn"
    layer = np.asarray(x, np.float64)
    out = alphas[0] * layer
    for a in alphas[1:]:
        layer = mhat @ layer
        out = out + a * layer
    return out


def blend_horner(mhat, x, alphas):
    "the same by t_L = alpha_L x, t_j = alpha_j x + M^ t_{j+1}"
    x = np.asarray(x, np.float64)
    t = alphas[-1] * x
    for a in alphas[-2::-1]:
        t = a * x + mhat @ t
    return t


# ---------------------------------------------------------------------------------------
# model + step on Torch
# ---------------------------------------------------------------------------------------
def sparse_operator(indptr, cols, d, dtype) -> torch.Tensor:
    "M^ as a Torch sparse CSR tensor of ``dtype``"
    d = torch.as_tensor(np.asarray(d, np.float64))
    indptr = torch.as_tensor(np.asarray(indptr, np.int64))
    cols = torch.as_tensor(np.asarray(cols, np.int64))
    rows = torch.repeat_interleave(torch.arange(len(indptr) - 1), indptr[1:] - indptr[:-1])
    vals = (d[rows] * d[cols]).to(dtype)
    return torch.sparse_coo_tensor(torch.stack([rows, cols]), vals,
                                   (len(indptr) - 1,) * 2).coalesce()


def batch_loss(loss: str, s_pos, s_neg):
    """pairwise: mean -log sigmoid(s+ - s-); logistic: (sum -log sigmoid(s+) + sum -log
    sigmoid(-s-)) / 2B, with -log sigmoid(x) = softplus(-x)"""
    if loss == "pairwise":
        return F.softplus(s_neg - s_pos).mean()
    return (F.softplus(-s_pos).sum() + F.softplus(s_neg).sum()) / (2 * s_pos.numel())


class TorchTrainer:
    "forward, loss, ``backward()`` and ``torch.optim.AdamW.step()`` on explicit node batches"

    def __init__(self, table, indptr, cols, d, alphas, *, loss="pairwise", regularization=0.01,
                 learning_rate=0.01, dtype=torch.float32, dense=False):
        self.loss, self.alphas = loss, [float(a) for a in alphas]
        self.X = torch.nn.Parameter(torch.as_tensor(np.array(table)).to(dtype))
        if dense:
            self.mhat = torch.as_tensor(dense_operator(indptr, cols, d)).to(dtype)
        else:
            self.mhat = sparse_operator(indptr, cols, d, dtype)
        self.opt = torch.optim.AdamW([self.X], lr=learning_rate,
                                     weight_decay=0.0 if regularization is None else regularization)

    def _mm(self, t):
        return self.mhat @ t if not self.mhat.is_sparse else torch.sparse.mm(self.mhat, t)

    def embeddings(self, x=None):
        "x~ = sum_l alpha_l M^^l x (layer-sum form)"
        layer = self.X if x is None else x
        out = self.alphas[0] * layer
        for a in self.alphas[1:]:
            layer = self._mm(layer)
            out = out + a * layer
        return out

    def loss_of_embeddings(self, xbar, users, pos, neg):
        users, pos, neg = (torch.as_tensor(np.asarray(v), dtype=torch.int64).reshape(-1)
                           for v in (users, pos, neg))
        u = xbar[users]
        return batch_loss(self.loss, (u * xbar[pos]).sum(-1), (u * xbar[neg]).sum(-1))

    def pair_gradient(self, xbar, users, pos, neg):
        "(loss, dloss/dxbar) with ``xbar`` [N x k] taken as the leaf"
        leaf = torch.as_tensor(np.asarray(xbar)).to(self.X.dtype).clone().requires_grad_(True)
        val = self.loss_of_embeddings(leaf, users, pos, neg)
        val.backward()
        return float(val.detach()), leaf.grad.double().numpy().copy()

    def table_gradient(self, users, pos, neg):
        "autograd's dloss/dX as a float64 array (no optimiser step)"
        self.loss_of_embeddings(self.embeddings(), users, pos, neg).backward()
        g = self.X.grad.double().numpy().copy()
        self.X.grad = None
        return g

    def step(self, users, pos, neg) -> float:
        val = self.loss_of_embeddings(self.embeddings(), users, pos, neg)
        val.backward()
        self.opt.step()
        self.opt.zero_grad()
        return float(val.detach())

    def table(self) -> np.ndarray:
        return self.X.detach().numpy().copy()

    def final_embeddings(self) -> np.ndarray:
        with torch.no_grad():
            return self.embeddings().numpy().copy()


def adamw_steps(param, grads, *, learning_rate=0.01, regularization=0.01, dtype=torch.float32):
    "``torch.optim.AdamW`` on one tensor over a list of given gradients: (param, exp_avg, exp_avg_sq)"
    p = torch.nn.Parameter(torch.as_tensor(np.array(param)).to(dtype))
    opt = torch.optim.AdamW([p], lr=learning_rate, weight_decay=regularization)
    for g in grads:
        p.grad = torch.as_tensor(np.array(g)).to(dtype)
        opt.step()
    st = opt.state[p]
    return tuple(t.detach().double().numpy().copy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))


# ---------------------------------------------------------------------------------------
# the whole trainer, end to end on the CPU (tests/golden/make_lightgcn_quality.py)
# ---------------------------------------------------------------------------------------
def train_restatement(ds, config, seed: int, dtype=torch.float32):
    """``LightGCNScorer.train`` on the CPU from this file's parts: the package's seeding and
    initialisation, per-epoch permutation, host sampling of one uniform negative per positive,
    Torch step.  Returns (item embeddings, user embeddings): the propagated x~."""
    from flexmf_restatement import pair_keys, sample_negatives_host
    from lkpy_amd.graphs.lightgcn import graph_adjacency, initial_table
    from lkpy_amd.training import TrainingOptions

    opts = TrainingOptions(rng=seed)
    rng = opts.random_generator()
    gen = opts.random_generator(type="torch")
    n_users, n_items = ds.user_count, ds.item_count
    m_ptr, m_cols, d = graph_adjacency(ds._indptr, ds._cols, n_users, n_items)
    table = initial_table(n_users, n_items, config.embedding_size, gen, degrees=np.diff(m_ptr))
    tr = TorchTrainer(table, m_ptr, m_cols, d, config.blend_weights(), loss=config.loss,
                      regularization=config.regularization, learning_rate=config.learning_rate,
                      dtype=dtype)
    keys = pair_keys(ds._indptr, ds._cols, n_items)
    for _ in range(config.epochs):
        perm = rng.permutation(len(ds._rows))
        for start in range(0, len(perm), config.batch_size):
            sel = perm[start:start + config.batch_size]
            users, pos = ds._rows[sel], ds._cols[sel]
            neg = sample_negatives_host(keys, ds._cols, n_items, users, 1, rng).reshape(-1)
            tr.step(users.astype(np.int64) + n_items, pos, neg)
    xbar = tr.final_embeddings()
    return xbar[:n_items], xbar[n_items:]
