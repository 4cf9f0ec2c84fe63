"""
CPU restatement of FlexMF implicit (src/lenskit/flexmf/_model.py, _implicit.py:253-415,
_training.py:157-252), the yardstick of ``tests/test_flexmf_host.py`` and
``tests/test_gpu_flexmf.py``:

* :class:`TorchTrainer` -- one training step / a whole trainer from ``nn.Embedding``, autograd and
  the REAL ``torch.optim.AdamW`` / ``torch.optim.SparseAdam`` (they are the definition of the two
  updates), in float32 or float64 on request;
* :func:`numpy_gradients` -- the hand-derived gradients in NumPy float64, the formulas the kernels
  of ``csrc/flexmf.hip`` follow;
* :func:`reject`, :func:`sample_negatives_host` -- the sampler's rejection rule;
* :func:`warp_search_masked` / :func:`warp_search_sequential` -- the WARP search in the
  reference's form (masked batches of ten) and in the sequential form the device runs.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from lkpy_amd.flexmf import WARP_MAX_TRIES  # the package's try budget is the yardstick's too

TABLES = ("u_bias.weight", "i_bias.weight", "u_embed.weight", "i_embed.weight")
CANDIDATE_BLOCK = 10  # candidates the reference draws at a time for the rows still searching
MAX_TRIES = WARP_MAX_TRIES


# ---------------------------------------------------------------------------------------
# model + step on Torch
# ---------------------------------------------------------------------------------------
class Model(nn.Module):
    "score = b_u + b_i + p_u . q_i (absent biases count as 0); optionally the L2 factor r"

    def __init__(self, tabs: dict, dtype, sparse: bool):
        super().__init__()
        self.u_bias = self.i_bias = None
        for name in TABLES:
            w = tabs.get(name)
            if w is None:
                continue
            w = torch.as_tensor(np.array(w)).to(dtype).reshape(len(w), -1)
            emb = nn.Embedding(w.shape[0], w.shape[1], sparse=sparse, dtype=dtype)
            with torch.no_grad():
                emb.weight.copy_(w)
            setattr(self, name.split(".")[0], emb)

    def _bias(self, table, index):
        return None if table is None else table(index).squeeze(-1)

    def forward(self, user, item, with_norm: bool):
        """``user`` [B x 1], ``item`` [B x n] -> scores [B x n] (and the L2 factor of each score:
        squared biases plus the 2-norms -- not squared -- of the two embedding rows)."""
        p, q = self.u_embed(user), self.i_embed(item)
        score = (p * q).sum(dim=-1)
        b_user, b_item = self._bias(self.u_bias, user), self._bias(self.i_bias, item)
        for b in (b_item, b_user):
            if b is not None:
                score = score + b
        if not with_norm:
            return score, None
        factor = p.norm(dim=-1) + q.norm(dim=-1) + torch.zeros_like(score)
        for b in (b_item, b_user):
            if b is not None:
                factor = factor + b * b
        return score, factor


def batch_loss(loss: str, s_pos, s_neg, pos_weight: float, weights):
    """The issue's three losses on scores [B x 1] and [B x n], softplus(x) = log(1 + e^x):
    logistic  (w+ sum softplus(-s+) + sum softplus(s-)) / (B + B n);
    pairwise  mean softplus(-(s+ - s-));  warp  the same with each sample's weight."""
    if loss == "logistic":
        total = pos_weight * F.softplus(-s_pos).sum() + F.softplus(s_neg).sum()
        return total / (s_pos.numel() + s_neg.numel())
    per_pair = F.softplus(s_neg - s_pos)
    if loss == "warp":
        per_pair = per_pair * weights.reshape(per_pair.shape)
    return per_pair.mean()


class TorchTrainer:
    "``train_batch`` + ``opt.step()`` on explicit (users, positives, negatives[, weights])"

    def __init__(self, tabs: dict, *, loss="logistic", reg_method="AdamW", regularization=0.01,
                 learning_rate=0.01, positive_weight=1.0, dtype=torch.float32, optimizer=None):
        self.loss, self.reg_method, self.reg = loss, reg_method, regularization
        self.pos_weight = positive_weight
        self.model = Model(tabs, dtype, sparse=reg_method != "AdamW")
        if optimizer is not None:  # (the power check's deliberately wrong optimiser)
            self.opt = optimizer(self.model.parameters())
        elif reg_method == "AdamW":
            self.opt = torch.optim.AdamW(self.model.parameters(), lr=learning_rate,
                                         weight_decay=regularization)
        else:
            self.opt = torch.optim.SparseAdam(self.model.parameters(), lr=learning_rate)
        self.squared_norms = False  # (the power check's other deliberate error)

    def loss_of(self, users, pos, neg, weights=None):
        users = torch.as_tensor(np.asarray(users), dtype=torch.int64).reshape(-1, 1)
        pos = torch.as_tensor(np.asarray(pos), dtype=torch.int64).reshape(-1, 1)
        neg = torch.as_tensor(np.asarray(neg), dtype=torch.int64).reshape(len(users), -1)
        l2 = self.reg_method == "L2"
        sp, rp = self.model(users, pos, l2)
        sn, rn = self.model(users, neg, l2)
        if weights is not None:
            weights = torch.as_tensor(np.asarray(weights), dtype=torch.float64)
        val = batch_loss(self.loss, sp, sn, self.pos_weight, weights)
        if l2:
            if self.squared_norms:
                rp, rn = self._squared(users, pos), self._squared(users, neg)
            val = val + self.reg * 0.5 * (rp.mean() + rn.mean())
        return val

    def _squared(self, user, item):
        "the deliberate error of the power check: squared norms where the model has norms"
        m = self.model
        out = m.u_embed(user).square().sum(-1) + m.i_embed(item).square().sum(-1)
        for b in (m._bias(m.u_bias, user), m._bias(m.i_bias, item)):
            if b is not None:
                out = out + b * b
        return out

    def step(self, users, pos, neg, weights=None) -> float:
        val = self.loss_of(users, pos, neg, weights)
        val.backward()
        self.opt.step()
        self.opt.zero_grad()
        return float(val.detach())

    def tables(self) -> dict:
        return {name: getattr(self.model, name.split(".")[0]).weight.detach().numpy().copy()
                for name in TABLES if getattr(self.model, name.split(".")[0]) is not None}

    def dense_gradients(self, users, pos, neg, weights=None) -> dict:
        "autograd's gradient of every table as a dense float64 array (no optimiser step)"
        self.loss_of(users, pos, neg, weights).backward()
        out = {}
        for name in TABLES:
            emb = getattr(self.model, name.split(".")[0])
            if emb is not None:
                g = emb.weight.grad
                out[name] = (g.to_dense() if g.is_sparse else g).double().numpy().copy()
                emb.weight.grad = None
        return out


def table_distance(a: dict, b: dict) -> float:
    "largest absolute difference over all tables"
    worst = 0.0
    for name in TABLES:
        if a.get(name) is None:
            continue
        x = np.asarray(a[name], np.float64).reshape(-1)
        y = np.asarray(b[name], np.float64).reshape(-1)
        worst = max(worst, float(np.abs(x - y).max()))
    return worst


# ---------------------------------------------------------------------------------------
# hand-derived gradients (NumPy float64): what the kernels compute
# ---------------------------------------------------------------------------------------
def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))),
                    np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def numpy_gradients(tabs: dict, users, pos, neg, weights=None, *, loss="logistic", l2=False,
                    reg=0.01, pos_weight=1.0):
    """
    (loss, {table: dense gradient}).  Per sample b and negative j, with d = s+ - s-:
      pairwise  g-_bj = sigma(-d) / (B n),  g+_b = -sum_j g-_bj
      logistic  g+_b = -w+ sigma(-s+) / (B + B n),  g-_bj = sigma(s-) / (B + B n)
      warp      g-_b = sigma(-d) w_b / B,  g+_b = -g-_b
    then  dP[u] += g+ q+ + sum_j g-_j q-_j,  dQ[i+] += g+ p,  dQ[i-_j] += g-_j p, the biases take
    the coefficients themselves; the L2 term adds reg/B p/|p| to the user row (its norm occurs in
    r+ and in each of the n r-), 0.5 reg/B q/|q| to the positive's and 0.5 reg/(B n) q/|q| to each
    negative's row (0 where the norm is 0), 2 reg b_u / B, reg b_i / B and reg b_i / (B n).
    """
    P = np.asarray(tabs["u_embed.weight"], np.float64)
    Q = np.asarray(tabs["i_embed.weight"], np.float64)
    bu = tabs.get("u_bias.weight")
    bi = tabs.get("i_bias.weight")
    bu = None if bu is None else np.asarray(bu, np.float64).reshape(-1)
    bi = None if bi is None else np.asarray(bi, np.float64).reshape(-1)
    users, pos = np.asarray(users, np.int64), np.asarray(pos, np.int64)
    B = len(users)
    neg = np.asarray(neg, np.int64).reshape(B, -1)
    n = neg.shape[1]
    ubv = bu[users] if bu is not None else np.zeros(B)
    sp = ubv + (bi[pos] if bi is not None else 0.0) + np.einsum("bk,bk->b", P[users], Q[pos])
    sn = ubv[:, None] + (bi[neg] if bi is not None else 0.0) + \
        np.einsum("bk,bjk->bj", P[users], Q[neg])
    if loss == "logistic":
        tot = B + B * n
        val = (pos_weight * _softplus(-sp).sum() + _softplus(sn).sum()) / tot
        gp = -pos_weight * _sigmoid(-sp) / tot
        gn = _sigmoid(sn) / tot
    else:
        d = sp[:, None] - sn
        w = np.ones((B, 1)) if loss == "pairwise" else np.asarray(weights, np.float64).reshape(B, 1)
        val = (_softplus(-d) * w).mean()
        gn = _sigmoid(-d) * w / (B * n)
        gp = -gn.sum(axis=1)
    dP, dQ = np.zeros_like(P), np.zeros_like(Q)
    dbu = None if bu is None else np.zeros_like(bu)
    dbi = None if bi is None else np.zeros_like(bi)
    np.add.at(dP, users, gp[:, None] * Q[pos] + np.einsum("bj,bjk->bk", gn, Q[neg]))
    np.add.at(dQ, pos, gp[:, None] * P[users])
    np.add.at(dQ, neg.reshape(-1), (gn[:, :, None] * P[users][:, None, :]).reshape(B * n, -1))
    if dbu is not None:
        np.add.at(dbu, users, gp + gn.sum(axis=1))
    if dbi is not None:
        np.add.at(dbi, pos, gp)
        np.add.at(dbi, neg.reshape(-1), gn.reshape(-1))
    if l2:
        pn, qpn, qnn = (np.linalg.norm(P[users], axis=1), np.linalg.norm(Q[pos], axis=1),
                        np.linalg.norm(Q[neg], axis=2))
        ub2 = ubv ** 2
        ibp2 = bi[pos] ** 2 if bi is not None else 0.0
        ibn2 = bi[neg] ** 2 if bi is not None else 0.0
        rp = ub2 + ibp2 + pn + qpn
        rn = ub2[:, None] + ibn2 + pn[:, None] + qnn
        val = val + reg * 0.5 * (rp.mean() + rn.mean())

        def unit(x, nrm):
            return np.divide(x, nrm[..., None], out=np.zeros_like(x), where=nrm[..., None] > 0)

        np.add.at(dP, users, reg / B * unit(P[users], pn))
        np.add.at(dQ, pos, 0.5 * reg / B * unit(Q[pos], qpn))
        np.add.at(dQ, neg.reshape(-1), (0.5 * reg / (B * n) * unit(Q[neg], qnn)).reshape(B * n, -1))
        if dbu is not None:
            np.add.at(dbu, users, 2.0 * reg / B * ubv)
        if dbi is not None:
            np.add.at(dbi, pos, reg / B * bi[pos])
            np.add.at(dbi, neg.reshape(-1), (reg / (B * n) * bi[neg]).reshape(-1))
    grads = {"u_embed.weight": dP, "i_embed.weight": dQ}
    if dbu is not None:
        grads["u_bias.weight"] = dbu.reshape(-1, 1)
    if dbi is not None:
        grads["i_bias.weight"] = dbi.reshape(-1, 1)
    return float(val), grads


# ---------------------------------------------------------------------------------------
# negative sampling: the rejection rule (src/accel/data/sampling.rs:38-57)
# ---------------------------------------------------------------------------------------
def pair_keys(indptr, cols, n_cols: int) -> np.ndarray:
    "sorted unique row * n_cols + col of the training interactions"
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    return np.unique(rows * n_cols + np.asarray(cols, np.int64))


def reject(keys: np.ndarray, n_cols: int, rows, cols) -> np.ndarray:
    "True where (row, col) is a training interaction -- the draw that must be repeated"
    k = np.asarray(rows, np.int64) * n_cols + np.asarray(cols, np.int64)
    pos = np.searchsorted(keys, k)
    pos[pos >= len(keys)] = len(keys) - 1
    return keys[pos] == k if len(keys) else np.zeros(k.shape, bool)


def sample_negatives_host(keys, all_cols, n_cols: int, rows, n: int, rng, *, popular=False,
                          max_attempts=10) -> np.ndarray:
    """[len(rows) x n]: a draw (uniform column, or the column of a uniformly drawn interaction) is
    redrawn while the pair is a training interaction, at most ``max_attempts`` times."""
    rows = np.repeat(np.asarray(rows, np.int64), n)

    def draw(m):
        if popular:
            return np.asarray(all_cols)[rng.integers(0, len(all_cols), size=m)].astype(np.int64)
        return rng.integers(0, n_cols, size=m)

    out = draw(len(rows))
    for _ in range(max_attempts):
        bad = np.flatnonzero(reject(keys, n_cols, rows, out))
        if not len(bad):
            break
        out[bad] = draw(len(bad))
    return out.reshape(-1, n).astype(np.int32)


# ---------------------------------------------------------------------------------------
# WARP search over a candidate table (src/lenskit/flexmf/_implicit.py:293-396)
# ---------------------------------------------------------------------------------------
def warp_weights(counts, n_items: int) -> np.ndarray:
    """The sample weight of a negative found at try ``count``: the harmonic number of the
    estimated rank (n_items - 1) / (count + 1), by its asymptotic series
    ln r + gamma + 1/(2r) - 1/(12 r^2) + 1/(120 r^4), in float64 (here in powers of x = 1/r)."""
    x = (np.asarray(counts, np.float64) + 1.0) / (n_items - 1)
    return np.euler_gamma - np.log(x) + x * (0.5 + x * (-1.0 / 12.0 + x * x / 120.0))


def warp_search_sequential(pos_scores, cand_items, cand_scores):
    """
    Per sample, try t = 1.. takes candidate t - 1; a strictly greater score replaces the best so
    far (count = t); stop once best >= s+.  Returns (items, counts, margin): margin = the
    smallest |candidate - best| and |best - s+| over the visited tries (how close any decision
    of the search came to going the other way).
    """
    B, T = cand_items.shape
    items, counts = np.zeros(B, np.int32), np.zeros(B, np.int32)
    margin = np.full(B, np.inf)
    for b in range(B):
        best = -math.inf
        for t in range(1, T + 1):
            s = cand_scores[b, t - 1]
            if math.isfinite(best):
                margin[b] = min(margin[b], abs(float(s) - best))
            if s > best:
                best, items[b], counts[b] = float(s), cand_items[b, t - 1], t
            margin[b] = min(margin[b], abs(best - float(pos_scores[b])))
            if best >= pos_scores[b]:
                break
    return items, counts, margin


def warp_search_masked(pos_scores, cand_items, cand_scores, block: int = CANDIDATE_BLOCK):
    """
    The search a block of candidates at a time, as the reference schedules it: only the rows still
    searching when a block starts take that block's columns of the table, and inside the block a
    row stops looking once its best reaches the positive's score.  Whole blocks are handled with
    running maxima instead of one try at a time.  Returns (items, counts).
    """
    B, T = cand_items.shape
    best = np.full(B, -np.inf)
    items, counts = np.zeros(B, np.int32), np.zeros(B, np.int32)
    searching = np.ones(B, bool)
    for start in range(0, T, block):
        rows = np.flatnonzero(searching)
        if not len(rows):
            break
        S = cand_scores[rows, start:start + block].astype(np.float64)
        # running[:, j] = the row's best before try j of the block, running[:, j + 1] = after it
        running = np.maximum.accumulate(np.column_stack([best[rows], S]), axis=1)
        improves = S > running[:, :-1]
        done = running[:, 1:] >= np.asarray(pos_scores, np.float64)[rows, None]
        visited = np.cumsum(done, axis=1) - done == 0  # up to and including the stopping try
        improves &= visited
        found = improves.any(axis=1)
        last = S.shape[1] - 1 - np.argmax(improves[:, ::-1], axis=1)  # the last improving try
        r, j = rows[found], last[found]
        best[r] = S[found, j]
        items[r] = cand_items[r, start + j]
        counts[r] = start + j + 1
        searching[rows] = ~done.any(axis=1)
    return items, counts


# ---------------------------------------------------------------------------------------
# the whole trainer, end to end on the CPU (tests/golden/make_flexmf_quality.py)
# ---------------------------------------------------------------------------------------
def train_restatement(ds, config, seed: int, dtype=torch.float32) -> dict:
    """``FlexMFImplicitScorer.train`` on the CPU from this file's parts: the reference's seeding
    and initialisation, per-epoch permutation, host sampling, WARP search, Torch step."""
    from lkpy_amd.flexmf import initial_tables
    from lkpy_amd.training import TrainingOptions

    opts = TrainingOptions(rng=seed)
    rng = opts.random_generator()
    gen = opts.random_generator(type="torch")
    n_users, n_items = ds.user_count, ds.item_count
    tabs = initial_tables(n_users, n_items, config.embedding_size, gen,
                          user_bias=config.selected_user_bias(), item_bias=config.item_bias,
                          user_counts=np.diff(ds._indptr),
                          item_counts=np.bincount(ds._cols, minlength=n_items))
    tr = TorchTrainer(tabs, loss=config.loss, reg_method=config.reg_method,
                      regularization=config.regularization, learning_rate=config.learning_rate,
                      positive_weight=config.positive_weight, dtype=dtype)
    keys = pair_keys(ds._indptr, ds._cols, n_items)
    strategy = config.selected_negative_strategy()
    for _ in range(config.epochs):
        perm = rng.permutation(len(ds._rows))
        for start in range(0, len(perm), config.batch_size):
            sel = perm[start:start + config.batch_size]
            users, pos = ds._rows[sel], ds._cols[sel]
            weights = None
            if strategy == "misranked":
                cand = sample_negatives_host(keys, ds._cols, n_items, users, MAX_TRIES, rng)
                with torch.no_grad():
                    u = torch.as_tensor(users, dtype=torch.int64).reshape(-1, 1)
                    sp = tr.model(u, torch.as_tensor(pos, dtype=torch.int64).reshape(-1, 1),
                                  False)[0].numpy().reshape(-1)
                    sc = tr.model(u, torch.as_tensor(cand, dtype=torch.int64), False)[0].numpy()
                neg, counts = warp_search_masked(sp, cand, sc)
                if config.loss == "warp":
                    weights = warp_weights(counts, n_items)
            else:
                neg = sample_negatives_host(keys, ds._cols, n_items, users, config.negative_count,
                                            rng, popular=strategy == "popular")
            tr.step(users, pos, neg, weights)
    return tr.tables()
