"""
CPU restatements of the batch scoring kernels, written in NumPy from each kernel's stated
summation order: the yardstick of ``tests/test_batch_restatement_host.py`` and
``tests/test_gpu_batch_kernels.py``.

``ease_score`` / ``slim_score`` keep one float32 accumulator row per query and add the history
items' weight rows in history order, once per occurrence (``q_vec @ weights``,
src/lenskit/knn/ease.py:161-168; ``x @ self.weights``, src/lenskit/knn/slim.py:133-144).  The
arithmetic is float32 adds only, and a NumPy float32 add is the same IEEE operation as the
kernel's.  ``csr_rows_dot`` and ``dense_scores`` are ``fmaf`` chains, which NumPy cannot restate;
they go through the oracle's ``lko_score_dense`` (``acc = fmaf(a_j, b_j, acc)`` from 0 in j order).
"""
from __future__ import annotations

import numpy as np

MARK_HISTORY = 1  # the query's own in-range items become NaN
MARK_EMPTY = 2    # a query with an empty history (ptr[q] == ptr[q + 1]) becomes all NaN


def magnitudes(rng, shape) -> np.ndarray:
    "float32 values with magnitudes in [1e-3, 1] and random signs: no subnormal partial sums."
    mag = np.power(10.0, rng.uniform(-3.0, 0.0, shape))
    return (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def ease_score(weights: np.ndarray, ptr, items) -> np.ndarray:
    "[B x n_items] float32: the sum of the history items' rows of the dense ``weights``."
    n_items = weights.shape[0]
    out = np.zeros((len(ptr) - 1, n_items), np.float32)
    for q in range(len(ptr) - 1):
        acc = np.zeros(n_items, np.float32)
        for it in items[ptr[q]:ptr[q + 1]]:
            if it < 0 or it >= n_items:
                continue
            acc = acc + weights[it, :n_items]
        out[q] = acc
    return out


def slim_score(w_csr, ptr, items, mark: int = 0) -> np.ndarray:
    """
    [B x n_items] float32: the history items' rows of the SciPy CSR ``w_csr`` (unique column
    indices per row) added to their target cells, then the ``mark`` bits.
    """
    n_items = w_csr.shape[1]
    w_ptr, w_idx, w_val = w_csr.indptr, w_csr.indices, w_csr.data.astype(np.float32)
    out = np.zeros((len(ptr) - 1, n_items), np.float32)
    for q in range(len(ptr) - 1):
        hist = np.asarray(items[ptr[q]:ptr[q + 1]])
        acc = np.zeros(n_items, np.float32)
        for it in hist:
            if it < 0 or it >= n_items:
                continue
            b, e = w_ptr[it], w_ptr[it + 1]
            acc[w_idx[b:e]] = acc[w_idx[b:e]] + w_val[b:e]
        if mark & MARK_HISTORY:
            acc[hist[(hist >= 0) & (hist < n_items)]] = np.nan
        if (mark & MARK_EMPTY) and ptr[q] == ptr[q + 1]:
            acc[:] = np.nan
        out[q] = acc
    return out


def take_scores(panel: np.ndarray, idx: np.ndarray) -> np.ndarray:
    "[B x n] float32: ``panel[r, idx[r, j]]`` bit for bit, NaN where idx < 0 or idx >= row_len."
    panel = np.ascontiguousarray(panel, np.float32)
    row_len = panel.shape[1]
    ok = (idx >= 0) & (idx < row_len)
    rows = np.broadcast_to(np.arange(idx.shape[0])[:, None], idx.shape)
    out = np.full(idx.shape, np.nan, np.float32)
    # through the bit view: a float copy may quieten a signalling NaN
    out.view(np.uint32)[ok] = panel.view(np.uint32)[rows[ok], idx[ok]]
    return out


def csr_rows_dot(csr, x: np.ndarray, oracle) -> np.ndarray:
    "[B x rows] float32: per (row, query) the fmaf chain over the row's entries in entry order."
    n_rows, n_queries = csr.shape[0], x.shape[1]
    out = np.zeros((n_queries, n_rows), np.float32)
    for r in range(n_rows):
        b, e = csr.indptr[r], csr.indptr[r + 1]
        if b == e:
            continue
        out[:, r] = oracle.score_dense(x[csr.indices[b:e], :].T, csr.data[b:e])
    return out


def dense_scores(items: np.ndarray, users: np.ndarray, oracle) -> np.ndarray:
    "[B x I] float32: ``oracle.score_dense(items, users[b])`` per user."
    return np.stack([oracle.score_dense(items, users[b]) for b in range(users.shape[0])])


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    "NaN where NaN, the same bits everywhere else."
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = ~np.isnan(want)
    return bool(np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]))
