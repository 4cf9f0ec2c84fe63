"""CPU: the batch-kernel restatements (``tests/batch_restatement.py``) against float64 dense
computations and against the reference lines the kernels cite.

The float64 bound per cell is ``(terms + 1) * 2^-24 * sum|terms|``: a chain of ``terms`` float32
operations each rounds by at most 2^-24 relative to a partial sum that never exceeds the sum of
the magnitudes (the standard recursive-summation bound, first order, with one term of slack)."""
import numpy as np
import pytest
import scipy.sparse as sps

import batch_restatement as R

U = 2.0 ** -24


def _histories(rng, n_items, n_queries):
    "Random histories with repeats and unknown items; query 0 is empty, query 1 unknown-only."
    hist = [np.zeros(0, np.int32), np.array([-1, n_items, n_items + 5], np.int32)]
    while len(hist) < n_queries:
        h = rng.integers(0, n_items, int(rng.integers(1, 40))).astype(np.int32)
        h[rng.random(len(h)) < 0.1] = rng.choice([-1, -7, n_items, n_items + 3])
        if len(h) > 4:
            h[3] = h[1]  # a repeat
        hist.append(h)
    ptr = np.zeros(n_queries + 1, np.int64)
    np.cumsum([len(h) for h in hist], out=ptr[1:])
    return ptr, np.concatenate(hist).astype(np.int32), hist


def _counts(hist, n_items):
    "The per-occurrence count vectors, float64 CSR [B x n_items], unknown items dropped."
    x = np.zeros((len(hist), n_items))
    for q, h in enumerate(hist):
        ok = h[(h >= 0) & (h < n_items)]
        np.add.at(x[q], ok, 1.0)
    return sps.csr_array(x)


def test_magnitudes_range(rng):
    v = R.magnitudes(rng, 10000)
    assert v.dtype == np.float32 and (v < 0).any() and (v > 0).any()
    # 1e-3 and 1 are not float32 numbers: allow the cast's own rounding at the two ends
    assert np.abs(v).min() >= np.float32(1e-3) * (1 - 2 * U) and np.abs(v).max() <= 1.0


def test_ease_score_vs_float64(rng):
    n = 300
    w = R.magnitudes(rng, (n, n))
    ptr, items, hist = _histories(rng, n, 25)
    got = R.ease_score(w, ptr, items)
    x = _counts(hist, n)
    want = x @ w.astype(np.float64)
    terms = np.asarray(x.sum(axis=1)).reshape(-1, 1)
    bound = (terms + 1) * U * (x @ np.abs(w).astype(np.float64))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.all(np.abs(got - want) <= bound)
    assert terms.max() > 20 and np.abs(want).max() > 1.0  # a vacuous zero would not pass
    # the rules the kernel cites (ease.py:161-168): negative (unknown) items are dropped, and the
    # query vector of what is left is summed; at this level an all-unknown history is all zeros
    assert not got[0].any() and not got[1].any()
    # a padded weight matrix: only the first n columns are read
    wp = np.full((n, n + 3), np.nan, np.float32)
    wp[:, :n] = w
    assert np.array_equal(R.ease_score(wp, ptr, items).view(np.uint32), got.view(np.uint32))


def test_ease_score_counts_each_occurrence():
    w = np.array([[0.5, 0.25], [1.0, 2.0]], np.float32)
    ptr = np.array([0, 2, 5], np.int64)
    items = np.array([1, 1, 0, 2, 0], np.int32)  # item 2 == n_items: skipped
    assert np.array_equal(R.ease_score(w, ptr, items), [[2.0, 4.0], [1.0, 0.5]])


def _slim_weights(rng, n, density=0.05):
    w = sps.random_array((n, n), density=density, format="csr", rng=rng, dtype=np.float32)
    w.data = R.magnitudes(rng, w.nnz)
    w.sort_indices()
    return w


def test_slim_score_vs_float64(rng):
    n = 400
    w = _slim_weights(rng, n)
    ptr, items, hist = _histories(rng, n, 25)
    got = R.slim_score(w, ptr, items, 0)
    x = _counts(hist, n)
    w64 = sps.csr_array(w, dtype=np.float64)
    want = (x @ w64).toarray()
    terms = (x @ sps.csr_array((np.ones(w.nnz), w.indices, w.indptr), shape=w.shape)).toarray()
    bound = (terms + 1) * U * (x @ abs(w64)).toarray()
    assert got.dtype == np.float32 and np.all(np.abs(got - want) <= bound)
    assert terms.max() >= 3 and np.count_nonzero(want) > n


def test_slim_mark_and_unknown_rules(rng):
    """slim.py:128-134: an empty history scores NaN everywhere; unknown items (negative numbers)
    are dropped, and an all-unknown history is ``x = 0`` -- zeros, not NaN.  Candidates are the
    items minus the query's own (basic/candidates.py:77-94): mark bit 1."""
    n = 400
    w = _slim_weights(rng, n)
    ptr, items, hist = _histories(rng, n, 12)
    plain = R.slim_score(w, ptr, items, 0)
    for mark in (1, 2, 3):
        got = R.slim_score(w, ptr, items, mark)
        for q, h in enumerate(hist):
            own = np.zeros(n, bool)
            own[h[(h >= 0) & (h < n)]] = True
            if (mark & R.MARK_EMPTY) and len(h) == 0:
                assert np.isnan(got[q]).all()
                continue
            if mark & R.MARK_HISTORY:
                assert np.isnan(got[q][own]).all()
            else:
                own[:] = False
            assert np.array_equal(got[q][~own].view(np.uint32), plain[q][~own].view(np.uint32))
    assert not plain[0].any() and not plain[1].any()
    assert not R.slim_score(w, ptr, items, 3)[1].any()  # unknown-only: zeros under every mark
    assert not np.isnan(R.slim_score(w, ptr, items, 1)[0]).any()  # bit 1 alone: empty stays 0


def test_history_order_is_part_of_the_restatement():
    "Three rows that share a target, with values whose float32 sum depends on the order."
    vals = np.array([1.0, 2.0 ** -24, 2.0 ** -24], np.float32)
    w = sps.csr_array((vals, np.zeros(3, np.int32), np.arange(4)), shape=(3, 3))
    ptr = np.array([0, 3], np.int64)
    fwd = R.slim_score(w, ptr, np.array([0, 1, 2], np.int32))
    rev = R.slim_score(w, ptr, np.array([2, 1, 0], np.int32))
    assert fwd[0, 0] == np.float32(1.0) and rev[0, 0] == np.float32(1.0) + np.float32(2.0 ** -23)
    dense = w.toarray()
    assert R.ease_score(dense, ptr, np.array([0, 1, 2], np.int32))[0, 0] == fwd[0, 0]
    assert R.ease_score(dense, ptr, np.array([2, 1, 0], np.int32))[0, 0] == rev[0, 0]


def test_take_scores_rules(rng):
    panel = rng.standard_normal((5, 11)).astype(np.float32)
    panel.view(np.uint32)[2, 3] = 0x7F800001  # a signalling NaN keeps its payload
    panel[1, 0] = -0.0
    idx = rng.integers(0, 11, (5, 4)).astype(np.int32)
    idx[0, 0], idx[1, 1], idx[2, 2], idx[2, 0], idx[1, 3] = -1, 11, 2 ** 31 - 1, 3, 0
    got = R.take_scores(panel, idx)
    for r in range(5):
        for j in range(4):
            c = idx[r, j]
            if 0 <= c < 11:
                assert got.view(np.uint32)[r, j] == panel.view(np.uint32)[r, c]
            else:
                assert np.isnan(got[r, j])
    assert got.view(np.uint32)[2, 0] == 0x7F800001 and np.signbit(got[1, 3])
    assert R.same_bits(got, got) and not R.same_bits(got, -got)


def _oracle():
    try:
        from oracle import lk_oracle

        lk_oracle.lib()
    except Exception as exc:  # noqa: BLE001
        pytest.skip(f"the oracle library cannot be built here: {exc}")
    return lk_oracle


def test_csr_rows_dot_vs_float64(rng):
    oracle = _oracle()
    lens = [0, 1, 63, 64, 65, 129, 200]
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = np.concatenate([np.sort(rng.choice(300, m, replace=False)) for m in lens]).astype(np.int32)
    csr = sps.csr_array((R.magnitudes(rng, len(idx)), idx, ptr), shape=(len(lens), 300))
    x = R.magnitudes(rng, (300, 9))
    got = R.csr_rows_dot(csr, x, oracle)
    c64, x64 = sps.csr_array(csr, dtype=np.float64), x.astype(np.float64)
    want = (c64 @ x64).T
    bound = (np.asarray(lens)[None, :] + 1) * U * (abs(c64) @ np.abs(x64)).T
    assert got.dtype == np.float32 and got.shape == (9, 7)
    assert np.all(np.abs(got - want) <= bound) and not got[:, 0].any()
    assert np.abs(want[:, 1:]).min() > 0


def test_dense_scores_vs_float64(rng):
    oracle = _oracle()
    q, u = R.magnitudes(rng, (50, 25)), R.magnitudes(rng, (3, 25))
    got = R.dense_scores(q, u, oracle)
    want = u.astype(np.float64) @ q.astype(np.float64).T
    bound = 26 * U * (np.abs(u).astype(np.float64) @ np.abs(q).astype(np.float64).T)
    assert got.shape == (3, 50) and np.all(np.abs(got - want) <= bound)
