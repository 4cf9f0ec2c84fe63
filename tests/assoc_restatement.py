"""
NumPy / SciPy restatement of the association-rule scorer (``AssociationScorer``,
src/lenskit/knn/association.py:91-163), written from its arithmetic contract:

* counts: ``C = X^T X`` of the binary interaction matrix without its diagonal (the number of users
  that hold both items); item counts = interaction records per item; ``N`` = the matrix's rows;
* scaling: NumPy's own in-place expression -- float32 values ``/=`` an ``int32 + float`` (float64)
  array, for lift ``*=`` a Python int and ``/=`` the column's ``int32 + float`` array;
* scoring: the reference items' rows densified, ``np.mean`` / ``np.max`` over axis 0 (a cell's sum
  is the sequential float32 sum in reference-item order; absent cells are 0.0);
* top-N: candidates = all items minus the query's own, selected by a heap ``argtopn`` the caller
  passes in (``oracle.argtopn``).

It also makes the synthetic input of the kernel tests (``kernel_case``), so that the host test can
check on the very same input that the order of the reference items matters to the mean.
"""
from functools import lru_cache

import numpy as np
import scipy.sparse as sps


def cooc_counts(rmat):
    "(off-diagonal co-occurrence counts as a sorted int64 CSR, item record counts int32, n_groups)"
    x = sps.csr_array(rmat)
    item_counts = np.bincount(x.indices, minlength=x.shape[1]).astype(np.int32)
    x = sps.csr_array((np.ones(x.nnz, np.int64), x.indices, x.indptr), shape=x.shape)
    x.sum_duplicates()
    x.data[:] = 1
    c = sps.coo_array(x.T @ x)
    off = c.row != c.col
    c = sps.csr_array((c.data[off], (c.row[off], c.col[off])), shape=c.shape)
    c.sort_indices()
    return c, item_counts, int(x.shape[0])


def scale(counts, rows, cols, item_counts, n_groups: int, method: str, damping: float):
    "association.py:110-124 on COO triplets: float32 values out"
    vals = np.asarray(counts).astype(np.float32)
    item_counts = np.asarray(item_counts, dtype=np.int32)
    vals /= item_counts[rows] + float(damping)
    if method == "lift":
        vals *= int(n_groups)
        vals /= item_counts[cols] + float(damping)
    return vals


def train(cooc, item_counts, n_groups, method="probability", damping=0.0):
    "the stored ``assoc_scores`` (float32 CSR, rows = reference items, columns ascending)"
    n = cooc.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(cooc.indptr))
    vals = scale(cooc.data, rows, cooc.indices, item_counts, n_groups, method, damping)
    return sps.csr_array((vals, cooc.indices.astype(np.int32), cooc.indptr.astype(np.int64)),
                         shape=cooc.shape)


def reduce_rows(s, refs, max_nbrs=None):
    """association.py:139-155 for already numbered reference items (negative = unknown, dropped;
    order and repeats kept): float32 [n_items]; None when no reference item is left."""
    refs = np.asarray(refs, dtype=np.int64)
    refs = refs[refs >= 0]
    if len(refs) == 0:
        return None
    dense = np.asarray(s[refs, :].todense(), dtype=np.float32)
    if max_nbrs == 1:
        return np.max(dense, axis=0)
    if max_nbrs is None:
        if dense.shape[1] == 1:
            # NumPy folds a one-column matrix into a vector and sums THAT pairwise (blocks of 8
            # and more); the contract is the sequential sum it forms for every wider matrix, so
            # a one-item vocabulary gets a zero column beside it for the reduction
            wide = np.concatenate([dense, np.zeros_like(dense)], axis=1)
            return np.mean(wide, axis=0)[:1]
        return np.mean(dense, axis=0)
    raise NotImplementedError("limited reference items not yet implemented")


def scores(s, refs, max_nbrs=None):
    "every item's score for one query: NaN everywhere without a known reference item"
    row = reduce_rows(s, refs, max_nbrs)
    return np.full(s.shape[1], np.nan, np.float32) if row is None else row


def mark_row(row, refs, n_items: int, mark: int):
    """a reduced row (None: no known reference item) as lk_assoc_score_batch's panel holds it:
    mark bit 0 strikes the query's own items, bit 1 turns the row of an empty query into NaN (it
    is 0.0 otherwise)"""
    if row is None:
        return np.full(n_items, np.nan if mark & 2 else 0.0, np.float32)
    if mark & 1:
        refs = np.asarray(refs)
        row = row.copy()
        row[refs[refs >= 0]] = np.nan
    return row


def panel_row(s, refs, reduce: str, mark: int):
    "one row of lk_assoc_score_batch's panel"
    return mark_row(reduce_rows(s, refs, 1 if reduce == "max" else None), refs, s.shape[1], mark)


def topn(row, refs, n, argtopn):
    "(item numbers, scores) of the top-n candidates: every item minus the query's own"
    cand = np.array(row, dtype=np.float32)
    refs = np.asarray(refs)
    cand[refs[refs >= 0]] = np.nan
    keep = int((~np.isnan(cand)).sum())
    idx = np.asarray(argtopn(cand, keep if n is None or n < 0 else n))
    return idx, cand[idx]


# -- the synthetic input of the kernel tests ---------------------------------------------------

N_QUERIES = 9
PROBE = 7  # the query that is also scored alone


@lru_cache(maxsize=None)
def kernel_case(n_items: int, seed: int = 20261018):
    """
    (scores CSR, queries): a random square CSR that need not come from training -- values
    log-uniform over 1e-6 ... 1e3 so that the order of a sum shows in its bits; row 0 full, row 1
    empty, row 2 one entry, row 3 longer than a 256-thread stride where the vocabulary allows it;
    every row but the empty one names the column ``n_items // 2``.  Nine queries: no items; only
    unknown items; one item; one item three times; 300 items (all their rows name the shared
    column); known items in descending number order around an unknown one; three random ones
    (query ``PROBE`` is the one scored alone too).
    """
    rng = np.random.default_rng(seed + n_items)
    n = n_items
    shared = n // 2
    lengths = rng.integers(0, min(n, 80) + 1, n)
    rows = []
    for r in range(n):
        if r == 0:
            cols = np.arange(n)
        elif r == 1:
            cols = np.zeros(0, np.int64)
        elif r == 2:
            cols = np.array([shared])
        elif r == 3:
            cols = np.union1d(rng.choice(n, min(n, 700), replace=False), [shared])
        else:
            cols = np.union1d(rng.integers(0, n, lengths[r]), [shared])
        rows.append(cols)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(c) for c in rows], out=indptr[1:])
    indices = np.concatenate(rows).astype(np.int32)
    values = np.exp(rng.uniform(np.log(1e-6), np.log(1e3), len(indices))).astype(np.float32)
    s = sps.csr_array((values, indices, indptr), shape=(n, n))
    named = np.array([r for r in range(n) if r != 1])
    desc = np.sort(rng.choice(n, min(n, 40), replace=False))[::-1]
    queries = [
        np.zeros(0, np.int32),
        np.full(3, -1, np.int32),
        np.array([0]),
        np.full(3, min(3, n - 1)),
        rng.choice(named, 300),
        np.concatenate([desc[:len(desc) // 2], [-1], desc[len(desc) // 2:]]),
        np.concatenate([rng.integers(0, n, 20), [-1], rng.integers(0, n, 5)]),
        rng.integers(0, n, 50),
        rng.integers(0, n, 5),
    ]
    assert len(queries) == N_QUERIES
    return s, [np.asarray(q, dtype=np.int32) for q in queries]
