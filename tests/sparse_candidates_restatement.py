"""NumPy / float32 restatement of ``lk_sparse_score_candidates`` (csrc/sparse_candidates.hip),
written from its contract in include/lkamd.h, not from the kernel: per target a chain over the
query's history rows of a sparse item-item model, one float32 operation per history item in
history order."""
import numpy as np


def sparse_score_candidates_ref(hist_ptr, hist_items, rows, m_ptr, m_idx, m_val, n_items,
                                tgt_ptr, tgt_items, reduce):
    """
    f32 [len(tgt_items)].  ``hist_ptr`` / ``hist_items``: the histories (CSR, -1 = unknown item);
    ``rows``: the history row of each query (outside the CSR = no history), None: query q reads
    row q.  ``m_ptr`` / ``m_idx`` / ``m_val``: the model CSR, columns ascending inside a row.
    ``reduce``: ``"sum"`` (NaN for a history without entries), ``"mean"`` / ``"max"`` (NaN
    without a known history item).  NaN for a target outside ``[0, n_items)``.
    """
    assert reduce in ("sum", "mean", "max")
    hist_ptr = np.asarray(hist_ptr, np.int64)
    hist_items = np.asarray(hist_items, np.int32)
    m_ptr = np.asarray(m_ptr, np.int64)
    m_idx = np.asarray(m_idx, np.int32)
    m_val = np.asarray(m_val, np.float32)
    tgt_ptr = np.asarray(tgt_ptr, np.int64)
    tgt_items = np.asarray(tgt_items, np.int32)
    out = np.full(len(tgt_items), np.nan, np.float32)
    for q in range(len(tgt_ptr) - 1):
        lo, hi = int(tgt_ptr[q]), int(tgt_ptr[q + 1])
        r = q if rows is None else int(rows[q])
        hist = hist_items[hist_ptr[r]:hist_ptr[r + 1]] if 0 <= r < len(hist_ptr) - 1 else \
            hist_items[:0]
        known = hist[(hist >= 0) & (hist < n_items)]
        cols = tgt_items[lo:hi]
        ok = (cols >= 0) & (cols < n_items)
        acc = np.zeros(hi - lo, np.float32)
        for it in known.tolist():  # history order; a repeated item is walked again
            b, e = int(m_ptr[it]), int(m_ptr[it + 1])
            if b == e:
                continue
            at = np.searchsorted(m_idx[b:e], cols)
            hit = ok & (at < e - b)
            hit[hit] = m_idx[b:e][at[hit]] == cols[hit]
            v = m_val[b:e][at[hit]]
            if reduce == "max":
                acc[hit] = np.where(v > acc[hit], v, acc[hit])
            else:
                acc[hit] = acc[hit] + v  # (float32 + float32, rounded once)
        if reduce == "sum":
            empty = len(hist) == 0
        else:
            empty = len(known) == 0
        if empty:
            continue
        if reduce == "mean":
            acc = (acc.astype(np.float64) / np.float64(len(known))).astype(np.float32)
        out[lo:hi][ok] = acc[ok]
    return out


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
