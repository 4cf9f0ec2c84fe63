"""NumPy restatement of the ragged candidate kernels (csrc/candidates.hip), written from their
contract in include/lkamd.h, not from the kernels: what ``lk_ragged_topn`` and
``lk_panel_take_ragged`` must give.  The chain reference of ``lk_score_candidates`` is
``oracle.score_dense`` gathered at the targets (:func:`score_candidates_ref`)."""
import numpy as np


def f2key(x) -> np.ndarray:
    """The selection kernels' order-preserving unsigned image of a float32 (csrc/common.h):
    -0.0 first becomes +0.0, then negative values are complemented and the others get the top bit."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ragged_topn_ref(ptr, items, scores, n):
    """
    (item numbers int32 [Q x width] padded with -1, scores f32 [Q x width] padded with NaN): per
    segment the entries with a non-NaN score and an item >= 0, by (f2key descending, position
    ascending), at most ``n`` of them; ``n < 0``: all, ``width`` = the longest segment.
    """
    ptr = np.asarray(ptr, np.int64)
    items = np.asarray(items, np.int32)
    scores = np.asarray(scores, np.float32)
    nq = len(ptr) - 1
    lens = np.diff(ptr)
    width = (int(lens.max()) if nq else 0) if n < 0 else int(n)
    out_i = np.full((nq, width), -1, np.int32)
    out_s = np.full((nq, width), np.nan, np.float32)
    for q in range(nq):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        it, sc = items[lo:hi], scores[lo:hi]
        pos = np.flatnonzero(~np.isnan(sc) & (it >= 0))
        keys = f2key(sc[pos]).astype(np.int64)
        order = pos[np.lexsort((pos, -keys))][:width]  # last key is the primary one
        out_i[q, :len(order)] = it[order]
        out_s[q, :len(order)] = sc[order]
    return out_i, out_s


def take_ragged_ref(panel, n_items, ptr, items):
    "out[t] = panel[q, items[t]] for t in segment q, NaN for an item outside [0, n_items)"
    ptr = np.asarray(ptr, np.int64)
    items = np.asarray(items, np.int32)
    out = np.full(len(items), np.nan, np.float32)
    for q in range(len(ptr) - 1):
        for t in range(int(ptr[q]), int(ptr[q + 1])):
            if 0 <= items[t] < n_items:
                out[t] = panel[q, items[t]]
    return out


def score_candidates_ref(oracle, users, items_mat, user_rows, ptr, items):
    """``oracle.score_dense`` -- the k-ordered fmaf chain restated in C -- of each query's user row
    against the whole item table, gathered at the targets; NaN for a row or item outside its table."""
    ptr = np.asarray(ptr, np.int64)
    out = np.full(len(items), np.nan, np.float32)
    dense = {}
    for q in range(len(ptr) - 1):
        r = int(user_rows[q])
        if not 0 <= r < len(users) or ptr[q] == ptr[q + 1]:
            continue
        if r not in dense:
            dense[r] = oracle.score_dense(items_mat, users[r])
        seg = np.asarray(items[ptr[q]:ptr[q + 1]], np.int64)
        ok = (seg >= 0) & (seg < len(items_mat))
        out[int(ptr[q]):int(ptr[q + 1])][ok] = dense[r][seg[ok]]
    return out


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
