"""
CPU restatement of one SLIM column (``compute_column``, src/accel/slim/mod.rs:147-300), written
in NumPy from the algorithm: the yardstick of ``tests/test_slim_host.py`` and
``tests/test_gpu_slim.py``.  Every float32 step is a separate NumPy float32 operation, and the one
sequential sum is ``np.cumsum(..., dtype=float32)`` (NumPy accumulates a cumsum entry by entry).
"""
from __future__ import annotations

import numpy as np

EPSILON = np.float32(1.0e-12)
OPT_TOLERANCE = np.float32(1e-3)


def csr_pair(mat):
    "users x items SciPy matrix -> (ui indptr, ui indices, iu indptr, iu indices), rows sorted."
    import scipy.sparse as sps

    ui = sps.csr_array(mat)
    ui.sort_indices()
    iu = sps.csr_array(ui.T)
    iu.sort_indices()
    return (ui.indptr.astype(np.int64), ui.indices.astype(np.int32),
            iu.indptr.astype(np.int64), iu.indices.astype(np.int32))


def slim_column(ui_ptr, ui_idx, iu_ptr, iu_idx, item: int, l1: float, l2: float, max_iters: int,
                max_nbrs: int | None, info: dict | None = None):
    """
    Row ``item`` of the transposed weight matrix: (indices int32 ascending, values float32).
    ``info`` receives ``rounds``, ``active`` (list length before the cut), ``kept``, ``cut``,
    ``tie_at_cut``, ``coord_updates`` and ``resid_entries``.
    """
    n_users, n_items = len(ui_ptr) - 1, len(iu_ptr) - 1
    l1, l2 = np.float32(l1), np.float32(l2)
    i_users = iu_idx[iu_ptr[item]:iu_ptr[item + 1]]
    resid = np.zeros(n_users, np.float32)
    resid[i_users] = np.float32(1.0)

    # active list in first-encounter order + co-rating counts
    stream = np.concatenate([ui_idx[ui_ptr[u]:ui_ptr[u + 1]] for u in i_users]) \
        if len(i_users) else np.zeros(0, np.int32)
    stream = stream[stream != item]
    uniq, first = np.unique(stream, return_index=True)
    active = uniq[np.argsort(first, kind="stable")].astype(np.int64)
    counts = np.bincount(stream, minlength=n_items)
    n_of = np.diff(iu_ptr)

    cut = max_nbrs is not None and max_nbrs < len(active)
    tie = False
    n_active = len(active)
    if cut:
        i_norm = np.sqrt(np.float64(len(i_users)))
        j_norm = np.sqrt(n_of[active].astype(np.float64))
        key = -(counts[active].astype(np.float64)) / (i_norm * j_norm)
        order = np.argsort(key, kind="stable")
        tie = bool(key[order[max_nbrs - 1]] == key[order[max_nbrs]])
        active = active[order[:max_nbrs]]

    users_of = [iu_idx[iu_ptr[j]:iu_ptr[j + 1]] for j in active]
    n_f32 = [np.float32(len(nz)) for nz in users_of]
    w = np.zeros(len(active), np.float32)
    rounds = 0
    zero = np.float32(0.0)
    for _ in range(int(max_iters)):
        rounds += 1
        dmax = zero
        for p, nz in enumerate(users_of):
            cur = w[p]
            upd = np.cumsum(resid[nz] + cur, dtype=np.float32)[-1] if len(nz) else zero
            new = (upd - l1) / (n_f32[p] + l2) if upd >= l1 else zero
            diff = np.float32(new - cur)
            w[p] = new
            resid[nz] -= diff
            if abs(diff) > dmax:
                dmax = abs(diff)
        if dmax <= OPT_TOLERANCE:
            break
    if info is not None:
        info.update(rounds=rounds, active=n_active, kept=len(active), cut=bool(cut),
                    tie_at_cut=tie, coord_updates=rounds * len(active),
                    resid_entries=rounds * int(sum(len(nz) for nz in users_of)))
    keep = w >= EPSILON
    idx, val = active[keep], w[keep]
    order = np.argsort(idx, kind="stable")
    return idx[order].astype(np.int32), val[order].astype(np.float32)


def slim_rows(ui_ptr, ui_idx, iu_ptr, iu_idx, columns, l1, l2, max_iters, max_nbrs, infos=None):
    "The columns' rows as CSR arrays (indptr int64, indices int32, values float32)."
    ptr, idx, val = [0], [], []
    for c in columns:
        info = {} if infos is not None else None
        i, v = slim_column(ui_ptr, ui_idx, iu_ptr, iu_idx, int(c), l1, l2, max_iters, max_nbrs,
                           info)
        if infos is not None:
            infos.append(info)
        idx.append(i)
        val.append(v)
        ptr.append(ptr[-1] + len(i))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return np.asarray(ptr, np.int64), cat(idx, np.int32), cat(val, np.float32)
